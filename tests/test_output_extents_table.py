"""CPU: the table of output extents (tests/guard_bands.py EXTENTS) names every output parameter include/deepsignal_hip.h
declares, so a new ABI entry fails here until its extents are held behind guard bands."""
import os
import re

import guard_bands as gb


def test_every_output_parameter_of_the_header_is_in_the_table():
    decl = gb.declared_functions()
    assert len(decl) >= 100 and "ds_forward" in decl and "ds_train_get_tap" in decl
    want = {}
    for name, plist in decl.items():
        outs = gb.output_params(plist)
        if outs:
            want[name] = outs
    assert sorted(gb.EXTENTS) == sorted(want), "functions missing from / unknown to the table: %s" % sorted(set(gb.EXTENTS) ^ set(want))
    for name, outs in want.items():
        assert sorted(gb.EXTENTS[name]) == sorted(p for p, _, _ in outs), "%s: the table lists %s, the header has %s" % (
            name, sorted(gb.EXTENTS[name]), sorted(p for p, _, _ in outs))


def test_only_handle_out_pointers_are_exempt():
    decl = gb.declared_functions()
    for name, params in gb.EXTENTS.items():
        kinds = {p: handle_out for p, _, handle_out in gb.output_params(decl[name])}
        for p, where in params.items():
            if where.startswith("exempt"):
                assert kinds[p] or (name, p) in gb.NOT_OUTPUTS, "%s(%s) is an output and may not be exempt" % (name, p)
            else:
                assert not kinds[p], "%s(%s) is a handle out-pointer" % (name, p)
    assert list(gb.NOT_OUTPUTS) == [("ds_free_host", "p")]


def test_the_files_the_table_names_call_the_entries_they_cover():
    """An entry listed as covered by a test file is reached there through guard_bands.call."""
    tests = os.path.dirname(os.path.abspath(__file__))
    src = {f: open(os.path.join(gb.ROOT, f)).read() for f in (gb.GPU, gb.HOST)}
    assert os.path.samefile(os.path.join(gb.ROOT, gb.GPU), os.path.join(tests, os.path.basename(gb.GPU)))
    for name, params in gb.EXTENTS.items():
        for where in set(params.values()):
            if where.startswith("exempt"):
                continue
            for f in (gb.GPU, gb.HOST):
                if f in where:
                    assert re.search(r'"%s"' % name, src[f]), "%s does not call %s" % (f, name)
