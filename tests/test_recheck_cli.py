"""Cascaded precision (`call_mods --precision bf16_all --recheck_margin M`), the parts that need no GPU: the two flags and
their usage error, and the C ABI's new entry points in the built library."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["call_mods", "-i", "x", "-m", "w", "-o", "o"]


def test_flags_parse_with_their_defaults():
    from deepsignal_amd.deepsignal import build_parser
    a = build_parser().parse_args(BASE)
    assert a.recheck_margin == 0.0 and a.recheck_precision == "fp32"
    a = build_parser().parse_args(BASE + ["--precision", "bf16_all", "--recheck_margin", "0.1", "--recheck_precision", "bf16x3"])
    assert a.recheck_margin == pytest.approx(0.1) and a.recheck_precision == "bf16x3" and a.precision == "bf16_all"
    with pytest.raises(SystemExit):
        build_parser().parse_args(BASE + ["--recheck_precision", "bf16"])       # not an fp32-class mode


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_margin_with_an_fp32_class_precision_is_a_usage_error(precision, capsys):
    """Nothing to recheck: refused by the command line (exit status 2, before the input is looked at) and by the functions."""
    from deepsignal_amd import call_modifications as cm
    from deepsignal_amd.deepsignal import main
    with pytest.raises(SystemExit) as ei:
        main(BASE + ["--recheck_margin", "0.1", "--precision", precision])
    assert ei.value.code == 2
    assert "nothing to recheck" in capsys.readouterr().err
    with pytest.raises(ValueError, match="nothing to recheck"):
        cm.call_mods("x", "w", "o", 17, 360, 512, 0.001, 2, 1, False, True, True, True, None, precision=precision,
                     recheck_margin=0.1)
    with pytest.raises(ValueError, match="nothing to recheck"):
        cm.make_engine("w", 17, 360, 2, 512, precision=precision, recheck_margin=0.1)
    cm.check_recheck_args(precision, 0.0, "fp32")                               # margin 0 = off: fine with any precision
    cm.check_recheck_args("bf16_all", 0.1, "bf16x3")
    cm.check_recheck_args("bf16", 0.1, "fp32")
    with pytest.raises(ValueError):
        cm.check_recheck_args("bf16_all", -0.1, "fp32")
    with pytest.raises(ValueError):
        cm.check_recheck_args("bf16_all", float("nan"), "fp32")
    with pytest.raises(ValueError):
        cm.check_recheck_args("bf16_all", 0.1, "bf16")


def test_library_exports_the_recheck_entry_points():
    """ds_set_recheck / ds_get_recheck_stats: declared in the header with the documented signatures, exported by the built
    library, bound by the Python layer with matching ctypes signatures. Symbol lookup only, no GPU call."""
    from deepsignal_amd import engine
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "deepsignal_hip.h")).read())
    assert "int ds_set_recheck(ds_handle *coarse, ds_handle *fine, float margin);" in text
    assert ("int ds_get_recheck_stats(ds_handle *coarse, int64_t *sites, int64_t *rechecked, int64_t *fine_forwards);") in text
    raw = ctypes.CDLL(engine.LIB_PATH)
    for name in ("ds_set_recheck", "ds_get_recheck_stats"):
        assert name in engine.EXPORTED_SYMBOLS
        assert ctypes.cast(getattr(raw, name), ctypes.c_void_p).value
    lib = engine.load_library()
    p64 = ctypes.POINTER(ctypes.c_int64)
    assert list(lib.ds_set_recheck.argtypes) == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float]
    assert list(lib.ds_get_recheck_stats.argtypes) == [ctypes.c_void_p, p64, p64, p64]
    assert lib.ds_set_recheck.restype is ctypes.c_int and lib.ds_get_recheck_stats.restype is ctypes.c_int
    # a null handle is refused before anything touches a device
    assert lib.ds_set_recheck(None, None, 0.1) == -1
    assert lib.ds_get_recheck_stats(None, None, None, None) == -1
    assert hasattr(engine.Engine, "set_recheck") and hasattr(engine.Engine, "recheck_stats")
