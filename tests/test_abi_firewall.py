"""The C ABI's exception firewall (include/deepsignal_hip.h: no entry point throws; csrc/ds_abi.h).

test_every_entry_point_is_defined_once_behind_the_handler reads the sources: every function the header declares has exactly one
definition under csrc, and every one that returns int or int64_t is a function-try-block that ends in the shared handler. An entry
point written without the block fails here by name.

test_fault_injection builds tools/abi_firewall.cpp against the built library and runs it: an allocation failure (and a
std::runtime_error) injected at every allocation of every entry point that needs no GPU comes back as a DS_ERR_* code.
Neither test needs a GPU."""
import functools
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepsignal_amd", "csrc")

HANDLER = re.compile(r"^\} catch \(\.\.\.\) \{ return abi_error\((\w+)\); \}$")


def declared():
    """name -> return type text ("int", "int64_t", "const char *", ...) of every function the header declares"""
    text = open(os.path.join(ROOT, "include", "deepsignal_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"^([A-Za-z_][\w \*]*?)\b(ds_\w+)\(", text, re.M):
        assert m.group(2) not in out, "declared twice: " + m.group(2)
        out[m.group(2)] = " ".join(m.group(1).split())
    return out


@functools.lru_cache(maxsize=None)
def source_lines(csrc):
    paths = sorted(glob.glob(os.path.join(csrc, "*.cpp")) + glob.glob(os.path.join(csrc, "*.hip")))
    return [(path, open(path).read().split("\n")) for path in paths]


def definitions(name, csrc=CSRC):
    """(file, the definition's text from its first line to the line that closes it) for every definition of `name` under csrc"""
    found = []
    start = re.compile(r"^(?:static )?[A-Za-z_][\w \*]*?\b%s\(" % re.escape(name))
    for path, lines in source_lines(csrc):
        for i, line in enumerate(lines):
            if name not in line or not start.match(line) or line.rstrip().endswith(";"):
                continue
            j = i
            if not line.rstrip().endswith("}"):      # not a one-line definition: runs to the first brace in column 0
                j = next(k for k in range(i + 1, len(lines)) if lines[k].startswith("}"))
            found.append((os.path.basename(path), "\n".join(lines[i:j + 1])))
    return found


def test_every_entry_point_is_defined_once_behind_the_handler():
    names = declared()
    assert len(names) >= 102, len(names)
    bad = []
    for name, ret in sorted(names.items()):
        defs = definitions(name)
        if len(defs) != 1:
            bad.append("%s: %d definitions %s" % (name, len(defs), [d[0] for d in defs]))
            continue
        where, text = defs[0]
        if text.startswith("static "):
            bad.append("%s (%s): the definition is static" % (name, where))
        if ret not in ("int", "int64_t"):
            continue
        head = text[:text.index("{")]
        if not re.search(r"\)\s*try\s*$", head):
            bad.append("%s (%s): not a function-try-block" % (name, where))
            continue
        last = text.split("\n")[-1]
        tail = last[last.rindex("} catch"):] if "\n" not in text and "} catch" in last else last
        m = HANDLER.match(tail)
        if not m:
            bad.append("%s (%s): does not end in `} catch (...) { return abi_error(...); }` but in %r" % (name, where, tail[-80:]))
            continue
        # the error text goes to the object the entry was given: its first parameter when that is a handle or a reader it may write
        first = re.match(r"\s*(?:ds_handle|ds_tsv)\s*\*\s*(\w+)\s*[,)]", head[head.index("(") + 1:])
        want = first.group(1) if first else "nullptr"
        if m.group(1) != want:
            bad.append("%s (%s): the handler is given %s, expected %s" % (name, where, m.group(1), want))
    assert not bad, "\n".join(bad)
    # the twins and the opt-in guard this replaced stay gone
    for path in glob.glob(os.path.join(CSRC, "*")):
        if os.path.isfile(path) and not path.endswith((".so", ".o")):
            text = open(path, errors="replace").read()
            assert "_impl(" not in text and "guarded(" not in text, path


def test_the_check_sees_an_unguarded_definition(tmp_path):
    """the parser above is not vacuous: it tells a plain definition from a block, on one line or several"""
    (tmp_path / "x.cpp").write_text(
        "int ds_sync(ds_handle* h)\n{\n    return 0;\n}\n\n"
        "int ds_wait(ds_handle* h) try {\n    return 0;\n} catch (...) { return abi_error(h); }\n"
        "int ds_num_slots(ds_handle* h) try { return 1; } catch (...) { return abi_error(h); }\n")
    (_, plain), = definitions("ds_sync", str(tmp_path))
    assert not re.search(r"\)\s*try\s*$", plain[:plain.index("{")])
    (_, block), = definitions("ds_wait", str(tmp_path))
    assert re.search(r"\)\s*try\s*$", block[:block.index("{")]) and HANDLER.match(block.split("\n")[-1])
    (_, one), = definitions("ds_num_slots", str(tmp_path))
    assert "\n" not in one and HANDLER.match(one[one.rindex("} catch"):])


def test_fault_injection(tmp_path):
    """tools/abi_firewall.cpp: every allocation of every GPU-free entry point fails once, with std::bad_alloc and with a
    std::runtime_error, and the call returns the handler's code and text; the program states what it swept and exits 0"""
    cxx = shutil.which("g++")
    lib = os.path.join(ROOT, "deepsignal_amd", "libdeepsignal_hip.so")
    if cxx is None:
        pytest.skip("no g++")
    assert os.path.exists(lib), "build the library first (__graft_entry__.build)"
    exe = os.path.join(str(tmp_path), "abi_firewall")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread", os.path.join(ROOT, "tools", "abi_firewall.cpp"), lib,
                    "-Wl,-rpath," + os.path.dirname(lib), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode(errors="replace")
    print(text)
    assert out.returncode == 0, text[-4000:]
    assert "abi_firewall: ok" in text
