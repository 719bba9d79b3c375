"""The run-time switches of the native library (csrc/fa_switches.h), without a GPU: every parse rule against a hand-written table,
one reader of the environment in csrc/, and the names the library reports against the table of docs/SWITCHES.md."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import PKG, ROOT

CSRC = os.path.join(PKG, "csrc")
PARSE_SRC = os.path.join(ROOT, "tests", "switches_parse.cpp")


@pytest.mark.parametrize("define", [[], ["-DAULE_DEBUG_HOOKS"]], ids=["product", "debug-hooks"])
def test_parse_rules_match_the_recorded_table(tmp_path, define):
    """tests/switches_parse.cpp: read_switches() on fake environments, every switch unset, at each documented value, at the lenient
    spellings and at the number edge cases -- host code with its own main, built under ASan + UBSan (a header that needs anything but
    the standard library does not compile here)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "switches_parse")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, PARSE_SRC, "-o", exe] + define
    # (the runtimes linked into the program: it then runs whatever else the environment loads into every process; clang does so by itself)
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and re.search(r"^PARSE OK \d+$", r.stdout, re.M), r.stdout[-3000:] + r.stderr[-3000:]


def test_one_reader_of_the_environment_in_csrc():
    """`getenv` occurs in csrc/ in fa_switches.h (once: switches()) and in aule_init's two reads, which are per call on purpose."""
    sites = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h", ".cpp", ".inc")):
            lines = [ln for ln in open(os.path.join(CSRC, name), errors="replace").read().splitlines() if "getenv" in ln]
            if lines:
                sites[name] = lines
    assert sorted(sites) == ["aule_capi.cpp", "fa_switches.h"], sites
    assert len(sites["fa_switches.h"]) == 1 and sum(ln.count("getenv") for ln in sites["fa_switches.h"]) == 1, sites
    assert len(sites["aule_capi.cpp"]) == 2 and 'getenv("AULE_BACKEND")' in sites["aule_capi.cpp"][0] and 'getenv("AULE_HIP_DEVICE")' in sites["aule_capi.cpp"][1], sites


def _doc_rows():
    """{name: 'read by' cell} of the run-time table of docs/SWITCHES.md (a row may name two values of one variable, never two variables)."""
    text = open(os.path.join(ROOT, "docs", "SWITCHES.md")).read()
    table = text[text.index("| run-time (environment) |"):text.index("| build flag (default) |")]
    rows = {}
    for line in table.splitlines()[2:]:
        if not line.startswith("|"):
            continue
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        names = set(re.findall(r"AULE_[A-Z0-9_]+", cells[0]))
        assert len(names) == 1 and len(cells) == 4 and cells[1] and cells[2], line
        name = names.pop()
        assert name not in rows, name
        rows[name] = cells[2]
    return rows


_HOOK_CHILD = r'''
import json, os, sys
sys.path[:0] = [os.path.join(sys.argv[1], "aule-attention_amd"), os.path.join(sys.argv[1], "tests")]
from util import switches_in_force
print("SWITCHES " + json.dumps(switches_in_force()))
'''


def _reported(env):
    import json
    e = {k: v for k, v in os.environ.items() if not k.startswith(("AULE_HIP_", "AULE_TL", "AULE_DBG_", "AULE_ROCTX"))}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _HOOK_CHILD, ROOT], env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("SWITCHES ")][-1][9:])


def test_reported_switches_are_the_documented_ones():
    """aule_hip_debug_switches (through ctypes, before any aule_init) names exactly the rows of docs/SWITCHES.md that the library reads
    once; the rest of the table belongs to aule_init and to Python.  A switch added to the header without a row, or a row without a
    switch, fails here."""
    rows = _doc_rows()
    library = {n for n, by in rows.items() if by == "library"}
    got = _reported({})
    assert set(got) == library and len(library) == 25, (sorted(set(got) ^ library), len(library))
    others = {n: by for n, by in rows.items() if by != "library"}
    assert set(others) == {"AULE_BACKEND", "AULE_HIP_DEVICE", "AULE_LIBRARY_PATH", "AULE_HIP_ROPE_FUSE", "AULE_HIP_ALWAYS_AUTOGRAD", "AULE_PEER_CACHE_KEYS"}, others
    assert all(by.startswith("`aule_init`") for n, by in others.items() if n in ("AULE_BACKEND", "AULE_HIP_DEVICE"))
    assert all(by.startswith("Python") for n, by in others.items() if n not in ("AULE_BACKEND", "AULE_HIP_DEVICE"))
    # the unset environment, spelt like any other value
    assert got["AULE_HIP_BWD_MODE"] == "auto" and got["AULE_HIP_BWD_DKV"] == "default" and got["AULE_HIP_FWD_KERNEL"] == "default"
    assert got["AULE_HIP_BWD_DS_AUTO_MB"] == "160" and got["AULE_HIP_BWD_DS_CAP_MB"] == "8192" and got["AULE_HIP_W4_WTAIL"] == "4"
    assert got["AULE_HIP_FWD_SPLIT"] == "8" and got["AULE_HIP_FWD_SPLIT_MIN"] == "16" and got["AULE_HIP_W4_SUMLO"] == "default"
    # the buffer contract: the size answered without a buffer, a short buffer truncated and terminated, never written past
    import ctypes
    from aule import _capi
    lib = _capi.load()
    need = int(lib.aule_hip_debug_switches(None, 0))
    buf = ctypes.create_string_buffer(b"\xff" * 64, 64)
    assert int(lib.aule_hip_debug_switches(buf, 16)) == need and buf.raw[:16] == b"AULE_HIP_FWD_KE\x00" and buf.raw[16:] == b"\xff" * 48


def test_a_child_reports_the_switches_it_was_started_with():
    """Three switches set: resolved as set, everything else at its default.  A misspelt name: the default -- which is how a leg of the
    GPU suites finds out that it would test something else (tests/util.py: assert_switches)."""
    dflt = _reported({})
    got = _reported({"AULE_HIP_BWD_MODE": "spill", "AULE_HIP_W4_WTAIL": "99", "AULE_HIP_FWD_COMBINE": "wg"})
    want = dict(dflt, AULE_HIP_BWD_MODE="spill", AULE_HIP_W4_WTAIL="99", AULE_HIP_FWD_COMBINE="wg")
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert _reported({"AULE_HIP_BWD_MODES": "spill", "AULE_HIP_FWD_KERNAL": "pp", "AULE_HIP_W4_BODY": "generic"}) == dflt
    assert _reported({"AULE_HIP_FWD_KERNEL": "ppp"})["AULE_HIP_FWD_KERNEL"] == "default"      # (a misspelt value: warned about, and the default)
