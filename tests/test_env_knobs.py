"""The environment helpers of csrc/mph_env.h (CPU only): a stand-alone program
(tests/native/env_check.cpp) prints what each helper returns for a value of one variable; compared
here with the rules the library's knobs are built from (the table in INTEGRATION.md)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# value (None: unset) -> int0/int1 = env_int with default 0/1, dbl = env_double with default 0.25,
# env_is against "0", "1", "auto", "", and env_str
EXPECT = {
    None:   dict(int0=0, int1=1, dbl="0.25", is0=0, is1=0, isauto=0, isempty=0, str=""),
    "":     dict(int0=0, int1=0, dbl="0", is0=0, is1=0, isauto=0, isempty=1, str=""),
    "0":    dict(int0=0, int1=0, dbl="0", is0=1, is1=0, isauto=0, isempty=0, str="0"),
    "1":    dict(int0=1, int1=1, dbl="1", is0=0, is1=1, isauto=0, isempty=0, str="1"),
    "auto": dict(int0=0, int1=0, dbl="0", is0=0, is1=0, isauto=1, isempty=0, str="auto"),
    "2":    dict(int0=2, int1=2, dbl="2", is0=0, is1=0, isauto=0, isempty=0, str="2"),
    "x":    dict(int0=0, int1=0, dbl="0", is0=0, is1=0, isauto=0, isempty=0, str="x"),
}

# the knobs' rules at these values, as the library spells them from the helpers:
#   MPH_SLAB_OVERLAP                  1 / 0 forced, anything else (unset, "auto") probes (-1)
#   MPH_SLAB_EARLY, _VIRTUAL_C, _GRAPHS  off only at "0":       not is0
#   MPH_LIST_FULL                     on only at 1:             int0 == 1
#   MPH_LAZY_WALLS                    off at a zero number:     int1 != 0 (so off only at "0" among 0/1/unset)
KNOBS = {
    None:   dict(overlap=-1, off_only_at_0=True, list_full=False, lazy_walls=True),
    "":     dict(overlap=-1, off_only_at_0=True, list_full=False, lazy_walls=False),
    "0":    dict(overlap=0, off_only_at_0=False, list_full=False, lazy_walls=False),
    "1":    dict(overlap=1, off_only_at_0=True, list_full=True, lazy_walls=True),
    "auto": dict(overlap=-1, off_only_at_0=True, list_full=False, lazy_walls=False),
    "2":    dict(overlap=-1, off_only_at_0=True, list_full=False, lazy_walls=True),
    "x":    dict(overlap=-1, off_only_at_0=True, list_full=False, lazy_walls=False),
}


@pytest.fixture(scope="module")
def env_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("env") / "env_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "particlemethod_fsi_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "env_check.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _run(binary, value):
    env = {k: v for k, v in os.environ.items() if k != "MPH_T"}
    if value is not None:
        env["MPH_T"] = value
    r = subprocess.run([binary], capture_output=True, text=True, env=env, timeout=30)
    assert r.returncode == 0, r.stderr
    line = r.stdout.strip()
    head, s = line.split(" str=[")
    got = dict(kv.split("=") for kv in head.split())
    got["str"] = s[:-1]
    return got


@pytest.mark.parametrize("value", list(EXPECT), ids=lambda v: "unset" if v is None else repr(v))
def test_env_helpers(env_check, value):
    got = _run(env_check, value)
    print(value, got)
    want = EXPECT[value]
    for k in ("int0", "int1", "is0", "is1", "isauto", "isempty"):
        assert int(got[k]) == want[k], (value, k, got)
    assert got["dbl"] == want["dbl"] and got["str"] == want["str"], (value, got)
    knobs = KNOBS[value]
    assert (1 if int(got["is1"]) else (0 if int(got["is0"]) else -1)) == knobs["overlap"]
    assert (not int(got["is0"])) == knobs["off_only_at_0"]
    assert (int(got["int0"]) == 1) == knobs["list_full"]
    assert (int(got["int1"]) != 0) == knobs["lazy_walls"]
