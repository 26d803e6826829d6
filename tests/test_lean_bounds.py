"""The lean search's radii (csrc/mph_params.h set_uniforms, lean_search_ok),
CPU only: a stand-alone program (tests/native/lean_bounds.cpp) fills a DevParams with the radii and
domains of d1m, d16m, box3d and dam2d and checks that the list radius lies below the search
radius' FP32 band, that the lean trimming bound lies between the list radius and the full search's
bound, and that the guard turns the lean search off when the lists keep every pair."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lean_bounds(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path / "lean_bounds")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "native", "lean_bounds.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=30)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("lean_bounds ok")
