"""Sanitizers on the host half of the kinematics (CPU only): mph_kinematics_arrays, _n0, _parse, _layout
and the .vtu writer of csrc/mph_host.cpp, with the inlines of csrc/mph_params.h that the device
shares, compiled with -fsanitize=address,undefined into a small stand-alone program
(tests/native/kin_asan.cpp) and run once, as tests/test_native_asan.py does for the rest of the host
layer."""
import os
import shutil
import subprocess

import pytest

from particlemethod_fsi_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kinematics_host_functions_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "kin_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=all", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-pthread",
           os.path.join(ROOT, "tests", "native", "kin_asan.cpp"),
           os.path.join(ROOT, "particlemethod_fsi_amd", "csrc", "mph_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer build unavailable: " + r.stderr[-500:])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "kin_asan: ok" in r.stdout
    for f in ("k2.vtu", "k3.vtu"):   # (the last write of each run: no particles)
        assert len(solver.read_vtu(str(tmp_path / f))["Count"]) == 0
