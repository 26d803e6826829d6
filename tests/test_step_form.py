"""A step's form (csrc/mph_kernels.h seq_step, trim_outputs), CPU only: a
stand-alone program (tests/native/step_form.cpp) walks the 64 combinations of last step, surface
tension, coarse map, monitors, MPH_LEAN_STEPS and the lean-search capability and checks the three
fields of the form, the nullness of the nine trimmed outputs and that every other field of the Launch
comes through unchanged, against rules written out in the program itself."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_form(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    rocm_include = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    assert os.path.isfile(os.path.join(rocm_include, "hip", "hip_runtime.h")), rocm_include
    out = str(tmp_path / "step_form")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + rocm_include,
                        "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "native", "step_form.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=30)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("step_form ok")
