"""A call's batches and the key fold's form (csrc/mph_kernels.h replay_plan, seq_step; DESIGN.md
sections 3.1 and 3.2), CPU only: a stand-alone program (tests/native/replay_plan.cpp) walks the plan
for n = 1 ... 80 with and without the all-lean 8-step graph and the lean single step -- the step
total, which steps store the output-only fields, the count of lean batches, the sequence below 16
steps -- and the two key-fold fields of a step's form over the sequences a context enqueues and all
combinations of structures, monitors, a slab's set, the coarse map and the toggle, against rules
written out in the program itself."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_replay_plan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    rocm_include = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    assert os.path.isfile(os.path.join(rocm_include, "hip", "hip_runtime.h")), rocm_include
    out = str(tmp_path / "replay_plan")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + rocm_include,
                        "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "native", "replay_plan.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=30)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("replay_plan ok")
