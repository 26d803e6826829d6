"""The 16-bit list rows' format (csrc/mph_params.h kOff16Bits), CPU only: a
stand-alone program (tests/native/list16_check.cpp) checks the host-callable helpers the search, the
passes and the host readers share -- an entry's encode / decode over the whole 13-bit range and all
types, the store counter of both formats against a plain row / lane computation for rows 0-639 and
lanes 0-63, the "group of row k" walk against a linear search for headers with empty and non-empty
groups, and HostRows::entry -- under ASan + UBSan where the host compiler has them."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_list16_format(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]
    # whether the sanitizers are there is decided on an empty program; without them the plain build runs
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(base + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    flags = base + (san if r.returncode == 0 else [])
    out = str(tmp_path / "list16_check")
    r = subprocess.run(flags + [os.path.join(ROOT, "tests", "native", "list16_check.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr
    assert r.stdout.strip().endswith("list16_check ok")
