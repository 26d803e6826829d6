"""CPU: the monitors' part of the C ABI (include/mph_gpu.h) against its Python mirror.

The sample layout is shared by the header's enum MphMonitorSlot, the kernels and
solver.MONITOR_SLOTS; the configuration struct by the header and solver.MphMonitorConfig.
"""
import ctypes
import os
import re

from particlemethod_fsi_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mph_gpu.h")


def _header():
    txt = open(HEADER).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_monitor_slots_match_the_header_enum():
    txt = _header()
    body = re.search(r"typedef enum MphMonitorSlot \{(.*?)\} MphMonitorSlot;", txt, re.S).group(1)
    slots = {m.group(1): int(m.group(2)) for m in re.finditer(r"MPH_MON_([A-Z0-9_]+)\s*=\s*(\d+)", body)}
    assert len(slots) == 32
    assert sorted(slots.values()) == list(range(32))
    assert slots == solver.MONITOR_SLOTS
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+MPH_MONITOR_(\w+)\s+(\d+)", txt)}
    assert defs == {"MAX_TRACK": solver.MONITOR_MAX_TRACK, "MAX_PROBES": solver.MONITOR_MAX_PROBES,
                    "HEAD": solver.MONITOR_HEAD}
    assert solver.MONITOR_HEAD == len(slots)


def test_monitor_config_mirror_layout():
    # struct MphMonitorConfig on LP64: int stride, capacity, ntrack at 0, 4, 8; 4 bytes of padding;
    # const int* track at 16; int nprobe at 24 and 4 bytes of padding; const double* probes at 32;
    # double probe_radius at 40: 48 bytes, aligned to 8
    M = solver.MphMonitorConfig
    body = re.search(r"typedef struct MphMonitorConfig \{(.*?)\} MphMonitorConfig;", _header(), re.S).group(1)
    names = re.findall(r"(\w+)\s*;", body)
    assert names == [f[0] for f in M._fields_]
    assert ctypes.sizeof(ctypes.c_void_p) == 8
    expect = {"stride": 0, "capacity": 4, "ntrack": 8, "track": 16, "nprobe": 24, "probes": 32,
              "probe_radius": 40}
    assert {n: getattr(M, n).offset for n in names} == expect
    assert ctypes.sizeof(M) == 48
    assert ctypes.alignment(M) == 8


def test_abi_version_and_symbols():
    txt = _header()
    assert int(re.search(r"#define\s+MPH_ABI_VERSION\s+(\d+)", txt).group(1)) == solver.ABI_VERSION == 6
    for name in ("mph_monitor_configure", "mph_monitor_sample_doubles", "mph_monitor_read"):
        assert name in solver.EXPORTED_SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, txt)


def test_monitor_split_shapes():
    import numpy as np
    rows = np.arange(2 * (32 + 6 * 3 + 2 * 2), dtype=float).reshape(2, -1)
    head, trk, prb = solver.monitor_split(rows, 3, 2)
    assert head.shape == (2, 32) and trk.shape == (2, 3, 6) and prb.shape == (2, 2, 2)
    assert trk[0, 1, 0] == 32 + 6 and prb[0, 1, 1] == 32 + 18 + 3
    h1, t1, p1 = solver.monitor_split(rows[0], 3, 2)
    assert h1.shape == (32,) and t1.shape == (3, 6) and p1.shape == (2, 2)
