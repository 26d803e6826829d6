"""CPU: the free-surface-gauge part of the C ABI (include/mph_gpu.h mph_gauge_*) against its Python
mirror, and the row helpers monitor_gauges / monitor_split.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from particlemethod_fsi_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mph_gpu.h")
SYMBOLS = ("mph_gauge_configure", "mph_gauge_grid")


def _header():
    txt = open(HEADER).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_symbols_declared_and_exported():
    txt = _header()
    L = solver.load_library()
    for name in SYMBOLS:
        assert name in solver.EXPORTED_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(L, name), name
    assert int(re.search(r"#define\s+MPH_ABI_VERSION\s+(\d+)", txt).group(1)) == solver.ABI_VERSION == 6
    assert L.mph_abi_version() == 6


def test_gauge_channels_and_defines_match_the_header():
    txt = _header()
    body = re.search(r"typedef enum MphGaugeChannel \{(.*?)\} MphGaugeChannel;", txt, re.S).group(1)
    ch = {m.group(1): int(m.group(2)) for m in re.finditer(r"MPH_GAUGE_([A-Z]+)\s*=\s*(\d+)", body)}
    assert ch == solver.GAUGE_CHANNELS == {"COUNT": 0, "TOP": 1, "BOTTOM": 2, "WET": 3}
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+MPH_GAUGE_(\w+)\s+(\d+)\s*$", txt, re.M)}
    assert defs == {"MAX": 64, "CHANNELS": 4, "MAX_BINS": 8192}
    assert defs["MAX"] == solver.GAUGE_MAX and defs["MAX_BINS"] == solver.GAUGE_MAX_BINS
    assert defs["CHANNELS"] == len(ch)
    m = re.search(r"#define\s+MPH_GAUGE_GRID_MAX_LINES\s+\(1\s*<<\s*(\d+)\)", txt)
    assert 1 << int(m.group(1)) == solver.GAUGE_GRID_MAX_LINES == 2 ** 20
    # the monitors' ABI test collects every MPH_MONITOR_* define: none of the new ones is one
    assert not re.search(r"#define\s+MPH_MONITOR_\w*GAUGE", txt)


def test_gauge_config_mirror_layout():
    G = solver.MphGaugeConfig
    body = re.search(r"typedef struct MphGaugeConfig \{(.*?)\} MphGaugeConfig;", _header(), re.S).group(1)
    names = re.findall(r"(\w+)\s*;", body)
    assert names == [f[0] for f in G._fields_] == ["axis", "ngauge", "points", "radius"]
    assert {n: getattr(G, n).offset for n in names} == {"axis": 0, "ngauge": 4, "points": 8, "radius": 16}
    assert ctypes.sizeof(G) == 24
    assert ctypes.alignment(G) == 8


def test_gauge_grid_mirror_layout():
    G = solver.MphGaugeGrid
    body = re.search(r"typedef struct MphGaugeGrid \{(.*?)\} MphGaugeGrid;", _header(), re.S).group(1)
    names = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*;", body)
    assert names == [f[0] for f in G._fields_] == ["origin", "spacing", "count", "axis", "radius"]
    expect = {"origin": 0, "spacing": 24, "count": 48, "axis": 60, "radius": 64}
    assert {n: getattr(G, n).offset for n in names} == expect
    assert ctypes.sizeof(G) == 72
    assert ctypes.alignment(G) == 8


def test_monitor_gauges_takes_the_tail():
    nt, npr, ng = 2, 3, 5
    w = 32 + 6 * nt + 2 * npr + 4 * ng
    row = np.arange(w, dtype=np.float64)
    g = solver.monitor_gauges(row, nt, npr, ng)
    assert g.shape == (ng, 4)
    assert np.array_equal(g.reshape(-1), np.arange(w - 4 * ng, w))
    rows = np.arange(7 * w, dtype=np.float64).reshape(7, w)
    g = solver.monitor_gauges(rows, nt, npr, ng)
    assert g.shape == (7, ng, 4)
    assert np.array_equal(g[3, 4], rows[3, -4:])
    assert solver.monitor_gauges(row[:w - 4 * ng], nt, npr, 0).shape == (0, 4)
    with pytest.raises(ValueError):
        solver.monitor_gauges(row, nt, npr, ng - 1)
    # monitor_split keeps its meaning: a row with a gauge tail is not a sample of (nt, npr)
    with pytest.raises(ValueError):
        solver.monitor_split(row, nt, npr)
    head, trk, prb = solver.monitor_split(row[:w - 4 * ng], nt, npr)
    assert head.shape == (32,) and trk.shape == (nt, 6) and prb.shape == (npr, 2)
