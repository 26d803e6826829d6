"""CPU: the lattice-sampling part of the C ABI (include/mph_gpu.h) against its Python mirror, and
the host-only .vti writer against solver.read_vti.
"""
import ctypes
import os
import re
import xml.etree.ElementTree as ET

import numpy as np

from particlemethod_fsi_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mph_gpu.h")
SYMBOLS = ("mph_sample_grid", "mph_write_vti_arrays")


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


def test_sample_grid_mirror_layout():
    G = solver.MphSampleGrid
    body = re.search(r"typedef struct MphSampleGrid \{(.*?)\} MphSampleGrid;", _header(), re.S).group(1)
    names = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*;", body)
    assert names == [f[0] for f in G._fields_] == ["origin", "spacing", "count", "classes", "radius"]
    expect = {"origin": 0, "spacing": 24, "count": 48, "classes": 60, "radius": 64}
    assert {n: getattr(G, n).offset for n in names} == expect
    assert ctypes.sizeof(G) == 72
    assert ctypes.alignment(G) == 8


def test_sample_channels_match_the_header_enum():
    txt = _header()
    body = re.search(r"typedef enum MphSampleChannel \{(.*?)\} MphSampleChannel;", txt, re.S).group(1)
    ch = {m.group(1): int(m.group(2)) for m in re.finditer(r"MPH_SAMPLE_([A-Z]+)\s*=\s*(\d+)", body)}
    assert ch == solver.SAMPLE_CHANNELS
    assert sorted(ch.values()) == list(range(6))
    assert int(re.search(r"#define\s+MPH_SAMPLE_CHANNELS\s+(\d+)", txt).group(1)) == len(ch)
    m = re.search(r"#define\s+MPH_SAMPLE_MAX_POINTS\s+\(1\s*<<\s*(\d+)\)", txt)
    assert 1 << int(m.group(1)) == solver.SAMPLE_MAX_POINTS == 2 ** 24
    # the monitors' ABI test collects every MPH_MONITOR_* define: none of the new ones is one
    assert not re.search(r"#define\s+MPH_MONITOR_\w*SAMPLE", txt)


def _array():
    rng = np.random.default_rng(20240607)
    a = rng.standard_normal((5, 4, 3, 6))          # nz, ny, nx = 5, 4, 3: a 3 x 4 x 5 lattice
    a[0, 0, 0] = 0.0
    a[1, 2, 1, 2] = 5e-324                          # a denormal, the largest double, a negative zero
    a[2, 3, 2, 3] = np.finfo(float).max
    a[4, 0, 1, 5] = -0.0
    return a


def test_vti_round_trip_bitwise(tmp_path):
    a = _array()
    origin, spacing = (-0.00372, 0.1, 1.0 / 3.0), (0.00113, 2.0 ** -20, 0.7)
    path = str(tmp_path / "lattice.vti")
    solver.write_vti(path, a, origin, spacing)
    r = solver.read_vti(path)
    assert r["origin"] == list(origin) and r["spacing"] == list(spacing)
    assert r["extent"] == [0, 2, 0, 3, 0, 4]
    C = solver.SAMPLE_CHANNELS
    assert r["Count"].shape == (5, 4, 3) and r["Velocity"].shape == (5, 4, 3, 3)
    assert r["Count"].tobytes() == np.ascontiguousarray(a[..., C["COUNT"]]).tobytes()
    assert r["WSum"].tobytes() == np.ascontiguousarray(a[..., C["WSUM"]]).tobytes()
    assert r["PressureP"].tobytes() == np.ascontiguousarray(a[..., C["P"]]).tobytes()
    assert r["Velocity"].tobytes() == np.ascontiguousarray(a[..., C["VX"]:C["VZ"] + 1]).tobytes()
    assert sorted(k for k in r if k[0].isupper()) == ["Count", "PressureP", "Velocity", "WSum"]


def test_vti_header_is_xml(tmp_path):
    a = _array()
    path = str(tmp_path / "lattice.vti")
    solver.write_vti(path, a, (0.0, 0.0, 0.0), (0.001, 0.002, 0.003))
    raw = open(path, "rb").read()
    head, tag, rest = raw.partition(b'<AppendedData encoding="raw">')
    assert tag
    root = ET.fromstring(head + b"</VTKFile>")
    assert root.tag == "VTKFile" and root.get("type") == "ImageData"
    assert root.get("header_type") == "UInt64" and root.get("byte_order") == "LittleEndian"
    img = root.find("ImageData")
    assert img.get("WholeExtent") == "0 2 0 3 0 4"
    assert [float(v) for v in img.get("Spacing").split()] == [0.001, 0.002, 0.003]
    piece = img.find("Piece")
    assert piece.get("Extent") == img.get("WholeExtent")
    arrays = piece.find("PointData").findall("DataArray")
    assert [(d.get("Name"), d.get("type"), d.get("NumberOfComponents")) for d in arrays] == [
        ("Count", "Float64", None), ("WSum", "Float64", None), ("PressureP", "Float64", None),
        ("Velocity", "Float64", "3")]
    n = 60
    offs = [int(d.get("offset")) for d in arrays]
    assert offs == [0, 8 + 8 * n, 2 * (8 + 8 * n), 3 * (8 + 8 * n)]
    # the appended section: '_', then per array a UInt64 byte count and the doubles
    body = rest[rest.index(b"_") + 1:]
    assert int(np.frombuffer(body[:8], np.uint64)[0]) == 8 * n
    assert len(body) >= offs[3] + 8 + 24 * n
    assert body[offs[3] + 8 + 24 * n:].strip() == b"</AppendedData>\n</VTKFile>"


def test_write_vti_argument_errors(tmp_path):
    with np.testing.assert_raises(ValueError):
        solver.write_vti(str(tmp_path / "x.vti"), np.zeros((2, 2, 6)), (0, 0, 0), (1, 1, 1))
    with np.testing.assert_raises(solver.MphError):
        solver.write_vti(str(tmp_path / "no_such_dir" / "x.vti"), np.zeros((1, 1, 1, 6)), (0, 0, 0), (1, 1, 1))
