"""CPU: the particle-selection part of the C ABI (include/mph_gpu.h mph_select*, mph_selection_*)
against its Python mirror: the symbols, the layout of MphSelection, the spec parser and the predicate
mph_selection_accepts -- the function the device evaluates -- against a plain Python model.
"""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest

from particlemethod_fsi_amd import solver
from particlemethod_fsi_amd.solver import MphError, MphSelection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mph_gpu.h")
SYMBOLS = ("mph_selection_parse", "mph_selection_accepts", "mph_select", "mph_selected_ids", "mph_get_selected",
           "mph_selection_totals", "mph_write_vtk_selected", "mph_write_vtu_selected")


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
    assert re.search(r"MPH_FIELD_COUNT\s*=\s*26\b", txt)


def test_selection_mirror_layout():
    body = re.search(r"typedef struct MphSelection \{(.*?)\} MphSelection;", _header(), re.S).group(1)
    names = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*[;,]", body)
    assert names == [f[0] for f in MphSelection._fields_] == ["type_mask", "box", "every", "phase", "lo", "hi"]
    expect = {"type_mask": 0, "box": 4, "every": 8, "phase": 12, "lo": 16, "hi": 40}
    assert {n: getattr(MphSelection, n).offset for n in names} == expect
    assert ctypes.sizeof(MphSelection) == 64
    # and as the library was compiled
    out = (ctypes.c_int * 7)()
    assert solver.load_library().mph_selection_layout(out) == 0
    assert list(out) == [64, 0, 4, 8, 12, 16, 40]


def test_total_slots_match_the_header():
    txt = _header()
    body = re.search(r"typedef enum MphTotalSlot \{(.*?)\} MphTotalSlot;", txt, re.S).group(1)
    slots = {m.group(1): int(m.group(2)) for m in re.finditer(r"MPH_TOT_(\w+)\s*=\s*(\d+)", body)}
    assert slots == solver.TOTAL_SLOTS
    assert sorted(slots.values()) == list(range(24))
    assert int(re.search(r"#define\s+MPH_TOTALS\s+(\d+)", txt).group(1)) == solver.TOTALS == 24


def _fields(s):
    return (s.type_mask, s.box, s.every, s.phase, tuple(s.lo), tuple(s.hi))


def test_parse_round_trips_defaults_and_key_order():
    p = solver.parse_selection
    assert _fields(p("")) == (0, 0, 1, 0, (0.0,) * 3, (0.0,) * 3)
    full = "types=0,1;box=-0.5,0.25,1e-3,2,3.5,0.125;on=initial;every=4;phase=1"
    want = (3, 2, 4, 1, (-0.5, 0.25, 1e-3), (2.0, 3.5, 0.125))
    assert _fields(p(full)) == want
    for perm in itertools.permutations(full.split(";")):
        assert _fields(p(";".join(perm))) == want, perm
    assert _fields(p("box=0,0,0,1,1,1")) == (0, 1, 1, 0, (0.0,) * 3, (1.0,) * 3)      # on=position is the default
    assert _fields(p("on=position;box=0,0,0,1,1,1"))[1] == 1
    assert _fields(p("types=5")) == (32, 0, 1, 0, (0.0,) * 3, (0.0,) * 3)
    assert _fields(p("types=2,3,2"))[0] == 12
    assert _fields(p("every=3;phase=2"))[2:4] == (3, 2)
    assert _fields(p("every=7"))[2:4] == (7, 0)
    # doubles round-trip through %.17g
    lo = (0.1, 1.0 / 3.0, -2.0 / 7.0)
    s = p("box=%.17g,%.17g,%.17g,1,1,1" % lo)
    assert tuple(s.lo) == lo
    # make_selection builds the same struct
    m = solver.make_selection(types=(0, 1), box=((-0.5, 0.25, 1e-3), (2, 3.5, 0.125)), on="initial", every=4, phase=1)
    assert _fields(m) == want


@pytest.mark.parametrize("spec", [
    "colour=1", "types", "types=", "types=6", "types=-1", "types=1.5", "types=0,,1", "types=a",
    "box=0,0,0,1,1", "box=0,0,0,1,1,1,1", "box=", "box=0,0,0,1,1,x",
    "on=initial", "on=position", "on=elsewhere;box=0,0,0,1,1,1",
    "every=0", "every=-2", "every=2.5", "every=1,2", "phase=-1", "phase=1", "every=3;phase=3",
    "types=0;types=1", "every=2;every=2", "types=0 1", "every=4 ",
])
def test_parse_refuses(spec):
    with pytest.raises(MphError) as e:
        solver.parse_selection(spec)
    assert e.value.code == -1, spec


def _model(s, dim, index, ptype, pos, pos0):
    """The selection rule in plain Python (include/mph_gpu.h)."""
    if s.type_mask and not (0 <= ptype < 6 and (s.type_mask >> ptype) & 1):
        return 0
    if index % s.every != s.phase:
        return 0
    if s.box:
        x = pos if s.box == 1 else pos0
        for d in range(dim):
            if not (s.lo[d] <= x[d] < s.hi[d]):   # (false for a NaN)
                return 0
    return 1


def test_accepts_against_the_model():
    acc = solver.selection_accepts
    mk = solver.make_selection
    n = 0
    # each mask bit, alone and in pairs, against each type
    for mask_types in [None] + [(t,) for t in range(6)] + [(0, 1), (2, 3), (4, 5), (0, 5)]:
        s = mk(types=mask_types)
        for t in range(6):
            assert acc(s, 3, 7, t) == _model(s, 3, 7, t, None, None), (mask_types, t)
            n += 1
    # box edges: lo is in, hi is out, just inside / outside, both boxes, 2-D ignores z, NaN never in
    lo, hi = (0.25, -1.0, 0.5), (0.75, 1.0, 0.5 + 2.0 ** -20)
    xs = [0.25, math.nextafter(0.25, 0.0), math.nextafter(0.25, 1.0), 0.5, math.nextafter(0.75, 0.0), 0.75, math.nan]
    ys = [-1.0, 0.0, 1.0, math.nan]
    zs = [0.5, math.nextafter(0.5, 0.0), 0.5 + 2.0 ** -21, 0.5 + 2.0 ** -20, math.nan, 99.0]
    far = (99.0, 99.0, 99.0)
    for on in ("position", "initial"):
        s = mk(box=(lo, hi), on=on)
        for dim in (2, 3):
            for p in itertools.product(xs, ys, zs):
                pos, pos0 = (p, far) if on == "position" else (far, p)
                assert acc(s, dim, 0, 1, pos, pos0) == _model(s, dim, 0, 1, pos, pos0), (on, dim, p)
                n += 1
    assert acc(mk(box=(lo, hi)), 2, 0, 1, (0.25, 0.0, math.nan), far) == 1
    assert acc(mk(box=(lo, hi)), 3, 0, 1, (0.25, 0.0, math.nan), far) == 0
    assert acc(mk(box=(lo, hi)), 3, 0, 1, (0.25, -1.0, 0.5), far) == 1
    assert acc(mk(box=(lo, hi)), 3, 0, 1, (0.75, -1.0, 0.5), far) == 0
    # an empty box (lo == hi) is legal and holds nothing
    assert acc(mk(box=((0.5,) * 3, (0.5,) * 3)), 3, 0, 1, (0.5,) * 3, far) == 0
    # every / phase, every > index included
    for every in (1, 2, 3, 7, 1000):
        for phase in sorted({0, 1 % every, every - 1}):
            s = mk(every=every, phase=phase)
            for i in (0, 1, 2, 3, 6, 7, 999, 1000, 1999, 2 ** 31 - 1):
                assert acc(s, 3, i, 0) == _model(s, 3, i, 0, None, None), (every, phase, i)
                n += 1
    # everything at once
    s = mk(types=(1, 4), box=(lo, hi), on="initial", every=3, phase=2)
    for i, t, x in itertools.product((2, 3, 5), (0, 1, 4), (0.25, 0.75)):
        assert acc(s, 3, i, t, far, (x, 0.0, 0.5)) == _model(s, 3, i, t, far, (x, 0.0, 0.5))
        n += 1
    assert n > 700


def test_accepts_argument_errors():
    L = solver.load_library()
    pos = (ctypes.c_double * 3)(0.5, 0.5, 0.5)

    def call(s, dim=3, index=0, ptype=0):
        return L.mph_selection_accepts(ctypes.byref(s), dim, index, ptype, pos, pos)

    def sel(**kw):
        s = MphSelection()
        s.every = 1
        for d in range(3):
            s.hi[d] = 1.0
        for k, v in kw.items():
            if k in ("lo", "hi"):
                for d in range(3):
                    getattr(s, k)[d] = v[d]
            else:
                setattr(s, k, v)
        return s

    assert call(sel()) == 1
    assert call(sel(box=1)) == 1
    for bad in (dict(every=0), dict(every=-1), dict(every=2, phase=2), dict(phase=-1), dict(box=3), dict(box=-1),
                dict(type_mask=0x40), dict(type_mask=-1), dict(box=1, lo=(2.0, 0.0, 0.0)),
                dict(box=2, lo=(0.0, 2.0, 0.0)), dict(box=1, lo=(0.0, 0.0, 2.0)),
                dict(box=1, lo=(math.nan, 0.0, 0.0))):
        assert call(sel(**bad)) == -1, bad
    # an inactive axis is not checked: z of a 2-D box, any bound without a box
    assert call(sel(box=1, lo=(0.0, 0.0, 2.0)), dim=2) == 1
    assert call(sel(box=0, lo=(2.0, 2.0, 2.0))) == 1
    assert call(sel(), dim=1) == -1 and call(sel(), dim=4) == -1
    assert call(sel(), index=-1) == -1
    assert L.mph_selection_accepts(None, 3, 0, 0, pos, pos) == -1
    # a box needs the coordinates it tests
    assert L.mph_selection_accepts(ctypes.byref(sel(box=1)), 3, 0, 0, None, pos) == -1
    assert L.mph_selection_accepts(ctypes.byref(sel(box=2)), 3, 0, 0, pos, None) == -1
    assert L.mph_selection_accepts(ctypes.byref(sel(box=2)), 3, 0, 0, None, pos) == 1
