"""GPU, end to end: the drop-in executable's MPH_DIST_OUTPUT_SELECT and MPH_DIST_LOADS options
(csrc/mph_main.cpp).

mph_explicit runs dam2d for 16 steps as two slab ranks on the one GPU (host transport) with a VTK output
every 10 (after steps 1 and 11), MPH_DIST_OUTPUT_SELECT="types=0,1" and MPH_DIST_LOADS on the walls at
stride 5.  Each cropped .vtk is, byte for byte, the array writer over the collective
dist_gather_selected() of two Python slab ranks with the same slabs stepped the same way, and each CSV
row (printed as %.17g) parses back to their collective dist_selection_totals(), bit for bit.  The .prof
files and output.vtk keep the whole count.  Both options are refused without slabs.
"""
import os
import re

import numpy as np
import pytest

from particlemethod_fsi_amd import solver
from particlemethod_fsi_amd.solver import TOTAL_SLOTS, read_case_files

import dist_worker
import select_ranks
from test_gpu_dist_monitor_driver import SLABS
from test_gpu_sample_driver import _run, _write_case

pytestmark = pytest.mark.gpu

CENTER = (0.01, 0.02, 0.0)
LOADS = dict(MPH_LOADS_SELECT="types=4,5", MPH_LOADS_STRIDE="5", MPH_LOADS_CENTER=",".join(repr(v) for v in CENTER))


def test_driver_crops_the_frames_and_writes_the_loads_from_slab_ranks(tmp_path):
    d = str(tmp_path / "run")
    os.makedirs(d)
    _write_case(d)
    r = _run(d, dict(SLABS, MPH_DIST_OUTPUT_SELECT="types=0,1", MPH_DIST_LOADS="loads.csv", **LOADS))
    assert r.returncode == 0, r.stderr[-2000:]
    cfg, parts = read_case_files(os.path.join(d, "dam.data"), os.path.join(d, "dam.grid"), 2, "bar")
    nfluid = int((parts.property < 2).sum())
    assert 0 < nfluid < parts.n
    vtk = sorted(f for f in os.listdir(d) if re.fullmatch(r"dam\d+\.vtk", f))
    assert len(vtk) == 2, os.listdir(d)
    steps = [int(f[3:-4]) + 1 for f in vtk]          # file k is written after step k + 1
    lines = open(os.path.join(d, "loads.csv")).read().splitlines()
    names = lines[0].split(",")
    assert names[:2] == ["step", "time"]
    assert [n.upper() for n in names[2:]] == sorted(TOTAL_SLOTS, key=TOTAL_SLOTS.get)
    rows = np.array([[float(t) for t in ln.split(",")] for ln in lines[1:]])
    assert rows.shape == (3, 2 + 24) and list(rows[:, 0]) == [5.0, 10.0, 15.0]
    # two Python slab ranks, the same slabs, stepped to the same steps
    out = str(tmp_path / "ranks.npz")
    files = (os.path.join(d, "dam.data"), os.path.join(d, "dam.grid"), 2, "bar")
    dist_worker.run_ranks(select_ranks.driver_worker, 2, files, steps, [5, 10, 15], LOADS["MPH_LOADS_SELECT"], CENTER,
                          out, timeout=300)
    ref = np.load(out)
    L = solver.load_library()
    for f, k in zip(vtk, steps):
        got = open(os.path.join(d, f), "rb").read()
        assert ("POINTS %d float\n" % nfluid).encode() in got
        assert np.array_equal(ref["ids%d" % k], np.nonzero(parts.property < 2)[0])
        arrs = [np.ascontiguousarray(ref["g%d/%s" % (k, name)]) for name in select_ranks.FRAME]
        want = str(tmp_path / ("ref%d.vtk" % k))
        solver._check(L.mph_write_vtk_arrays(want.encode(), nfluid, *[a.ctypes.data for a in arrs]))
        assert got == open(want, "rb").read(), f
    for row in rows:
        want = ref["t%d" % int(row[0])]
        assert row[1:].tobytes() == want.tobytes(), (row, want)
    # not vacuous: every wall particle counted, and the walls carry the water's weight
    assert rows[-1, 2 + TOTAL_SLOTS["COUNT"]] == float((parts.property >= 4).sum())
    assert rows[-1, 2 + TOTAL_SLOTS["FY"]] != 0.0 and rows[-1, 2 + TOTAL_SLOTS["TZ"]] != 0.0
    # the first frame of the reference's loop and the restart files stay whole
    assert ("POINTS %d float\n" % parts.n).encode() in open(os.path.join(d, "output.vtk"), "rb").read()
    assert len(open(os.path.join(d, "dam000.prof")).read().splitlines()) >= parts.n + 2


def test_driver_slab_selection_options_without_slabs_are_refused(tmp_path):
    d = str(tmp_path)
    _write_case(d)
    for var, single in (("MPH_DIST_OUTPUT_SELECT", "MPH_OUTPUT_SELECT"), ("MPH_DIST_LOADS", "MPH_LOADS")):
        r = _run(d, {var: "types=0,1" if "SELECT" in var else "loads.csv"})
        assert r.returncode != 0
        assert var in r.stderr and single in r.stderr and "MPH_SLABS" in r.stderr
    assert not os.path.exists(os.path.join(d, "loads.csv"))
    assert not [f for f in os.listdir(d) if re.fullmatch(r"dam\d+\.vtk", f)]
