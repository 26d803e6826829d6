"""GPU, end to end: the drop-in executable's MPH_DIST_SAMPLE option (csrc/mph_main.cpp).

mph_explicit runs dam2d for 16 steps as two slab ranks on the one GPU (host transport) with a VTK output
every 10 (after steps 1 and 11) and MPH_DIST_SAMPLE set: beside each .vtk rank 0 writes a .vti whose
arrays are bit for bit the collective dist_sample_grid() result of two Python slab ranks with the same
slabs after the same number of steps.  Without slabs the option is refused, and MPH_SAMPLE with slabs
stays refused.
"""
import os
import re

import numpy as np
import pytest

from particlemethod_fsi_amd.solver import SAMPLE_CHANNELS as C, read_vti

import dist_worker
import lattice_ranks
from test_gpu_dist_monitor_driver import SLABS
from test_gpu_sample_driver import COUNT, ORIGIN, RADIUS, SAMPLE, SPACING, _run, _write_case

pytestmark = pytest.mark.gpu


def test_driver_dist_sample_writes_a_vti_per_vtk(tmp_path):
    d = str(tmp_path / "run")
    os.makedirs(d)
    _write_case(d)
    r = _run(d, dict(SLABS, MPH_DIST_SAMPLE=SAMPLE, MPH_SAMPLE_FILE="lat%03d.vti", MPH_SAMPLE_RADIUS=repr(RADIUS),
                     MPH_SAMPLE_CLASSES="5"))
    assert r.returncode == 0, r.stderr[-2000:]
    vtk = sorted(f for f in os.listdir(d) if re.fullmatch(r"dam\d+\.vtk", f))
    assert len(vtk) == 2, os.listdir(d)
    assert sorted(f for f in os.listdir(d) if f.endswith(".vti")) == ["lat%s.vti" % f[3:-4] for f in vtk]
    steps = [int(f[3:-4]) + 1 for f in vtk]          # file k is written after step k + 1
    out = str(tmp_path / "ranks.npz")
    files = (os.path.join(d, "dam.data"), os.path.join(d, "dam.grid"), 2, "bar")
    lattice = dict(origin=ORIGIN, spacing=SPACING, count=COUNT, radius=RADIUS, classes=5)
    dist_worker.run_ranks(lattice_ranks.driver_worker, 2, files, steps, lattice, out, timeout=300)
    ref = np.load(out)
    for f, k in zip(vtk, steps):
        want = ref["c%d" % k]
        got = read_vti(os.path.join(d, "lat" + f[3:-4] + ".vti"))
        assert got["extent"] == [0, COUNT[0] - 1, 0, COUNT[1] - 1, 0, 0]
        assert got["origin"] == list(ORIGIN) and got["spacing"] == list(SPACING)
        assert got["Count"].tobytes() == np.ascontiguousarray(want[..., C["COUNT"]]).tobytes(), f
        assert got["WSum"].tobytes() == np.ascontiguousarray(want[..., C["WSUM"]]).tobytes(), f
        assert got["PressureP"].tobytes() == np.ascontiguousarray(want[..., C["P"]]).tobytes(), f
        assert got["Velocity"].tobytes() == np.ascontiguousarray(want[..., C["VX"]:]).tobytes(), f
        assert (want[..., C["COUNT"]] > 0).sum() > 1000
    assert steps[-1] > 1 and np.abs(want[..., C["P"]]).max() > 0.0


def test_driver_dist_sample_without_slabs_is_refused(tmp_path):
    d = str(tmp_path)
    _write_case(d)
    r = _run(d, {"MPH_DIST_SAMPLE": SAMPLE})
    assert r.returncode != 0
    assert "MPH_DIST_SAMPLE" in r.stderr and "MPH_SAMPLE" in r.stderr and "MPH_SLABS" in r.stderr
    assert not [f for f in os.listdir(d) if f.endswith(".vti")]


def test_driver_sample_with_slabs_is_still_refused(tmp_path):
    d = str(tmp_path)
    _write_case(d)
    r = _run(d, dict(SLABS, MPH_SAMPLE=SAMPLE))
    assert r.returncode != 0
    assert "MPH_SAMPLE" in r.stderr and "MPH_SLABS" in r.stderr and "MPH_DIST_SAMPLE" in r.stderr
    assert not [f for f in os.listdir(d) if f.endswith(".vti")]
