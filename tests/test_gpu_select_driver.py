"""GPU, end to end: the drop-in executable's MPH_OUTPUT_SELECT and MPH_LOADS options (csrc/mph_main.cpp).

mph_explicit runs dam2d for 20 steps.  With MPH_OUTPUT_SELECT="types=0,1" every VTK-step file holds
the fluid alone and is, byte for byte, what the array writer gives for that subset of the state of an
MphSolver stepped the same way.  With MPH_LOADS the CSV gets one row per MPH_LOADS_STRIDE steps whose
numbers (printed as %.17g) parse back to selection_totals of such a twin, bit for bit.  Both are
refused with MPH_SLABS=2 before a rank starts.
"""
import os
import subprocess

import numpy as np
import pytest

from particlemethod_fsi_amd import MphSolver, cases, solver
from particlemethod_fsi_amd.solver import TOTAL_SLOTS, read_case_files

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "particlemethod_fsi_amd", "lib", "mph_explicit")
# 20 steps of Dt = 1e-4 (the loop runs while Time < EndTime + 1e-5 Dt); a VTK frame after steps 1 and 11
RUN = {"EndTime": [0.0019], "OutputInterval": [0.001], "VtkOutputInterval": [0.001]}
VTK_NAMES = ("Property", "Position", "InitialPosition", "Velocity", "Acceleration", "Force", "Stress", "Strain",
             "InitialStructureNeighborCount", "NeighborCount")


def _write_case(d):
    c = cases.get("dam2d")
    values = c.data()
    values.update(RUN)
    with open(os.path.join(d, "dam.data"), "w") as fh:
        fh.write(cases.data_text(values))
    with open(os.path.join(d, "dam.grid"), "w") as fh:
        fh.write(c.grid_text())


def _run(d, extra):
    env = dict(os.environ, MPH_DIM="2", MPH_MODULE="bar")
    env.update(extra)
    cmd = [DRIVER, "dam.data", "dam.grid", "dam%03d.prof", "dam%03d.vtk", "dam.log", "4"]
    return subprocess.run(cmd, cwd=d, env=env, capture_output=True, text=True, timeout=300)


def _twin(d):
    cfg, parts = read_case_files(os.path.join(d, "dam.data"), os.path.join(d, "dam.grid"), 2, "bar")
    assert abs(cfg.dt - 1.0e-4) < 1e-12
    return cfg, parts


def test_driver_output_select(tmp_path):
    d = str(tmp_path)
    _write_case(d)
    r = _run(d, {"MPH_OUTPUT_SELECT": "types=0,1"})
    assert r.returncode == 0, r.stderr[-2000:]
    cfg, parts = _twin(d)
    fluid = np.nonzero(parts.property < 2)[0]
    assert 0 < len(fluid) < parts.n
    with MphSolver(cfg, parts) as s:
        done = 0
        for istep in (0, 10):      # the frame of index istep is written after step istep + 1
            s.step(istep + 1 - done)
            done = istep + 1
            s.compute_virial()
            got = open(os.path.join(d, "dam%03d.vtk" % istep), "rb").read()
            assert ("POINTS %d float\n" % len(fluid)).encode() in got
            arrs = [np.ascontiguousarray(s.get(k)[fluid]) for k in VTK_NAMES]
            ref = os.path.join(d, "ref%03d.vtk" % istep)
            solver._check(s._L.mph_write_vtk_arrays(ref.encode(), len(fluid), *[a.ctypes.data for a in arrs]))
            assert got == open(ref, "rb").read(), istep
    # the first frame of the reference's loop and the restart files stay whole
    assert ("POINTS %d float\n" % parts.n).encode() in open(os.path.join(d, "output.vtk"), "rb").read()
    prof = open(os.path.join(d, "dam000.prof")).read().splitlines()
    assert len(prof) >= parts.n + 2
    # a bad spec is refused with the variable's name
    r = _run(d, {"MPH_OUTPUT_SELECT": "types=0,1;colour=3"})
    assert r.returncode != 0 and "MPH_OUTPUT_SELECT" in r.stderr


def test_driver_loads_rows(tmp_path):
    d = str(tmp_path)
    _write_case(d)
    center = (0.01, 0.02, 0.0)
    r = _run(d, {"MPH_LOADS": "loads.csv", "MPH_LOADS_SELECT": "types=4,5", "MPH_LOADS_STRIDE": "5",
                 "MPH_LOADS_CENTER": ",".join(repr(v) for v in center)})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(os.path.join(d, "loads.csv")).read().splitlines()
    names = lines[0].split(",")
    assert names[:2] == ["step", "time"]
    assert [n.upper() for n in names[2:]] == sorted(TOTAL_SLOTS, key=TOTAL_SLOTS.get)
    rows = np.array([[float(t) for t in ln.split(",")] for ln in lines[1:]])
    assert rows.shape == (4, 2 + 24)
    assert list(rows[:, 0]) == [5.0, 10.0, 15.0, 20.0]
    cfg, parts = _twin(d)
    with MphSolver(cfg, parts) as s:
        for k in range(4):
            s.step(5)
            assert s.select(spec="types=4,5") == int((parts.property >= 4).sum())
            t = s.selection_totals(center)
            ref = np.array([5.0 * (k + 1), s.time] + [t[n] for n in sorted(TOTAL_SLOTS, key=TOTAL_SLOTS.get)])
            assert rows[k].tobytes() == ref.tobytes(), (k, rows[k], ref)
        # not vacuous: the walls carry the water's weight
        assert rows[-1, 2 + TOTAL_SLOTS["COUNT"]] > 0 and rows[-1, 2 + TOTAL_SLOTS["FY"]] != 0.0
    # both options together, the frames cropped and the rows unchanged
    r = _run(d, {"MPH_LOADS": "both.csv", "MPH_LOADS_SELECT": "types=4,5", "MPH_LOADS_STRIDE": "5",
                 "MPH_LOADS_CENTER": ",".join(repr(v) for v in center), "MPH_OUTPUT_SELECT": "types=0,1"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(os.path.join(d, "both.csv")).read().splitlines() == lines


def test_driver_refuses_selections_on_slabs(tmp_path):
    d = str(tmp_path)
    _write_case(d)
    r = _run(d, {"MPH_SLABS": "2", "MPH_OUTPUT_SELECT": "types=0,1", "MPH_LOADS": "loads.csv"})
    assert r.returncode != 0
    assert "MPH_OUTPUT_SELECT" in r.stderr and "MPH_LOADS" in r.stderr
    assert not os.path.exists(os.path.join(d, "loads.csv"))
    for var in ("MPH_OUTPUT_SELECT", "MPH_LOADS"):
        r = _run(d, {"MPH_SLABS": "2", var: "types=0,1"})
        assert r.returncode != 0 and var in r.stderr
