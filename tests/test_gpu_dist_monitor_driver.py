"""GPU, end to end: the drop-in executable's MPH_DIST_MONITOR option (csrc/mph_main.cpp).

mph_explicit runs dam2d for the 31 steps of test_gpu_monitor_driver.RUN as two slab ranks on the one GPU
(host transport) with MPH_DIST_MONITOR=<csv>, two tracked particles and one probe: rank 0 writes the
header and one row per step, and the numbers (printed as %.17g) are bit for bit the dist_monitor_read()
samples of two Python slab ranks with the same slabs and configuration.
"""
import os

import numpy as np
import pytest

import dist_worker
import monitor_ranks
from test_gpu_monitor_driver import PROBE, TRACK, _run, _write_case

pytestmark = pytest.mark.gpu

SLABS = {"MPH_SLABS": "2", "MPH_SLAB_TRANSPORT": "host", "MPH_SLAB_SHARE_DEVICE": "1"}


def test_driver_dist_monitor_csv(tmp_path):
    d = str(tmp_path / "run")
    os.makedirs(d)
    _write_case(d)
    r = _run(d, dict(SLABS, MPH_DIST_MONITOR="mon.csv", MPH_MONITOR_TRACK=",".join(map(str, TRACK)),
                     MPH_MONITOR_PROBES=",".join(repr(v) for v in PROBE)))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "monitor ring" not in r.stderr
    with open(os.path.join(d, "mon.csv")) as fh:
        lines = fh.read().splitlines()
    width = 32 + 6 * len(TRACK) + 2
    names = lines[0].split(",")
    assert len(names) == width and names[:3] == ["step", "time", "fluid_count"]
    assert names[32] == "p17_x" and names[-2:] == ["probe0_value", "probe0_count"]
    rows = np.array([[float(t) for t in ln.split(",")] for ln in lines[1:]])
    assert rows.shape == (31, width)
    # the same case through the files the driver read, the same slabs (two equal ones along x)
    out = str(tmp_path / "ranks.npz")
    spec = dict(case="dam2d", files=(os.path.join(d, "dam.data"), os.path.join(d, "dam.grid"), 2, "bar"),
                monitor=dict(stride=1, capacity=31, track=TRACK, probes=[PROBE]),
                schedule=[dict(steps=31, read="c")])
    dist_worker.run_ranks(monitor_ranks.monitor_worker, 2, spec, out, timeout=300)
    ref = np.load(out)
    assert (ref["lost0"] == 0).all() and ref["c0"].shape == rows.shape
    assert list(rows[:, 0]) == list(range(1, 32))
    assert rows.tobytes() == ref["c0"].tobytes()
    assert rows[-1, 32 + 12 + 1] >= 10   # the probe lies in the water column


def test_driver_dist_monitor_without_slabs_is_refused(tmp_path):
    d = str(tmp_path)
    _write_case(d)
    r = _run(d, {"MPH_DIST_MONITOR": "mon.csv"})
    assert r.returncode != 0
    assert "MPH_DIST_MONITOR" in r.stderr and "MPH_MONITOR" in r.stderr and "MPH_SLABS" in r.stderr
    assert not os.path.exists(os.path.join(d, "mon.csv"))
