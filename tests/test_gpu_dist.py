"""GPU: the slab-decomposed multi-rank path against the CPU oracle and the single-GPU path.

2-4 ranks share the one GPU of the test box (one process each, host-staged transport over gloo,
csrc/mph_dist.hip); the RCCL transport differs only in who moves the message bytes.  The
channel cases stream at 0.5 m/s along the slab axis, so every face-adjacent layer migrates and
the periodic seam is crossed within the checked steps.

Tolerances (tests/parity.py): NeighborCount exact (bit-identical acceptance on owned particles);
positions 1e-12 m, velocities 1e-9 m/s; other fields relative REL_STEPS of the field's max plus its
roundoff floor (the slab's local cell grid orders neighbour sums differently from the oracle).
"""
import numpy as np
import pytest

from particlemethod_fsi_amd import MphSolver, cases

import dist_worker
from parity import REL_STEPS, assert_close, elastic_rel

pytestmark = pytest.mark.gpu

FIELDS = ["Position", "Velocity", "PressureP", "NeighborCount", "Force", "VolStrainP", "DivergenceP",
          "DensityA", "GravityCenter", "PressureA", "Acceleration"]
# elastic-solid cases: the per-slot tensors of the owned structure particles as well
STRUCT_FIELDS = FIELDS + ["DeformGradient", "Strain", "Stress"]


def run_slab(case, world, checkpoints, out, fields=FIELDS, local=False, cuts_mode=None):
    dist_worker.run_ranks(dist_worker.gpu_worker, world, case, checkpoints, fields, out, local, cuts_mode,
                          timeout=300)
    return np.load(out)


@pytest.mark.parametrize("case,world,local,cuts", [("channel3d", 2, False, None), ("channel3d", 3, False, None),
                                                   ("channel2d", 4, False, None), ("channel3d_st", 2, False, None),
                                                   ("dam2d", 2, False, None), ("channel3d", 3, True, None),
                                                   ("channel2d", 4, True, None), ("channel3d", 3, True, "skew"),
                                                   ("channel2d", 4, False, "skew"), ("dam2d", 3, True, "balanced")])
def test_slab_ranks_match_oracle(tmp_path, case, world, local, cuts):
    """local: every rank is created from its own window of the case (slab-local creation);
    cuts: unequal slabs (MphSlabOptions.cuts)."""
    from oracle_bindings import OracleSolver
    checkpoints = [1, 5, 20]
    r = run_slab(case, world, checkpoints, str(tmp_path / "slab.npz"), local=local, cuts_mode=cuts)
    cfg, parts = cases.get(case).build()
    assert (r["owner0"] >= 0).all()
    o = OracleSolver(cfg, parts)
    o.init()
    done = 0
    moved = False
    for k in checkpoints:
        o.step(k - done)
        done = k
        owner = r["s%d/owner" % k]
        assert (owner >= 0).all()
        if not np.array_equal(owner, r["owner0"]):
            moved = True
        for f in FIELDS:
            assert_close(f, r["s%d/%s" % (k, f)], o.get(f), REL_STEPS, context=(case, world, k))
    if case.startswith("channel"):
        assert moved, "no particle migrated between slabs"


@pytest.mark.parametrize("case,world,local,cuts", [("bar2d", 2, False, None), ("bar2d", 3, False, None),
                                                   ("bar3d", 2, False, None), ("gate2d_sub", 2, False, None),
                                                   ("bar2d", 3, True, None), ("gate2d_sub", 2, True, None),
                                                   ("bar2d", 3, True, "skew")])
def test_slab_structure_ranks_match_oracle(tmp_path, case, world, local, cuts):
    """Elastic-solid particles across slab faces: static owners by InitialPosition, ghost slots of
    the fixed Lagrangian lists exchanged before every stress / velocity half-substep.  local: the
    structure lists are built from each rank's window only; cuts: unequal slabs."""
    from oracle_bindings import OracleSolver
    checkpoints = [1, 10, 30]
    r = run_slab(case, world, checkpoints, str(tmp_path / "slab.npz"), STRUCT_FIELDS, local=local,
                 cuts_mode=cuts)
    cfg, parts = cases.get(case).build()
    o = OracleSolver(cfg, parts)
    o.init()
    done = 0
    for k in checkpoints:
        o.step(k - done)
        done = k
        assert (r["s%d/owner" % k] >= 0).all()
        for f in STRUCT_FIELDS:   # the tensors over all rows; parity.elastic_rel: REL_ELASTIC, DivergenceP wider
            assert_close(f, r["s%d/%s" % (k, f)], o.get(f), elastic_rel(f), context=(case, world, k))
    # the structure straddles a slab face (elastic ghosts in use) except in the gate case
    prop = parts.property
    sown = r["owner0"][(prop == 2) | (prop == 3)]
    assert case.startswith("gate") or len(set(sown.tolist())) > 1


def test_slab_matches_single_gpu(tmp_path):
    """Same case, 2 slabs vs one context: identical neighbour counts, values within roundoff."""
    r = run_slab("channel3d", 2, [10], str(tmp_path / "slab.npz"))
    cfg, parts = cases.get("channel3d").build()
    with MphSolver(cfg, parts) as s:
        s.step(10)
        for f in FIELDS:
            assert_close(f, r["s10/%s" % f], s.get(f), REL_STEPS)


def test_rccl_exchange_selftest():
    """The RCCL transport on a one-rank communicator (left = right = self): message routing and
    the per-peer ordering that two ranks rely on."""
    from particlemethod_fsi_amd.solver import load_library
    L = load_library()
    rc = L.mph_dist_selftest(0)
    assert rc == 0, (rc, (L.mph_last_error(None) or b"").decode())


@pytest.mark.parametrize("case,world", [("channel3d", 3), ("channel2d", 4), ("bar2d", 3), ("gate2d_sub", 2)])
def test_slab_early_send_bitwise(tmp_path, case, world, monkeypatch):
    """The early send of the redistribution messages (MPH_SLAB_EARLY, default on with the overlap: inside a batch,
    the next step's messages leave from pass B's face wavefronts while the interior ones run;
    with elastic particles, after the substeps) sends exactly the bytes the late pack would, so
    every field is bit-identical to MPH_SLAB_EARLY=0 -- over batches of 1, 4 and 15 steps.  The early
    send rides on the split pass B, so the overlap is forced on (MPH_SLAB_OVERLAP=1; unset, the
    ranks choose the mode at creation, test_slab_overlap_probe)."""
    fields = STRUCT_FIELDS if case.startswith(("bar", "gate")) else FIELDS
    monkeypatch.setenv("MPH_SLAB_OVERLAP", "1")
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MPH_SLAB_EARLY", mode)
        out[mode] = run_slab(case, world, [1, 5, 20], str(tmp_path / ("slab%s.npz" % mode)), fields,
                             local=True)
    for k in out["1"].files:
        if k != "overlap":   # (the pass-B mode report differs by construction)
            assert np.array_equal(out["1"][k], out["0"][k]), k


@pytest.mark.parametrize("case,world", [("bar2d", 3), ("bar3d", 2)])
def test_slab_structure_overlap_bitwise(tmp_path, case, world, monkeypatch):
    """The elastic ghost exchanges beside the inner slots (the u / P messages on the second stream
    while the slots whose lists hold no ghost run their half-substep) and the split pass B give
    the bits of the serial order (MPH_SLAB_OVERLAP=0: halo, one pass B, exchange, every slot)."""
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MPH_SLAB_OVERLAP", mode)
        out[mode] = run_slab(case, world, [1, 7], str(tmp_path / ("slab%s.npz" % mode)), STRUCT_FIELDS)
    for k in out["1"].files:
        if k != "overlap":   # (the pass-B mode report differs by construction)
            assert np.array_equal(out["1"][k], out["0"][k]), k


def test_slab_overlap_probe(tmp_path, monkeypatch):
    """MPH_SLAB_OVERLAP unset: the ranks choose the pass-B mode together at creation from their
    measured halo / redistribution exchange times against the cost of splitting pass B (max over
    ranks, mph_dist_overlap).  With 25 ms injected into every host exchange (a slow link) the
    exchanges dominate and the overlap is chosen; the rule holds in every run; and the chosen mode
    gives the bits of either forced mode: the probe writes no live buffer (its halo, messages and
    trial pass B go to the redistribution scratch set, overlap_probe in mph_dist.hip)."""
    monkeypatch.delenv("MPH_SLAB_OVERLAP", raising=False)
    monkeypatch.setenv("MPH_HOST_EXCHANGE_DELAY_MS", "25")
    slow = run_slab("channel3d", 2, [1, 9], str(tmp_path / "slow.npz"))
    on, th, tr, ts = slow["overlap"]
    assert th >= 25.0 and tr >= 25.0, (th, tr, ts)
    assert on == 1.0, slow["overlap"]
    monkeypatch.delenv("MPH_HOST_EXCHANGE_DELAY_MS")
    fast = run_slab("channel3d", 2, [1, 9], str(tmp_path / "fast.npz"))
    on, th, tr, ts = fast["overlap"]
    assert th >= 0.0 and tr >= 0.0 and on == float(th + tr > ts), fast["overlap"]
    for mode in ("0", "1"):
        monkeypatch.setenv("MPH_SLAB_OVERLAP", mode)
        forced = run_slab("channel3d", 2, [1, 9], str(tmp_path / ("forced%s.npz" % mode)))
        assert forced["overlap"][0] == float(mode) and forced["overlap"][1] == -1.0   # not probed
        for k in forced.files:
            if k != "overlap":
                assert np.array_equal(forced[k], slow[k]) and np.array_equal(forced[k], fast[k]), (mode, k)


def test_slab_profile_graphs_leave_state_unchanged(tmp_path, monkeypatch):
    """mph_profile_graphs on slab ranks (tools/slab_serial.py times the list kernels that way):
    each rank replays its search, pass A and pass B on its own state, no exchange; the run then
    continues bit for bit as without it (pass B in one launch: MPH_SLAB_OVERLAP=0)."""
    monkeypatch.setenv("MPH_SLAB_OVERLAP", "0")
    plain = run_slab("channel3d", 2, [1, 9], str(tmp_path / "plain.npz"))
    monkeypatch.setenv("MPH_TEST_PROFILE_GRAPHS", "1")
    prof = run_slab("channel3d", 2, [1, 9], str(tmp_path / "prof.npz"))
    assert (prof["graph_ms"] > 0).all(), prof["graph_ms"]
    for k in plain.files:
        if k != "overlap":
            assert np.array_equal(plain[k], prof[k]), k


def _run_capacity(tmp_path, tag, case, world, batches):
    d = tmp_path / tag
    d.mkdir()
    dist_worker.run_ranks(dist_worker.gpu_capacity_worker, world, case, batches, str(d), timeout=300)
    return [dict(np.load(str(d / ("rank%d.npz" % r)))) for r in range(world)]


def test_slab_message_capacity_growth(tmp_path, monkeypatch):
    """Message capacities grow at the capacity checks (every 32 steps, also inside one mph_step
    call): with the first sizing at 1.05 x the first counts and no slack (MPH_SLAB_MSG_CAP0_FRAC)
    the first check finds a direction past 90 % and re-allocates the buffers (and would re-capture
    the RCCL graphs); the results are bit-identical to the default sizing's, which never grows."""
    batches = [4, 40, 9]
    monkeypatch.setenv("MPH_SLAB_MSG_CAP0_FRAC", "1.05")
    tight = _run_capacity(tmp_path, "tight", "channel3d", 3, batches)
    monkeypatch.delenv("MPH_SLAB_MSG_CAP0_FRAC")
    loose = _run_capacity(tmp_path, "loose", "channel3d", 3, batches)
    for r in range(3):
        assert int(tight[r]["code"][0]) == 0 and int(loose[r]["code"][0]) == 0
        assert tight[r]["caps"][0].max() < loose[r]["caps"][0].min()   # first sizing: far smaller
        assert (tight[r]["caps"][1] > tight[r]["caps"][0]).all()        # grown at the first check
        for f in ("ids", "Position", "Velocity", "PressureP", "NeighborCount"):
            assert np.array_equal(tight[r][f], loose[r][f]), (r, f)



def test_slab_message_overflow_reported(tmp_path, monkeypatch):
    """A redistribution message larger than its capacity (MPH_SLAB_MSG_CAP forces 64 particles)
    ends in MPH_ERR_CAPACITY on the ranks -- the late and the early pack both clamp their writes to
    the buffer, so there is no fault and the process stays usable."""
    monkeypatch.setenv("MPH_SLAB_MSG_CAP", "64")
    res = _run_capacity(tmp_path, "over", "channel3d", 2, [4])   # the create's own exchange overflows
    assert all(int(r["code"][0]) == -11 for r in res), [int(r["code"][0]) for r in res]
