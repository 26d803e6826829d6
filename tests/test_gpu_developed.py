"""GPU parity in the DEVELOPED 3-D dam break.

The full-size tests of test_gpu_fullsize.py stop at 52 steps, where D1M's fluid has moved ~0.01 dx
and every neighbour set is still the initial lattice's.  The reference's own Dam run is 10,001
steps (main.cpp:581; results/Dam/dam.data EndTime 1.0 at Dt 1e-4).  Here the GPU runs D1M
(BASELINE configs[1], 1,397,200 particles) to t = 0.25 s (2,500 steps) and to t = 1.0 s (10,000
steps, the end of the reference's run): the column has collapsed
along the floor, particles are off the lattice and the neighbour sets have changed.  That exact
state (Position, Velocity, Time -- everything the step carries; walls are static in this case) is
handed to the CPU oracle, bit-identical to the reference, as the reference's own restart from a
.prof file would read it (main.cpp:788-955), and both advance 1 and 10 more steps:

  * NeighborCount exact; the neighbour SETS of sample ranges (mph_neighbor_rows of a context built
    from the state with the reference's whole lists) equal to the oracle's lists (main.cpp:1764-1772);
  * Position 1e-12 m, Velocity 1e-9 m/s, PressureP / VolStrainP / DivergenceP / Force within
    REL_STEPS of their largest magnitude plus their roundoff floors (tests/parity.py);
  * the state did leave the lattice: NeighborCount differs from the creation's for >= 1 % of the
    particles, and the fluid front moved by more than 10 dx.
"""
import os

import numpy as np
import pytest

from parity import REL_STEPS, assert_close, check_rank_files
from particlemethod_fsi_amd import MphSolver, cases, mphio

pytestmark = pytest.mark.gpu

DEVELOPED_STEPS = 2500           # t = 0.25 s at Dt = 1e-4
SAMPLE_ROWS = [(0, 4000), (485000, 4000), (966000, 4000), (1200000, 4000)]   # fluid (3) and wall


@pytest.mark.parametrize("steps", [DEVELOPED_STEPS, 10000])   # t = 0.25 s, and t = 1.0 s: the reference's whole Dam run
def test_d1m_developed_matches_oracle(steps):
    from oracle_bindings import OracleSolver, use_oracle_threads
    use_oracle_threads()
    cfg, parts = cases.get("d1m").build()
    fluid = parts.property < 2
    with MphSolver(cfg, parts) as s:
        nc0 = s.get("NeighborCount")
        s.step(steps)
        pos, vel = s.get("Position"), s.get("Velocity")
        nc_dev = s.get("NeighborCount")
        changed = float((nc_dev != nc0).mean())
        front0 = float(parts.position[fluid, 0].max())
        front = float(pos[fluid, 0].max())
        print("developed: t=%.4f changed=%.3f front %.4f -> %.4f m, max|v| %.3f m/s"
              % (s.time, changed, front0, front, float(np.abs(vel).max())))
        assert changed >= 0.01, changed
        assert front - front0 > 10 * cfg.particle_spacing, (front0, front)
        # restart of the reference from that state (a .prof holds Time, x, x0, v)
        rcfg = cfg.copy()
        rcfg.time = s.time
        state = mphio.Particles(parts.property, pos, parts.initial_position, vel)
        o = OracleSolver(rcfg, state)
        o.init()
        # the neighbour SETS of sample ranges at the restart (main.cpp:1764-1772): a context built
        # from that state with the reference's whole lists (MPH_LIST_FULL=1) against the oracle's
        os.environ["MPH_LIST_FULL"] = "1"
        try:
            with MphSolver(rcfg, state) as full:
                for first, count in SAMPLE_ROWS:
                    counts, offsets, ids = full.neighbor_rows(first, count)
                    for i in range(count):
                        assert np.array_equal(ids[offsets[i]:offsets[i + 1]], np.sort(o.neighbors(first + i))), first + i
        finally:
            del os.environ["MPH_LIST_FULL"]
        done = 0
        for k in (1, 10):
            s.step(k - done)
            o.step(k - done)
            done = k
            assert np.array_equal(s.get("NeighborCount"), o.get("NeighborCount")), k
            for f in ["Position", "Velocity", "PressureP", "VolStrainP", "DivergenceP", "Force"]:
                assert_close(f, s.get(f), o.get(f), REL_STEPS, context=(k,))
        assert s.time == o.time


SLAB_FIELDS = ["Position", "Velocity", "PressureP", "NeighborCount", "VolStrainP", "DivergenceP"]


def test_d1m_developed_slab8_matches_single_context(tmp_path):
    """The multi-GPU path in the developed flow: the D1M state at t = 0.25 s
    (2,500 steps on one context; off the lattice, NeighborCount changed for most particles) split
    into the 8 z slabs of bench.py --gpus 8 (8 ranks sharing the test GPU, host-staged transport;
    every rank created from the whole state, equal cuts) against one context started from the same
    state, 10 steps: ownership a partition of all particles, NeighborCount exact, positions 1e-12 m,
    velocities 1e-9 m/s, the sums REL_STEPS of the whole array's max + their floors
    (parity.check_rank_files) -- and particles did migrate between slabs (owner at the end differs
    from the owner at creation)."""
    import dist_worker
    world, steps = 8, 10
    cfg, parts = cases.get("d1m").build()
    with MphSolver(cfg, parts) as s:
        nc0 = s.get("NeighborCount")
        s.step(DEVELOPED_STEPS)
        pos, vel, t = s.get("Position"), s.get("Velocity"), s.time
        assert float((s.get("NeighborCount") != nc0).mean()) >= 0.01
    state = str(tmp_path / "state.npz")
    np.savez(state, position=pos, velocity=vel, time=np.array([t]))
    rcfg = cfg.copy()
    rcfg.time = t
    with MphSolver(rcfg, mphio.Particles(parts.property, pos, parts.initial_position, vel)) as s:
        s.step(steps)
        ref = {f: s.get(f) for f in SLAB_FIELDS}
        ref_time = s.time
    dist_worker.run_ranks(dist_worker.gpu_state_worker, world, "d1m", state, 2, steps, SLAB_FIELDS, str(tmp_path),
                          timeout=600)
    owner0, owner1 = check_rank_files(tmp_path, world, parts.n, ref, ref_time, SLAB_FIELDS)
    migrants = int((owner0 != owner1).sum())
    print("developed slab8: %d particles changed slab in %d steps" % (migrants, steps))
    assert (owner0 >= 0).all() and migrants > 0, migrants
