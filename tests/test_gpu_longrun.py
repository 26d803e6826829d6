"""GPU parity over long horizons in the elastic and coupled regimes.

test_gpu_parity.py and test_gpu_fullsize.py stop the Bar at 100 steps, where F = I + O(1e-4): the
St-Venant-Kirchhoff nonlinearity (E = (F^T F - I) / 2, main.cpp:2756-2811) and the large-rotation
path of DeformationVector / Stress / StressForce / updateElasticPosition (main.cpp:2673-2890,
1910-1943) are never compared there.

* bar2d (configs[2] at parity size, Dt = ElasticDt = 1e-4): the cantilever under gravity, GPU and
  oracle side by side to 3,000 steps (t = 0.3 s).  The tip then hangs ~88 mm (88 dx) below its
  start and F - I reaches 0.6 (rotation), so the test cannot pass at small strain: it asserts a
  deflection of > 50 dx and a Green-Lagrange strain whose quadratic part (F-I)^T (F-I) / 2 is
  > 0.05.  The reference itself is stable there and does not amplify roundoff (tools/ulp_study.py:
  one ulp on every start position is 2e-15 m of position and 2e-12 of F after 3,000 steps,
  tests/golden/ulp_bar2d_longrun.json), so the comparison is direct: measured on the GPU 2.3e-15 m
  and 2.3e-12 (profiles/r06/fsi3d_sub/pytest_bar2d_longrun.log).  (Past t ~ 0.305 s the reference's beam itself breaks up: the oracle's tip
  jumps by metres by step 3,300 -- nothing to compare there.)

* fsi3d_sub (configs[3] geometry, 2,259,700 particles, 4 elastic substeps): the GPU runs the dam
  break onto the gate to t = 0.35 s, after the fluid has hit it (t ~ 0.29 s; F - I reaches 0.27
  in the gate); the state (Position, Velocity, InitialPosition, Time -- a .prof restart,
  main.cpp:788-955) goes to the oracle, and both advance 1 and 10 steps: NeighborCount
  exact, the gate's DeformGradient and Stress, the fluid's pressure and the forces within the
  bounds of test_gpu_developed.py (parity.REL_STEPS); the gate has been hit (fluid front past its
  face, gate displaced).
"""
import os

import numpy as np
import pytest

from parity import REL_ONE_STEP, REL_STEPS, assert_close
from particlemethod_fsi_amd import MphSolver, cases, mphio

pytestmark = pytest.mark.gpu


def test_bar2d_large_deformation_matches_oracle():
    from oracle_bindings import OracleSolver, use_oracle_threads
    use_oracle_threads()
    cfg, parts = cases.get("bar2d").build()
    solid = (parts.property >= 2) & (parts.property < 4)
    tip = int(np.argmax(np.where(solid, parts.position[:, 0], -np.inf)))
    o = OracleSolver(cfg, parts)
    o.init()
    with MphSolver(cfg, parts) as s:
        assert np.array_equal(s.get("InitialStructureNeighborCount"), o.get("InitialStructureNeighborCount"))
        done = 0
        for k in (1000, 2000, 3000):
            s.step(k - done)
            o.step(k - done)
            done = k
            assert s.time == o.time, k
            assert np.array_equal(s.get("NeighborCount"), o.get("NeighborCount")), k
            assert np.array_equal(s.get("InitialStructureNeighborCount"),
                                  o.get("InitialStructureNeighborCount")), k
            rep = {}
            for f in ("Position", "Velocity", "DeformGradient", "Strain", "Stress", "PressureP", "Force"):
                rows = solid if f in ("DeformGradient", "Strain", "Stress") else None
                rep[f] = assert_close(f, s.get(f), o.get(f), REL_ONE_STEP, rows=rows, context=(k,))
            print("bar2d step %d: %s" % (k, " ".join("%s %.2e" % kv for kv in rep.items())))
        # the regime: large deflection and a strain whose nonlinear part is not small
        pos, F = o.get("Position"), o.get("DeformGradient")[solid][:, :2, :2]
        defl = parts.position[tip, 1] - pos[tip, 1]
        H = F - np.eye(2)
        quad = 0.5 * np.einsum("nki,nkj->nij", H, H)
        print("bar2d t=%.3f: tip deflection %.4f m, max|F-I| %.3f, max|(F-I)^T(F-I)/2| %.3f"
              % (o.time, defl, float(np.abs(H).max()), float(np.abs(quad).max())))
        assert defl > 50 * cfg.particle_spacing, defl
        assert float(np.abs(quad).max()) > 0.05


# t = 0.35 s at Dt = 1e-4: with the example's gravity (1 m/s^2, results/Dam/dam.data) the front
# reaches the gate at t ~ 0.29 s (tools/fsi_sub_probe.py, profiles/r06/fsi3d_sub/)
FSI_STEPS = int(os.environ.get("MPH_FSI_HANDOFF", "3500"))


def test_fsi3d_sub_developed_matches_oracle():
    from oracle_bindings import OracleSolver, use_oracle_threads
    use_oracle_threads()
    cfg, parts = cases.get("fsi3d_sub").build()
    solid = (parts.property >= 2) & (parts.property < 4)
    fluid = parts.property < 2
    gate_face = float(parts.position[solid, 0].min())
    with MphSolver(cfg, parts) as s:
        s.step(FSI_STEPS)
        pos, vel = s.get("Position"), s.get("Velocity")
        front = float(pos[fluid, 0].max())
        gate_disp = float(np.abs(pos[solid] - parts.position[solid]).max())
        F = s.get("DeformGradient")[solid]
        print("fsi3d_sub t=%.4f: fluid front %.4f m (gate face %.4f), gate displacement %.3e m, "
              "max|F-I| %.3e, max|v| %.3f" % (s.time, front, gate_face, gate_disp,
                                              float(np.abs(F - np.eye(3)).max()), float(np.abs(vel).max())))
        assert np.isfinite(pos).all() and np.isfinite(vel).all()
        assert front >= gate_face - 2 * cfg.particle_spacing, (front, gate_face)
        assert gate_disp > 1e-4, gate_disp   # before the impact the gate moves < 7e-5 m
        rcfg = cfg.copy()
        rcfg.time = s.time
        state = mphio.Particles(parts.property, pos, parts.initial_position, vel)
        o = OracleSolver(rcfg, state)
        o.init()
        done = 0
        for k in (1, 10):
            s.step(k - done)
            o.step(k - done)
            done = k
            assert np.array_equal(s.get("NeighborCount"), o.get("NeighborCount")), k
            rep = {}
            for f in ("Position", "Velocity", "PressureP", "VolStrainP", "DivergenceP", "Force",
                      "DeformGradient", "Stress"):
                rows = solid if f in ("DeformGradient", "Stress") else None
                rep[f] = assert_close(f, s.get(f), o.get(f), REL_STEPS, rows=rows, context=(k,))
            print("fsi3d_sub +%d: %s" % (k, " ".join("%s %.2e" % kv for kv in rep.items())))
        assert s.time == o.time
