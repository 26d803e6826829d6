"""The ways a step reaches the device (csrc/mph_step.hip enqueue_steps): replayed
from the captured graphs, launched directly with the phase events (mph_phase_timing), launched directly
under the per-kernel profiler (mph_profile_steps).  All of them take a step's form from the one
function (mph_kernels.h seq_step), so nine steps give the same bits whichever way they run, with
lazy and lean steps among them -- the monitors, which the other direct-launch comparison
(test_batch_shapes_give_the_same_samples) turns on, make every step full.

The counters say which steps were lazy and lean: none of nine single steps; seven of a batch of eight
followed by one full step (mph_step(9), with or without phase timing); eight of the profiler's nine,
which stores the outputs on its last step only.  With surface tension (box3d_st) pass B reads
GravityCenter and PressureA on every step, so pass A is never lean.
"""
import pytest

from parity import assert_same, snapshot, step_counters
from particlemethod_fsi_amd import MphSolver, cases

pytestmark = pytest.mark.gpu

STEPS = 9


def single_steps(s):
    for _ in range(STEPS):
        s.step(1)


def one_call(s):
    s.step(STEPS)


def phase_timed(s):
    s.phase_timing(True)
    s.step(STEPS)


def profiled(s):
    s.profile(STEPS)


def run(cfg, parts, way):
    with MphSolver(cfg, parts) as s:
        way(s)
        c = step_counters(s)
        return snapshot(s), (c["lean_search"], c["lean_pass_a"], c["lazy"])


# case -> [(way, (lean search steps, lean pass A steps, lazy steps))]; the first way is the reference
WAYS = {
    "box3d_jit": [(single_steps, (0, 0, 0)), (one_call, (7, 7, 7)), (phase_timed, (7, 7, 7)), (profiled, (8, 8, 8))],
    "box3d_st": [(single_steps, (0, 0, 0)), (phase_timed, (7, 0, 7))],
}


@pytest.mark.parametrize("case", sorted(WAYS))
def test_step_paths_agree(case):
    cfg, parts = cases.get(case).build()
    ref = None
    for way, counters in WAYS[case]:
        snaps, got = run(cfg, parts, way)
        print(case, way.__name__, "lean search / lean pass A / lazy steps:", got)
        assert got == counters, (case, way.__name__, got, counters)
        if ref is None:
            ref = snaps
        else:
            assert_same(snaps, ref, (case, way.__name__))
