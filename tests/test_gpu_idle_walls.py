"""Lazy wall steps: on the steps of a batch that store no output-only field
the search skips the waves of wall particles that no fluid or structure particle can reach, and
pass A sums nothing for them.  Nothing a caller can read may change: every comparison here is
bitwise.

The case (`tank`): a 3-D dam tank of 30 x 30 x 16 dx with three-layer walls on the floor, on both x
sides and on both z sides, and a fluid block of 10 x 12 x 10 dx in the corner x = z = 0 -- 12,000
particles, 10,800 of them walls.  Under the example's gravity (1 m/s^2) the block would need some
450 steps to move by one dx, so the outer half of the block (x > 5 dx) starts at 0.8 m/s along +x
(0.08 dx per step): it runs out over the floor and along the z = 0 wall while the inner half keeps
the corner's walls in reach.

The step count, 64, was chosen on the CPU with the oracle (tests/oracle_bindings.py): at t = 0,
9,804 walls have no non-wall particle within MaxRadius + MARGIN = 2.6 dx; after 64 steps 265 of
them have one, 9,648 walls still have none, and the front has advanced by 4.6 dx -- more than one
coarse cell of the map (3.5 dx), so whole waves of the floor ahead of the toe stop being idle.
"""
import numpy as np
import pytest

from parity import assert_same, run_calls, tank
from particlemethod_fsi_amd import cases

pytestmark = pytest.mark.gpu

STEPS = 64


def run(cfg, parts, calls, snap_at, monitors=False):
    """parity.run_calls as this file reads it: the snapshots, the idle-wall counters after every call
    as mph_idle_wall_stats gives them, the monitor samples."""
    snaps, counters, idle, samples = run_calls(cfg, parts, calls, snap_at, 256 if monitors else 0)
    return snaps, [{"idle_wave_steps": i, "lazy_steps": c["lazy"]} for i, c in zip(idle, counters)], samples


EVERY8 = set(range(8, STEPS + 1, 8))


@pytest.fixture(scope="module")
def tank_case():
    return tank()


@pytest.fixture(scope="module")
def tank_single(tank_case):
    """64 x mph_step(1): every step stores every field, no step is lazy.  Snapshots after every 8th
    step and after the 13th."""
    snaps, counters, _ = run(*tank_case, [1] * STEPS, EVERY8 | {13})
    assert counters[-1] == {"idle_wave_steps": 0, "lazy_steps": 0}
    return snaps


@pytest.fixture(scope="module")
def tank_lazy(tank_case):
    """8 x mph_step(8): seven lazy steps in every batch."""
    snaps, counters, _ = run(*tank_case, [8] * (STEPS // 8), EVERY8)
    return snaps, counters


def test_lazy_steps_bit_identical_to_full_steps(tank_single, tank_lazy):
    assert_same(tank_lazy[0], {k: v for k, v in tank_single.items() if k in EVERY8}, "step(8) vs step(1)")


def test_remainder_graph(tank_case, tank_single):
    """mph_step(13): an 8-step batch, four lazy single steps and a full one."""
    snaps, counters, _ = run(*tank_case, [13], {13})
    assert counters[0]["lazy_steps"] == 7 + 4
    assert_same(snaps, {13: tank_single[13]}, "step(13) vs 13 x step(1)")


def test_on_equals_off(tank_case, tank_lazy, monkeypatch):
    monkeypatch.setenv("MPH_LAZY_WALLS", "0")
    snaps, counters, _ = run(*tank_case, [8] * (STEPS // 8), EVERY8)
    monkeypatch.delenv("MPH_LAZY_WALLS")
    assert all(c == {"idle_wave_steps": 0, "lazy_steps": 0} for c in counters), counters
    assert_same(snaps, tank_lazy[0], "MPH_LAZY_WALLS=0 vs default")


def test_path_ran_and_followed_the_flow(tank_lazy):
    c = tank_lazy[1]
    print("idle wall counters after every step(8):", c)
    assert [k["lazy_steps"] for k in c] == [7 * (b + 1) for b in range(STEPS // 8)]
    first = c[0]["idle_wave_steps"]
    last = c[-1]["idle_wave_steps"] - c[-2]["idle_wave_steps"]
    assert first > 0
    assert last < first, (first, last)   # (both over 7 lazy steps)


@pytest.mark.parametrize("case", ["movwall3d", "gate3d", "box3d_st"])
def test_other_cases(case):
    """Moving walls with a restart time, structure particles, surface tension: two 8-step batches."""
    cfg, parts = cases.get(case).build()
    a, ca, _ = run(cfg, parts, [8, 8], {8, 16})
    b, cb, _ = run(cfg, parts, [1] * 16, {8, 16})
    assert ca[-1]["lazy_steps"] == 14 and cb[-1]["lazy_steps"] == 0
    assert_same(a, b, case)


def test_balanced_xcd_map(tank_case, monkeypatch):
    """The work-balanced XCD map of the passes on a small case: an idle wave adds only its fixed
    cost to the work histogram."""
    monkeypatch.setenv("MPH_XCD_BAL_MIN", "0")
    a, ca, _ = run(*tank_case, [8] * (STEPS // 8), EVERY8)
    b, _, _ = run(*tank_case, [1] * STEPS, EVERY8)
    monkeypatch.delenv("MPH_XCD_BAL_MIN")
    assert ca[0]["idle_wave_steps"] > 0
    assert_same(a, b, "MPH_XCD_BAL_MIN=0")


def test_monitors_keep_every_step_full(tank_case, monkeypatch):
    """The monitor kernels read the walls' pressure on every step: no step is lazy."""
    a, ca, sa = run(*tank_case, [8, 8], {16}, monitors=True)
    assert ca[-1] == {"idle_wave_steps": 0, "lazy_steps": 0}
    monkeypatch.setenv("MPH_LAZY_WALLS", "0")
    b, _, sb = run(*tank_case, [8, 8], {16}, monitors=True)
    monkeypatch.delenv("MPH_LAZY_WALLS")
    assert sa.shape[0] == 16 and np.array_equal(sa, sb, equal_nan=True)
    assert_same(a, b, "monitors")
