"""Lean steps: a lazy step -- a step of a batch that stores no output-only
field -- also leaves out the work inside its kernels whose result it drops.  Its search accepts
only the pairs it stores (r <= MaxRadius), trims its columns to that radius and counts no
NeighborCount; its pass A leaves out the DensityA and GravityCenter sums.  Nothing a caller can read
may change: every comparison here is bitwise.

The main case is box3d_jit (9,798 particles, 7,350 of them walls): it is off the lattice, so the
shell MaxRadius < r <= MaxRadius + MARGIN (2.5 to 2.6 dx) holds pairs -- 9.6 % of the pairs within
2.6 dx, counted with a k-d tree on the case's positions (51.8 against 57.3 neighbours per
particle); box3d, channel3d and seam3d have none.  test_shell_is_populated asserts it on the device.
"""
import pytest

from parity import assert_same, run_calls
from particlemethod_fsi_amd import MphSolver, cases

pytestmark = pytest.mark.gpu

ZERO = {"search_steps": 0, "pass_a_steps": 0}


def run(cfg, parts, calls, snap_at, monitors=False):
    """parity.run_calls as this file reads it: the snapshots, and the lean counters (as
    mph_lean_step_stats gives them) and the lazy steps after every call."""
    snaps, counters, _, _ = run_calls(cfg, parts, calls, snap_at, 64 if monitors else 0)
    lean = [{"search_steps": c["lean_search"], "pass_a_steps": c["lean_pass_a"]} for c in counters]
    return snaps, lean, [c["lazy"] for c in counters]


@pytest.fixture(scope="module")
def box():
    return cases.get("box3d_jit").build()


@pytest.fixture(scope="module")
def box_single(box):
    """16 x mph_step(1): every step is full.  Snapshots after steps 8, 13 and 16."""
    snaps, lean, lazy = run(*box, [1] * 16, {8, 13, 16})
    assert all(c == ZERO for c in lean), lean
    assert lazy[-1] == 0
    return snaps


@pytest.fixture(scope="module")
def box_lean(box):
    """2 x mph_step(8): seven lean steps in each batch."""
    return run(*box, [8, 8], {8, 16})


def test_shell_is_populated(box):
    """After a full step the stored lists (r <= MaxRadius) are shorter than NeighborCount's (r <=
    MaxRadius + MARGIN): the lean search has candidates to leave out."""
    with MphSolver(*box) as s:
        s.step(1)
        stored, counted = s.list_stats()[0], s.neighbor_stats()[0]
    print("mean stored list %.2f, mean NeighborCount %.2f" % (stored, counted))
    assert stored < counted, (stored, counted)


def test_lean_steps_bit_identical_to_full_steps(box_single, box_lean):
    assert_same(box_lean[0], {k: box_single[k] for k in (8, 16)}, "step(8) vs step(1)")


def test_lean_counters(box_lean):
    _, lean, lazy = box_lean
    assert lean == [{"search_steps": 7, "pass_a_steps": 7}, {"search_steps": 14, "pass_a_steps": 14}], lean
    assert lazy == [7, 14]


def test_on_equals_off(box, box_lean, monkeypatch):
    monkeypatch.setenv("MPH_LEAN_STEPS", "0")
    snaps, lean, lazy = run(*box, [8, 8], {8, 16})
    monkeypatch.delenv("MPH_LEAN_STEPS")
    assert all(c == ZERO for c in lean), lean
    assert lazy == [7, 14]   # (the steps stay lazy)
    assert_same(snaps, box_lean[0], "MPH_LEAN_STEPS=0 vs default")


def test_remainder_graph(box, box_single):
    """mph_step(13): an 8-step batch, four lean single steps and a full one."""
    snaps, lean, _ = run(*box, [13], {13})
    assert lean[0] == {"search_steps": 7 + 4, "pass_a_steps": 7 + 4}
    assert_same(snaps, {13: box_single[13]}, "step(13) vs 13 x step(1)")


def test_monitors_keep_every_step_full(box, box_single):
    """The monitor kernels read every particle's pressure on every step: no step is lazy, none lean."""
    snaps, lean, lazy = run(*box, [8, 8], {8, 16}, monitors=True)
    assert all(c == ZERO for c in lean) and lazy == [0, 0], (lean, lazy)
    assert_same(snaps, {k: box_single[k] for k in (8, 16)}, "monitors")


def test_whole_lists_keep_the_full_search(box, monkeypatch):
    """MPH_LIST_FULL=1: the lists keep the shell's pairs, so the guard (lean_search_ok) leaves the
    lazy steps the full acceptance; pass A is lean as before."""
    monkeypatch.setenv("MPH_LIST_FULL", "1")
    a, lean, lazy = run(*box, [8, 8], {8, 16})
    b, _, _ = run(*box, [1] * 16, {8, 16})
    monkeypatch.delenv("MPH_LIST_FULL")
    assert lean[-1] == {"search_steps": 0, "pass_a_steps": 14} and lazy == [7, 14], (lean, lazy)
    assert_same(a, b, "MPH_LIST_FULL=1")


# seam3d: periodic faces, waves on the search's slow path; movwall3d: moving walls; gate3d_jit:
# structure lanes off the lattice; box3d_st: surface tension -- pass B reads GravityCenter and
# PressureA, so pass A keeps every sum and only the search is lean; dam2d: 2-D; box3d_r262131_jit:
# RadiusRatioA / P / V = 2.6 / 2.1 / 3.1 off the lattice, pass A's general form
@pytest.mark.parametrize("case,pass_a", [("seam3d", 14), ("movwall3d", 14), ("gate3d_jit", 14), ("box3d_st", 0),
                                         ("dam2d", 14), ("box3d_r262131_jit", 14)])
def test_other_cases(case, pass_a):
    """Two 8-step batches against 16 single steps."""
    cfg, parts = cases.get(case).build()
    a, lean, lazy = run(cfg, parts, [8, 8], {8, 16})
    b, none, _ = run(cfg, parts, [1] * 16, {8, 16})
    assert lean[-1] == {"search_steps": 14, "pass_a_steps": pass_a} and lazy == [7, 14], (lean, lazy)
    assert all(c == ZERO for c in none), none
    assert_same(a, b, case)
