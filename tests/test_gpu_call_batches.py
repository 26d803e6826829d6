"""Lean batches up to a call's last (csrc/mph_kernels.h replay_plan): a call can
only be observed after it returns, so of the whole 8-step batches of one mph_step(n) only the last
ends in a step that stores the output-only fields; the batches before it come from an 8-step graph
whose steps are all lazy (kSeq8t).  And the key fold (seq_step): inside a
graph, pass B moves and wraps the particles and leaves the next step's cell keys, slots and
histogram, so only the graph's first step launches k_prep.  Nothing a caller can read may change:
every comparison here is bitwise, mph_step(n) in one call against n x mph_step(1), over
parity.CHUNK_FIELDS and both virial fields.

n = 16 is kSeq8t + kSeq8 (15 lazy steps), n = 29 is 2 x kSeq8t + kSeq8 + 4 x kSeq1t + kSeq1
(23 + 4), n = 40 is 4 x kSeq8t + kSeq8 (39).  The cases: the 12,000-particle tank of
test_gpu_idle_walls.py (a partial last wave, idle walls, a moving fluid block), also under the
work-balanced XCD map; box3d_jit (off the lattice: the shell pairs the lean search leaves out);
seam3d (periodic faces); movwall3d (rigid wall motion across Time 0.2); rolling3d; turek2d (the
inlet profile; its elastic plate keeps the fold off) and turek2d_fluid, the same channel with fluid
in the plate's place, which takes the inlet profile through the fold; dam2d; box3d_st (surface
tension: pass A never lean); gate3d (structures: fold off, plan on).
"""
import pytest

from parity import assert_same, run_calls, snapshot, step_counters as counters, tank
from particlemethod_fsi_amd import MphSolver, cases

pytestmark = pytest.mark.gpu

CALLS = (16, 29, 40)
CASES = ["tank", "box3d_jit", "seam3d", "movwall3d", "rolling3d", "turek2d", "turek2d_fluid", "dam2d", "box3d_st",
         "gate3d"]
STRUCTURES = {"turek2d", "gate3d"}   # cases with structure particles: the fold stays off


ZERO = {"lazy": 0, "lean_search": 0, "lean_pass_a": 0, "folded": 0}


def one_call(cfg, parts, n, monitors=False):
    snaps, c, _, _ = run_calls(cfg, parts, [n], {n}, 64 if monitors else 0)
    return snaps[n], c[0]


_built, _single = {}, {}


def build(case):
    if case not in _built:
        # (turek2d_fluid, cases.SLAB_MOTION_CASES: turek2d with fluid where its elastic plate is -- no
        # structure particle, so the fold is on and the inlet profile runs in pass B's tail)
        _built[case] = tank() if case == "tank" else cases.get(case).build()
    return _built[case]


def single_steps(case):
    """40 x mph_step(1) on `case`, every step full: the snapshots after 16, 29 and 40 steps.  Computed
    once per case and shared, never changed."""
    if case not in _single:
        snaps = {}
        with MphSolver(*build(case)) as s:
            for k in range(1, max(CALLS) + 1):
                s.step(1)
                if k in CALLS:
                    snaps[k] = snapshot(s)
            assert counters(s) == dict(ZERO, prep=max(CALLS))
        _single[case] = snaps
    return _single[case]


def lazy_steps(n):
    """Every step of one mph_step(n) is lazy but the last of the last whole batch and the call's last."""
    return n - 1 - (1 if n >= 8 and n % 8 else 0)


def folded_steps(n):
    """Seven of every 8-step graph's steps leave the next one's keys; a single-step graph folds nothing."""
    return 7 * (n // 8)


@pytest.mark.parametrize("n", CALLS)
@pytest.mark.parametrize("case", CASES)
def test_one_call_equals_single_steps(case, n):
    snap, c = one_call(*build(case), n)
    print(case, n, c)
    assert c["lazy"] == lazy_steps(n), c
    assert c["folded"] == (0 if case in STRUCTURES else folded_steps(n)) and c["prep"] == n - c["folded"], c
    assert_same(snap, single_steps(case)[n], (case, n))


@pytest.mark.parametrize("n", CALLS)
def test_balanced_xcd_map(n, monkeypatch):
    """The tank with the work-balanced XCD map of the passes forced on: a full step's map is now as
    old as the previous call's end (list_block falls back to the equal ranges where a range does
    not fit)."""
    monkeypatch.setenv("MPH_XCD_BAL_MIN", "0")
    snap, c = one_call(*build("tank"), n)
    monkeypatch.delenv("MPH_XCD_BAL_MIN")
    assert c["lazy"] == lazy_steps(n) and c["folded"] == folded_steps(n), c
    assert_same(snap, single_steps("tank")[n], ("tank, MPH_XCD_BAL_MIN=0", n))


def test_counters():
    """step(40) on the tank: 39 lazy steps, all of them lean, 35 folded, 5 k_prep launches; step(13): 7 +
    4 lazy as before, 7 folded; step(8) and step(9): 7 and 7.  Structures (gate3d): none folded."""
    cfg, parts = build("tank")
    assert one_call(cfg, parts, 40)[1] == {"lazy": 39, "lean_search": 39, "lean_pass_a": 39, "folded": 35, "prep": 5}
    assert one_call(cfg, parts, 13)[1] == {"lazy": 11, "lean_search": 11, "lean_pass_a": 11, "folded": 7, "prep": 6}
    for n in (8, 9):
        c = one_call(cfg, parts, n)[1]
        assert c["lazy"] == 7 and c["folded"] == 7, (n, c)
    c = one_call(*build("gate3d"), 40)[1]
    assert c["lazy"] == 39 and c["folded"] == 0 and c["prep"] == 40, c


def test_two_calls_store_twice():
    """Calls of 16 and 24 steps: each ends in a storing step of its own (15 + 23 lazy steps), and a
    reader between them sees the 16th step's outputs."""
    with MphSolver(*build("tank")) as s:
        s.step(16)
        mid = snapshot(s)
        s.step(24)
        c = counters(s)
        end = snapshot(s)
    assert c["lazy"] == 15 + 23, c
    assert_same(mid, single_steps("tank")[16], "first call")
    assert_same(end, single_steps("tank")[40], "second call")


def test_monitors_keep_every_step_full():
    """With monitors no step is lazy; the batches before a call's last still store no output-only field."""
    snap, c = one_call(*build("tank"), 40, monitors=True)
    assert c == dict(ZERO, prep=40), c
    assert_same(snap, single_steps("tank")[40], "monitors")


def test_step_paths_fold_alike():
    """Nine steps phase-timed and nine profiled (one direct-launch batch each, folded like a graph)
    against nine single steps, on the off-lattice box."""
    cfg, parts = build("box3d_jit")
    snaps = []
    for way in ("single", "phase", "profile"):
        with MphSolver(cfg, parts) as s:
            if way == "single":
                for _ in range(9):
                    s.step(1)
            elif way == "phase":
                s.phase_timing(True)
                s.step(9)
            else:
                s.profile(9)
            c = counters(s)
            snaps.append(snapshot(s))
        assert c["folded"] == {"single": 0, "phase": 7, "profile": 8}[way], (way, c)
    assert_same(snaps[1], snaps[0], "phase-timed")
    assert_same(snaps[2], snaps[0], "profiled")


def test_fold_on_equals_off(monkeypatch):
    """MPH_KEY_FOLD=0 at creation: no step folded, every step opens with k_prep, the lazy counts and
    the bits of the default."""
    monkeypatch.setenv("MPH_KEY_FOLD", "0")
    off, c = one_call(*build("tank"), 40)
    off_seam, c_seam = one_call(*build("seam3d"), 29)
    monkeypatch.delenv("MPH_KEY_FOLD")
    assert c == {"lazy": 39, "lean_search": 39, "lean_pass_a": 39, "folded": 0, "prep": 40}, c
    assert c_seam["folded"] == 0 and c_seam["lazy"] == lazy_steps(29), c_seam
    assert_same(off, single_steps("tank")[40], "MPH_KEY_FOLD=0")
    assert_same(off_seam, single_steps("seam3d")[29], "MPH_KEY_FOLD=0, seam3d")


def test_on_equals_off(monkeypatch):
    """MPH_LEAN_CALLS=0 at creation: every whole batch ends in a storing step (35 lazy steps of 40, 7 + 7
    + 4 of 29), the same bits."""
    monkeypatch.setenv("MPH_LEAN_CALLS", "0")
    off40, c40 = one_call(*build("tank"), 40)
    off29, c29 = one_call(*build("tank"), 29)
    monkeypatch.delenv("MPH_LEAN_CALLS")
    assert c40["lazy"] == 35 and c29["lazy"] == 7 * 3 + 4, (c40, c29)
    assert_same(off40, single_steps("tank")[40], "MPH_LEAN_CALLS=0, 40")
    assert_same(off29, single_steps("tank")[29], "MPH_LEAN_CALLS=0, 29")
