"""CPU: the host part of particle selections on slab ranks (include/mph_gpu.h mph_dist_select and its
readers, mph_totals_combine) and a model check of the runs the GPU tests use (tests/select_ranks.py
CASES), so that those tests cannot pass vacuously.

What a run is taken to reach is decided by the trajectories, the cuts and the step counts, so it is
checked here on the oracle alone (OracleSolver, which test_oracle.py pins to the reference) with the
library's own host rule for owners (solver.slab_owner; structure particles by InitialPosition): every
selection is non-empty on the ranks it is meant for and empty on the rank meant to be empty, a box has
members on both sides of a cut and of the periodic face, a selected particle changes owner within the
steps, a rank owns a particle from outside its creation window, particles sit exactly on both bounds of
a box.  The asserted numbers are conditions; the counts the oracle gave are in the docstrings.
"""
import ctypes

import numpy as np
import pytest

from particlemethod_fsi_amd import solver
from particlemethod_fsi_amd.solver import TOTAL_SLOTS as S, TOTALS, MphError, totals_combine

import select_ranks
from oracle_bindings import OracleSolver
from select_ranks import CASES, mask_of, selections, setup

NEW = ("mph_dist_select", "mph_dist_selected_ids", "mph_dist_get_selected", "mph_dist_selection_totals_partial",
       "mph_totals_combine", "mph_dist_selection_totals", "mph_dist_gather_selected", "mph_dist_write_vtk_selected",
       "mph_dist_write_vtu_selected")


def test_symbols_signatures_and_abi_version():
    L = solver.load_library()
    vp, ip = ctypes.c_void_p, ctypes.c_int
    for name in NEW:
        assert hasattr(L, name), name
        assert name in solver.EXPORTED_SYMBOLS
    assert L.mph_abi_version() == 6
    assert L.mph_dist_select.argtypes == [vp, ctypes.POINTER(solver.MphSelection), ctypes.POINTER(ip)]
    assert L.mph_dist_get_selected.argtypes == [vp, ip, vp] and L.mph_dist_get_selected.restype == ip
    assert L.mph_dist_gather_selected.restype == ctypes.c_longlong
    assert L.mph_dist_gather_selected.argtypes == [vp, ip, vp, vp, ctypes.c_longlong]
    assert L.mph_totals_combine.argtypes == [ip, vp, vp]
    for name in ("dist_select", "dist_selected_ids", "dist_get_selected", "dist_selection_totals", "dist_gather_selected",
                 "dist_write_vtk_selected", "dist_write_vtu_selected"):
        assert callable(getattr(solver.MphSolver, name)), name


def test_null_contexts():
    L = solver.load_library()
    sel = solver.make_selection()
    c, out = np.zeros(3), np.zeros(TOTALS)
    assert L.mph_dist_select(None, ctypes.byref(sel), None) == -1
    assert L.mph_dist_selected_ids(None, None) == -1
    assert L.mph_dist_get_selected(None, 0, None) == -1
    assert L.mph_dist_selection_totals_partial(None, c.ctypes.data, out.ctypes.data) == -1
    assert L.mph_dist_selection_totals(None, c.ctypes.data, out.ctypes.data) == -1
    assert L.mph_dist_gather_selected(None, 0, None, None, 0) == -1
    assert L.mph_dist_write_vtk_selected(None, b"unused.vtk") == -1
    assert L.mph_dist_write_vtu_selected(None, b"unused.vtu") == -1


# ---- mph_totals_combine --------------------------------------------------------------------------

MINS = [S[k] for k in ("XMIN", "YMIN", "ZMIN")]
MAXS = [S[k] for k in ("XMAX", "YMAX", "ZMAX", "VMAX2")]
EMPTY = np.zeros(TOTALS)
EMPTY[MINS] = np.inf
EMPTY[[S[k] for k in ("XMAX", "YMAX", "ZMAX")]] = -np.inf


def _loop(records):
    """Rank 0's record combined with ranks 1, 2, ... in order, slot by slot, in Python floats."""
    out = [float(v) for v in records[0]]
    for r in records[1:]:
        for k in range(TOTALS):
            a, b = out[k], float(r[k])
            out[k] = min(a, b) if k in MINS else (max(a, b) if k in MAXS else a + b)
    out[S["RESERVED0"]] = out[S["RESERVED1"]] = 0.0
    return np.array(out)


def _record(rng, n):
    """A record as a rank of n selected particles could give it."""
    if n == 0:
        return EMPTY.copy()
    r = rng.normal(size=TOTALS) * 10.0 ** rng.integers(-8, 8, TOTALS)
    r[S["COUNT"]] = n
    for lo, hi in zip(MINS, MAXS[:3]):
        r[lo], r[hi] = sorted((r[lo], r[hi]))
    r[S["VMAX2"]] = abs(r[S["VMAX2"]])
    r[S["RESERVED0"]] = r[S["RESERVED1"]] = 0.0
    return r


@pytest.mark.parametrize("nranks", [1, 2, 3, 8])
def test_totals_combine_is_the_loop_in_rank_order(nranks):
    rng = np.random.default_rng(77 + nranks)
    for trial in range(50):
        counts = rng.integers(0, 4, nranks) * rng.integers(0, 2, nranks)     # empty ranks among them
        recs = [_record(rng, int(n)) for n in counts]
        got, ref = totals_combine(recs), _loop(recs)
        assert got.tobytes() == ref.tobytes(), (trial, got, ref)
    # the extrema do not depend on the rank order
    assert totals_combine(recs[::-1])[MINS + MAXS].tobytes() == got[MINS + MAXS].tobytes()


def test_totals_combine_adds_in_rank_order():
    """Plain FP64 from rank 0 on: (1 + 1e16) - 1e16 is 0, (-1e16 + 1e16) + 1 is 1."""
    recs = []
    for fx in (1.0, 1.0e16, -1.0e16):
        r = EMPTY.copy()
        r[S["COUNT"]], r[S["FX"]] = 1.0, fx
        recs.append(r)
    assert totals_combine(recs)[S["FX"]] == 0.0 and totals_combine(recs[::-1])[S["FX"]] == 1.0
    assert totals_combine(recs)[S["COUNT"]] == 3.0


def test_totals_combine_identities():
    """An all-empty set is the empty record; an empty rank changes nothing; a single rank is itself."""
    rng = np.random.default_rng(5)
    assert totals_combine([EMPTY] * 3).tobytes() == EMPTY.tobytes()
    assert totals_combine([EMPTY]).tobytes() == EMPTY.tobytes()
    r = _record(rng, 7)
    assert totals_combine([r]).tobytes() == r.tobytes()
    assert totals_combine([EMPTY, r, EMPTY]).tobytes() == r.tobytes()
    # the reserved slots are 0 whatever the records hold
    junk = r.copy()
    junk[S["RESERVED0"]] = 3.0
    assert totals_combine([junk, r])[S["RESERVED0"]] == 0.0


def test_totals_combine_argument_errors():
    L = solver.load_library()
    r, out = EMPTY.copy(), np.zeros(TOTALS)
    ptrs = (ctypes.c_void_p * 2)(r.ctypes.data, r.ctypes.data)
    assert L.mph_totals_combine(0, ptrs, out.ctypes.data) == -1
    assert L.mph_totals_combine(-1, ptrs, out.ctypes.data) == -1
    assert L.mph_totals_combine(2, None, out.ctypes.data) == -1
    assert L.mph_totals_combine(2, ptrs, None) == -1
    assert L.mph_totals_combine(2, (ctypes.c_void_p * 2)(r.ctypes.data, None), out.ctypes.data) == -1
    assert L.mph_totals_combine(2, ptrs, out.ctypes.data) == 0
    with pytest.raises(MphError) as e:
        totals_combine([])
    assert e.value.code == -1


# ---- the runs of the GPU tests, on the oracle ---------------------------------------------------------

_traj = {}


def trajectory(run):
    """(Position at creation, Position after the run's steps) of the oracle; a case is stepped once,
    through the step counts of all its runs."""
    name = CASES[run]["case"]
    if name not in _traj:
        _, cfg, parts, _, _ = setup(run)
        o = OracleSolver(cfg, parts)
        o.init()
        at, done = {0: o.get("Position").copy()}, 0
        for k in sorted({C["steps"] for C in CASES.values() if C["case"] == name}):
            o.step(k - done)
            done = k
            at[k] = o.get("Position").copy()
        _traj[name] = at
    return _traj[name][0], _traj[name][CASES[run]["steps"]]


def owners(cfg, parts, axis, world, cuts, X):
    """Owner ranks as the slab layer assigns them: structure particles by InitialPosition, others by X."""
    struct = (parts.property == 2) | (parts.property == 3)
    a = np.where(struct, parts.initial_position[:, axis], X[:, axis])
    return np.array([solver.slab_owner(cfg, world, axis, float(v), cuts) for v in a], np.int32)


def _counts(run, X):
    """{label: selected per rank} of the run's selections on the state X."""
    _, cfg, parts, axis, cuts = setup(run)
    world = CASES[run]["world"]
    own = owners(cfg, parts, axis, world, cuts, X)
    out = {}
    for lab, sel in selections(cfg, parts, axis, world, cuts, X):
        m = mask_of(sel, cfg.dim, parts.property, X, parts.initial_position)
        out[lab] = np.bincount(own[m], minlength=world)
    return out, own


# the ranks a selection is meant to leave empty (every other rank holds some of it)
EMPTY_RANKS = {
    ("channel3d", "cut"): (2,), ("channel3d_local", "cut"): (2,),     # the first cut is ranks 0 and 1's
    ("channel3d_local", "onpart"): (0,),
    ("dam2d", "fluid"): (1,), ("dam2d", "onpart"): (1,),              # rank 1 holds walls alone
    ("gate2d_sub", "fluid"): (1,), ("gate2d_sub", "onpart"): (1,),
    ("gate2d_sub", "body"): (0,),                                     # the gate stands in rank 1's slab
    ("movwall2d_slab", "fluid"): (0,), ("movwall2d_slab", "onpart"): (0,),   # rank 0: left-wall columns alone
}


@pytest.mark.parametrize("run", sorted(CASES))
def test_selections_reach_the_ranks_they_are_meant_for(run):
    """Selected particles per rank after the run's steps, on the oracle:

        channel3d        fluid 1872/1440/1872  walls 2028/1560/2028  onpart 82/323/64  cut 900/900/0  face 741/570/741
        channel3d_local  fluid 1040/1118/3026  walls 1092/1248/3276  onpart 0/116/267  cut 900/900/0  face 424/476/1260
        dam2d            fluid 4850/0  walls 900/900  onpart 798/0  cut 9/9  face 1696/96
        gate2d_sub       fluid 4850/0  walls 900/885  onpart 798/0  cut 9/240  face 1696/256  body 0/400
        movwall2d_slab   fluid 0/4850  walls 467/1333 (600/1200 at creation)  onpart 0/780  cut 467/363  face 64/1761

    (printed below in full).  "none" is empty and "all" is everything on every run."""
    X0, X = trajectory(run)
    world = CASES[run]["world"]
    for tag, Y in (("creation", X0), ("stepped", X)):
        counts, own = _counts(run, Y)
        print(run, tag, {k: v.tolist() for k, v in counts.items()})
        assert counts["none"].sum() == 0 and counts["all"].sum() == len(Y)
        assert (np.bincount(own, minlength=world) > 0).all()
        for lab, per_rank in counts.items():
            if lab in ("none",):
                continue
            empty = EMPTY_RANKS.get((run, lab), ())
            for r in range(world):
                assert (per_rank[r] == 0) == (r in empty), (run, tag, lab, per_rank.tolist())
        # the disjoint pair of the stale-flag check
        assert counts["fluid"].sum() > 0 and counts["walls"].sum() > 0
        # the box at the cut has members on both sides of it
        assert counts["cut"][0] > 0 and counts["cut"][1] > 0


def test_an_intended_empty_rank():
    _, X = trajectory("dam2d")
    counts, _ = _counts("dam2d", X)
    assert counts["fluid"][1] == 0 and counts["fluid"][0] > 1000 and counts["walls"][1] >= 100


def test_a_box_spans_the_periodic_face():
    """channel3d "face": the slab axis z is periodic; the box holds particles within one spacing of both
    ends of the domain, owned by the first and the last rank, and particles of every rank."""
    _, cfg, parts, axis, cuts = setup("channel3d")
    _, X = trajectory("channel3d")
    sel = dict(selections(cfg, parts, axis, 3, cuts, X))["face"]
    m = mask_of(sel, cfg.dim, parts.property, X, parts.initial_position)
    own = owners(cfg, parts, axis, 3, cuts, X)
    dx = cfg.particle_spacing
    low, high = m & (X[:, axis] < cfg.domain_min[axis] + dx), m & (X[:, axis] >= cfg.domain_max[axis] - dx)
    print("face: %d selected, %d at the lower end, %d at the upper" % (m.sum(), low.sum(), high.sum()))
    assert low.sum() >= 10 and high.sum() >= 10
    assert set(own[low].tolist()) == {0} and set(own[high].tolist()) == {2}
    assert (np.bincount(own[m], minlength=3) > 0).all() and 0 < m.sum() < len(m)


@pytest.mark.parametrize("run", sorted(CASES))
def test_particles_on_both_bounds_of_the_box(run):
    _, cfg, parts, axis, cuts = setup(run)
    X0, X = trajectory(run)
    for Y in (X0, X):
        sel = dict(selections(cfg, parts, axis, CASES[run]["world"], cuts, Y))["onpart"]
        fl = parts.property < 2
        for d in range(cfg.dim):
            assert (Y[fl, d] == sel.lo[d]).any() and (Y[fl, d] == sel.hi[d]).any()
        m = mask_of(sel, cfg.dim, parts.property, Y, parts.initial_position)
        assert 0 < m.sum() < fl.sum()


@pytest.mark.parametrize("run,kind", [("channel3d", "fluid"), ("movwall2d_slab", "walls"), ("channel3d_local", "fluid")])
def test_a_selected_particle_changes_owner(run, kind):
    """Particles of the "all" selection (and of `kind`) whose owner at creation is not their owner after
    the steps: channel3d fluid across every cut and the periodic face, movwall2d_slab left-wall columns
    across the cut at -0.00048."""
    _, cfg, parts, axis, cuts = setup(run)
    world = CASES[run]["world"]
    X0, X = trajectory(run)
    a, b = owners(cfg, parts, axis, world, cuts, X0), owners(cfg, parts, axis, world, cuts, X)
    T = parts.property
    moved = (a != b) & ((T < 2) if kind == "fluid" else (T >= 4))
    print(run, "owner changes:", int(moved.sum()), "by (from, to):",
          {(int(f), int(t)): int(((a == f) & (b == t) & moved).sum()) for f in range(world) for t in range(world) if f != t})
    assert moved.sum() >= 4


def test_an_immigrant_from_outside_the_creation_window():
    """channel3d_local at step 300: ranks 0 and 1 own fluid particles (type 1) that were outside their
    creation windows (solver.slab_window) -- 286 and 254 on the oracle -- and none before step 264."""
    run = "channel3d_local"
    _, cfg, parts, axis, cuts = setup(run)
    X0, X = trajectory(run)
    own = owners(cfg, parts, axis, 3, cuts, X)
    W = cfg.domain_max[axis] - cfg.domain_min[axis]
    found = []
    for r in range(3):
        lo, hi = solver.slab_window(cfg, r, 3, axis, cuts)
        inside = ((X0[:, axis] - lo) % W) < (hi - lo)
        found.append(int((~inside & (own == r)).sum()))
        assert set(parts.property[~inside & (own == r)].tolist()) <= {0, 1}
    print("immigrants from outside the creation window:", found)
    assert found[0] >= 10 and found[1] >= 10
    dx = cfg.particle_spacing
    for r in range(3):
        lo, hi, h = solver.slab_bounds(cfg, r, 3, axis, cuts)
        assert hi - lo >= 2 * h + 2 * dx
