"""GPU: particle selections on slab ranks (include/mph_gpu.h mph_dist_select and its readers; the slab
forms of the kernels in csrc/mph_select.hip, the collective calls in csrc/mph_dist_select.hip).

Ranks share the one GPU over the host-staged transport (tests/select_ranks.py, which also names the
runs, cuts and selections; tests/test_dist_select_abi.py checks on the CPU that they reach the ranks,
the cuts, the periodic face, owner changes and a particle from outside a creation window).  One run per
case, made once: the calls at creation and after the run's steps (20; the slab-local run 300) -- owners
have changed by then.  Every reference is numpy on the gathered state (dist.gather_field: every rank's
mph_get merged): the ids are the selection rule's mask, a rank's rows are the gathered field at its
ids, bit for bit, and the totals are recomputed from the gathered rows -- COUNT, the extent, VMAX2 and
the reserved slots bit for bit, the sums within 2 (n + 8) 2^-53 sum |term|, the bound of
tests/test_gpu_select.py, which holds for any order of addition.
"""
import math

import numpy as np
import pytest

from particlemethod_fsi_amd import MphSolver, cases, solver
from particlemethod_fsi_amd.solver import FIELDS, TOTAL_SLOTS as S, TOTALS, MphError, totals_combine

import dist_worker
import select_ranks
from select_ranks import BAD, CASES, CENTER, EDGE_TARGETS, FRAME, GATHERED, LOCAL_FIELDS, STATIC, mask_of, selections, setup
from test_gpu_dist import STRUCT_FIELDS

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
MORE = 8
RUNS = sorted(CASES)
WHOLE = [r for r in RUNS if not CASES[r]["local"]]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """A run per (run, with or without the calls, the step calls), made once and shared."""
    made = {}

    def get(run, calls=True, split=None):
        split = tuple(split or (CASES[run]["steps"],))
        if (run, calls, split) not in made:
            tmp = tmp_path_factory.mktemp("select")
            out = str(tmp / "run.npz")
            spec = dict(run=run, calls=calls, split=split, more=MORE, fields=STRUCT_FIELDS, tmp=str(tmp))
            dist_worker.run_ranks(select_ranks.select_worker, CASES[run]["world"], spec, out, timeout=300)
            made[(run, calls, split)] = np.load(out)
        return made[(run, calls, split)]
    return get


def _labels(run, cfg, parts, axis, cuts, X):
    return [(lab, sel) for lab, sel in selections(cfg, parts, axis, CASES[run]["world"], cuts, X)
            if not (CASES[run]["local"] and sel.box == 2)]


# ---- 1. ids, 3. stale flags -----------------------------------------------------------------------

@pytest.mark.parametrize("run", RUNS)
def test_ids_partition_the_selection(runs, run):
    r = runs(run)
    _, cfg, parts, axis, cuts = setup(run)
    world, T, X0 = CASES[run]["world"], parts.property, parts.initial_position
    for tag in ("s0", "s1"):
        X, owner = r[tag + "/X"], r[tag + "/owner"]
        assert (owner >= 0).all()
        got = {}
        for lab, sel in _labels(run, cfg, parts, axis, cuts, X):
            ref = np.nonzero(mask_of(sel, cfg.dim, T, X, X0))[0]
            per_rank = [r["%s/%s/ids%d" % (tag, lab, k)] for k in range(world)]
            for k, ids in enumerate(per_rank):
                assert ids.dtype == np.int32 and (np.diff(ids) > 0).all(), (tag, lab, k, "ascending")
                assert (owner[ids] == k).all(), (tag, lab, k, "a subset of owned_ids()")
                # Position is what mph_get returns on the rank
                assert r["%s/%s/pos%d" % (tag, lab, k)].tobytes() == X[ids].tobytes(), (tag, lab, k)
            union = np.concatenate(per_rank)
            assert len(np.unique(union)) == len(union), (tag, lab, "duplicates")
            assert np.array_equal(np.sort(union), ref), (tag, lab, len(union), len(ref))
            got[lab] = per_rank
        # stale flags: "walls" was made right after the disjoint "fluid", without a step -- no id of it
        fluid, walls = np.concatenate(got["fluid"]), np.concatenate(got["walls"])
        assert len(fluid) and len(walls) and not np.intersect1d(fluid, walls).size
        assert sum(len(i) for i in got["all"]) == parts.n and sum(len(i) for i in got["none"]) == 0
    # a selected particle has changed owner between the two blocks, and is on its new rank only
    a, b = r["s0/owner"], r["s1/owner"]
    moved = np.nonzero(a != b)[0]
    print(run, "owner changes:", len(moved))
    if run in ("channel3d", "channel3d_local", "movwall2d_slab"):
        assert len(moved) >= 4
        for i in moved[:50]:
            assert i in r["s0/all/ids%d" % a[i]] and i in r["s1/all/ids%d" % b[i]] and i not in r["s1/all/ids%d" % a[i]]


# ---- 2. the scan's edges per rank ---------------------------------------------------------------

def test_scan_edges_per_rank(tmp_path):
    """A fluid block of 4,230 particles (not a multiple of 4) cut in two: boxes that hold 0, 1, 1,023,
    1,024 and 1,025 particles of one rank and none of the other."""
    out = str(tmp_path / "edge.npz")
    dist_worker.run_ranks(select_ranks.edge_worker, 2, out, timeout=300)
    r = np.load(out)
    n = select_ranks.EDGE_NX * select_ranks.EDGE_NY
    assert n % 4 != 0
    names = ("Position", "Velocity", "Force", "PressureP", "NeighborCount", "Mass")
    for tag in ("s0", "s2"):
        owner = r[tag + "/owner"]
        G = {name: r["%s/g/%s" % (tag, name)] for name in names}
        assert len(owner) == n and (np.bincount(owner, minlength=2) > 1025).all()
        for r0 in (0, 1):
            for t in EDGE_TARGETS:
                key = "%s/r%dt%d/" % (tag, r0, t)
                box = r[key + "box"]
                sel = solver.make_selection(box=box)
                ref = np.nonzero(mask_of(sel, 2, np.ones(n, np.int32), G["Position"], G["Position"]))[0]
                assert len(ref) == t and (owner[ref] == r0).all(), (key, len(ref))
                for k in (0, 1):
                    ids = r[key + "ids%d" % k]
                    assert np.array_equal(ids, ref if k == r0 else ref[:0]), (key, k)
                    for name in names:
                        assert r["%s%s%d" % (key, name, k)].tobytes() == G[name][ids].tobytes(), (key, name, k)
                    _check_record(r[key + "tp%d" % k], ids, G["Position"], G["Velocity"], G["Force"], G["Mass"], (key, k))


# ---- 5. totals -----------------------------------------------------------------------------------

def _reference(ids, X, V, F, M, center):
    """numpy form of the totals over the rows `ids`: ({slot: value} exact, {slot: (sum, sum |term|)})."""
    X, V, F, M = X[ids], V[ids], F[ids], M[ids]
    n = len(ids)
    v2 = V[:, 0] * V[:, 0] + V[:, 1] * V[:, 1] + V[:, 2] * V[:, 2]
    exact = {"COUNT": float(n), "VMAX2": float(v2.max()) if n else 0.0, "RESERVED0": 0.0, "RESERVED1": 0.0}
    for d, ax in enumerate("XYZ"):
        exact[ax + "MIN"] = float(X[:, d].min()) if n else np.inf
        exact[ax + "MAX"] = float(X[:, d].max()) if n else -np.inf
    D = X - np.asarray(center, np.float64)
    terms = {"MASS": (M, None), "KE": ((0.5 * M) * v2, None)}
    for d, ax in enumerate("XYZ"):
        terms["P" + ax] = (M * V[:, d], None)
        terms["F" + ax] = (F[:, d], None)
        terms["M" + ax] = (M * X[:, d], None)
        a, b = (d + 1) % 3, (d + 2) % 3
        p, q = D[:, a] * F[:, b], D[:, b] * F[:, a]
        terms["T" + ax] = (p - q, np.abs(p) + np.abs(q))
    sums = {k: (math.fsum(t), math.fsum(np.abs(t) if a is None else a)) for k, (t, a) in terms.items()}
    return exact, sums


def _check_record(rec, ids, X, V, F, M, label):
    assert rec.shape == (TOTALS,)
    exact, sums = _reference(ids, X, V, F, M, CENTER)
    n = len(ids)
    for k, v in exact.items():
        assert rec[S[k]] == v, (label, k, rec[S[k]], v)
    for k, (v, a) in sums.items():
        tol = 2.0 * (n + 8) * EPS * a
        assert abs(rec[S[k]] - v) <= tol, (label, k, rec[S[k]], v, tol)


def _mass(runs, run):
    """Mass by original index: the gathered field of the run with whole inputs (Mass follows the type)."""
    return runs("channel3d" if CASES[run]["local"] else run)["g/Mass"]


@pytest.mark.parametrize("run", RUNS)
def test_totals_against_numpy(runs, run):
    r = runs(run)
    _, cfg, parts, axis, cuts = setup(run)
    world = CASES[run]["world"]
    M = _mass(runs, run)
    assert (M > 0.0).all()
    for tag in ("s0", "s1"):
        X, V, F = r[tag + "/X"], r[tag + "/V"], r[tag + "/F"]
        for lab, sel in _labels(run, cfg, parts, axis, cuts, X):
            key = "%s/%s/" % (tag, lab)
            tp = r[key + "tp"]
            assert tp.shape == (world, TOTALS)
            for k in range(world):
                _check_record(tp[k], r[key + "ids%d" % k], X, V, F, M, (run, tag, lab, k))
            # the collective result is the combine of the partial records, and repeats bit for bit
            assert r[key + "tc"].tobytes() == totals_combine(list(tp)).tobytes(), key
            assert r[key + "tc2"].tobytes() == r[key + "tc"].tobytes(), key
            whole = np.sort(np.concatenate([r[key + "ids%d" % k] for k in range(world)]))
            exact, _ = _reference(whole, X, V, F, M, CENTER)
            for name, v in exact.items():
                assert r[key + "tc"][S[name]] == v, (key, name)
        empty = r[tag + "/none/tc"]
        assert empty[S["COUNT"]] == 0.0 and empty[S["XMIN"]] == np.inf and empty[S["ZMAX"]] == -np.inf and empty[S["VMAX2"]] == 0.0
    tc = r["s1/walls/tc"]
    print(run, "load on the walls", tc[S["FX"]], tc[S["FY"]], "torque", tc[S["TZ"]])
    if run == "movwall2d_slab":
        assert (tc[S["FX"]] != 0.0 or tc[S["FY"]] != 0.0) and tc[S["TZ"]] != 0.0
        # another centre, another torque: the origin's differs from CENTER's
        X, F = r["s1/X"], r["s1/F"]
        w = np.nonzero(parts.property >= 4)[0]
        origin = math.fsum(X[w, 0] * F[w, 1] - X[w, 1] * F[w, 0])
        assert abs(origin - tc[S["TZ"]]) > 1e-6 * abs(origin)


def test_partial_totals_do_not_depend_on_the_batch_shape(runs):
    """dam2d after step(20) and after step(7); step(13): the gathered states are bit-identical, and so
    are every rank's partial records."""
    a, b = runs("dam2d"), runs("dam2d", calls=False, split=(7, 13))
    for k in ("X", "V", "F"):
        assert a["s1/" + k].tobytes() == b["s1/" + k].tobytes(), "the slab steps differ between the batch shapes: " + k
    for lab in ("fluid", "walls", "onpart"):
        assert a["s1/%s/tp" % lab].tobytes() == b["s1/%s/tp" % lab].tobytes(), lab


# ---- 4. fields -----------------------------------------------------------------------------------

@pytest.mark.parametrize("run", RUNS)
def test_every_field_equals_the_gathered_field_at_the_ids(runs, run):
    r = runs(run)
    _, cfg, parts, axis, cuts = setup(run)
    world, local = CASES[run]["world"], CASES[run]["local"]
    whole = runs("channel3d") if local else r      # the static fields of the same case with whole inputs
    names = LOCAL_FIELDS if local else tuple(FIELDS)
    ids = [r["fld/ids%d" % k] for k in range(world)]
    assert all(len(i) > 0 for i in ids)
    for name in names:
        ref = whole["g/" + name] if (local and name in STATIC) else r["g/" + name]
        for k in range(world):
            got = r["fld/%s/%d" % (name, k)]
            assert got.dtype == ref.dtype and got.shape == ref[ids[k]].shape, (name, k)
            assert got.tobytes() == ref[ids[k]].tobytes(), (run, name, k)
    # the collective gather is the merge of the rank rows, ids ascending
    merged = np.sort(np.concatenate(ids))
    for name in (GATHERED if not local else ("Position", "Force", "NeighborCount", "Property")):
        ref = whole["g/" + name] if (local and name in STATIC) else r["g/" + name]
        assert np.array_equal(r["cg/%s/ids" % name], merged) and r["cg/%s/ids" % name].dtype == np.int32
        assert r["cg/%s/rows" % name].tobytes() == ref[merged].tobytes(), (run, name)
    fluid = np.nonzero(parts.property < 2)[0]
    assert np.array_equal(r["cgf/ids"], fluid) and r["cgf/rows"].tobytes() == r["g/Velocity"][fluid].tobytes()
    if run == "dam2d":     # (rank 1 sent an empty message)
        assert len(r["s1/fluid/ids1"]) == 0
    if run == "gate2d_sub":
        sel = np.concatenate(ids)
        assert np.abs(r["g/Stress"][sel]).max() > 0.0 and np.abs(r["g/DeformGradient"][sel]).max() > 0.0
        assert np.abs(r["g/VirialStressAtParticle"][sel]).max() > 0.0
    if local:
        # among the selected rows: particles from outside the rank's creation window, whose Property and
        # Mass (compared above) no host table of the rank holds
        W = cfg.domain_max[axis] - cfg.domain_min[axis]
        X0 = r["s0/X"]
        found = []
        for k in range(world):
            lo, hi = solver.slab_window(cfg, k, world, axis, cuts)
            outside = ~(((X0[ids[k], axis] - lo) % W) < (hi - lo))
            found.append(int(outside.sum()))
        print("selected particles from outside the creation window:", found)
        assert found[0] > 0 and found[1] > 0
        # InitialPosition of such a row, and a box on InitialPosition over such a particle: MPH_ERR_ARG,
        # and the selection made before it stays
        codes = r["local/codes"]
        for k in range(world):
            if found[k]:
                assert codes[k].tolist() == [-1, -1, 1], (k, codes[k])


# ---- 6. files ------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", ["gate2d_sub", "channel3d"])
def test_selected_files_are_the_array_writers_of_the_gathered_subset(runs, run, tmp_path):
    r = runs(run)
    world = CASES[run]["world"]
    L = solver.load_library()
    for lab in ("some", "empty"):
        ids = np.sort(np.concatenate([r["file/%s/ids%d" % (lab, k)] for k in range(world)]))
        assert (len(ids) == 0) == (lab == "empty")
        arrs = [np.ascontiguousarray(r["g/" + k][ids]) for k in FRAME]
        if not len(ids):
            arrs = [np.zeros((1,) + a.shape[1:], a.dtype) for a in arrs]
        for ext, writer in (("vtk", L.mph_write_vtk_arrays), ("vtu", L.mph_write_vtu_arrays)):
            ref = str(tmp_path / ("ref_%s.%s" % (lab, ext)))
            solver._check(writer(ref.encode(), len(ids), *[a.ctypes.data for a in arrs]))
            assert r["file/%s/%s" % (lab, ext)].tobytes() == open(ref, "rb").read(), (run, lab, ext)
        assert ("POINTS %d " % len(ids)).encode() in r["file/%s/vtk" % lab].tobytes()
    if run == "gate2d_sub":
        T = setup(run)[2].property
        some = np.concatenate([r["file/some/ids%d" % k] for k in range(world)])
        assert set((T[some] >> 1).tolist()) == {0, 1, 2}     # fluid, structure and walls in the frame


# ---- 7. rules ------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", WHOLE)
def test_stale_selections_and_bad_arguments(runs, run):
    r = runs(run)
    world = CASES[run]["world"]
    assert r["early/codes"].tolist() == [[-1] * 3] * world            # before any mph_dist_select
    # the bad selections and the bad spec are refused, the earlier selection stays; after a set every
    # consumer refuses; after a new selection none does
    after_set = [-1] * 3 if run in select_ranks.SET_RUNS else []
    assert r["rules/codes"].tolist() == [[-1] * (len(BAD) + 1) + [1] + after_set + [0] * 3] * world
    assert r["stale/codes"].tolist() == [[-1] * 3] * world            # after a step


def test_every_slab_call_on_a_single_context_is_unsupported(tmp_path):
    cfg, parts = cases.get("dam2d").build()
    with MphSolver(cfg, parts) as s:
        s.select()
        calls = [s.dist_select, s.dist_selected_ids, lambda: s.dist_get_selected("Position"),
                 lambda: s.dist_selection_totals(partial=True), s.dist_selection_totals,
                 lambda: solver._check(s._L.mph_dist_gather_selected(s._h, 0, None, None, 0), s._h),
                 lambda: s.dist_write_vtk_selected(str(tmp_path / "unused.vtk")),
                 lambda: s.dist_write_vtu_selected(str(tmp_path / "unused.vtu"))]
        for f in calls:
            with pytest.raises(MphError) as e:
                f()
            assert e.value.code == -8
        assert len(s.selected_ids()) == parts.n     # the single context's selection is untouched


@pytest.mark.parametrize("run", ["gate2d_sub", "channel3d"])
def test_selections_do_not_change_the_run(runs, run):
    a, b = runs(run), runs(run, calls=False)
    assert a["time"].tobytes() == b["time"].tobytes()
    for name in STRUCT_FIELDS:
        assert a["f/" + name].tobytes() == b["f/" + name].tobytes(), name
