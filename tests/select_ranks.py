"""Worker processes of the slab selection tests (tests/test_gpu_dist_select.py; the cases are also what
tests/test_dist_select_abi.py checks on the CPU): one slab rank each on cuda:0 over the host-staged
transport, started with dist_worker.run_ranks.

CASES names, per run, the case, the ranks, the cuts (dist_worker.make_cuts) and whether the ranks are
created from their own windows (slab-local creation).  selections() builds a run's selections from the
gathered state, the same on every rank and in the CPU model check.  A run is described by a `spec`:

    run       a key of CASES
    calls     True: the selection calls at creation ("s0/...") and after `split` ("s1/...")
    split     the step calls before the second block, (20,) or (7, 13)
    more      steps after it, then gather_field of `fields` ("f/<name>") and every rank's time
    tmp       a directory for the files rank 0 writes

What a block records per selection `lab` (rank r): "<tag>/<lab>/ids<r>", the rank's Position rows
"<tag>/<lab>/pos<r>", the partial totals of all ranks "<tag>/<lab>/tp" [world, 24], the collective
totals "<tag>/<lab>/tc" and the same call again "<tag>/<lab>/tc2"; and per block the gathered state
"<tag>/X", "/V", "/F" and the owners "<tag>/owner".  Rank 0 saves everything to out_path (.npz).
"""
from __future__ import annotations

import os

import numpy as np

from dist_worker import _init, case_axis, make_cuts

STEPS = 20
CENTER = (0.0123, -0.0045, 0.0067)   # off the origin: the torque is not the origin's

CASES = {
    # slabs along z (periodic), cuts at 0.0132 and 0.0228
    "channel3d": dict(case="channel3d", world=3, cuts="skew", local=False, steps=STEPS),
    # The same flow, every rank created from its own window (slab-local creation).  A rank's window is
    # its slab and 13.2 dx to either side (mph_slab_window), and the fastest fluid moves 0.05 dx a step:
    # no rank can own a particle from outside its window before step 264, and with equal or skew cuts
    # every window of this 36 dx domain is the whole domain.  So ranks 0 and 1 get the narrowest slabs
    # the library accepts (7.3 dx; their windows leave out 2.3 dx of the domain each) and the run goes
    # on to step 300, when both own fluid particles they have no static inputs for (the CPU oracle: 286
    # and 254; tests/test_dist_select_abi.py).
    "channel3d_local": dict(case="channel3d", world=3, cuts=(0.0073, 0.0146), local=True, steps=300),
    # slabs along x, the cut at 0.10: rank 1 holds walls alone
    "dam2d": dict(case="dam2d", world=2, cuts=None, local=False, steps=STEPS),
    "gate2d_sub": dict(case="gate2d_sub", world=2, cuts=None, local=False, steps=STEPS),
    # the left wall's columns cross the cut (tests/motion_runs.py)
    "movwall2d_slab": dict(case="movwall2d_slab", world=2, cuts=(-0.00048,), local=False, steps=STEPS),
}

# the fields mph_get takes from the host's static inputs
STATIC = ("InitialPosition", "Mass", "Kappa", "Lambda", "Mu", "Property", "InitialStructureNeighborCount",
          "Normalizer", "LambdaLames", "MuLames")
# what a slab-local rank reads of a particle it has no static inputs for: the sorted device arrays, and
# the fields that follow from the device's type
LOCAL_FIELDS = ("Position", "Velocity", "Force", "Acceleration", "PressureP", "NeighborCount", "Property", "Mass",
                "Lambda", "Mu")
GATHERED = ("Position", "Force", "NeighborCount", "Stress", "Property")
FRAME = ("Property", "Position", "InitialPosition", "Velocity", "Acceleration", "Force", "Stress", "Strain",
         "InitialStructureNeighborCount", "NeighborCount")

# the runs whose rules block also calls mph_set (the others are compared with runs without any call)
SET_RUNS = ("dam2d", "movwall2d_slab")
BAD = (dict(every=0), dict(every=2, phase=2), dict(phase=-1), dict(box=((1.0, 0.0, 0.0), (0.0, 1.0, 1.0))))


def setup(run):
    """(case object, cfg, particles of the whole problem, slab axis, cuts) of a run of CASES."""
    from particlemethod_fsi_amd import cases
    C = CASES[run]
    name, axis = case_axis(C["case"])
    c = cases.get(name)
    cfg, parts = c.build()
    return c, cfg, parts, axis, make_cuts(c, C["world"], axis, C["cuts"])


def box_on_particles(X, dim, a=0.3, b=0.7):
    """A box whose bounds are coordinates of actual particles: some sit exactly on lo, some on hi."""
    lo, hi = [-1.0] * 3, [1.0] * 3
    for d in range(dim):
        v = np.sort(X[:, d])
        lo[d], hi[d] = float(v[int(a * (len(v) - 1))]), float(v[int(b * (len(v) - 1))])
    return lo, hi


def selections(cfg, parts, axis, world, cuts, X):
    """[(label, MphSelection)] of a run, from the gathered Position X.  In this order: "fluid" and then
    the disjoint "walls"; "every"; "onpart", a box on fluid particles' own coordinates; "cut", 3 dx to
    either side of the first cut; "face", the whole slab axis and the middle of the next axis -- members
    on every rank, on both sides of every cut and of the periodic face; "body", the structure by
    InitialPosition (cases with one); "none"; "all"."""
    from particlemethod_fsi_amd import solver
    from particlemethod_fsi_amd.solver import make_selection
    dim, dx, T = cfg.dim, cfg.particle_spacing, parts.property
    wide_lo, wide_hi = [-1.0e3] * 3, [1.0e3] * 3
    cut = solver.slab_bounds(cfg, 0, world, axis, cuts)[1]
    at_cut = (list(wide_lo), list(wide_hi))
    at_cut[0][axis], at_cut[1][axis] = cut - 3.0 * dx, cut + 3.0 * dx
    other = (axis + 1) % dim
    face = (list(wide_lo), list(wide_hi))
    v = np.sort(X[T < 2, other])
    face[0][other], face[1][other] = float(v[len(v) // 3]), float(v[2 * len(v) // 3])
    out = [("fluid", make_selection(types=(0, 1))), ("walls", make_selection(types=(4, 5))),
           ("every", make_selection(every=3, phase=2)),
           ("onpart", make_selection(box=box_on_particles(X[T < 2], dim))),
           ("cut", make_selection(box=at_cut)), ("face", make_selection(box=face))]
    body = (T == 2) | (T == 3)
    if body.any():
        X0 = parts.initial_position
        lo, hi = list(X0[body].min(axis=0) - 0.5 * dx), list(X0[body].max(axis=0) + 0.5 * dx)
        out.append(("body", make_selection(box=(lo, hi), on="initial")))
    out += [("none", make_selection(box=((0.0,) * 3, (0.0,) * 3))), ("all", make_selection())]
    return out


def mask_of(sel, dim, T, X, X0):
    """The selection rule (sel_accepts) in numpy."""
    n = len(T)
    m = np.ones(n, bool)
    if sel.type_mask:
        m &= ((sel.type_mask >> T) & 1).astype(bool)
    m &= (np.arange(n) % sel.every) == sel.phase
    if sel.box:
        Y = X if sel.box == 1 else X0
        for d in range(dim):
            m &= (Y[:, d] >= sel.lo[d]) & (Y[:, d] < sel.hi[d])
    return m


def _code(f, *a, **kw):
    from particlemethod_fsi_amd.solver import MphError
    try:
        f(*a, **kw)
        return 0
    except MphError as e:
        return e.code


def select_worker(rank, world, port, spec, out_path):
    dist = _init(rank, world, port)
    from particlemethod_fsi_amd import MphSolver
    from particlemethod_fsi_amd.dist import build_local, gather_field, gloo_slab
    from particlemethod_fsi_amd.solver import FIELDS
    C = CASES[spec["run"]]
    assert world == C["world"]
    c, cfg, whole, axis, cuts = setup(spec["run"])
    if C["local"]:
        lcfg, parts, ids, n_glob = build_local(c, rank, world, axis, cuts)
        slab = gloo_slab(rank, world, axis, ids=ids, n_glob=n_glob, cuts=cuts)
    else:
        lcfg, parts = cfg, whole
        slab = gloo_slab(rank, world, axis, cuts=cuts)

    def everyone(x):
        out = [None] * world
        dist.all_gather_object(out, x)
        return out

    res = {}

    def consumers(s):
        return [s.dist_selected_ids, lambda: s.dist_get_selected("Position"),
                lambda: s.dist_selection_totals(CENTER, partial=True)]

    def block(s, tag):
        X = gather_field(s, "Position")
        res[tag + "/X"], res[tag + "/V"], res[tag + "/F"] = X, gather_field(s, "Velocity"), gather_field(s, "Force")
        owner = np.full(s.n, -1, np.int32)
        for r, o in enumerate(everyone(s.owned_ids())):
            owner[o] = r
        res[tag + "/owner"] = owner
        for lab, sel in selections(cfg, whole, axis, world, cuts, X):
            key = "%s/%s/" % (tag, lab)
            if C["local"] and sel.box == 2:
                continue
            cnt = s.dist_select(spec=sel)
            ids = s.dist_selected_ids()
            assert cnt == len(ids)
            pos = s.dist_get_selected("Position")
            tp = s.dist_selection_totals(CENTER, partial=True)
            tc = s.dist_selection_totals(CENTER)
            tc2 = s.dist_selection_totals(CENTER)
            for r, (i, p, t) in enumerate(everyone((ids, pos, tp))):
                res[key + "ids%d" % r], res[key + "pos%d" % r] = i, p
                res.setdefault(key + "tp", []).append(t)
            res[key + "tp"] = np.stack(res[key + "tp"])
            if rank == 0:
                res[key + "tc"] = np.array(list(tc.values()))
                res[key + "tc2"] = np.array(list(tc2.values()))
            else:
                assert tc is None and tc2 is None

    def fields_block(s):
        """Every field of a mixed selection, rank by rank and gathered; the frames; the rules."""
        s.compute_virial()
        names = LOCAL_FIELDS if C["local"] else tuple(FIELDS)
        # the references: mph_get of every rank merged (a slab-local rank's mph_get has no static field
        # of a particle from outside its window: those come from the run with whole inputs)
        for name in names:
            if not (C["local"] and name in STATIC):
                res["g/" + name] = gather_field(s, name)
        cnt = s.dist_select(every=5, phase=3)
        ids = s.dist_selected_ids()
        for r, i in enumerate(everyone(ids)):
            res["fld/ids%d" % r] = i
        for name in names:
            rows = s.dist_get_selected(name)
            assert len(rows) == cnt
            for r, v in enumerate(everyone(rows)):
                res["fld/%s/%d" % (name, r)] = v
        for name in GATHERED if not C["local"] else ("Position", "Force", "NeighborCount", "Property"):
            got = s.dist_gather_selected(name)
            if rank == 0:
                res["cg/%s/ids" % name], res["cg/%s/rows" % name] = got
            else:
                assert got is None
        # the collective gather where a rank may have selected nothing (dam2d: rank 1 holds no fluid)
        s.dist_select(types=(0, 1))
        got = s.dist_gather_selected("Velocity")
        if rank == 0:
            res["cgf/ids"], res["cgf/rows"] = got
        s.dist_select(every=5, phase=3)
        if C["local"]:
            # InitialPosition of a selection with a particle from outside the creation window, and a box
            # on InitialPosition over such a particle: refused, and the selection made before stays
            before = s.dist_selected_ids()
            codes = [_code(s.dist_get_selected, "InitialPosition"),
                     _code(s.dist_select, box=((-1.0e3,) * 3, (1.0e3,) * 3), on="initial")]
            kept = bool(np.array_equal(s.dist_selected_ids(), before))
            res["local/codes"] = np.array(everyone(codes + [int(kept)]), np.int64)
            return
        # the frames of a selection, and of an empty one
        for lab, kw in (("some", dict(types=(1, 2, 3, 4), every=3, phase=1)), ("empty", dict(box=((0.0,) * 3, (0.0,) * 3)))):
            s.dist_select(**kw)
            for r, i in enumerate(everyone(s.dist_selected_ids())):
                res["file/%s/ids%d" % (lab, r)] = i
            for ext, write in (("vtk", s.dist_write_vtk_selected), ("vtu", s.dist_write_vtu_selected)):
                path = os.path.join(spec["tmp"], "%s_%s.%s" % (spec["run"], lab, ext))
                write(path)
                if rank == 0:
                    res["file/%s/%s" % (lab, ext)] = np.frombuffer(open(path, "rb").read(), np.uint8)
        # bad selections are refused and leave the earlier selection usable
        s.dist_select(types=(0, 1))
        before = s.dist_selected_ids()
        codes = [_code(s.dist_select, **bad) for bad in BAD]
        codes.append(_code(s.dist_select, spec="types=0;colour=1"))
        codes.append(int(np.array_equal(s.dist_selected_ids(), before)))
        # stale after a set (and, below, after a step)
        if spec["run"] in SET_RUNS:
            s.set("Velocity", s.get("Velocity"))
            codes += [_code(f) for f in consumers(s)]
        s.dist_select()
        codes += [_code(f) for f in consumers(s)]
        res["rules/codes"] = np.array(everyone(codes), np.int64)

    with MphSolver(lcfg, parts, device=0, slab=slab) as s:
        if spec["calls"]:
            res["early/codes"] = np.array(everyone([_code(f) for f in consumers(s)]), np.int64)   # no selection yet
            block(s, "s0")
        for k in spec["split"]:
            s.step(k)
        if spec["calls"]:
            block(s, "s1")
            fields_block(s)
        else:
            # the state and the partial totals alone (the batch-shape comparison)
            X = gather_field(s, "Position")
            res["s1/X"], res["s1/V"], res["s1/F"] = X, gather_field(s, "Velocity"), gather_field(s, "Force")
            for lab, sel in selections(cfg, whole, axis, world, cuts, X):
                if lab in ("fluid", "walls", "onpart"):
                    s.dist_select(spec=sel)
                    res["s1/%s/tp" % lab] = np.stack(everyone(s.dist_selection_totals(CENTER, partial=True)))
        s.step(spec["more"])
        if spec["calls"] and not C["local"]:
            res["stale/codes"] = np.array(everyone([_code(f) for f in consumers(s)]), np.int64)
        for f in spec["fields"]:
            res["f/" + f] = gather_field(s, f)
        res["time"] = np.array(everyone(float(s.time)))
    if rank == 0:
        np.savez(out_path, **res)
    dist.barrier()
    dist.destroy_process_group()


# ---- the scan's edges ----------------------------------------------------------------------------

EDGE_NX, EDGE_NY = 90, 47            # 4,230 fluid particles: not a multiple of 4 (the tail of sel_flags4)
EDGE_TARGETS = (0, 1, 1023, 1024, 1025)


def edge_case():
    """EDGE_NX x EDGE_NY fluid particles (2-D, dx = 1 mm) alone in a periodic box, as
    tests/test_gpu_select.py _fluid_block; two equal slabs along x cut the block in two."""
    from particlemethod_fsi_amd import cases
    from particlemethod_fsi_amd.mphio import Cuboid
    nx, ny = EDGE_NX, EDGE_NY
    return cases.Case("sel_edge", 2, "dam", 0.001, (-0.01, 0.0, 0.0), (0.001 * nx + 0.02, 0.001 * ny + 0.03, 0.001),
                      [Cuboid(1, (0.0, 0.01, 0.0), (0.001 * nx, 0.01 + 0.001 * ny, 0.001), 0.001, (0.03, -0.02, 0.0))])


def edge_boxes(X, owner):
    """{(rank, target): box}: a Position box holding exactly `target` particles, all of them rank's --
    a columns by b rows from the lower corner of the rank's part of the block, its upper bounds the
    coordinates of the next column and row (a particle on hi is out)."""
    col = np.rint((X[:, 0] - X[:, 0].min()) / 0.001).astype(int)
    row = np.rint((X[:, 1] - X[:, 1].min()) / 0.001).astype(int)
    out = {}
    for r in (0, 1):
        cols = np.unique(col[owner == r])
        assert (np.diff(cols) == 1).all()
        c0, nc = int(cols[0]), len(cols)
        for t in EDGE_TARGETS:
            if t == 0:
                out[(r, t)] = ((0.0,) * 3, (0.0,) * 3)
                continue
            a = next(a for a in range(min(nc - 1, t), 0, -1) if t % a == 0 and t // a < EDGE_NY)
            b = t // a
            lo = (float(X[col == c0, 0].min()), float(X[:, 1].min()), -1.0)
            hi = (float(X[col == c0 + a, 0].min()), float(X[row == b, 1].min()), 1.0)
            out[(r, t)] = (lo, hi)
    return out


def edge_worker(rank, world, port, out_path):
    dist = _init(rank, world, port)
    from particlemethod_fsi_amd import MphSolver
    from particlemethod_fsi_amd.dist import gather_field, gloo_slab
    cfg, parts = edge_case().build()

    def everyone(x):
        out = [None] * world
        dist.all_gather_object(out, x)
        return out

    res = {}
    with MphSolver(cfg, parts, device=0, slab=gloo_slab(rank, world, 0)) as s:
        for steps in (0, 2):
            if steps:
                s.step(steps)
            tag = "s%d" % steps
            G = {name: gather_field(s, name) for name in ("Position", "Velocity", "Force", "PressureP", "NeighborCount", "Mass")}
            owner = np.full(s.n, -1, np.int32)
            for r, o in enumerate(everyone(s.owned_ids())):
                owner[o] = r
            res[tag + "/owner"] = owner
            for name, v in G.items():
                res["%s/g/%s" % (tag, name)] = v
            for (r0, t), box in sorted(edge_boxes(G["Position"], owner).items()):
                key = "%s/r%dt%d/" % (tag, r0, t)
                res[key + "box"] = np.array(box)
                cnt = s.dist_select(box=box)
                ids = s.dist_selected_ids()
                assert cnt == len(ids)
                rows = {name: s.dist_get_selected(name) for name in G}
                tp = s.dist_selection_totals(CENTER, partial=True)
                for r, (i, v, t_) in enumerate(everyone((ids, rows, tp))):
                    res[key + "ids%d" % r], res[key + "tp%d" % r] = i, t_
                    for name in v:
                        res["%s%s%d" % (key, name, r)] = v[name]
    if rank == 0:
        np.savez(out_path, **res)
    dist.barrier()
    dist.destroy_process_group()


def driver_worker(rank, world, port, files, checkpoints, loads_steps, loads_spec, center, out_path):
    """The case as the driver reads it (files: data file, grid file, dim, module) in `world` equal slabs
    along x, stepped as the driver steps it: at every step of loads_steps the time and the collective
    totals of loads_spec about `center` ("t<step>"), at every checkpoint the collective gather of the
    fluid's rows of every field of a frame ("ids<step>", "g<step>/<name>")."""
    dist = _init(rank, world, port)
    from particlemethod_fsi_amd import MphSolver
    from particlemethod_fsi_amd.dist import gloo_slab
    from particlemethod_fsi_amd.solver import read_case_files
    cfg, parts = read_case_files(*files)
    res, done = {}, 0
    with MphSolver(cfg, parts, device=0, slab=gloo_slab(rank, world, 0)) as s:
        for k in sorted(set(checkpoints) | set(loads_steps)):
            s.step(k - done)
            done = k
            if k in loads_steps:
                s.dist_select(spec=loads_spec)
                t = s.dist_selection_totals(center)
                if rank == 0:
                    res["t%d" % k] = np.array([float(s.time)] + list(t.values()))
            if k in checkpoints:
                s.compute_virial()
                s.dist_select(spec="types=0,1")
                for name in FRAME:
                    got = s.dist_gather_selected(name)
                    if rank == 0:
                        res["ids%d" % k], res["g%d/%s" % (k, name)] = got
    if rank == 0:
        np.savez(out_path, **res)
    dist.barrier()
    dist.destroy_process_group()
