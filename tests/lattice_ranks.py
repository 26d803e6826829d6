"""Worker processes of the slab lattice tests (tests/test_gpu_dist_lattice.py; the cases are also what
tests/test_dist_lattice_abi.py checks on the CPU): one slab rank each on cuda:0 over the host-staged
transport, started with dist_worker.run_ranks.

CASES names, per case, the ranks, the cuts (dist_worker.make_cuts), the sampled lattices (origin,
spacing, count, radius) and the lattices of gauge lines (origin, spacing, count, axis).  A run is
described by a `spec` dictionary:

    case      a key of CASES
    early     True: before the first step every rank tries the partial calls and the bad lattices of
              BAD (no communication) -> "early" [rank, 2 + len(BAD)] status codes
    steps     steps before the calls: steps - 1, then Position and Velocity are gathered ("X", "V"),
              one more step, then PressureP ("P")
    calls     True: per sampled lattice i and class mask m of MASKS the collective result on rank 0
              ("s<i>m<m>/c"), the same call again ("s<i>m<m>/again"), every rank's partial array
              pre-filled with NaN ("s<i>m<m>/p" [rank, nz, ny, nx, 6]) and owned points
              ("s<i>m<m>/owned"); per line lattice i the collective map ("g<i>/c") and every rank's
              records ("g<i>/p" [rank, nz, ny, nx, 6])
    more      steps after the calls, then gather_field of `fields` ("f/<name>") and every rank's time

Rank 0 saves everything to out_path (.npz).
"""
from __future__ import annotations

import numpy as np

from dist_worker import _init, case_axis, make_cuts

DX = 0.001
H = 2.4137 * DX   # the sampled lattices' radius, as tests/test_gpu_sample.py
MASKS = (1, 7)

# tests/test_gpu_sample.py LATTICES["channel3d"] and ["dam2d"] (origin, spacing, count), kept equal to
# them by test_dist_lattice_abi.py: importing that module here would pull pytest into the workers
_CHANNEL3D = ((-0.0137, 0.00049, -0.0041), (0.00127, 0.00119, 0.00123), (33, 30, 12))
_DAM2D = ((-0.00871, 0.00053, 0.0), (0.00137, 0.00131, 0.001), (158, 90, 1))

CASES = {
    # slabs along z, cuts at 0.0108 and 0.0252.  The first lattice is test_gpu_sample's: its planes lie
    # in z = -0.0041 .. 0.0094, across the periodic face and short of the first cut, so rank 1 owns
    # none of it (0 owned points is legal); the second runs through all three slabs and once more
    # across the face, with planes within H of both cuts on both sides.
    "channel3d": dict(world=3, cuts="skew",
                      sample=[_CHANNEL3D + (H,),
                              ((-0.0021, 0.00053, 0.0013), (0.00137, 0.00171, 0.00241), (13, 11, 16), H)],
                      lines=[((-0.0013, 0.00211, 0.0), (0.00231, 0.00273, 0.0), (7, 8, 1), 2),
                             ((0.0, 0.0021, 0.0013), (0.0, 0.0031, 0.00241), (1, 5, 16), 0),
                             ((-0.0021, 0.0, 0.0013), (0.0029, 0.0, 0.00241), (6, 1, 16), 1)]),
    # slabs along x, the cut at 0.10: rank 1 holds walls alone
    "dam2d": dict(world=2, cuts=None,
                  sample=[_DAM2D + (H,)],
                  lines=[((0.0, 0.0011, 0.0), (0.0, 0.0047, 0.0), (1, 23, 1), 0),
                         ((-0.0113, 0.0, 0.0), (0.00371, 0.0, 0.0), (60, 1, 1), 1)]),
    # slabs along x.  The cut lies inside the bin [0.020, 0.021) of the lines along x, and inside the
    # column of particles that occupies it after 19 steps: the stream has carried the column from
    # x = 0.0195 to 0.02045, its lowest row, slowed by the floor, to 0.0204484 and the next one to
    # 0.0204499 (the CPU oracle's figures), so a line along x through both rows finds the bin occupied
    # on both ranks.  The lattices start in rank 1's slab, cross the periodic face at 0.04 and end in
    # rank 1's slab again (two runs of planes there); the line lattice is longer than the domain.
    "channel2d": dict(world=2, cuts=(0.0204492,),
                      sample=[((0.0313, 0.00047, 0.0), (0.00119, 0.00113, 0.001), (30, 17, 1), H)],
                      lines=[((0.0, 0.0007, 0.0), (0.0, 0.00113, 0.0), (1, 19, 1), 0),
                             ((0.0313, 0.0, 0.0), (0.00119, 0.0, 0.0), (37, 1, 1), 1)]),
}

# lattices that must be refused as on a single context (keyword arguments of dist_sample_grid, or of
# dist_gauge_grid where "axis" is given): MPH_ERR_ARG
BAD = [dict(origin=(0.0, 0.0, 0.0), spacing=(DX, DX, DX), count=(0, 2, 1)),
       dict(origin=(0.0, 0.0, 0.0), spacing=(DX, -DX, DX), count=(2, 2, 1)),
       dict(origin=(0.0, float("nan"), 0.0), spacing=(DX, DX, DX), count=(2, 2, 1)),
       dict(origin=(0.0, 0.0, 0.0), spacing=(DX, DX, DX), count=(2, 2, 1), radius=2.7 * DX),
       dict(origin=(0.0, 0.0, 0.0), spacing=(DX, DX, DX), count=(2, 2, 1), classes=8),
       dict(origin=(0.0, 0.0, 0.0), spacing=(1e-9, 1e-9, 1e-9), count=(1 << 13, 1 << 12, 1)),
       dict(origin=(0.0, 0.0, 0.0), spacing=(DX, DX, DX), count=(2, 2, 1), axis=0),     # count[axis] != 1
       dict(origin=(0.0, 0.0, 0.0), spacing=(DX, DX, DX), count=(2, 1, 1), axis=5),
       dict(origin=(0.0, 0.0, 0.0), spacing=(DX, DX, DX), count=(2, 1, 1), axis=1, radius=-DX)]


def lattice_worker(rank, world, port, spec, out_path):
    dist = _init(rank, world, port)
    from particlemethod_fsi_amd import MphSolver, cases
    from particlemethod_fsi_amd.dist import gather_field, gloo_slab
    from particlemethod_fsi_amd.solver import MphError
    case, axis = case_axis(spec["case"])
    C = CASES[spec["case"]]
    assert world == C["world"]
    c = cases.get(case)
    cuts = make_cuts(c, world, axis, C["cuts"])
    cfg, parts = c.build()

    def everyone(x):
        out = [None] * world
        dist.all_gather_object(out, x)
        return out

    def code(f, **kw):
        try:
            f(**kw)
            return 0
        except MphError as e:
            return e.code

    res = {}
    with MphSolver(cfg, parts, device=0, slab=gloo_slab(rank, world, axis, cuts=cuts)) as s:
        if spec.get("early"):
            o, sp, n, h = C["sample"][0]
            lo, lsp, ln, la = C["lines"][0]
            codes = [code(s.dist_sample_grid, origin=o, spacing=sp, count=n, radius=h, partial=True),
                     code(s.dist_gauge_grid, origin=lo, spacing=lsp, count=ln, axis=la, partial=True)]
            s.step(1)
            for kw in BAD:
                codes.append(code(s.dist_gauge_grid if "axis" in kw else s.dist_sample_grid, partial=True, **kw))
            res["early"] = np.array(everyone(codes), np.int64)
        else:
            s.step(spec["steps"] - 1)
            res["X"], res["V"] = gather_field(s, "Position"), gather_field(s, "Velocity")
            s.step(1)
            res["P"] = gather_field(s, "PressureP")
            if spec.get("calls"):
                for i, (o, sp, n, h) in enumerate(C["sample"]):
                    for m in MASKS:
                        key = "s%dm%d/" % (i, m)
                        got = s.dist_sample_grid(o, sp, n, radius=h, classes=m)
                        again = s.dist_sample_grid(o, sp, n, radius=h, classes=m)
                        part, owned = s.dist_sample_grid(o, sp, n, radius=h, classes=m, partial=True)
                        parts_ = everyone(part)
                        counts = everyone(owned)
                        if rank == 0:
                            res[key + "c"], res[key + "again"] = got, again
                            res[key + "p"], res[key + "owned"] = np.stack(parts_), np.array(counts, np.int64)
                        else:
                            assert got is None and again is None
                for i, (o, sp, n, a) in enumerate(C["lines"]):
                    got = s.dist_gauge_grid(o, sp, n, axis=a)
                    recs = everyone(s.dist_gauge_grid(o, sp, n, axis=a, partial=True))
                    if rank == 0:
                        res["g%d/c" % i], res["g%d/p" % i] = got, np.stack(recs)
            s.step(spec["more"])
            for f in spec["fields"]:
                res["f/" + f] = gather_field(s, f)
            res["time"] = np.array(everyone(float(s.time)))
    if rank == 0:
        np.savez(out_path, **res)
    dist.barrier()
    dist.destroy_process_group()


def driver_worker(rank, world, port, files, checkpoints, lattice, out_path):
    """The case as the driver reads it (files: data file, grid file, dim, module) in `world` equal slabs
    along x: at every checkpoint (cumulative step count) the collective dist_sample_grid(**lattice);
    rank 0 saves the results ("c<steps>") to out_path (.npz)."""
    dist = _init(rank, world, port)
    from particlemethod_fsi_amd import MphSolver
    from particlemethod_fsi_amd.dist import gloo_slab
    from particlemethod_fsi_amd.solver import read_case_files
    cfg, parts = read_case_files(*files)
    res, done = {}, 0
    with MphSolver(cfg, parts, device=0, slab=gloo_slab(rank, world, 0)) as s:
        for k in checkpoints:
            s.step(k - done)
            done = k
            got = s.dist_sample_grid(**lattice)
            if rank == 0:
                res["c%d" % k] = got
    if rank == 0:
        np.savez(out_path, **res)
    dist.barrier()
    dist.destroy_process_group()
