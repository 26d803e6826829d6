"""Worker processes of the slab-monitor tests (tests/test_gpu_dist_monitor.py,
test_gpu_dist_monitor_driver.py): one slab rank each on cuda:0 over the host-staged transport, started
with dist_worker.run_ranks.  A run is described by a `spec` dictionary:

    case      case_axis's argument; cuts: make_cuts's mode; local: slab-local creation; files: the
              case read from the driver's input files instead (data, grid, dim, module)
    monitor   keyword arguments of MphSolver.dist_monitor (None: the monitors stay off)
    bad       configurations that must be refused, tried first: their status codes -> "bad"
    schedule  a list of entries {steps, read, fields, before, off, profile}, in order: `off` turns the
              monitors off, `before` gathers Position ("b<i>/Position"), `profile` runs that many steps
              under mph_profile_steps (rank 0's monitor kernels as "name:launches" -> "prof<i>"), then
              `steps` steps in one step() call,
              then the read -- "c": the collective dist_monitor_read, rank 0's samples -> "c<i>";
              "p": every rank's dist_monitor_read_partial -> "p<i>" [rank, k, width] -- with every
              rank's lost count ("lost<i>"), then gather_field of `fields` ("f<i>/<name>"), every
              rank's time ("t<i>") and the owner of every particle ("owner<i>")

Rank 0 saves everything to out_path (.npz).
"""
from __future__ import annotations

import numpy as np

from dist_worker import _init, case_axis, make_cuts


def monitor_worker(rank, world, port, spec, out_path):
    dist = _init(rank, world, port)
    from particlemethod_fsi_amd import MphSolver, cases
    from particlemethod_fsi_amd.dist import build_local, gather_field, gloo_slab
    from particlemethod_fsi_amd.solver import MphError
    case, axis = case_axis(spec["case"])
    c = cases.get(case)
    cuts = make_cuts(c, world, axis, spec.get("cuts"))
    if spec.get("local"):
        cfg, parts, ids, n_glob = build_local(c, rank, world, axis, cuts)
        slab = gloo_slab(rank, world, axis, ids=ids, n_glob=n_glob, cuts=cuts)
    else:
        cfg, parts = c.build()
        if spec.get("files"):   # the case as the driver reads it: (data file, grid file, dim, module)
            from particlemethod_fsi_amd.solver import read_case_files
            cfg, parts = read_case_files(*spec["files"])
        slab = gloo_slab(rank, world, axis, cuts=cuts)

    def everyone(x):
        out = [None] * world
        dist.all_gather_object(out, x)
        return out

    res = {}
    with MphSolver(cfg, parts, device=0, slab=slab) as s:
        codes = []
        for kw in spec.get("bad", ()):
            try:
                s.dist_monitor(**kw)
                codes.append(0)
            except MphError as e:
                codes.append(e.code)
        res["bad"] = np.array(everyone(codes), np.int64).reshape(world, -1)
        if spec.get("monitor") is not None:
            s.dist_monitor(**spec["monitor"])
        for i, e in enumerate(spec["schedule"]):
            if e.get("off"):
                s.dist_monitor(None)
            if e.get("before"):
                res["b%d/Position" % i] = gather_field(s, "Position")
            if e.get("profile"):
                prof = s.profile(e["profile"])
                res["prof%d" % i] = np.array(sorted("%s:%d" % (k, v["launches"]) for k, v in prof.items()
                                                    if k.startswith("monitor")))
            s.step(e["steps"])
            if e.get("read") == "c":
                rows, lost = s.dist_monitor_read()
                res["c%d" % i] = rows
                res["lost%d" % i] = np.array(everyone(lost))
            elif e.get("read") == "p":
                rows, lost = s.dist_monitor_read_partial()
                res["p%d" % i] = np.stack(everyone(rows))
                res["lost%d" % i] = np.array(everyone(lost))
            for f in e.get("fields", ()):
                res["f%d/%s" % (i, f)] = gather_field(s, f)
            res["t%d" % i] = np.array(everyone(float(s.time)))
            owner = np.full(s.n, -1, np.int32)
            for r, ids_r in enumerate(everyone(s.owned_ids())):
                owner[ids_r] = r
            res["owner%d" % i] = owner
    if rank == 0:
        np.savez(out_path, **res)
    dist.barrier()
    dist.destroy_process_group()
