#!/usr/bin/env python3
"""What lattice sampling and the elevation map cost on slab ranks (DESIGN.md sections 10.1 and 11).

CASE (default d1m) runs as --ranks slab ranks (default 2) that share one GPU over the host-staged
transport, each created from its own window (balanced cuts, as bench.py).  After --steps steps, for the
lattices of tools/sample_cost.py (the z mid-plane at 0.5 mm, the whole domain at 2 mm) and the map of
tools/gauge_cost.py (lines along gravity over the floor at 2 mm) and one of lines along the slab axis:

  partial_ms   every rank's partial call (mph_dist_sample_grid_partial / mph_dist_gauge_grid_partial:
               its kernels over the planes it owns, the copy of those planes to the host, the
               synchronise) from the host clock, the ranks taking turns so that the call has the device
               to itself: an upper bound of the rank's kernel time;
  collective_ms  one collective call on rank 0, wall clock, the gather through the process group
               included -- every rank's partial work runs at once here, on the one device.

The kernels' own times come from the profiler: run the script under `rocprofv3 --kernel-trace --stats`
and read the dist_sample_grid / dist_gauge_grid (k_sample_grid<.., true>, k_gauge_grid<.., true>) rows
of every rank's process.  The ranks share the device, so these are upper bounds of what a rank with a
GPU of its own would see.  Rank 0 prints one JSON line and, with --out, writes it there.

  python tools/dist_lattice_cost.py [--case d1m] [--ranks 2] [--axis 0] [--steps 8] [--rounds 3] [--out FILE]
"""
import argparse
import json
import math
import multiprocessing as mp
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def rank_main(rank, world, port, a, queue):
    import numpy as np
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from particlemethod_fsi_amd import MphSolver, cases
    from particlemethod_fsi_amd.dist import balanced_cuts, build_local, gloo_slab
    from sample_cost import lattices
    c = cases.get(a.case)
    cuts = balanced_cuts(c, world, a.axis)
    cfg, parts, ids, n_glob = build_local(c, rank, world, a.axis, cuts)
    g = [abs(v) for v in cfg.gravity[:cfg.dim]]
    up = g.index(max(g))
    lo, hi = cfg.domain_min, cfg.domain_max
    sp = 0.002
    maps = {}
    for name, ax in (("map_up", up), ("map_along_slabs", a.axis)):
        count = [1 if d == ax or d >= cfg.dim else int(math.ceil((hi[d] - lo[d]) / sp)) for d in range(3)]
        maps[name] = ([lo[d] + 0.37 * sp for d in range(3)], [sp] * 3, count, ax)
    calls = {}
    for name, (o, s_, n) in lattices(cfg).items():
        calls[name] = (lambda s, partial, o=o, s_=s_, n=n: s.dist_sample_grid(o, s_, n, partial=partial), list(n))
    for name, (o, s_, n, ax) in maps.items():
        calls[name] = (lambda s, partial, o=o, s_=s_, n=n, ax=ax: s.dist_gauge_grid(o, s_, n, axis=ax, partial=partial), list(n))
    out = {"rank": rank, "partial_ms": {k: [] for k in calls}, "collective_ms": {k: [] for k in calls}}
    with MphSolver(cfg, parts, device=0, slab=gloo_slab(rank, world, a.axis, ids=ids, n_glob=n_glob, cuts=cuts)) as s:
        del parts
        s.step(a.steps)
        out["owned"] = int(len(s.owned_ids()))
        for name, (call, n) in calls.items():
            call(s, True)     # untimed: allocation, code load
            call(s, False)
            for _ in range(a.rounds):
                for turn in range(world):   # the ranks take turns: a partial call has the device to itself
                    dist.barrier()
                    if turn == rank:
                        t0 = time.perf_counter()
                        got = call(s, True)
                        out["partial_ms"][name].append(1e3 * (time.perf_counter() - t0))
                dist.barrier()
                t0 = time.perf_counter()
                call(s, False)
                out["collective_ms"][name].append(1e3 * (time.perf_counter() - t0))
            if isinstance(got, tuple):
                out.setdefault("owned_points", {})[name] = int(got[1])
            else:
                out.setdefault("lines_computed", {})[name] = int((got[..., 0] >= 0).sum())
    everyone = [None] * world
    dist.all_gather_object(everyone, out)
    if rank == 0:
        med = {k: {"partial_ms_by_rank": [float(np.median(r["partial_ms"][k])) for r in everyone],
                   "collective_ms_rank0": float(np.median(everyone[0]["collective_ms"][k])), "count": calls[k][1]}
               for k in calls}
        queue.put({"case": a.case, "ranks": world, "axis": a.axis, "steps": a.steps, "rounds": a.rounds,
                   "note": "ranks share one device: upper bounds", "median": med, "per_rank": everyone})
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="d1m")
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--axis", type=int, default=0)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    queue = ctx.Queue()
    ps = [ctx.Process(target=rank_main, args=(r, a.ranks, port, a, queue)) for r in range(a.ranks)]
    for p in ps:
        p.start()
    res = None
    while res is None and any(p.is_alive() for p in ps):   # (a rank that died ends the wait)
        try:
            res = queue.get(timeout=1.0)
        except Exception:
            pass
    for p in ps:
        p.join()
    if res is None or any(p.exitcode != 0 for p in ps):
        sys.exit("rank exit codes %s" % [p.exitcode for p in ps])
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
