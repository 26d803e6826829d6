#!/usr/bin/env python3
"""What the slab monitors cost: the three kernels' own times on a slab rank, and the collective read.

CASE (default d1m) runs as --ranks slab ranks (default 2) that share one GPU over the host-staged
transport, each created from its own window (balanced cuts, as bench.py).  With 8 tracked particles and
8 probes in the water column at stride 1, every rank profiles --steps steps (mph_profile_steps: direct
launches, HIP events around every kernel) and reports the monitor kernels' average ms per launch; then
the ranks take --samples more steps and time one dist_monitor_read() of that many samples (wall clock,
gather through the process group included).  The ranks share the device, so only the kernels' own times
mean anything, not the step rate.  Rank 0 prints one JSON line.

  python tools/dist_monitor_cost.py [--case d1m] [--ranks 2] [--axis 0] [--steps 8] [--samples 64]
"""
import argparse
import json
import multiprocessing as mp
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rank_main(rank, world, port, a, queue):
    import numpy as np
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from particlemethod_fsi_amd import MphSolver, cases
    from particlemethod_fsi_amd.dist import balanced_cuts, build_local, gloo_slab
    c = cases.get(a.case)
    cuts = balanced_cuts(c, world, a.axis)
    cfg, parts, ids, n_glob = build_local(c, rank, world, a.axis, cuts)
    # the same configuration on every rank: eight fluid particles of the whole problem by index, and
    # probes at lattice sites of the column, moved off the lattice
    _, full = c.build()
    fluid = np.nonzero(full.property < 2)[0]
    pick = fluid[np.linspace(0, len(fluid) - 1, 10).astype(int)[1:9]]
    track = [int(i) for i in pick]
    probes = full.position[pick] + 0.37 * cfg.particle_spacing
    del full
    with MphSolver(cfg, parts, device=0, slab=gloo_slab(rank, world, a.axis, ids=ids, n_glob=n_glob, cuts=cuts)) as s:
        s.step(4)
        s.dist_monitor(stride=1, capacity=a.samples, track=track, probes=probes)
        prof = s.profile(a.steps)
        kernels = {k: v for k, v in prof.items() if k.startswith("monitor")}
        s.dist_monitor_read()
        s.step(a.samples)
        s.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        rows, lost = s.dist_monitor_read()
        read_ms = 1e3 * (time.perf_counter() - t0)
        out = {"rank": rank, "owned": int(len(s.owned_ids())), "kernels_ms": kernels, "read_ms": read_ms,
               "samples": int(rows.shape[0]), "lost": lost}
    everyone = [None] * world
    dist.all_gather_object(everyone, out)
    if rank == 0:
        queue.put({"case": a.case, "ranks": world, "profiled_steps": a.steps, "per_rank": everyone})
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="d1m")
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--axis", type=int, default=0)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--samples", type=int, default=64)
    a = ap.parse_args()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    queue = ctx.Queue()
    ps = [ctx.Process(target=rank_main, args=(r, a.ranks, port, a, queue)) for r in range(a.ranks)]
    for p in ps:
        p.start()
    for p in ps:
        p.join()
    if any(p.exitcode != 0 for p in ps):
        sys.exit("rank exit codes %s" % [p.exitcode for p in ps])
    print(json.dumps(queue.get(timeout=10)))


if __name__ == "__main__":
    main()
