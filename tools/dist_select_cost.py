#!/usr/bin/env python3
"""What a particle selection costs on slab ranks, beside the whole-array way to the same numbers
(the slab subsection).

D1M as two slab ranks along z on one GPU, 8 steps in.  The ranks are two threads of this process over
the host-staged transport (each rank's messages go to the other through a queue), so one profiler run
sees both.  The two selections of tools/select_cost.py: (a) the fluid in a slab 10 dx thick across z --
the cut runs through its middle -- and (b) all walls.  Five rounds alternate, per selection and timed on
rank 0 between barriers,

  selected   dist_select; dist_gather_selected of Position, Velocity and PressureP; dist_selection_totals
  local      the same without transport: dist_select, dist_get_selected of the three, the partial totals
             (the slower rank's time: the kernels, the two waits of a select and the copies of the rows)
  whole      the path it replaces: per field, every rank's get()[owned_ids()] merged on rank 0
             (dist.gather_field's work), then the numpy mask and the three indexed copies

and, for the fluid alone, write_vtk of the whole frame against dist_write_vtk_selected.  Medians, one
JSON line.  selected - local is what the transport and rank 0's merge cost.

  python tools/dist_select_cost.py [--case d1m] [--rounds 5] [--steps 8] [--tmp DIR]
"""
import argparse
import json
import os
import queue
import sys
import tempfile
import threading
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from particlemethod_fsi_amd import MphSolver, cases   # noqa: E402
from particlemethod_fsi_amd.solver import FIELDS, Slab, make_selection   # noqa: E402

NAMES = ("Position", "Velocity", "PressureP")
WORLD, AXIS = 2, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="d1m")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--tmp", default=None)
    a = ap.parse_args()
    tmp = a.tmp or tempfile.mkdtemp()
    cfg, parts = cases.get(a.case).build()
    dx = cfg.particle_spacing
    lo, hi = list(cfg.domain_min), list(cfg.domain_max)
    zmid = 0.5 * (lo[2] + hi[2])
    sels = {"fluid_slab_10dx": make_selection(types=(0, 1), box=((lo[0], lo[1], zmid - 5 * dx), (hi[0], hi[1], zmid + 5 * dx))),
            "walls": make_selection(types=(4, 5))}
    T = parts.property
    box = [queue.Queue(), queue.Queue()]          # the exchange's messages, per receiving rank
    up = queue.Queue()                            # rank 1's owned rows on their way to rank 0 (the whole path)
    gate = threading.Barrier(WORLD)
    keys = ("selected_ms", "select_ms", "gather_3_ms", "totals_ms", "local_ms", "whole_gather_3_ms", "whole_mask_ms")
    runs = {k: {m: [] for m in keys} for k in sels}
    files = {"write_vtk_ms": [], "dist_write_vtk_selected_ms": []}
    counts, local = {}, [{k: [] for k in sels} for _ in range(WORLD)]
    errors = []

    def timed(f):
        """f() on every rank between two barriers -> (milliseconds of the slowest rank's span, result)."""
        gate.wait()
        t0 = time.perf_counter()
        r = f()
        gate.wait()
        return (time.perf_counter() - t0) * 1e3, r

    def rank(r):
        def exchange(sl, sr, rl, rr):
            box[1 - r].put((bytes(sl), bytes(sr)))
            x, y = box[r].get(timeout=600)
            rr[:len(x)] = x
            rl[:len(y)] = y

        def whole_gather(s, name):
            ids = s.owned_ids()
            vals = s.get(name)[ids]
            if r:
                up.put((ids, vals))
                return None
            fid, w, dt = FIELDS[name]
            out = np.zeros((s.n,) if w == 1 else (s.n, 3), dt)
            out[ids] = vals
            i2, v2 = up.get(timeout=600)
            out[i2] = v2
            return out

        try:
            with MphSolver(cfg, parts, slab=Slab(r, WORLD, AXIS, exchange=exchange)) as s:
                s.step(a.steps)
                for rnd in range(a.rounds + 1):       # round 0 carries the first use of kernels and buffers
                    for name, sel in sels.items():
                        t_sel, cnt = timed(lambda: s.dist_select(spec=sel))
                        t_g, got = timed(lambda: [s.dist_gather_selected(k) for k in NAMES])
                        t_t, tot = timed(s.dist_selection_totals)
                        t0 = time.perf_counter()
                        s.dist_select(spec=sel)
                        for k in NAMES:
                            s.dist_get_selected(k)
                        s.dist_selection_totals(partial=True)
                        mine = (time.perf_counter() - t0) * 1e3
                        t_w, whole = timed(lambda: [whole_gather(s, k) for k in NAMES])
                        if r == 0:
                            t0 = time.perf_counter()
                            m = ((sel.type_mask >> T) & 1).astype(bool)
                            if sel.box:
                                for d in range(3):
                                    m &= (whole[0][:, d] >= sel.lo[d]) & (whole[0][:, d] < sel.hi[d])
                            ref = [w[m] for w in whole]
                            t_m = (time.perf_counter() - t0) * 1e3
                            assert all(np.array_equal(g[1], x) for g, x in zip(got, ref)) and tot["COUNT"] == len(ref[0])
                            counts[name] = int(tot["COUNT"])
                        if rnd:
                            local[r][name].append(mine)
                            if r == 0:
                                for k, v in zip(keys, (t_sel + t_g + t_t, t_sel, t_g, t_t, None, t_w, t_m)):
                                    if v is not None:
                                        runs[name][k].append(v)
                    t_v, _ = timed(lambda: s.write_vtk(os.path.join(tmp, "whole.vtk")))
                    s.dist_select(types=(0, 1))
                    t_s, _ = timed(lambda: s.dist_write_vtk_selected(os.path.join(tmp, "fluid.vtk")))
                    if rnd and r == 0:
                        files["write_vtk_ms"].append(t_v)
                        files["dist_write_vtk_selected_ms"].append(t_s)
        except Exception as e:   # noqa: BLE001 -- reported below; the other rank is released
            errors.append(repr(e))
            gate.abort()

    t = threading.Thread(target=rank, args=(1,))
    t.start()
    rank(0)
    t.join()
    if errors:
        sys.exit("dist_select_cost: " + "; ".join(errors))
    out = {"case": a.case, "n": parts.n, "ranks": WORLD, "steps": a.steps, "rounds": a.rounds, "selections": {},
           "fluid_count": int((T < 2).sum())}
    for name in sels:
        runs[name]["local_ms"] = [max(x, y) for x, y in zip(local[0][name], local[1][name])]
        med = {k: float(np.median(v)) for k, v in runs[name].items()}
        med["whole_path_ms"] = med["whole_gather_3_ms"] + med["whole_mask_ms"]
        med["transport_and_merge_ms"] = med["selected_ms"] - med["local_ms"]
        out["selections"][name] = {"count": counts[name], "runs": runs[name], "median": med}
    out["files"] = {"runs": files, "median": {k: float(np.median(v)) for k, v in files.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
