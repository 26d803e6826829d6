#!/usr/bin/env python3
"""What lattice sampling costs on D1M, beside the route it replaces.

One context, stepped --steps steps; rounds alternate, per lattice, one mph_sample_grid call (its
kernel timed from HIP events through mph_sample_grid_timed, the whole call -- kernel, copy of the
result to the host, synchronise -- from the host clock) and the three mph_get calls a user would
grid on the host instead (Position, Velocity, PressureP).  Lattices: (a) the z mid-plane at 0.5 mm
over the whole x-y domain, 440 x 800 x 1 on D1M; (b) the whole domain at 2 mm, 110 x 200 x 60.
Prints one JSON line with every round's times and their medians.

  python tools/sample_cost.py [--case d1m] [--rounds 5] [--steps 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from particlemethod_fsi_amd import MphSolver, cases   # noqa: E402
from particlemethod_fsi_amd.solver import SAMPLE_CHANNELS as C   # noqa: E402


def lattices(cfg):
    lo = [cfg.domain_min[d] for d in range(3)]
    hi = [cfg.domain_max[d] for d in range(3)]
    out = {}
    s = 0.0005   # (a): points at the centres of 0.5 mm squares, in the plane half way up z
    out["slice"] = ((lo[0] + 0.5 * s, lo[1] + 0.5 * s, 0.5 * (lo[2] + hi[2])), (s, s, s),
                    (int(round((hi[0] - lo[0]) / s)), int(round((hi[1] - lo[1]) / s)), 1))
    s = 0.002    # (b): points at the centres of 2 mm cubes
    out["volume"] = (tuple(lo[d] + 0.5 * s for d in range(3)), (s, s, s),
                     tuple(int(round((hi[d] - lo[d]) / s)) for d in range(3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="d1m")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    a = ap.parse_args()
    cfg, parts = cases.get(a.case).build()
    lat = lattices(cfg)
    runs = {name: {"kernel_ms": [], "call_ms": []} for name in lat}
    gets = []
    facts, bufs = {}, {}
    with MphSolver(cfg, parts) as s:
        s.step(a.steps)
        for name, (o, sp, n) in lat.items():   # untimed: allocation, code load, the bits
            bufs[name] = np.zeros((n[2], n[1], n[0], len(C)))   # one host buffer per lattice, reused
            cnt = s.sample_grid(o, sp, n, out=bufs[name])[..., C["COUNT"]]
            facts[name] = {"count": list(n), "points": int(cnt.size), "non_empty": int((cnt > 0).sum()),
                           "pairs": int(cnt.sum())}
        for f in ("Position", "Velocity", "PressureP"):
            s.get(f)
        for _ in range(a.rounds):
            for name, (o, sp, n) in lat.items():
                t0 = time.perf_counter()
                _, ms, kname = s.sample_grid(o, sp, n, timed=True, out=bufs[name])
                runs[name]["call_ms"].append((time.perf_counter() - t0) * 1e3)
                runs[name]["kernel_ms"].append(ms)
                assert kname == "sample_grid"
            t0 = time.perf_counter()
            for f in ("Position", "Velocity", "PressureP"):
                s.get(f)
            gets.append((time.perf_counter() - t0) * 1e3)
    res = {"case": a.case, "n": parts.n, "steps": a.steps, "rounds": a.rounds, "lattices": facts, "runs": runs,
           "three_gets_ms": gets, "median_three_gets_ms": float(np.median(gets)), "median": {}}
    for name in lat:
        k, c = float(np.median(runs[name]["kernel_ms"])), float(np.median(runs[name]["call_ms"]))
        res["median"][name] = {"kernel_ms": k, "call_ms": c, "points_per_s": facts[name]["points"] / (c * 1e-3),
                               "call_over_three_gets": c / res["median_three_gets_ms"]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
