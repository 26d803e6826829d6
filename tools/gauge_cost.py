#!/usr/bin/env python3
"""What the free-surface gauges cost on D1M: same-box, same-process A/B.

One context.  Rounds alternate timed runs with monitors off, with the monitors of
tools/monitor_overhead.py (stride 1, 8 tracked particles, 8 probes), and with 8 gauges beside them
along gravity's axis and along a horizontal one (the two cell forms of gauge_line).  Each run
re-captures the step graphs, runs --warmup steps untimed and --steps steps timed as one mph_step
call.  Then the monitor kernels' own times from mph_profile_steps for both gauge sets, and the
elevation map: a lattice of lines along gravity over the whole floor at --map-spacing, the whole
call timed with one line and with four lines per block (MPH_GAUGE_GRID_WAVES), beside the
mph_sample_grid volume whose WSUM column a host-side reduction would need.  Prints one JSON line.

  python tools/gauge_cost.py [--case d1m] [--rounds 4] [--steps 40] [--warmup 8] [--map-only]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from particlemethod_fsi_amd import MphSolver, cases   # noqa: E402
from particlemethod_fsi_amd.solver import GAUGE_CHANNELS as C   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="d1m")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--map-spacing", type=float, default=0.002)
    ap.add_argument("--map-only", action="store_true")
    a = ap.parse_args()
    cfg, parts = cases.get(a.case).build()
    fluid = np.nonzero(parts.property < 2)[0]
    track = [int(i) for i in fluid[np.linspace(0, len(fluid) - 1, 8).astype(int)]]
    pts = parts.position[fluid[np.linspace(0, len(fluid) - 1, 10).astype(int)[1:9]]] + 0.37 * cfg.particle_spacing
    g = [abs(v) for v in cfg.gravity[:cfg.dim]]
    up = g.index(max(g))
    flat = 0 if up != 0 else 1
    modes = {"off": None, "monitors": dict(), "gauges_up": dict(gauges=pts, gauge_axis=up),
             "gauges_flat": dict(gauges=pts, gauge_axis=flat)}
    runs = {m: [] for m in modes}
    out = {"case": a.case, "n": parts.n, "steps": a.steps, "rounds": a.rounds, "axis_up": up, "axis_flat": flat}
    with MphSolver(cfg, parts) as s:
        s.step(a.warmup)
        if not a.map_only:
            for _ in range(a.rounds):
                for mode, kw in modes.items():
                    if kw is None:
                        s.monitor(None)
                    else:
                        s.monitor(stride=1, capacity=a.steps + a.warmup, track=track, probes=pts, **kw)
                    s.step(a.warmup)
                    t0 = time.perf_counter()
                    s.step(a.steps)
                    runs[mode].append((time.perf_counter() - t0) * 1e3 / a.steps)
            out["ms_per_step"] = runs
            out["median_ms"] = {m: float(np.median(v)) for m, v in runs.items()}
            for mode in ("gauges_up", "gauges_flat"):
                s.monitor(stride=1, capacity=8, track=track, probes=pts, **modes[mode])
                prof = s.profile(8)
                out["kernels_ms_" + mode] = {k: v["avg_ms"] for k, v in prof.items() if k.startswith("monitor")}
                out["counts_" + mode] = [float(v) for v in s.monitor_gauges(s.monitor_read()[0])[-1, :, C["COUNT"]]]
            s.monitor(None)
            s.step(8)
        # the map: lines along gravity through every node of the floor's lattice
        lo, hi = cfg.domain_min, cfg.domain_max
        count = [1 if d == up or d >= cfg.dim else int(math.ceil((hi[d] - lo[d]) / a.map_spacing)) for d in range(3)]
        origin = [lo[d] + 0.37 * a.map_spacing for d in range(3)]
        spacing = [a.map_spacing] * 3
        calls = {"1": [], "4": []}
        for _ in range(5):
            for w in calls:
                os.environ["MPH_GAUGE_GRID_WAVES"] = w
                t0 = time.perf_counter()
                m = s.gauge_grid(origin, spacing, count, axis=up)
                calls[w].append((time.perf_counter() - t0) * 1e3)
        del os.environ["MPH_GAUGE_GRID_WAVES"]
        vcount = [int(math.ceil((hi[d] - lo[d]) / a.map_spacing)) if d < cfg.dim else 1 for d in range(3)]
        vol = []
        buf = None
        for _ in range(5):
            t0 = time.perf_counter()
            buf = s.sample_grid(origin, spacing, vcount, out=buf)
            vol.append((time.perf_counter() - t0) * 1e3)
        out["map"] = {"count": count, "lines": int(np.prod(count)), "wet_lines": int((m[..., C["COUNT"]] > 0).sum()),
                      "bytes": int(m.nbytes), "call_ms_one_line_per_block": calls["1"], "call_ms_four_lines_per_block": calls["4"],
                      "volume_count": vcount, "volume_bytes": int(buf.nbytes), "volume_call_ms": vol}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
