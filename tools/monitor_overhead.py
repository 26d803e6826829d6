#!/usr/bin/env python3
"""What the per-step monitors cost on D1M: same-box, same-process A/B.

One context; rounds alternate timed runs with monitors off and on (stride 1, 8 tracked particles,
8 probes in the water column).  Each run re-captures the step graphs (mph_monitor_configure drops
them), runs --warmup steps untimed and --steps steps timed as one mph_step call.  Prints one JSON
line: ms/step of every run and their medians, the overhead, and the monitor kernels' own times
from mph_profile_steps (direct launches, so 3-8 % above their graph-replay times).

  python tools/monitor_overhead.py [--case d1m] [--rounds 4] [--steps 40] [--warmup 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from particlemethod_fsi_amd import MphSolver, cases   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="d1m")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--stride", type=int, default=1)
    a = ap.parse_args()
    cfg, parts = cases.get(a.case).build()
    fluid = np.nonzero(parts.property < 2)[0]
    track = [int(i) for i in fluid[np.linspace(0, len(fluid) - 1, 8).astype(int)]]
    # probes inside the fluid: at eight of its particles, moved off the lattice
    probes = parts.position[fluid[np.linspace(0, len(fluid) - 1, 10).astype(int)[1:9]]] + 0.37 * cfg.particle_spacing
    runs = {"off": [], "on": []}
    with MphSolver(cfg, parts) as s:
        s.step(a.warmup)
        for _ in range(a.rounds):
            for mode in ("off", "on"):
                if mode == "on":
                    s.monitor(stride=a.stride, capacity=a.steps + a.warmup, track=track, probes=probes)
                else:
                    s.monitor(None)
                s.step(a.warmup)
                t0 = time.perf_counter()
                s.step(a.steps)
                runs[mode].append((time.perf_counter() - t0) * 1e3 / a.steps)
                if mode == "on":
                    rows, lost = s.monitor_read()
                    assert len(rows) == (a.steps + a.warmup) // a.stride and lost == 0
        s.monitor(stride=a.stride, capacity=8, track=track, probes=probes)
        prof = s.profile(8)
        n_probe = [float(v) for v in s.monitor_split(s.monitor_read()[0])[2][-1, :, 1]] if a.stride <= 8 else []
    off, on = float(np.median(runs["off"])), float(np.median(runs["on"]))
    mon = {k: v["avg_ms"] for k, v in prof.items() if k.startswith("monitor")}
    print(json.dumps({"case": a.case, "n": parts.n, "steps": a.steps, "rounds": a.rounds, "stride": a.stride,
                      "ms_per_step_off": runs["off"], "ms_per_step_on": runs["on"],
                      "median_off_ms": off, "median_on_ms": on, "overhead_ms": on - off,
                      "overhead_pct": 100.0 * (on - off) / off,
                      "monitor_kernels_ms": mon, "monitor_kernels_sum_ms": sum(mon.values()),
                      "gpu_busy_ms": prof["gpu_busy"]["avg_ms"], "probe_counts": n_probe}))


if __name__ == "__main__":
    main()
