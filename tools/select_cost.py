#!/usr/bin/env python3
"""What a particle selection costs on D1M, beside the whole-array way to the same numbers (DESIGN.md
section 13).

One context, 8 steps in.  Two selections: (a) the fluid in a slab 10 dx thick across z, (b) all
walls.  Five rounds alternate, per selection, the selected path -- mph_select, get_selected of
Position, Velocity and PressureP, selection_totals, each timed on its own -- with the whole-array
path of the library before selections: three mph_get and a numpy mask on the host.  Medians, the
per-kernel times of one profiled pass (mph_select_profile), one JSON line.

  python tools/select_cost.py [--case d1m] [--rounds 5] [--steps 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from particlemethod_fsi_amd import MphSolver, cases   # noqa: E402
from particlemethod_fsi_amd.solver import make_selection   # noqa: E402

NAMES = ("Position", "Velocity", "PressureP")


def _ms(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="d1m")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    a = ap.parse_args()
    cfg, parts = cases.get(a.case).build()
    dx = cfg.particle_spacing
    lo, hi = list(cfg.domain_min), list(cfg.domain_max)
    zmid = 0.5 * (lo[2] + hi[2])
    sels = {"fluid_slab_10dx": make_selection(types=(0, 1), box=((lo[0], lo[1], zmid - 5 * dx), (hi[0], hi[1], zmid + 5 * dx))),
            "walls": make_selection(types=(4, 5))}
    out = {"case": a.case, "n": parts.n, "steps": a.steps, "rounds": a.rounds, "selections": {}}
    with MphSolver(cfg, parts) as s:
        s.step(a.steps)
        T = s.get("Property")
        runs = {k: {"select_ms": [], "get_selected_3_ms": [], "totals_ms": [], "whole_get_3_ms": [], "whole_mask_ms": []}
                for k in sels}
        for _ in range(a.rounds):
            for name, sel in sels.items():
                r = runs[name]
                t, cnt = _ms(lambda: s.select(spec=sel))
                r["select_ms"].append(t)
                t, got = _ms(lambda: [s.get_selected(k) for k in NAMES])
                r["get_selected_3_ms"].append(t)
                t, tot = _ms(s.selection_totals)
                r["totals_ms"].append(t)
                t, whole = _ms(lambda: [s.get(k) for k in NAMES])
                r["whole_get_3_ms"].append(t)

                def mask():
                    m = ((sel.type_mask >> T) & 1).astype(bool)
                    if sel.box:
                        X = whole[0]
                        for d in range(3):
                            m &= (X[:, d] >= sel.lo[d]) & (X[:, d] < sel.hi[d])
                    return [w[m] for w in whole]
                t, ref = _ms(mask)
                r["whole_mask_ms"].append(t)
                assert all(np.array_equal(x, y) for x, y in zip(got, ref)) and tot["COUNT"] == cnt == len(ref[0])
        for name, sel in sels.items():
            r = runs[name]
            med = {k: float(np.median(v)) for k, v in r.items()}
            med["selected_path_ms"] = med["select_ms"] + med["get_selected_3_ms"]
            med["whole_path_ms"] = med["whole_get_3_ms"] + med["whole_mask_ms"]
            kern = {}
            for k, ms in s.select_profile(sel):
                kern.setdefault(k, []).append(ms)
            out["selections"][name] = {"count": int(s.select(spec=sel)), "runs": r, "median": med,
                                       "kernels_ms": {k: [round(v, 5) for v in vs] for k, vs in kern.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
