#!/usr/bin/env python3
"""Bitwise A/B of two builds (e.g. the round-6 cleanup against e6081fe): run each case for a
few steps with the library of MPH_GPU_LIB and save every per-particle field, or compare two saved
runs.  `run` also saves, whatever the cases, what the point stencil of the monitors' probes and of the
lattice sampling produces (POINT_RUNS): the monitor ring of 11 steps with probes and tracked particles,
and a lattice slice and a small volume.

  MPH_GPU_LIB=.../libmph_gpu.so python tools/lib_bitwise.py run OUT.npz [cases...]
  MPH_GPU_LIB=.../libmph_gpu.so MPH_SLAB_OVERLAP=1 python tools/lib_bitwise.py slab OUT.npz
  python tools/lib_bitwise.py compare A.npz B.npz        (exit 1 on any difference)

`slab` saves the slab decomposition's results instead (SLAB_RUNS: 2-4 host-staged ranks on the one GPU).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FIELDS = ["Position", "Velocity", "PressureP", "PressureA", "NeighborCount", "Force", "Acceleration",
          "DensityA", "VolStrainP", "DivergenceP", "GravityCenter", "DeformGradient", "Strain", "Stress"]


# case -> (probes, tracked ids, lattices (origin, spacing, count, classes)): the probes of
# tests/test_gpu_monitor.py test_probes_in_a_tank and test_probe_across_the_periodic_face, a 2-D set,
# and per case a lattice slice and a small volume (seam3d's across the periodic y face)
POINT_RUNS = {
    "box3d_jit": ([(0.00613, 0.01021, 0.00587), (0.00587, 0.01957, 0.00611), (0.00071, 0.00813, 0.00493),
                   (0.0353, 0.0421, 0.0061)], [3, 0, 1500, 3],
                  [((0.0005, 0.0035, 0.006), (0.0007, 0.0007, 0.0007), (20, 30, 1), 0),
                   ((0.0005, 0.0035, 0.0005), (0.0011, 0.0013, 0.0012), (12, 10, 9), 7)]),
    "seam3d": ([(0.01531, 0.03931, 0.01013)], [7],
               [((0.014, 0.0, 0.0101), (0.0009, 0.0008, 0.0009), (7, 50, 1), 0),
                ((0.014, 0.036, 0.009), (0.0009, 0.0009, 0.0009), (6, 8, 5), 0)]),
    "dam2d": ([(0.0213, 0.0417, 0.0), (0.0007, 0.0513, 0.0), (0.1, 0.3, 0.0)], [11, 2000],
              [((0.001, 0.004, 0.0), (0.0013, 0.0017, 0.001), (40, 60, 1), 0),
               ((-0.002, 0.001, 0.0), (0.0009, 0.0009, 0.001), (9, 7, 1), 7)]),
}


# slab runs: (case, ranks, slab-local creation, fields); the fields of tests/test_gpu_dist.py
SLAB_FIELDS = ["Position", "Velocity", "PressureP", "NeighborCount", "Force", "VolStrainP", "DivergenceP",
               "DensityA", "GravityCenter", "PressureA", "Acceleration"]
SLAB_STRUCT_FIELDS = SLAB_FIELDS + ["DeformGradient", "Strain", "Stress"]
SLAB_RUNS = [("channel3d", 3, True, SLAB_FIELDS), ("channel2d", 4, False, SLAB_FIELDS),
             ("bar2d", 3, False, SLAB_STRUCT_FIELDS), ("gate2d_sub", 2, True, SLAB_STRUCT_FIELDS)]


def run_points(res):
    from particlemethod_fsi_amd import MphSolver, cases
    for name, (probes, track, lattices) in POINT_RUNS.items():
        cfg, parts = cases.get(name).build()
        with MphSolver(cfg, parts) as s:
            s.monitor(stride=1, capacity=16, track=track, probes=probes)
            s.step(3)
            s.step(8)
            rows, lost = s.monitor_read()
            assert rows.shape[0] == 11 and lost == 0, (rows.shape, lost)
            res["%s/monitor_ring" % name] = rows
            for k, (origin, spacing, count, classes) in enumerate(lattices):
                res["%s/sample_grid%d" % (name, k)] = s.sample_grid(origin, spacing, count, classes=classes)


def run(out, names):
    from particlemethod_fsi_amd import MphSolver, cases
    res = {}
    run_points(res)
    for name in names:
        cfg, parts = cases.get(name).build()
        with MphSolver(cfg, parts) as s:
            s.step(3)
            s.step(8)
            for f in FIELDS:
                res["%s/%s" % (name, f)] = s.get(f)
    np.savez(out, **res)


def run_slab(out):
    """Every SLAB_RUNS case as host-staged ranks sharing the GPU (tests/dist_worker.py), the gathered
    arrays of all checkpoints in one file.  Force MPH_SLAB_OVERLAP to 1 or 0: unset, the ranks time
    their exchanges and two builds may choose differently."""
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dist_worker
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case, world, local, fields in SLAB_RUNS:
            path = os.path.join(tmp, "%s.npz" % case)
            dist_worker.run_ranks(dist_worker.gpu_worker, world, case, [1, 5, 20], fields, path, local, None,
                                  timeout=300)
            with np.load(path) as z:
                for k in z.files:
                    res["slab/%s/%s" % (case, k)] = z[k]
    np.savez(out, **res)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = 0
    assert sorted(A.files) == sorted(B.files), "the two runs saved different arrays"
    keys = [k for k in sorted(A.files) if not k.endswith("/overlap")]   # the slab ranks' pass-B mode report: timings
    for k in keys:
        same = np.array_equal(A[k], B[k])
        if not same:
            bad += 1
            print("DIFF", k, float(np.max(np.abs(A[k].astype(float) - B[k].astype(float)))))
    print("compared %d arrays: %s" % (len(keys),"bit-identical" if not bad else "%d differ" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3:] or ["box3d", "box3d_st", "gate3d", "seam3d", "d1m"])
    elif sys.argv[1] == "slab":
        run_slab(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
