"""Generate the golden vectors of tests/golden/ from the REFERENCE solver itself.

Runs oracle/_ref/libmphref_<dim>_<module>.so (the reference's src/main.cpp compiled from
/root/reference by oracle/Makefile, driven by oracle/ref_harness.inc) on the cases of
particlemethod_fsi_amd/cases.py and stores snapshots as compressed .npz fixtures:

  <case>.npz   (for the cases of PARTS also <case>.1.npz ..., save_parts)
               s0/*  after the reference's initialisation (main.cpp:564-570)
               s<k>/* after k time steps (main.cpp:597-686 each)
               scalars (the 36 derived constants), meta (json)
  dam2d_output.vtk.gz / dam2d_000.prof.gz   the reference writers' output at step 0

Entries the reference leaves uninitialised (malloc'd and never written -- DensityA and
GravityCenter of structure particles, DivergenceP/PressureA before the first step) are stored
as NaN and skipped by the tests.  Each case runs in its own process because the reference
keeps its state in file-scope globals.

Usage:  python tests/golden/make_golden.py [case ...]
"""
from __future__ import annotations

import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FULL = ["Position", "Velocity", "Force", "Acceleration", "GravityCenter", "PressureP", "PressureA",
        "DensityA", "VolStrainP", "DivergenceP", "NeighborCount"]
SHORT = ["Position", "Velocity", "PressureP", "NeighborCount"]
SOLID = ["DeformGradient", "Strain", "Stress"]
INIT = ["NeighborCount", "DensityA", "VolStrainP", "GravityCenter", "InitialStructureNeighborCount",
        "Normalizer", "LambdaLames", "MuLames"]

PLAN = {  # case -> steps (cumulative) to snapshot; the first is the full-field snapshot
    "dam2d": [1, 10, 100, 1000],
    "gate2d": [1, 10, 100],
    "bar2d": [1, 10, 100],
    "box3d": [1, 10],
    "gate3d": [1, 10],
    "dam2d_st": [1, 10, 100],
    "box3d_st": [1, 10],
    "gate2d_sub": [1, 10, 100],
    "gate3d_sub": [1, 10, 50],
    "rolling2d": [1, 10, 100],
    "rolling3d": [1, 10, 30],
    "movwall2d": [1, 10, 100],
    "movwall3d": [1, 10, 30],
    "turek2d": [1, 10, 100],
    "gate2d_rolling1": [1, 10, 100],
    "hydro2d": [1, 10, 100],
    "bar2d_ivp": [1, 10, 100],
    # off-lattice (cases.py jitter): the 3-D search and sums away from lattice distances
    "box3d_jit": [1, 10, 100],
    "gate3d_jit": [1, 10, 100],
    # mixed materials (cases.MIX_GOLDEN_CASES): two fluids, two structures, two wall types
    "mix3d": [1, 10],      # (20 as well would pass the size of the largest golden, box3d_jit)
    "mix3d_st": [1, 10],
    "mix2d": [1, 10, 100],
    "mix2d_st": [1, 10, 100],
}


def run_case(name: str):
    from oracle_bindings import RefSolver, write_case_files
    from particlemethod_fsi_amd import cases
    c = cases.get(name)
    tmp = tempfile.mkdtemp(prefix="golden_")
    dp, gp = write_case_files(cases.data_text(c.data()), c.grid_text(), tmp)
    ref = RefSolver(c.dim, c.ref_variant, dp, gp)
    ref.init()
    for fn in c.init_calls:   # e.g. the commented setInitialVelocityProfile() of main.cpp:571
        ref.call(fn)
    prop = ref.get("Property")
    solid = (prop >= 2) & (prop < 4)
    out = {"scalars": ref.scalars(), "Property": prop}

    def snap(tag, names, stepped):
        for f in names:
            a = ref.get(f)
            if f in ("DensityA", "GravityCenter"):
                a = a.astype(np.float64)
                a[solid] = np.nan
            if not stepped and f in ("DivergenceP", "PressureA"):
                a = np.full_like(a, np.nan)
            if f in SOLID or f in ("Normalizer", "LambdaLames", "MuLames"):
                a = a[solid]
            out["%s/%s" % (tag, f)] = a

    snap("s0", INIT, False)
    if name == "dam2d":
        ref.write_vtk(os.path.join(tmp, "output.vtk"))
        ref.write_prof(os.path.join(tmp, "dam000.prof"))
        for src, dst in (("output.vtk", "dam2d_output.vtk.gz"), ("dam000.prof", "dam2d_000.prof.gz")):
            raw = open(os.path.join(tmp, src), "rb").read()
            with gzip.GzipFile(os.path.join(HERE, dst), "wb", mtime=0) as fh:
                fh.write(raw)
            out["sha256/" + src] = np.frombuffer(hashlib.sha256(raw).digest(), np.uint8)
    done = 0
    for k, s in enumerate(PLAN[name]):
        ref.step(s - done)
        done = s
        names = FULL if k == 0 else SHORT
        if solid.any():
            names = names + SOLID
        snap("s%d" % s, names, True)
        if k == 0:
            # the VTK-step diagnostic (main.cpp:672-673) on the first stepped state; it writes
            # only the two virial arrays, so the run continues unchanged
            ref.call("calculateVirialStressAtParticle")
            snap("s%d" % s, ["VirialStressAtParticle", "VirialPressureAtParticle"], True)
        if k == 0 and name in ("dam2d", "box3d_jit", "mix3d"):
            rows = [np.sort(ref.neighbors(i)) for i in range(ref.n)]
            out["s%d/nbr_offsets" % s] = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
            # mix3d: 16-bit indices (n < 65536), a quarter of the fixture otherwise
            out["s%d/nbr_ids" % s] = np.concatenate(rows).astype(np.uint16 if name == "mix3d" else np.int32)
    meta = {"case": name, "n": int(ref.n), "dim": c.dim, "module": c.module, "steps": PLAN[name],
            "time": ref.time, "generator": "tests/golden/make_golden.py",
            "init_calls": list(c.init_calls),
            "reference": "oracle/_ref/libmphref_%dd_%s.so" % (c.dim, c.ref_variant)}
    if name in PARTS:
        paths = save_parts(os.path.join(HERE, name), out, meta)
    else:
        out["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
        paths = [os.path.join(HERE, name + ".npz")]
        np.savez_compressed(paths[0], **out)
    print(name, "n=%d" % ref.n, "->", [os.path.getsize(p) for p in paths], "bytes")


# The mixed-material fixtures: off the lattice with all six types, so their arrays hardly compress.
# Each stays within the size of the largest single golden (box3d_jit.npz, 2,699,447 bytes) in all, its
# plan trimmed to that, and is written as files of at most PART_LIMIT bytes each.  Every other case is
# one .npz as before.
PARTS = ("mix3d", "mix3d_st", "mix2d", "mix2d_st")
PART_LIMIT = 1000000


def save_parts(base: str, out: dict, meta: dict):
    """<base>.npz, followed by <base>.1.npz, <base>.2.npz ... where one file would pass PART_LIMIT:
    whole arrays, first fit in the order of `out`, meta["parts"] the number of files
    (golden_utils.Golden reads them back as one mapping)."""
    bins, fill = [{}], [4096]   # room for meta in the first
    for k, v in out.items():
        size = len(zlib.compress(np.ascontiguousarray(v).tobytes(), 6)) + 256
        b = next((b for b in range(len(bins)) if fill[b] + size <= PART_LIMIT), len(bins))
        if b == len(bins):
            bins.append({})
            fill.append(0)
        bins[b][k] = v
        fill[b] += size
    meta["parts"] = len(bins)
    bins[0]["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    paths = [base + (".%d" % b if b else "") + ".npz" for b in range(len(bins))]
    for path, arrays in zip(paths, bins):
        np.savez_compressed(path, **arrays)
    return paths


def main(argv):
    names = argv or list(PLAN)
    if len(names) == 1:
        run_case(names[0])
        return
    for nm in names:   # one process per case (the reference uses globals)
        subprocess.run([sys.executable, __file__, nm], check=True, stderr=subprocess.DEVNULL)


if __name__ == "__main__":
    main(sys.argv[1:])
