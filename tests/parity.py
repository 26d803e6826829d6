"""The parity bounds of the GPU path: the one place where the numbers live.

Every GPU test that compares FP64 fields against the reference's golden vectors, the CPU oracle or
another GPU run takes its bound from `bound` (or `golden_bound`) and asserts through `assert_close`
(or `assert_close_golden`).  NeighborCount and the other integer fields are always bit-exact.
tests/test_parity_bounds.py pins the numbers of this module on the CPU.
"""
from __future__ import annotations

import os

import numpy as np

# absolute floors: the roundoff level of each quantity (P ~ Kappa * VolStrainP, so one ulp of
# VolStrainP ~ 1e-16 is 1e-12 Pa; at step 1 the reference's P is itself pure roundoff ~4e-11)
# Elastic tensors: at rest F = I + O(ulp), so Strain is pure roundoff (~1e-16) and Stress ~
# (lambda + 2 mu) * 1e-15 ~ 1e-10 Pa until gravity loads the solid.
FLOOR = {"PressureP": 1e-9, "PressureA": 1e-9, "Force": 1e-15, "Acceleration": 1e-12,
         "VolStrainP": 1e-13, "DivergenceP": 1e-12, "DensityA": 1e-13, "GravityCenter": 1e-16,
         "DeformGradient": 1e-13, "Strain": 1e-13, "Stress": 1e-8,
         "VirialStressAtParticle": 1e-9, "VirialPressureAtParticle": 1e-9}

# Relative bounds, as a fraction of the largest magnitude of the reference field.
# One step, the goldens and the bar2d long run (where the reference does not amplify roundoff,
# tests/golden/ulp_bar2d_longrun.json): the GPU sums in its own order with FMA; reassociation only.
REL_ONE_STEP = 1e-9
# Fluid against the oracle (or against another decomposition of the same run) over several steps:
# SURVEY 8c measured the chaotic growth of such differences.
REL_STEPS = 1e-8
# A case that holds elastic particles (types 2/3): the solid runs at dt*c/dx = 0.95 (ElasticDt 1e-4,
# c = 9.5 m/s); near the stability limit reassociation differences grow ~10x per few steps, and the
# fluid next to it inherits them.
REL_ELASTIC = 1e-7
# DivergenceP in such a case -- a difference of nearly equal sums: the growth one GPU context itself
# shows against the oracle on bar3d (tools/slab_diag.py: 8.9e-9 / 9.7e-8 / 7.4e-7 at steps 10 / 20 /
# 30).
REL_ELASTIC_DIVP = 1e-6


def elastic_rel(field: str) -> float:
    """Relative bound of `field` over tens of steps of a case with elastic particles."""
    return REL_ELASTIC_DIVP if field == "DivergenceP" else REL_ELASTIC


def bound(field: str, rel: float, scale: float) -> float:
    """THE bound rule: positions 1e-12 m, velocities 1e-9 m/s, any other float field `rel` of
    `scale` (the largest magnitude of the reference) plus the field's roundoff floor."""
    if field == "Position":
        return 1e-12
    if field == "Velocity":
        return 1e-9
    return rel * scale + FLOOR.get(field, 1e-12)


def golden_bound(field: str, step: int, scale: float) -> float:
    """The bound against the reference's golden vectors after `step` steps: up to 100 steps the
    rule above at REL_ONE_STEP, PressureP past the first step at 1e-8; at 1000 steps positions
    1e-10 m (dx = 1e-3 m), velocities 1e-7 m/s and PressureP 1e-6."""
    long = step >= 1000
    if long and field in ("Position", "Velocity"):
        return {"Position": 1e-10, "Velocity": 1e-7}[field]
    if field == "PressureP" and step > 1:
        return bound(field, 1e-6 if long else 1e-8, scale)
    return bound(field, REL_ONE_STEP, scale)


def _assert_within(field, got, ref, bound_of_scale, rows, scale, extra, context):
    if rows is not None:
        got, ref = got[rows], ref[rows]
    if ref.dtype.kind != "f":
        if not np.array_equal(got, ref):
            raise AssertionError("%s %s: %d mismatches" % (context, field, int((got != ref).sum())))
        return 0
    # no nanmax, no NaN mask: a NaN on either side makes `err <= t` false
    err = float(np.max(np.abs(got - ref))) if ref.size else 0.0
    if scale is None:
        scale = float(np.max(np.abs(ref))) if ref.size else 0.0
    t = max(bound_of_scale(scale), extra)
    if not err <= t:
        raise AssertionError("%s %s: max|diff| %.3e > bound %.3e" % (context, field, err, t))
    return err


def assert_close(field, got, ref, rel, *, rows=None, scale=None, extra=0.0, context=()):
    """Assert `got` within bound(field, rel, scale) of `ref`; integer fields bit-exact.  Returns
    the measured max|got - ref| (0 for integers).

    rows:    a mask or index applied to both arrays first.  No row left is error 0, scale 0.
    scale:   None scales by the compared rows, max|ref[rows]|; a number is taken as given (a
             rank's rows against a bound scaled by the whole reference array).
    extra:   a further absolute allowance, combined by max (the reference's own measured
             sensitivity, test_gpu_fullsize).
    context: goes into the failure message in front of the field, error and bound."""
    return _assert_within(field, got, ref, lambda s: bound(field, rel, s), rows, scale, extra, context)


def assert_close_golden(field, got, ref, step, *, context=()):
    """assert_close under golden_bound; the NaN slots of the golden `ref` (entries the reference
    leaves uninitialised) are skipped -- those of `ref` only, a NaN from the device fails."""
    rows = ~np.isnan(ref) if ref.dtype.kind == "f" else None
    return _assert_within(field, got, ref, lambda s: golden_bound(field, step, s), rows, None, 0.0,
                          context + (step,))


def compare(g, solver, step: int):
    """Every field the golden file of case `g` stores at `step` against the solver's."""
    from golden_utils import restrict
    report = {}
    if g.has(step, "VirialStressAtParticle"):
        solver.compute_virial()   # the reference's VTK-step diagnostic, main.cpp:672-673
    for f in g.fields(step):
        ref = g.get(step, f)
        err = assert_close_golden(f, restrict(g, f, solver.get(f)), ref, step, context=(g.case,))
        if ref.dtype.kind == "f":
            report[f] = err
    return report


def oracle_rel(parts) -> float:
    """Relative bound of the per-step sums against the oracle: REL_ELASTIC where the case holds
    elastic particles, else REL_STEPS."""
    solid = (parts.property >= 2) & (parts.property < 4)
    return REL_ELASTIC if solid.any() else REL_STEPS


ORACLE_FIELDS = ["Position", "Velocity", "Force", "PressureP", "VolStrainP", "DivergenceP",
                 "DensityA", "GravityCenter", "Acceleration"]
ORACLE_TENSORS = ["DeformGradient", "Stress", "Strain"]


def oracle_field_plan(parts):
    """[(field, rel, rows)]: the float comparisons of one step's state against the oracle's --
    every field of ORACLE_FIELDS at oracle_rel(parts), DensityA and GravityCenter off the structure
    rows (the reference never writes them there; left out where no other row exists, bar3d), and the
    tensors on the structure rows at REL_STEPS."""
    solid = (parts.property >= 2) & (parts.property < 4)
    rel = oracle_rel(parts)
    plan = []
    for f in ORACLE_FIELDS:
        rows = ~solid if f in ("DensityA", "GravityCenter") else None
        if rows is not None and not rows.any():
            continue
        plan.append((f, rel, rows))
    if solid.any():
        plan += [(f, REL_STEPS, solid) for f in ORACLE_TENSORS]
    return plan


def check_fields_against_oracle(s, o, parts, k):
    """One step's state against the oracle's: NeighborCount bit-exact, every comparison of
    oracle_field_plan(parts) within its bound (k: the step, for the failure message)."""
    assert_close("NeighborCount", s.get("NeighborCount"), o.get("NeighborCount"), oracle_rel(parts),
                 context=(k,))
    for f, rel, rows in oracle_field_plan(parts):
        assert_close(f, s.get(f), o.get(f), rel, rows=rows, context=(k,))


def _check_per_material(pairs, plan, parts, k, worst):
    for t in np.unique(parts.property):
        of_type = parts.property == t
        for f, rel, rows in plan:
            r = of_type if rows is None else of_type & rows
            if not r.any():
                continue
            got, ref = pairs[f]
            err = assert_close(f, got, ref, rel, rows=r, context=(k, "type %d" % t))
            if worst is not None:
                ratio = err / bound(f, rel, float(np.max(np.abs(ref[r]))))
                if ratio >= worst.get("ratio", -1.0):
                    worst.update(ratio=ratio, field=f, type=int(t), step=k, err=err)


def check_materials_against_oracle(s, o, parts, k, worst=None):
    """oracle_field_plan(parts) once more per particle type: the rows of one type against the bound
    scaled by THAT type's largest magnitude, so that a material whose field is small beside another's
    (a light fluid under a stiff wall's pressure) cannot hide a wrong table entry under the other's
    scale.  `worst` (a dict) keeps the largest error / bound seen, with its field, type and step."""
    plan = oracle_field_plan(parts)
    _check_per_material({f: (s.get(f), o.get(f)) for f, _, _ in plan}, plan, parts, k, worst)


def check_materials_virial_against_oracle(s, o, parts, k, worst=None):
    """check_virial_against_oracle per particle type (the virial fields as the solver and the oracle
    hold them: call it after check_virial_against_oracle)."""
    plan = [(f, oracle_rel(parts), None) for f in VIRIAL]
    _check_per_material({f: (s.get(f), o.get(f)) for f in VIRIAL}, plan, parts, k, worst)


def check_virial_against_oracle(s, o, parts, k):
    """The virial diagnostic of the current state against the oracle's."""
    rel = oracle_rel(parts)
    s.compute_virial()
    o.call("calculateVirialStressAtParticle")
    for f in ["VirialStressAtParticle", "VirialPressureAtParticle"]:
        assert_close(f, s.get(f), o.get(f), rel, context=(k,))


def run_against_oracle_every_step(cfg, parts, nsteps, per_material=False, worst=None):
    """Step-by-step against the oracle: NeighborCount and all fields after every step, the virial
    after the last; per_material: each of them per particle type as well
    (check_materials_against_oracle)."""
    from oracle_bindings import OracleSolver
    from particlemethod_fsi_amd import MphSolver
    o = OracleSolver(cfg, parts)
    o.init()
    with MphSolver(cfg, parts) as s:
        for k in range(nsteps):
            s.step(1)
            o.step(1)
            check_fields_against_oracle(s, o, parts, k)
            if per_material:
                check_materials_against_oracle(s, o, parts, k, worst)
            if k == nsteps - 1:
                check_virial_against_oracle(s, o, parts, k)
                if per_material:
                    check_materials_virial_against_oracle(s, o, parts, k, worst)


def check_rank_files(out_dir, world, n, ref, ref_time, fields, rel=REL_STEPS):
    """The rank<r>.npz files of `world` slab ranks (dist_worker.gpu_rank_worker / gpu_state_worker)
    against one context's `ref` fields over all `n` particles: every rank's time equals ref_time,
    its owned rows lie within the bound SCALED BY THE WHOLE REFERENCE ARRAY (one bound for all
    ranks, whichever rows a rank owns), and ownership is a partition.  Returns the owner of every
    particle at the ranks' creation (-1 where the files do not record it) and at the end."""
    scale = {f: float(np.max(np.abs(ref[f]))) for f in fields if ref[f].dtype.kind == "f"}
    seen = np.zeros(n, np.int32)
    owner0 = np.full(n, -1, np.int32)
    owner1 = np.full(n, -1, np.int32)
    for r in range(world):
        z = np.load(os.path.join(str(out_dir), "rank%d.npz" % r))
        ids = z["ids"]
        if "ids0" in z.files:
            owner0[z["ids0"]] = r
        owner1[ids] = r
        seen[ids] += 1
        assert float(z["time"][0]) == ref_time, (r, float(z["time"][0]), ref_time)
        for f in fields:
            assert_close(f, z[f], ref[f][ids], rel, scale=scale.get(f), context=(r,))
    assert (seen == 1).all(), "ownership is not a partition: %d missing, %d duplicated" % (
        int((seen == 0).sum()), int((seen > 1).sum()))
    return owner0, owner1


CHUNK_FIELDS = ["Position", "Velocity", "Force", "Acceleration", "GravityCenter", "PressureP",
                "PressureA", "DensityA", "VolStrainP", "DivergenceP", "NeighborCount", "Kappa",
                "DeformGradient", "Strain", "Stress"]

# ---- the step variants' bitwise comparisons (test_gpu_idle_walls, _lean_steps, _step_paths,
# _call_batches): what a caller can read after a step, compared bit for bit between two ways to run it
VIRIAL = ["VirialStressAtParticle", "VirialPressureAtParticle"]


def snapshot(s):
    """CHUNK_FIELDS (NeighborCount is one of them) and both virial fields of the solver's state."""
    out = {f: s.get(f) for f in CHUNK_FIELDS}
    s.compute_virial()
    out.update({f: s.get(f) for f in VIRIAL})
    return out


def assert_same(a, b, context):
    """Two snapshots, or two dicts {steps done: snapshot}, hold the same fields with the same bits."""
    assert sorted(a) == sorted(b), (context, sorted(a), sorted(b))
    for k in a:
        if isinstance(a[k], dict):
            assert_same(a[k], b[k], (context, k))
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), (context, k)


def step_counters(s):
    """The five step counters since the creation: lazy steps, lean searches, lean pass A's, steps whose
    pass B left the next one's keys, k_prep launches."""
    lean, fold = s.lean_step_stats(), s.key_fold_stats()
    return {"lazy": s.idle_wall_stats()["lazy_steps"], "lean_search": lean["search_steps"],
            "lean_pass_a": lean["pass_a_steps"], "folded": fold["folded_steps"], "prep": fold["prep_launches"]}


def run_calls(cfg, parts, calls, snap_at=(), monitors=0):
    """One context stepped by mph_step(k) for k in `calls`, with a monitor ring of `monitors` samples
    where that is not 0: ({steps done: snapshot} at the step counts of `snap_at`, step_counters after
    every call, the idle wall waves counted after every call, the monitor samples or None)."""
    from particlemethod_fsi_amd import MphSolver
    snaps, counters, idle = {}, [], []
    with MphSolver(cfg, parts) as s:
        if monitors:
            s.monitor(stride=1, capacity=monitors)
        done = 0
        for k in calls:
            s.step(k)
            done += k
            counters.append(step_counters(s))
            idle.append(s.idle_wall_stats()["idle_wave_steps"])
            if done in snap_at:
                snaps[done] = snapshot(s)
        samples = s.monitor_read()[0] if monitors else None
    return snaps, counters, idle, samples


def tank():
    """A 3-D dam tank of 30 x 30 x 16 dx with three-layer walls on the floor, on both x sides and on both
    z sides, and a fluid block of 10 x 12 x 10 dx in the corner x = z = 0 -- 12,000 particles, 10,800 of
    them walls -- the outer half of the block (x > 5 dx) started at 0.8 m/s along +x
    (test_gpu_idle_walls.py has the reasons)."""
    from particlemethod_fsi_amd import cases
    from particlemethod_fsi_amd.mphio import Cuboid
    dx = 0.001
    c = cases.Case("idle_tank", 3, "dam", dx, (-0.01, 0.0, -0.01), (0.045, 0.055, 0.03), [
        Cuboid(1, (0.0, 0.003, 0.0), (0.010, 0.015, 0.010), dx),
        Cuboid(4, (0.0, 0.0, 0.0), (0.030, 0.003, 0.016), dx),
        Cuboid(4, (0.030, 0.0, 0.0), (0.033, 0.030, 0.016), dx),
        Cuboid(4, (-0.003, 0.0, 0.0), (0.0, 0.030, 0.016), dx),
        Cuboid(4, (-0.003, 0.0, -0.003), (0.033, 0.030, 0.0), dx),
        Cuboid(4, (-0.003, 0.0, 0.016), (0.033, 0.030, 0.019), dx),
    ])
    cfg, parts = c.build()
    assert parts.n == 12000
    parts.velocity[(parts.property < 2) & (parts.position[:, 0] > 0.005)] = (0.8, 0.0, 0.0)
    return cfg, parts


def check_structure_init_equals_host_build(case, monkeypatch):
    """The structure lists built on the device against the host build: see
    test_gpu_structure_init_equals_host_build."""
    import ctypes
    from particlemethod_fsi_amd import MphSolver, cases, solver
    cfg, parts = cases.get(case).build()
    n = parts.n
    isnc = np.zeros(n, np.int32)
    nrm = np.zeros((n, 3, 3))
    ll, lm = np.zeros(n), np.zeros(n)
    prop = np.ascontiguousarray(parts.property, np.int32)
    x0 = np.ascontiguousarray(parts.initial_position)
    assert solver.load_library().mph_structure_init(ctypes.byref(cfg), n, prop.ctypes.data, x0.ctypes.data,
                                                    isnc.ctypes.data, nrm.ctypes.data, ll.ctypes.data,
                                                    lm.ctypes.data) == 0
    outs = []
    for mode in ("device", "host"):
        if mode == "host":
            monkeypatch.setenv("MPH_STRUCT_INIT", "host")
        with MphSolver(cfg, parts) as s:
            got = {f: s.get(f) for f in ("InitialStructureNeighborCount", "Normalizer", "LambdaLames", "MuLames")}
            s.step(5)
            got["Position"] = s.get("Position")
            got["Stress"] = s.get("Stress")
            outs.append(got)
    dev, host = outs
    assert np.array_equal(dev["InitialStructureNeighborCount"], isnc)
    assert np.array_equal(dev["Normalizer"], nrm)
    assert np.array_equal(dev["LambdaLames"], ll) and np.array_equal(dev["MuLames"], lm)
    for f in dev:
        assert np.array_equal(dev[f], host[f]), f
