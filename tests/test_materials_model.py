"""CPU: the mixed-material cases (cases.MIX_CASES) are worth what the GPU tests take them for.

tests/test_gpu_materials.py compares the device with the oracle on runs that hold both fluids, both
structures and both wall types.  That comparison finds a wrong per-type table entry or a transposed
InteractionRatio only if (1) every ordered type pair does occur in the neighbour lists, and (2) the
entry moves some compared field by far more than the bound it is compared under.  Both are checked
here on the oracle alone (which test_oracle.py pins to the reference on these cases).
"""
import numpy as np
import pytest

import parity
from oracle_bindings import OracleSolver
from particlemethod_fsi_amd import cases

# the step counts of test_gpu_materials.test_gpu_mixed_matches_oracle_every_step
STEPS = {3: 12, 2: 20}
MIN_PAIRS = {3: 100, 2: 10}
MIN_FACTOR = 1000.0   # "cannot hide under the tolerance": a floor, not a tuned number


def _pair_counts(o, prop):
    pairs = np.zeros((6, 6), np.int64)
    for i in range(o.n):
        pairs[prop[i]] += np.bincount(prop[o.neighbors(i)], minlength=6)
    return pairs


@pytest.mark.parametrize("case", cases.MIX_CASES)
def test_every_ordered_type_pair_is_in_the_lists(case):
    """At the first and the last compared step every ordered pair (ti, tj) of the types present
    has at least 100 (3-D) / 10 (2-D) list entries, and every type at least 100 particles.
    Measured minima at the last step: 483 (3-D, fluid 0 beside structure 3), 13 (2-D, structure 2
    beside wall 5)."""
    c = cases.get(case)
    cfg, parts = c.build()
    prop = parts.property
    present = np.unique(prop)
    assert list(present) == ([0, 1, 4, 5] if case.endswith("_st") else [0, 1, 2, 3, 4, 5])
    assert np.bincount(prop, minlength=6)[present].min() >= 100
    o = OracleSolver(cfg, parts)
    o.init()
    done = 0
    for step in (1, STEPS[c.dim]):
        o.step(step - done)
        done = step
        pairs = _pair_counts(o, prop)[np.ix_(present, present)]
        assert pairs.min() >= MIN_PAIRS[c.dim], (case, step, pairs)


def test_mix2d_clamps_rows_of_both_structure_types():
    """The DAM module holds structure rows with y0 < 0.002 (updateElasticPosition): both halves of
    mix2d's gate have some, so the clamp meets both sets of elastic constants."""
    _, parts = cases.get("mix2d").build()
    clamped = parts.initial_position[:, 1] < 0.002
    for t in (2, 3):
        assert (clamped & (parts.property == t)).any() and (~clamped & (parts.property == t)).any()


def _sibling(t):
    return t ^ 1


def _perturbations(cfg, present, surface_tension):
    """(name, function that changes a copy of cfg): every per-type entry the reference reads, set to
    its sibling type's value (0 <-> 1, 2 <-> 3, 4 <-> 5), and every InteractionRatio[i][j] <-> [j][i]
    swap but 2 <-> 3.  The reference never reads the walls' Density or the 2/3 ratios.  (The .data
    file's four YoungModulus / PoissonRatio values are those of types 2, 3, 4, 5 and its four
    SurfaceTension values those of types 0, 1, 4, 5: mphio._ARRAYS.)"""
    out = []

    def entry(table, t, src):
        def change(c):
            getattr(c, table)[t] = getattr(cfg, table)[src]
        assert getattr(cfg, table)[t] != getattr(cfg, table)[src], (table, t, src)
        return "%s[%d]" % (table, t), change

    for t in present:
        if t < 4:
            out.append(entry("density", t, _sibling(t)))
        for table in ("bulk_modulus", "bulk_viscosity", "shear_viscosity"):
            out.append(entry(table, t, _sibling(t)))
        if surface_tension and t < 2:
            out.append(entry("surface_tension", t, _sibling(t)))
        if t in (2, 3):
            out.append(entry("young_modulus", t, _sibling(t)))
            out.append(entry("poisson_ratio", t, _sibling(t)))
    for i in present:
        for j in present:
            if i < j and (i, j) != (2, 3):
                def swap(c, i=i, j=j):
                    r = c.interaction_ratio
                    r[i][j], r[j][i] = r[j][i], r[i][j]
                assert cfg.interaction_ratio[i][j] != cfg.interaction_ratio[j][i]
                out.append(("ratio[%d][%d]<->[%d][%d]" % (i, j, j, i), swap))
    return out


def _compared_state(cfg, parts, nsteps):
    o = OracleSolver(cfg, parts)
    o.init()
    o.step(nsteps)
    plan = parity.oracle_field_plan(parts)
    out = {f: o.get(f) for f, _, _ in plan}
    o.call("calculateVirialStressAtParticle")
    out.update({f: o.get(f) for f in parity.VIRIAL})
    return out, plan + [(f, parity.oracle_rel(parts), None) for f in parity.VIRIAL]


def _discrimination(plain, other, plan):
    """The largest |other - plain| / bound over the comparisons of `plan`, and its field."""
    best = (0.0, "none")
    for f, rel, rows in plan:
        a, b = (plain[f], other[f]) if rows is None else (plain[f][rows], other[f][rows])
        ratio = float(np.max(np.abs(b - a))) / parity.bound(f, rel, float(np.max(np.abs(a))))
        best = max(best, (ratio, f))
    return best


@pytest.mark.parametrize("case", cases.MIX_GOLDEN_CASES)
def test_every_table_entry_moves_a_compared_field(case):
    """Each perturbation of _perturbations moves some field that the GPU tests compare (the plan of
    parity.oracle_field_plan and the virial, at the last of their steps) by at least 1000 x the
    bound that field is compared under."""
    c = cases.get(case)
    cfg, parts = c.build()
    plain, plan = _compared_state(cfg, parts, STEPS[c.dim])
    measured = []
    present = [int(t) for t in np.unique(parts.property)]
    for name, change in _perturbations(cfg, present, case.endswith("_st")):
        other = cfg.copy()
        change(other)
        ratio, field = _discrimination(plain, _compared_state(other, parts, STEPS[c.dim])[0], plan)
        measured.append((ratio, name, field))
    report = "\n".join("%-28s %.3e x bound (%s)" % (n, r, f) for r, n, f in sorted(measured))
    print(report)
    assert min(measured)[0] >= MIN_FACTOR, "%s: difference / bound per perturbed entry\n%s" % (case, report)
