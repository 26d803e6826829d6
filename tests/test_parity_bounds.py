"""CPU: the numbers of tests/parity.py, the assertion every GPU parity test goes through, and the
rank launcher of the multi-rank tests.

The GPU suite's contract is its bounds; they live in one module, and this file pins them: the floor
table and the relative bounds literally, the bound of every call site against the expression that
site used to spell out, and the cases in which the assertion must fail.  No device, no library.
"""
import sys
import time
import types

import numpy as np
import pytest

import dist_worker
import parity
from parity import assert_close, assert_close_golden, bound, golden_bound


def test_floor_table_and_relative_bounds_are_pinned():
    assert parity.FLOOR == {
        "PressureP": 1e-9, "PressureA": 1e-9, "Force": 1e-15, "Acceleration": 1e-12,
        "VolStrainP": 1e-13, "DivergenceP": 1e-12, "DensityA": 1e-13, "GravityCenter": 1e-16,
        "DeformGradient": 1e-13, "Strain": 1e-13, "Stress": 1e-8,
        "VirialStressAtParticle": 1e-9, "VirialPressureAtParticle": 1e-9}
    assert len(parity.FLOOR) == 13
    assert (parity.REL_ONE_STEP, parity.REL_STEPS, parity.REL_ELASTIC, parity.REL_ELASTIC_DIVP) == (
        1e-9, 1e-8, 1e-7, 1e-6)
    assert parity.elastic_rel("DivergenceP") == 1e-6
    assert parity.elastic_rel("PressureP") == 1e-7 and parity.elastic_rel("Stress") == 1e-7
    fluid = types.SimpleNamespace(property=np.array([0, 1, 4, 5], np.int32))
    fsi = types.SimpleNamespace(property=np.array([1, 4, 2], np.int32))
    bar = types.SimpleNamespace(property=np.array([3, 3], np.int32))
    assert parity.oracle_rel(fluid) == 1e-8
    assert parity.oracle_rel(fsi) == 1e-7 and parity.oracle_rel(bar) == 1e-7


SCALES = (0.0, 1.0, 1e4)

# (call site, field, the rel the site passes, the site's former expression of the scale s)
SITES = [
    # check_fields_against_oracle / check_virial_against_oracle: 1e-8 fluid, 1e-7 with types 2/3
    ("per-step fluid", "Position", 1e-8, lambda s: 1e-12),
    ("per-step fluid", "Velocity", 1e-8, lambda s: 1e-9),
    ("per-step fluid", "Force", 1e-8, lambda s: 1e-8 * s + 1e-15),
    ("per-step fluid", "PressureP", 1e-8, lambda s: 1e-8 * s + 1e-9),
    ("per-step fluid", "VolStrainP", 1e-8, lambda s: 1e-8 * s + 1e-13),
    ("per-step fluid", "DivergenceP", 1e-8, lambda s: 1e-8 * s + 1e-12),
    ("per-step fluid", "DensityA", 1e-8, lambda s: 1e-8 * s + 1e-13),
    ("per-step fluid", "GravityCenter", 1e-8, lambda s: 1e-8 * s + 1e-16),
    ("per-step fluid", "Acceleration", 1e-8, lambda s: 1e-8 * s + 1e-12),
    ("per-step elastic", "Force", 1e-7, lambda s: 1e-7 * s + 1e-15),
    ("per-step elastic", "DivergenceP", 1e-7, lambda s: 1e-7 * s + 1e-12),
    ("per-step elastic", "GravityCenter", 1e-7, lambda s: 1e-7 * s + 1e-16),
    ("per-step tensors", "DeformGradient", 1e-8, lambda s: 1e-8 * s + 1e-13),
    ("per-step tensors", "Strain", 1e-8, lambda s: 1e-8 * s + 1e-13),
    ("per-step tensors", "Stress", 1e-8, lambda s: 1e-8 * s + 1e-8),
    ("virial fluid", "VirialStressAtParticle", 1e-8, lambda s: 1e-8 * s + 1e-9),
    ("virial elastic", "VirialPressureAtParticle", 1e-7, lambda s: 1e-7 * s + 1e-9),
    # test_gpu_struct_lanes_match_oracle: the per-step tensor rows above, Position and Velocity fixed
    ("struct lanes", "Position", 1e-8, lambda s: 1e-12),
    ("struct lanes", "Velocity", 1e-8, lambda s: 1e-9),
    # test_slab_ranks_match_oracle, test_slab_matches_single_gpu
    ("slab", "PressureA", 1e-8, lambda s: 1e-8 * s + 1e-9),
    ("slab", "Acceleration", 1e-8, lambda s: 1e-8 * s + 1e-12),
    ("slab", "Velocity", 1e-8, lambda s: 1e-9),
    # test_slab_structure_ranks_match_oracle, test_full_size_matches_oracle with solids
    ("slab elastic", "PressureP", 1e-7, lambda s: 1e-7 * s + 1e-9),
    ("slab elastic", "DivergenceP", 1e-6, lambda s: 1e-6 * s + 1e-12),
    ("slab elastic", "Stress", 1e-7, lambda s: 1e-7 * s + 1e-8),
    ("slab elastic", "Strain", 1e-7, lambda s: 1e-7 * s + 1e-13),
    ("slab elastic", "Position", 1e-7, lambda s: 1e-12),
    # test_full_size_matches_oracle (fluid), test_d1m_developed_matches_oracle, the fsi3d_sub hand-off,
    # the two slab8 tests (s: the whole reference array's max)
    ("developed", "PressureP", 1e-8, lambda s: 1e-8 * s + 1e-9),
    ("developed", "VolStrainP", 1e-8, lambda s: 1e-8 * s + 1e-13),
    ("developed", "DivergenceP", 1e-8, lambda s: 1e-8 * s + 1e-12),
    ("developed", "Force", 1e-8, lambda s: 1e-8 * s + 1e-15),
    ("developed", "DeformGradient", 1e-8, lambda s: 1e-8 * s + 1e-13),
    ("developed", "Stress", 1e-8, lambda s: 1e-8 * s + 1e-8),
    # test_bar2d_large_deformation_matches_oracle
    ("bar2d long run", "DeformGradient", 1e-9, lambda s: 1e-9 * s + 1e-13),
    ("bar2d long run", "Strain", 1e-9, lambda s: 1e-9 * s + 1e-13),
    ("bar2d long run", "Stress", 1e-9, lambda s: 1e-9 * s + 1e-8),
    ("bar2d long run", "PressureP", 1e-9, lambda s: 1e-9 * s + 1e-9),
    ("bar2d long run", "Force", 1e-9, lambda s: 1e-9 * s + 1e-15),
    # test_gpu_edge: 512 neighbours (Force), fluid type 0 / walls type 5 (PressureP)
    ("edge", "Force", 1e-9, lambda s: 1e-9 * s + 1e-15),
    ("edge", "PressureP", 1e-8, lambda s: 1e-8 * s + 1e-9),
    # a float field without a floor of its own
    ("no floor", "Kappa", 1e-8, lambda s: 1e-8 * s + 1e-12),
]


@pytest.mark.parametrize("site,field,rel,former", SITES, ids=["%s-%s" % r[:2] for r in SITES])
def test_bound_equals_the_sites_former_expression(site, field, rel, former):
    for s in SCALES:
        assert bound(field, rel, s) == former(s), (site, field, s)


def test_site_rels_are_the_named_constants():
    assert {r[2] for r in SITES} == {parity.REL_ONE_STEP, parity.REL_STEPS, parity.REL_ELASTIC,
                                     parity.REL_ELASTIC_DIVP}


def _former_tol(field, step, scale):
    """tol() of the former test_gpu_parity.py, with the scale already taken."""
    long = step >= 1000
    if field == "Position":
        return 1e-10 if long else 1e-12
    if field == "Velocity":
        return 1e-7 if long else 1e-9
    if field == "PressureP" and step > 1:
        return (1e-6 * scale + 1e-9) if long else (1e-8 * scale + 1e-9)
    return 1e-9 * scale + {"PressureP": 1e-9, "PressureA": 1e-9, "Force": 1e-15, "Acceleration": 1e-12,
                           "VolStrainP": 1e-13, "DivergenceP": 1e-12, "DensityA": 1e-13,
                           "GravityCenter": 1e-16, "DeformGradient": 1e-13, "Strain": 1e-13, "Stress": 1e-8,
                           "VirialStressAtParticle": 1e-9, "VirialPressureAtParticle": 1e-9}.get(field, 1e-12)


@pytest.mark.parametrize("step", [0, 1, 10, 100, 1000])
def test_golden_rule(step):
    for f in ["Position", "Velocity", "PressureP", "PressureA", "Force", "Stress", "Strain", "Kappa",
              "VirialStressAtParticle"]:
        for s in SCALES:
            assert golden_bound(f, step, s) == _former_tol(f, step, s), (f, step, s)
    # the literal figures of the rule
    assert golden_bound("Position", 100, 1.0) == 1e-12 and golden_bound("Position", 1000, 1.0) == 1e-10
    assert golden_bound("Velocity", 100, 1.0) == 1e-9 and golden_bound("Velocity", 1000, 1.0) == 1e-7
    assert golden_bound("PressureP", 1, 1e4) == 1e-9 * 1e4 + 1e-9
    assert golden_bound("PressureP", 10, 1e4) == 1e-8 * 1e4 + 1e-9
    assert golden_bound("PressureP", 1000, 1e4) == 1e-6 * 1e4 + 1e-9
    assert golden_bound("Force", 1000, 1e4) == 1e-9 * 1e4 + 1e-15


# --- the assertion --------------------------------------------------------------------------

REF = np.array([0.0, -2.0, 0.5])   # scale 2; the difference goes to the 0.0 slot, so it is exact


def _off_by(d):
    got = REF.copy()
    got[0] = d
    return got


def test_above_the_bound_raises_and_names_field_and_context():
    t = 1e-8 * 2.0 + 1e-9
    with pytest.raises(AssertionError) as e:
        assert_close("PressureP", _off_by(t * (1 + 1e-3)), REF, 1e-8, context=("dam2d", 7))
    msg = str(e.value)
    assert "PressureP" in msg and "dam2d" in msg and "7" in msg
    assert "%.3e" % (t * (1 + 1e-3)) in msg and "%.3e" % t in msg   # error and bound
    for f, t in (("Position", 1e-12), ("Velocity", 1e-9)):
        with pytest.raises(AssertionError):
            assert_close(f, _off_by(t * (1 + 1e-3)), REF, 1e-8)


def test_exactly_at_the_bound_passes_and_the_error_is_returned():
    t = 1e-8 * 2.0 + 1e-9
    assert assert_close("PressureP", _off_by(t), REF, 1e-8) == t
    assert assert_close("Position", _off_by(1e-12), REF, 1e-8) == 1e-12
    assert assert_close("Velocity", _off_by(-1e-9), REF, 1e-7) == 1e-9
    assert assert_close("PressureP", REF, REF, 1e-8) == 0.0


def test_extra_allowance_combines_by_max():
    t = 1e-7 * 2.0 + 1e-8
    assert assert_close("Stress", _off_by(5 * t), REF, 1e-7, extra=5 * t) == 5 * t
    with pytest.raises(AssertionError):
        assert_close("Stress", _off_by(5 * t), REF, 1e-7, extra=4 * t)
    assert assert_close("Stress", _off_by(t), REF, 1e-7, extra=0.5 * t) == t      # max, not the allowance alone
    with pytest.raises(AssertionError):
        assert_close("Stress", _off_by(1.2 * t), REF, 1e-7, extra=0.5 * t)        # max, not the sum


def test_integer_mismatch_raises_and_names_the_count():
    a = np.array([3, 4, 5, 6], np.int32)
    b = np.array([3, 9, 5, 7], np.int32)
    assert assert_close("NeighborCount", a, a.copy(), 1e-8) == 0
    with pytest.raises(AssertionError) as e:
        assert_close("NeighborCount", a, b, 1e-8, context=(2,))
    assert "NeighborCount" in str(e.value) and "2 mismatches" in str(e.value)
    with pytest.raises(AssertionError) as e:
        assert_close_golden("NeighborCount", a, b, 1, context=("box3d",))
    assert "2 mismatches" in str(e.value) and "box3d" in str(e.value)
    assert assert_close("NeighborCount", a, b, 1e-8, rows=np.array([True, False, True, False])) == 0


def test_nan_from_the_device_fails_nan_in_the_golden_is_skipped():
    got = REF.copy()
    got[1] = np.nan
    with pytest.raises(AssertionError):
        assert_close("PressureP", got, REF, 1e-8)
    with pytest.raises(AssertionError):
        assert_close("Position", got, REF, 1e-8)
    with pytest.raises(AssertionError):
        assert_close_golden("PressureP", got, REF, 1)
    ref = REF.copy()
    ref[1] = np.nan                       # a slot the reference leaves uninitialised
    for mine in (REF, got):               # whatever the device holds there
        assert assert_close_golden("PressureP", mine, ref, 1) == 0.0
    # the scale is the unmasked slots' (0.5), not the NaN's and not the masked -2.0
    t = 1e-9 * 0.5 + 1e-9
    assert assert_close_golden("PressureP", _off_by(t), ref, 1) == t
    with pytest.raises(AssertionError):
        assert_close_golden("PressureP", _off_by(t * (1 + 1e-3)), ref, 1)
    # against the oracle a NaN reference is no pass either
    with pytest.raises(AssertionError):
        assert_close("PressureP", REF, ref, 1e-8)
    # golden wrapper: the step selects the rule
    assert assert_close_golden("Position", _off_by(1e-10), REF, 1000, context=("dam2d",)) == 1e-10
    with pytest.raises(AssertionError) as e:
        assert_close_golden("Position", _off_by(1e-10), REF, 100, context=("dam2d",))
    assert "dam2d" in str(e.value) and "100" in str(e.value) and "Position" in str(e.value)


def test_row_mask_and_explicit_scale_are_honoured():
    ref = np.array([100.0, 1.0, 2.0])
    got = ref + np.array([0.0, 0.0, 5e-7])
    rows = np.array([1, 2])
    # a rank's rows under the bound of the whole array (1e-8 * 100 + 1e-9) ...
    assert assert_close("PressureP", got, ref, 1e-8, rows=rows, scale=100.0) == pytest.approx(5e-7)
    assert assert_close("PressureP", got[rows], ref[rows], 1e-8, scale=float(np.max(np.abs(ref)))) > 0
    # ... and under their own (1e-8 * 2 + 1e-9)
    with pytest.raises(AssertionError):
        assert_close("PressureP", got, ref, 1e-8, rows=rows)
    # rows outside the mask are not compared
    far = got.copy()
    far[0] = 0.0
    assert assert_close("PressureP", far, ref, 1e-8, rows=rows, scale=100.0) == pytest.approx(5e-7)
    with pytest.raises(AssertionError):
        assert_close("PressureP", far, ref, 1e-8, scale=100.0)
    # tensors on the solid rows: a boolean mask over the first axis
    T = np.zeros((3, 3, 3))
    G = T.copy()
    G[0, 1, 1] = 1.0
    assert assert_close("Stress", G, T, 1e-8, rows=np.array([False, True, True])) == 0.0
    with pytest.raises(AssertionError):
        assert_close("Stress", G, T, 1e-8, rows=np.array([True, False, True]))


def test_empty_rows_are_error_zero_scale_zero():
    none = np.zeros(3, bool)
    assert assert_close("DensityA", REF + 1.0, REF, 1e-8, rows=none) == 0.0
    assert assert_close("Stress", np.zeros((0, 3, 3)), np.zeros((0, 3, 3)), 1e-7, extra=0.0) == 0.0
    assert assert_close("Position", np.zeros((0, 3)), np.zeros((0, 3)), 1e-8) == 0.0
    assert assert_close_golden("Stress", np.zeros((0, 3, 3)), np.zeros((0, 3, 3)), 10) == 0.0


# --- the per-step plan and its per-material form (test_gpu_materials.py) ----------------------------

class _State:
    def __init__(self, fields):
        self.fields = fields

    def get(self, name):
        return self.fields[name]


def test_oracle_field_plan_is_the_per_step_sites():
    mixed = types.SimpleNamespace(property=np.array([0, 0, 1, 1, 2, 3, 4, 5], np.int32))
    solid = np.array([0, 0, 0, 0, 1, 1, 0, 0], bool)
    plan = parity.oracle_field_plan(mixed)
    assert [(f, rel) for f, rel, _ in plan] == [(f, 1e-7) for f in (
        "Position", "Velocity", "Force", "PressureP", "VolStrainP", "DivergenceP", "DensityA", "GravityCenter",
        "Acceleration")] + [(f, 1e-8) for f in ("DeformGradient", "Stress", "Strain")]
    for f, _, rows in plan:
        if f in ("DensityA", "GravityCenter"):
            assert np.array_equal(rows, ~solid)
        elif f in ("DeformGradient", "Stress", "Strain"):
            assert np.array_equal(rows, solid)
        else:
            assert rows is None
    fluid = types.SimpleNamespace(property=np.array([0, 1, 4, 5], np.int32))
    assert [(f, rel) for f, rel, _ in parity.oracle_field_plan(fluid)] == [(f, 1e-8) for f in parity.ORACLE_FIELDS]
    bar = types.SimpleNamespace(property=np.array([2, 3], np.int32))
    assert [f for f, _, _ in parity.oracle_field_plan(bar)] == [
        f for f in parity.ORACLE_FIELDS if f not in ("DensityA", "GravityCenter")] + parity.ORACLE_TENSORS


def test_per_material_check_scales_by_the_types_own_rows():
    """An error on the light material that the whole field's scale covers: check_fields_against_oracle
    passes, check_materials_against_oracle names the field and the type.  No new number: the bound
    is bound(field, rel of the plan, max |reference| over that type's rows)."""
    parts = types.SimpleNamespace(property=np.array([0, 0, 1, 1, 4, 5], np.int32))
    n = 6
    ref = {f: np.zeros((n, 3)) for f in ("Position", "Velocity", "Force", "GravityCenter", "Acceleration")}
    ref.update({f: np.zeros(n) for f in ("PressureP", "VolStrainP", "DivergenceP", "DensityA")})
    ref["NeighborCount"] = np.arange(n, dtype=np.int32)
    ref["PressureP"] = np.array([1.0, -2.0, 1e4, 5e3, 3.0, 4.0])
    got = {f: a.copy() for f, a in ref.items()}
    whole, own = bound("PressureP", 1e-8, 1e4), bound("PressureP", 1e-8, 2.0)
    assert own == 1e-8 * 2.0 + 1e-9
    got["PressureP"][0] += 0.5 * whole            # far above the type's own bound, below the field's
    s, o = _State(got), _State(ref)
    parity.check_fields_against_oracle(s, o, parts, 3)
    with pytest.raises(AssertionError) as e:
        parity.check_materials_against_oracle(s, o, parts, 3)
    assert "PressureP" in str(e.value) and "type 0" in str(e.value) and "%.3e" % own in str(e.value)
    got["PressureP"][0] = ref["PressureP"][0] + 0.5 * own
    worst = {}
    parity.check_materials_against_oracle(s, o, parts, 3, worst)
    assert worst["field"] == "PressureP" and worst["type"] == 0 and worst["step"] == 3
    assert worst["ratio"] == pytest.approx(0.5)
    # the virial form: both fields, every type, the per-step rel
    vir = {"VirialStressAtParticle": np.ones((n, 3, 3)), "VirialPressureAtParticle": np.ones(n)}
    bad = {f: a.copy() for f, a in vir.items()}
    bad["VirialPressureAtParticle"][5] += 2.0 * bound("VirialPressureAtParticle", 1e-8, 1.0)
    parity.check_materials_virial_against_oracle(_State(vir), _State(vir), parts, 0)
    with pytest.raises(AssertionError) as e:
        parity.check_materials_virial_against_oracle(_State(bad), _State(vir), parts, 0)
    assert "VirialPressureAtParticle" in str(e.value) and "type 5" in str(e.value)


# --- the rank launcher ----------------------------------------------------------------------

def _rank_ok(rank, world, port, tag):
    assert world == 2 and rank in (0, 1) and port > 0 and tag == "x"


def _rank_one_exits_3(rank, world, port):
    sys.exit(3 if rank == 1 else 0)


def _rank_one_sleeps(rank, world, port):
    if rank == 1:
        time.sleep(60)


def test_run_ranks_passes_when_every_rank_exits_0():
    dist_worker.run_ranks(_rank_ok, 2, "x", timeout=10)


def test_run_ranks_reports_a_failed_rank_with_the_codes():
    with pytest.raises(AssertionError) as e:
        dist_worker.run_ranks(_rank_one_exits_3, 2, timeout=10)
    assert "[0, 3]" in str(e.value)


def test_run_ranks_kills_a_rank_past_the_timeout():
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as e:
        dist_worker.run_ranks(_rank_one_sleeps, 2, timeout=2)
    assert "[0, -9]" in str(e.value)
    assert time.monotonic() - t0 < 30   # killed at the timeout, not waited for
