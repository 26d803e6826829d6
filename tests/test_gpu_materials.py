"""GPU: runs that hold two fluids (types 0, 1), two structures (2, 3) and two wall types (4, 5) at
once (cases.MIX_CASES: per-type tables without a shared value, a fully asymmetric InteractionRatio).

Every other case has one material per class, and in DAM_DATA types 1 and 4 even share their
constants: a pass that read table[tj] for table[ti], or ratio[tj][ti] for ratio[ti][tj], or decoded
a wrong neighbour type from a list entry, passes there.  Here it cannot: tests/test_materials_model.py
shows on the CPU that every ordered type pair occurs in the lists and that each table entry moves a
compared field by >= 1e5 x its bound.  The references: the reference's golden vectors for the four
cases it defines, the oracle (pinned to it on those, test_oracle.py) everywhere -- in the *_stgate
pair (surface tension beside a structure) the reference reads GravityCenter rows it never wrote,
and the oracle's zeros there are the definition.

Every bound is tests/parity.py's; the per-material checks scale each type's rows by that type's
own largest magnitude.
"""
import math

import numpy as np
import pytest

import dist_worker
import list16_ref
from golden_utils import Golden
from parity import assert_close, assert_same, compare, elastic_rel, run_against_oracle_every_step, snapshot
from particlemethod_fsi_amd import MphSolver, cases, solver

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
# test_gpu_dist.STRUCT_FIELDS: what the slab tests of cases with elastic particles compare
STRUCT_FIELDS = ["Position", "Velocity", "PressureP", "NeighborCount", "Force", "VolStrainP", "DivergenceP",
                 "DensityA", "GravityCenter", "PressureA", "Acceleration", "DeformGradient", "Strain", "Stress"]


@pytest.mark.parametrize("case", cases.MIX_GOLDEN_CASES)
def test_gpu_mixed_matches_reference_golden(case):
    g = Golden(case)
    cfg, parts = cases.get(case).build()
    with MphSolver(cfg, parts) as s:
        assert np.array_equal(s.scalars(), g.z["scalars"])
        compare(g, s, 0)
        if g.solid.any():
            # two sets of elastic constants, in the reference's initial state and on the device
            for f in ("LambdaLames", "MuLames"):
                assert len(np.unique(g.get(0, f))) == 2, (f, np.unique(g.get(0, f)))
                assert np.array_equal(np.unique(s.get(f)[g.solid]), np.unique(g.get(0, f))), f
        done = 0
        for step in g.steps:
            s.step(step - done)
            done = step
            compare(g, s, step)
        assert abs(s.time - g.meta["time"]) == 0.0


@pytest.mark.parametrize("case", cases.MIX_CASES)
def test_gpu_mixed_matches_oracle_every_step(case):
    """All fields after every step, the virial after the last; each of them also per particle type
    under the bound of that type's own scale (parity.check_materials_against_oracle)."""
    c = cases.get(case)
    cfg, parts = c.build()
    worst = {}
    run_against_oracle_every_step(cfg, parts, 12 if c.dim == 3 else 20, per_material=True, worst=worst)
    print(case, "largest per-material error / bound:", worst)


# ---- lists ----------------------------------------------------------------------------------------

def test_gpu_mixed_neighbor_sets_match_reference_golden(monkeypatch):
    monkeypatch.setenv("MPH_LIST_FULL", "1")
    g = Golden("mix3d")
    cfg, parts = cases.get("mix3d").build()
    with MphSolver(cfg, parts) as s:
        s.step(1)
        counts, offsets, ids = s.neighbor_rows()
        assert np.array_equal(offsets, g.get(1, "nbr_offsets"))
        assert np.array_equal(ids, g.get(1, "nbr_ids"))


def test_gpu_mixed_neighbor_sets_match_oracle(monkeypatch):
    from oracle_bindings import OracleSolver
    monkeypatch.setenv("MPH_LIST_FULL", "1")
    cfg, parts = cases.get("mix2d").build()
    o = OracleSolver(cfg, parts)
    o.init()
    o.step(10)
    with MphSolver(cfg, parts) as s:
        s.step(10)
        counts, offsets, ids = s.neighbor_rows()
    assert np.array_equal(counts, o.get("NeighborCount"))
    for i in range(parts.n):
        assert np.array_equal(ids[offsets[i]:offsets[i + 1]], np.sort(o.neighbors(i))), i


@pytest.mark.parametrize("case", ["mix3d", "mix3d_st"])
def test_gpu_mixed_list_forms_bitwise(case, monkeypatch):
    """The neighbour type travels in the list entry (both row formats) and the trimmed lists drop
    the shell's pairs: every field and the virial after mph_step(11) equal the default run's bit for
    bit with 32-bit rows only (MPH_LIST16=0) and with the reference's whole lists (MPH_LIST_FULL=1)."""
    cfg, parts = cases.get(case).build()
    snaps = {}
    for env in (None, "MPH_LIST16", "MPH_LIST_FULL"):
        if env:
            monkeypatch.setenv(env, "0" if env == "MPH_LIST16" else "1")
        try:
            with MphSolver(cfg, parts) as s:
                s.step(11)
                snaps[env] = snapshot(s)
                stats = s.list_format_stats()
        finally:
            if env:
                monkeypatch.delenv(env)
        if env != "MPH_LIST_FULL":   # the default run has waves with 16-bit rows, MPH_LIST16=0 none
            assert (stats["short_waves"] > 0) == (env is None), (env, stats)
    assert_same(snaps["MPH_LIST16"], snaps[None], (case, "MPH_LIST16=0"))
    assert_same(snaps["MPH_LIST_FULL"], snaps[None], (case, "MPH_LIST_FULL=1"))


def test_gpu_mixed_short_wave_holds_three_neighbour_types():
    """Some wave of mix3d whose list is in the 16-bit form (mph_list_wave_formats code 1 at the
    creation's search) has neighbours of at least three types: the particles of the cells that lie
    wholly inside the wave's 64 sorted slots (list16_ref.model) against every particle within the
    passes' radius."""
    cfg, parts = cases.get("mix3d").build()
    with MphSolver(cfg, parts) as s:
        codes, _ = s.list_wave_formats()
    m = list16_ref.model(cfg, parts, windows=False)
    assert len(codes) == m.waves
    X, T = parts.position, parts.property
    r2 = (cfg.radius_ratio_p * cfg.particle_spacing) ** 2
    most = 0
    for w in np.nonzero(codes == 1)[0]:
        a, b = 64 * w, min(parts.n, 64 * w + 64)
        k = m.key[a:b]
        ids = m.order[a:b][(m.start[k] >= a) & (m.start[k + 1] <= b)]
        if len(ids):
            d2 = ((X[ids][:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
            most = max(most, len(np.unique(T[(d2 < r2).any(axis=0)])))
    assert most >= 3, (most, np.bincount(codes))


# ---- step paths -----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["mix3d", "mix2d_st"])
def test_gpu_mixed_step_paths_bitwise(case):
    """13 x mph_step(1) == mph_step(13) (one 8-step batch whose lean steps store and load only what
    their readers see, remainder steps, the key fold where no structure is present) == 13 calls under
    step batching, for every field and the virial."""
    cfg, parts = cases.get(case).build()
    with MphSolver(cfg, parts) as a, MphSolver(cfg, parts) as b, MphSolver(cfg, parts) as c:
        for _ in range(13):
            a.step(1)
        b.step(13)
        c.step_batching(True)
        for _ in range(13):
            c.step(1)
        ref = snapshot(a)
        assert_same(snapshot(b), ref, (case, "mph_step(13)"))
        assert_same(snapshot(c), ref, (case, "step batching"))


# ---- slabs ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,world,axis,local", [("mix3d", 2, 0, False), ("mix2d", 3, 0, False),
                                                  ("mix2d_lat", 3, 0, True)])
def test_gpu_mixed_slab_ranks_match_oracle(tmp_path, case, world, axis, local):
    """All six types across slab faces, some rank's halo with at least three of them (counted at the
    faces between two ranks: the particles another rank owns within one halo width of the face).
    mix3d: the x face at 20 mm runs through the low fluid column 2 mm in front of the gate, so both
    fluids, both gate halves and both wall types are ghosts of the first rank (the tank is too thin
    along z for two slabs); mix2d in three ranks, and mix2d_lat (mix2d on the lattice) with every rank
    created from its own window of the case alone."""
    from oracle_bindings import OracleSolver
    assert dist_worker.SLAB_AXIS[case] == axis
    checkpoints = [1, 10, 20]
    out = str(tmp_path / "slab.npz")
    dist_worker.run_ranks(dist_worker.gpu_worker, world, case, checkpoints, STRUCT_FIELDS, out, local, None,
                          timeout=300)
    r = np.load(out)
    cfg, parts = cases.get(case).build()
    owner0 = r["owner0"]
    assert (owner0 >= 0).all()
    x = parts.position[:, axis]
    halo_types = []
    for rank in range(world):
        lo, hi, h = solver.slab_bounds(cfg, rank, world, axis)
        halo = np.zeros(parts.n, bool)
        if rank > 0:
            halo |= (x < lo) & (lo - x <= h)
        if rank < world - 1:
            halo |= (x >= hi) & (x - hi < h)
        halo &= owner0 != rank
        halo_types.append(len(np.unique(parts.property[halo])))
    assert max(halo_types) >= 3, halo_types
    o = OracleSolver(cfg, parts)
    o.init()
    done = 0
    for k in checkpoints:
        o.step(k - done)
        done = k
        assert (r["s%d/owner" % k] >= 0).all()
        for f in STRUCT_FIELDS:
            assert_close(f, r["s%d/%s" % (k, f)], o.get(f), elastic_rel(f), context=(case, world, k))


# ---- selections and loads -------------------------------------------------------------------------

def test_gpu_mixed_selections_and_loads():
    """types=t selects exactly the rows of type t, for each of the six; the summed Force of the two
    gate halves and of the whole gate match numpy within the selection totals' bound (2 (n + 8) 2^-53
    sum |term|, test_gpu_select.py), and the halves add up to the whole within the three bounds."""
    cfg, parts = cases.get("mix3d").build()
    T = parts.property
    with MphSolver(cfg, parts) as s:
        s.step(3)
        F = s.get("Force")
        for t in range(6):
            assert s.select(types=(t,)) == np.bincount(T, minlength=6)[t] > 0
            assert np.array_equal(s.selected_ids(), np.nonzero(T == t)[0])
        load, tol = {}, {}
        for types in ((2,), (3,), (2, 3)):
            rows = np.isin(T, types)
            assert s.select(types=types) == rows.sum()
            tot = s.selection_totals()
            load[types] = np.array([tot["F" + ax] for ax in "XYZ"])
            ref = np.array([math.fsum(F[rows, d]) for d in range(3)])
            mag = np.array([math.fsum(np.abs(F[rows, d])) for d in range(3)])
            assert mag.min() > 0.0, (types, mag)
            tol[types] = 2.0 * (int(rows.sum()) + 8) * EPS * mag
            assert (np.abs(load[types] - ref) <= tol[types]).all(), (types, load[types], ref, tol[types])
        both = load[(2,)] + load[(3,)]
        allowed = tol[(2,)] + tol[(3,)] + tol[(2, 3)] + EPS * np.abs(both)
        assert (np.abs(both - load[(2, 3)]) <= allowed).all(), (both, load[(2, 3)], allowed)
