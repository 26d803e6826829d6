"""GPU: kernel radii other than the example's 2.5 / 2.5 / 2.5 (cases.RADII_CASES, CUTOFF_CASES) and
the row layout of the stored lists.

A. Unequal RadiusRatioA / P / V: the general branch of pass A, the separate-radius tests of pass B
   and the virial, lists trimmed to the largest pass radius, grid and stencil sized from MaxRadius,
   the elastic weight with RadiusP below MaxRadius.
B. On-cutoff lattices: with every ratio at 2.9 (3.9, 4.9) the lattice pairs at 3 (4, 5) dx lie on
   the search's cutoff MaxRadius + MARGIN to within rounding; the reference takes or leaves each by
   the last bit of its own expression (main.cpp:1765), which the search evaluates only inside its
   innermost band.  A one-ulp change of a position flips thousands of these decisions, so only
   searches whose input positions equal the oracle's bit for bit are compared: at creation and in
   the first step.
C. The aligned rows' jumps (mph_list_layout): they happen off the lattice, stop at kAlignRows, and
   the rows decoded on the host hold exactly the reference's sets.

The reference is the CPU oracle, pinned to the compiled reference on these configurations by
test_oracle_per_kernel_against_live_reference.  Every bound is that of tests/parity.py (the
statement of the tolerances; the comparison itself is imported from there): the oracle's own
sensitivity to a one-ulp change of its input stays below 0.07 of them on every case here.
"""
import functools

import numpy as np
import pytest

from particlemethod_fsi_amd import MphSolver, cases, mphio
from parity import (CHUNK_FIELDS, check_fields_against_oracle, check_structure_init_equals_host_build,
                    run_against_oracle_every_step)

pytestmark = pytest.mark.gpu

K_MAX_JUMPS = 6      # mph_params.h kMaxJumps
K_ALIGN_ROWS = 128   # mph_params.h kAlignRows
MAX_NEIGHBOR = 512   # MPH_MAX_NEIGHBOR_COUNT


# --- A. unequal radii -------------------------------------------------------------------------

@pytest.mark.parametrize("case", cases.RADII_CASES)
def test_gpu_radii_match_oracle_every_step(case):
    """test_gpu_matches_oracle_every_step on every unequal-radii case (and the equal-radii 3.1 case
    with long lists): NeighborCount bit-exact and all fields after every step, the virial after the
    last -- 10 steps in 3-D, 20 in 2-D.  None of these cases has a pair on the cutoff."""
    c = cases.get(case)
    cfg, parts = c.build()
    run_against_oracle_every_step(cfg, parts, 10 if c.dim == 3 else 20)


@pytest.mark.parametrize("case", ["box3d_r312126", "box3d_st_r312126", "gate3d_sub_r213121"])
def test_gpu_radii_graph_chunking_equivalence(case):
    """mph_step(8) == 8 x mph_step(1) bitwise with unequal radii (fluid, surface tension, elastic
    gate): the general branches skip the output-only stores on a graph's first 7 steps too."""
    cfg, parts = cases.get(case).build()
    with MphSolver(cfg, parts) as a, MphSolver(cfg, parts) as b:
        a.step(8)
        for _ in range(8):
            b.step(1)
        for f in CHUNK_FIELDS:
            assert np.array_equal(a.get(f), b.get(f), equal_nan=True), (case, f)
        a.compute_virial()
        b.compute_virial()
        for f in ["VirialStressAtParticle", "VirialPressureAtParticle"]:
            assert np.array_equal(a.get(f), b.get(f), equal_nan=True), (case, f)


@pytest.mark.parametrize("case", ["box3d_r262131_jit", "box3d_st_r312126", "box3d_r313131_jit"])
def test_gpu_radii_trimmed_lists_equal_full_lists(case, monkeypatch):
    """test_gpu_trimmed_lists_equal_full_lists where the passes' radii differ: the default lists
    keep the pairs within the LARGEST pass radius, so a pass with a smaller radius must leave the
    stored pairs beyond its own out; against the whole lists (MPH_LIST_FULL=1) every field is
    bit-identical.  The third case (equal radii 3.1, up to 149 neighbours) drives pass A and pass B
    through row masks with gaps below row 128 and entries above it.  The trimming did happen in all
    three: off the lattice the shell holds pairs, and on the box3d_st lattice the pairs at
    sqrt(10) dx = 3.16 dx lie between the largest radius 3.1 dx and the cutoff 3.2 dx."""
    cfg, parts = cases.get(case).build()
    out, mean_len = {}, {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MPH_LIST_FULL", mode)
        with MphSolver(cfg, parts) as s:
            s.step(7)
            out[mode] = {f: s.get(f) for f in CHUNK_FIELDS}
            mean_len[mode] = s.list_stats()[0]
    for f in CHUNK_FIELDS:
        assert np.array_equal(out["0"][f], out["1"][f], equal_nan=True), f
    assert mean_len["1"] == pytest.approx(float(out["1"]["NeighborCount"].mean()))
    assert mean_len["0"] < mean_len["1"], mean_len


@pytest.mark.parametrize("case", ["gate3d_sub_r213121", "gate2d_sub_r262131"])
def test_gpu_radii_structure_init_equals_host_build(case, monkeypatch):
    """test_gpu_structure_init_equals_host_build with RadiusP = MaxRadius above RadiusA (3-D) and
    RadiusP below MaxRadius (2-D)."""
    check_structure_init_equals_host_build(case, monkeypatch)


# --- B. on-cutoff lattices --------------------------------------------------------------------

# the cloud as generated and translated by these multiples of dx (which of them: _cutoff_params)
SHIFTS = {"none": (0.0, 0.0, 0.0), "a": (0.37, 0.11, 0.53), "b": (1.0 / 3.0, 2.0 / 3.0, 0.1),
          "seam": (0.37, 0.11, 0.23)}


def on_cutoff_pairs(pos, rc):
    """(i, j), i < j: the pairs with |r^2 / rc^2 - 1| < 1e-10, plain distances (no periodic
    images), in numpy over x-sorted chunks."""
    order = np.argsort(pos[:, 0], kind="stable")
    p = pos[order]
    n = len(p)
    I, J = [], []
    for a in range(0, n, 512):
        b = min(a + 512, n)
        lo = np.searchsorted(p[:, 0], p[a, 0] - 1.001 * rc)
        hi = np.searchsorted(p[:, 0], p[b - 1, 0] + 1.001 * rc)
        d = p[a:b, None, :] - p[None, lo:hi, :]
        r2 = np.einsum("ijk,ijk->ij", d, d)
        i, j = np.nonzero(np.abs(r2 / (rc * rc) - 1.0) < 1e-10)
        i, j = order[i + a], order[j + lo]
        k = i < j
        I.append(i[k])
        J.append(j[k])
    return np.concatenate(I), np.concatenate(J)


@functools.lru_cache(maxsize=2)
def cutoff_reference(case, shift):
    """-> (cfg, parts, oracle after one step, NeighborCount at creation, its sorted rows after the
    step, (on-cutoff pairs, accepted, rejected)); computed once per (case, shift), read-only."""
    from oracle_bindings import OracleSolver
    c = cases.get(case)
    cfg, parts = c.build()
    off = np.zeros(3)
    off[:c.dim] = SHIFTS[shift][:c.dim]
    pos = parts.position + off * cfg.particle_spacing
    parts = mphio.Particles(parts.property, pos, parts.initial_position + off * cfg.particle_spacing, parts.velocity)
    lo, hi = np.array(cfg.domain_min[:]), np.array(cfg.domain_max[:])
    assert ((pos >= lo) & (pos < hi))[:, :c.dim].all(), "the translated cloud leaves the domain"
    o = OracleSolver(cfg, parts)
    o.init()
    count0 = o.get("NeighborCount")
    o.step(1)
    rows = [np.sort(o.neighbors(i)) for i in range(parts.n)]
    sc = o.scalars()
    i, j = on_cutoff_pairs(pos, sc[7] + 0.1 * sc[14])   # MaxRadius + MARGIN, MARGIN = 0.1 dx (main.cpp:116)
    keys = np.concatenate([np.int64(q) * parts.n + r for q, r in enumerate(rows)])
    acc = np.isin(i.astype(np.int64) * parts.n + j, keys)
    return cfg, parts, o, count0, rows, (len(i), int(acc.sum()), int((~acc).sum()))


# least (on-cutoff pairs, accepted, rejected) for a case to count as testing the decision
CUTOFF_FLOOR = {3: (10000, 1000, 1000), "dam2d": (5000, 500, 500), "channel2d": (500, 20, 20)}


def check_cutoff_case(case, shift):
    cfg, parts, o, count0, rows, stats = cutoff_reference(case, shift)
    base = case.split("_r")[0]
    need = CUTOFF_FLOOR[3] if cases.get(case).dim == 3 else CUTOFF_FLOOR[base]
    print("%s shift %s: %d on-cutoff pairs, %d accepted, %d rejected" % ((case, shift) + stats))
    assert all(s >= m for s, m in zip(stats, need)), (stats, need)
    with MphSolver(cfg, parts) as s:
        assert np.array_equal(s.get("NeighborCount"), count0)
        s.step(1)
        counts, offsets, ids = s.neighbor_rows()
        assert np.array_equal(counts, o.get("NeighborCount"))
        assert np.array_equal(s.get("NeighborCount"), counts)
        assert np.array_equal(ids, np.concatenate(rows)), [
            i for i in range(parts.n) if not np.array_equal(ids[offsets[i]:offsets[i + 1]], rows[i])][:10]
        # the on-cutoff pairs lie beyond every pass radius: the sums take none of them
        check_fields_against_oracle(s, o, parts, 0)


def _cutoff_params():
    """Every on-cutoff case as generated and under both translations.  seam3d and channel3d fill a
    periodic axis to half a spacing from its faces: 0.53 dx along z moves both clouds out of their
    domains, and so does 2/3 dx along y for seam3d, so there the z offset is 0.23 dx ("seam") and
    seam3d has the one translation."""
    out = []
    for case in cases.CUTOFF_CASES:
        base = case.split("_r")[0]
        shifts = {"seam3d": ("none", "seam"), "channel3d": ("none", "seam", "b")}.get(base, ("none", "a", "b"))
        out += [(case, s) for s in shifts]
    return out


@pytest.mark.parametrize("case,shift", _cutoff_params())
def test_gpu_on_cutoff_lattice_matches_oracle(case, shift, monkeypatch):
    """NeighborCount at creation, and NeighborCount, every neighbour set and all fields after the
    first step, on lattices with tens of thousands of pairs on the cutoff -- as generated (particles
    on the GPU's cell edges, where the search trims its column ranges in FP32) and translated off
    the cell edges by two offsets.  The search at creation runs on the positions as given and the
    first step's on those after calculatePeriodicBoundary (main.cpp:3330: with DomainMin != 0 its
    (x - min) mod w + min rounds, and moves thousands of these decisions again) -- no sum has
    touched either, no case here has moving walls, so both inputs are the oracle's bit for bit;
    later steps are not compared (module docstring).  First the test shows that it tests something:
    the counted on-cutoff pairs and how many of them the oracle takes and leaves."""
    monkeypatch.setenv("MPH_LIST_FULL", "1")
    check_cutoff_case(case, shift)


def test_gpu_on_cutoff_lattice_other_cell_order(monkeypatch):
    """box3d at 2.9 once more with another contiguous cell axis (MPH_SLAB_PERM=3), and with it
    another axis for the column trimming."""
    monkeypatch.setenv("MPH_LIST_FULL", "1")
    monkeypatch.setenv("MPH_SLAB_PERM", "3")
    check_cutoff_case("box3d_r292929", "none")


# --- C. row jumps -----------------------------------------------------------------------------

def check_layout(s, n, jumps_expected=True):
    """The layout's own invariants after a search with the whole lists: returns it."""
    lay = s.list_layout()
    count = s.get("NeighborCount")
    entries = int(np.minimum(count, MAX_NEIGHBOR).sum())
    mean, _ = s.list_stats()
    print("list layout:", lay, "entries", entries)
    assert lay["waves"] == (n + 63) // 64
    if jumps_expected:
        assert lay["waves_jumped"] > 0 and lay["jumps"] >= lay["waves_jumped"] and lay["gap_rows"] > 0
    assert lay["max_jumps"] <= K_MAX_JUMPS
    # the rows outside the gaps are the entries: mph_list_stats sums, per lane, its rows less its gap
    # rows (mean x n = sum(rows) - gap rows), and that is every neighbour up to 512 per particle
    assert abs(mean * n - entries) < 1e-6 * max(entries, 1), (mean * n, entries)
    assert lay["max_rows"] * n >= entries + lay["gap_rows"]
    return lay


def test_gpu_row_jumps_happen_off_the_lattice(monkeypatch):
    """box3d_jit: after a step some waves did jump rows (if the heuristic stopped firing every
    neighbour-set test would still pass on plain rows), none more than kMaxJumps times, and the
    rows outside the gaps hold every neighbour."""
    monkeypatch.setenv("MPH_LIST_FULL", "1")
    cfg, parts = cases.get("box3d_jit").build()
    with MphSolver(cfg, parts) as s:
        s.step(1)
        check_layout(s, parts.n)
        counts, offsets, ids = s.neighbor_rows()   # decodes every lane: rows less gaps == NeighborCount
        assert len(ids) == int(np.minimum(counts, MAX_NEIGHBOR).sum())


def test_gpu_row_jumps_with_long_lists(monkeypatch):
    """box3d at 3.1/3.1/3.1 with +-0.3 dx offsets (up to 149 neighbours), after 1 and after 5 steps:
    waves jump, a wave whose highest row reached kAlignRows stops jumping and its lanes' lists run
    on contiguously past row 128 (max rows >= 128) above the gaps below it, and the sets decoded
    from those rows equal the oracle's for every particle."""
    from oracle_bindings import OracleSolver
    monkeypatch.setenv("MPH_LIST_FULL", "1")
    cfg, parts = cases.get("box3d_r313131_jit").build()
    o = OracleSolver(cfg, parts)
    o.init()
    with MphSolver(cfg, parts) as s:
        for k in (1, 4):
            s.step(k)
            o.step(k)
            lay = check_layout(s, parts.n)
            assert lay["max_rows"] >= K_ALIGN_ROWS, lay
            counts, offsets, ids = s.neighbor_rows()
            assert np.array_equal(counts, o.get("NeighborCount"))
            for i in range(parts.n):
                assert np.array_equal(ids[offsets[i]:offsets[i + 1]], np.sort(o.neighbors(i))), i


def test_gpu_rows_never_jump_in_2d(monkeypatch):
    """dam2d: the 2-D search never jumps (its short lists drift little), so no wave records one."""
    monkeypatch.setenv("MPH_LIST_FULL", "1")
    cfg, parts = cases.get("dam2d").build()
    with MphSolver(cfg, parts) as s:
        s.step(1)
        lay = check_layout(s, parts.n, jumps_expected=False)
        assert lay["jumps"] == 0 and lay["waves_jumped"] == 0 and lay["gap_rows"] == 0
