"""GPU parity: the HIP path (libmph_gpu.so through the C ABI) against the reference's golden
vectors and against the CPU oracle on the same inputs.

Tolerances (FP64; the GPU sums neighbours in its own order with FMA, so results differ from the
reference by reassociation only; SURVEY 8c measured the chaotic growth of such differences):
  * NeighborCount / InitialStructureNeighborCount:  bit-exact (integer).
  * positions:   |dx|_inf <= 1e-12 m up to 100 steps, <= 1e-10 m at 1000 steps (dx = 1e-3 m).
  * velocities:  |dv|_inf <= 1e-9 m/s up to 100 steps, <= 1e-7 m/s at 1000 steps.
  * pressures / other per-step sums (one step): |d|_inf <= 1e-9 * max|ref| + 1e-12;
    PressureP at 10/100 steps <= 1e-8 * max|P| + 1e-9, at 1000 steps <= 1e-6 * max|P|.
  * elastic tensors (DeformGradient, Strain, Stress): <= 1e-9 * max|ref| + 1e-12.
"""
import numpy as np
import pytest

from golden_utils import CASES, Golden, restrict
from particlemethod_fsi_amd import MphSolver, cases

pytestmark = pytest.mark.gpu


# absolute floors: the roundoff level of each quantity (P ~ Kappa * VolStrainP, so one ulp of
# VolStrainP ~ 1e-16 is 1e-12 Pa; at step 1 the reference's P is itself pure roundoff ~4e-11)
# Elastic tensors: at rest F = I + O(ulp), so Strain is pure roundoff (~1e-16) and Stress ~
# (lambda + 2 mu) * 1e-15 ~ 1e-10 Pa until gravity loads the solid.
FLOOR = {"PressureP": 1e-9, "PressureA": 1e-9, "Force": 1e-15, "Acceleration": 1e-12,
         "VolStrainP": 1e-13, "DivergenceP": 1e-12, "DensityA": 1e-13, "GravityCenter": 1e-16,
         "DeformGradient": 1e-13, "Strain": 1e-13, "Stress": 1e-8,
         "VirialStressAtParticle": 1e-9, "VirialPressureAtParticle": 1e-9}


def tol(field: str, step: int, ref: np.ndarray) -> float:
    scale = float(np.nanmax(np.abs(ref))) if ref.size and ref.dtype.kind == "f" else 0.0
    long = step >= 1000
    if field == "Position":
        return 1e-10 if long else 1e-12
    if field == "Velocity":
        return 1e-7 if long else 1e-9
    if field == "PressureP" and step > 1:
        return (1e-6 * scale + 1e-9) if long else (1e-8 * scale + 1e-9)
    return 1e-9 * scale + FLOOR.get(field, 1e-12)


def compare(g: Golden, solver: MphSolver, step: int):
    report = {}
    if g.has(step, "VirialStressAtParticle"):
        solver.compute_virial()   # the reference's VTK-step diagnostic, main.cpp:672-673
    for f in g.fields(step):
        ref = g.get(step, f)
        mine = restrict(g, f, solver.get(f))
        if ref.dtype.kind != "f":
            assert np.array_equal(mine, ref), "%s step %d %s: %d mismatches" % (
                g.case, step, f, int((mine != ref).sum()))
            continue
        m = ~np.isnan(ref)
        err = float(np.max(np.abs(mine[m] - ref[m]))) if m.any() else 0.0
        report[f] = err
        t = tol(f, step, ref[m])
        assert err <= t, "%s step %d %s: max|diff| %.3e > tol %.3e" % (g.case, step, f, err, t)
    return report


@pytest.mark.parametrize("case", CASES)
def test_gpu_matches_reference_golden(case):
    g = Golden(case)
    cfg, parts = cases.get(case).build()
    with MphSolver(cfg, parts) as s:
        for fn in cases.get(case).init_calls:
            assert fn == "setInitialVelocityProfile", fn
            s.set_initial_velocity_profile()
        assert np.array_equal(s.scalars(), g.z["scalars"])
        compare(g, s, 0)
        done = 0
        for step in g.steps:
            s.step(step - done)
            done = step
            compare(g, s, step)
        assert abs(s.time - g.meta["time"]) == 0.0


def oracle_rel(parts) -> float:
    """Relative bound of the per-step sums against the oracle.  FSI: the solid runs at dt*c/dx =
    0.95 and amplifies reassociation differences (~10x per few steps); fluid next to it inherits
    them, hence the wider relative bound there."""
    solid = (parts.property >= 2) & (parts.property < 4)
    return 1e-7 if solid.any() else 1e-8


def check_fields_against_oracle(s, o, parts, k):
    """One step's state against the oracle's: NeighborCount bit-exact, every field within the
    bounds of this module's docstring (k: the step, for the failure message)."""
    solid = (parts.property >= 2) & (parts.property < 4)
    rel = oracle_rel(parts)
    assert np.array_equal(s.get("NeighborCount"), o.get("NeighborCount")), k
    for f in ["Position", "Velocity", "Force", "PressureP", "VolStrainP", "DivergenceP",
              "DensityA", "GravityCenter", "Acceleration"]:
        a, b = s.get(f), o.get(f)
        if f in ("DensityA", "GravityCenter"):
            a, b = a[~solid], b[~solid]
        if not b.size:   # an all-solid case (bar3d): no row of these two is defined
            continue
        scale = float(np.max(np.abs(b)))
        t = {"Position": 1e-12, "Velocity": 1e-9}.get(f, rel * scale + FLOOR.get(f, 1e-12))
        assert float(np.max(np.abs(a - b))) <= t, (k, f, float(np.max(np.abs(a - b))), t)
    if solid.any():
        for f in ["DeformGradient", "Stress", "Strain"]:
            a, b = s.get(f)[solid], o.get(f)[solid]
            # the solid runs at dt*c/dx = 0.95 (ElasticDt 1e-4, c = 9.5 m/s): near the
            # stability limit reassociation differences grow ~10x per few steps
            t = 1e-8 * float(np.max(np.abs(b))) + FLOOR[f]
            assert float(np.max(np.abs(a - b))) <= t, (k, f)


def check_virial_against_oracle(s, o, parts, k):
    """The virial diagnostic of the current state against the oracle's."""
    rel = oracle_rel(parts)
    s.compute_virial()
    o.call("calculateVirialStressAtParticle")
    for f in ["VirialStressAtParticle", "VirialPressureAtParticle"]:
        a, b = s.get(f), o.get(f)
        t = rel * float(np.max(np.abs(b))) + FLOOR[f]
        assert float(np.max(np.abs(a - b))) <= t, (k, f, float(np.max(np.abs(a - b))), t)


def run_against_oracle_every_step(cfg, parts, nsteps):
    """Step-by-step against the oracle: NeighborCount and all fields after every step, the virial
    after the last."""
    from oracle_bindings import OracleSolver
    o = OracleSolver(cfg, parts)
    o.init()
    with MphSolver(cfg, parts) as s:
        for k in range(nsteps):
            s.step(1)
            o.step(1)
            check_fields_against_oracle(s, o, parts, k)
            if k == nsteps - 1:
                check_virial_against_oracle(s, o, parts, k)


@pytest.mark.parametrize("case,nsteps", [("dam2d", 20), ("gate3d", 12), ("gate3d_sub", 20),
                                          ("box3d_st", 20), ("rolling2d", 20), ("rolling3d", 20),
                                          ("turek2d", 20), ("movwall3d", 10), ("hydro2d", 20),
                                          ("channel3d", 10), ("seam3d", 10), ("longz3d", 10)])
def test_gpu_matches_oracle_every_step(case, nsteps):
    """Step-by-step against the oracle: all fields, including the ones the golden files do not
    store at every step (Force, DensityA, GravityCenter, VolStrainP, ...).  gate3d (ElasticDt =
    Dt) is physically unstable after ~20 steps in the reference itself (perturbations grow ~2x per
    step), so it is checked over its stable window only."""
    cfg, parts = cases.get(case).build()
    run_against_oracle_every_step(cfg, parts, nsteps)


@pytest.mark.parametrize("case", ["dam2d", "box3d_jit"])
def test_gpu_neighbor_sets_match_reference_golden(case, monkeypatch):
    """The neighbour SETS themselves (mph_neighbor_rows), not only their sizes: after one step every
    particle's row equals the reference's Neighbor[i][0..count) (main.cpp:1764-1772, sorted; the
    golden rows of make_golden.py) -- on the lattice (dam2d) and off it (box3d_jit).  MPH_LIST_FULL=1:
    the lists keep the reference's whole set (by default only the pairs within the passes' radius)."""
    monkeypatch.setenv("MPH_LIST_FULL", "1")
    g = Golden(case)
    cfg, parts = cases.get(case).build()
    with MphSolver(cfg, parts) as s:
        s.step(1)
        counts, offsets, ids = s.neighbor_rows()
        assert np.array_equal(counts, np.diff(g.get(1, "nbr_offsets")))
        assert np.array_equal(offsets, g.get(1, "nbr_offsets"))
        assert np.array_equal(ids, g.get(1, "nbr_ids"))
        # a sub-range returns the same rows
        c2, o2, i2 = s.neighbor_rows(1000, 500)
        assert np.array_equal(i2, ids[offsets[1000]:offsets[1500]])


@pytest.mark.parametrize("case,nsteps", [("box3d", 10), ("gate3d_jit", 10), ("seam3d", 10)])
def test_gpu_neighbor_sets_match_oracle(case, nsteps, monkeypatch):
    """Neighbour sets after several steps against the oracle's lists (bit-identical to the
    reference's): every row, as sets of original indices (MPH_LIST_FULL=1: the whole lists)."""
    from oracle_bindings import OracleSolver
    monkeypatch.setenv("MPH_LIST_FULL", "1")
    cfg, parts = cases.get(case).build()
    o = OracleSolver(cfg, parts)
    o.init()
    o.step(nsteps)
    with MphSolver(cfg, parts) as s:
        s.step(nsteps)
        counts, offsets, ids = s.neighbor_rows()
        assert np.array_equal(counts, o.get("NeighborCount"))
        for i in range(parts.n):
            assert np.array_equal(ids[offsets[i]:offsets[i + 1]], np.sort(o.neighbors(i))), (case, i)


@pytest.mark.parametrize("case", ["box3d_jit", "gate3d_jit", "dam2d"])
def test_gpu_trimmed_lists_equal_full_lists(case, monkeypatch):
    """The default lists keep only the pairs within the largest radius of the passes' sums
    (DevParams.rlf); NeighborCount still counts every neighbour within MaxRadius + MARGIN.  Against
    the reference's whole lists (MPH_LIST_FULL=1): NeighborCount and every field bit-identical (a
    term outside its radius is never taken, so the shell's pairs add nothing), and the trimming did
    happen: off the lattice (*_jit) the stored lists are strictly shorter on average
    (mph_list_stats: the mean stored list length), on the lattice (dam2d: no pair between 2.5
    and 2.6 dx) equally long."""
    cfg, parts = cases.get(case).build()
    out, mean_len = {}, {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MPH_LIST_FULL", mode)
        with MphSolver(cfg, parts) as s:
            s.step(7)
            out[mode] = {f: s.get(f) for f in ["NeighborCount", "Position", "Velocity", "PressureP", "Force",
                                               "DensityA", "VolStrainP", "DivergenceP"]}
            mean_len[mode] = s.list_stats()[0]
    assert np.array_equal(out["0"]["NeighborCount"], out["1"]["NeighborCount"])
    for f in out["0"]:
        assert np.array_equal(out["0"][f], out["1"][f], equal_nan=True), f
    # the whole lists are NeighborCount long; the trimmed ones shorter where the shell holds pairs
    assert mean_len["1"] == pytest.approx(float(out["1"]["NeighborCount"].mean()))
    if case.endswith("_jit"):
        assert mean_len["0"] < mean_len["1"], mean_len
    else:
        assert mean_len["0"] == mean_len["1"], mean_len


@pytest.mark.parametrize("case", ["box3d_jit", "gate3d_jit"])
def test_gpu_profile_graphs_leave_state_unchanged(case):
    """mph_profile_graphs replays the search, pass A and pass B over the last step's state: positive
    times (pass B not measured with elastic slots), and the run continues bit for bit as without."""
    cfg, parts = cases.get(case).build()
    out = []
    for profiled in (False, True):
        with MphSolver(cfg, parts) as s:
            s.step(3)
            if profiled:
                t = s.profile_graphs(4)
                assert t["neighbors"] > 0 and t["pass_a"] > 0
                assert (t["pass_b"] is None) == (case == "gate3d_jit")
            s.step(5)
            out.append({f: s.get(f) for f in ["NeighborCount", "Position", "Velocity", "PressureP", "Force"]})
    for f in out[0]:
        assert np.array_equal(out[0][f], out[1][f], equal_nan=True), f


def test_gpu_deterministic_rerun():
    cfg, parts = cases.get("gate2d").build()
    outs = []
    for _ in range(2):
        with MphSolver(cfg, parts) as s:
            s.step(25)
            outs.append((s.get("Position"), s.get("Velocity"), s.get("PressureP")))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_gpu_vtk_byte_identical_at_step0(tmp_path):
    import gzip
    import hashlib
    import os
    g = Golden("dam2d")
    cfg, parts = cases.get("dam2d").build()
    with MphSolver(cfg, parts) as s:
        p = str(tmp_path / "output.vtk")
        s.write_vtk(p)
        assert hashlib.sha256(open(p, "rb").read()).digest() == bytes(g.z["sha256/output.vtk"])
        q = str(tmp_path / "dam000.prof")
        s.write_prof(q)
        assert hashlib.sha256(open(q, "rb").read()).digest() == bytes(g.z["sha256/dam000.prof"])


CHUNK_FIELDS = ["Position", "Velocity", "Force", "Acceleration", "GravityCenter", "PressureP",
                "PressureA", "DensityA", "VolStrainP", "DivergenceP", "NeighborCount", "Kappa",
                "DeformGradient", "Strain", "Stress"]


@pytest.mark.parametrize("case", ["box3d", "box3d_st", "gate2d", "bar2d"])
def test_gpu_graph_chunking_equivalence(case):
    """mph_step(8) (one 8-step graph, whose first 7 steps skip the output-only stores of pass A
    and pass B) == 8 x mph_step(1) (every step stores), bitwise, for every field mph_get returns
    and the virial diagnostic: without surface tension (box3d), with it (box3d_st) and with the
    elastic clamp that zeroes Force after pass B (gate2d, bar2d)."""
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


@pytest.mark.parametrize("case", ["box3d_st", "gate2d"])
def test_gpu_remainder_steps_equivalence(case):
    """mph_step(13) (one 8-step graph, then 4 single steps without the output-only stores and one
    with them) == 13 x mph_step(1), bitwise, for every field mph_get returns and the virial."""
    cfg, parts = cases.get(case).build()
    with MphSolver(cfg, parts) as a, MphSolver(cfg, parts) as b:
        a.step(13)
        for _ in range(13):
            b.step(1)
        for f in CHUNK_FIELDS:
            assert np.array_equal(a.get(f), b.get(f), equal_nan=True), (case, f)
        a.compute_virial()
        b.compute_virial()
        for f in ["VirialStressAtParticle", "VirialPressureAtParticle"]:
            assert np.array_equal(a.get(f), b.get(f), equal_nan=True), (case, f)


@pytest.mark.parametrize("case", ["box3d", "box3d_st", "gate2d", "bar2d"])
def test_gpu_step_batching_equivalence(case):
    """mph_set_step_batching: 21 x mph_step(1) (two 8-step graphs launched by the calls, 5 steps
    pending) then mph_get == mph_step(21), bitwise, for every field and the virial; Time advances
    per call; after a flush the context steps on unbatched (the drop-in loop of INTEGRATION.md)."""
    cfg, parts = cases.get(case).build()
    with MphSolver(cfg, parts) as a, MphSolver(cfg, parts) as b:
        a.step(21)
        b.step_batching(True)
        for k in range(21):
            b.step(1)
        assert a.time == b.time
        for f in CHUNK_FIELDS:   # the first get launches the 5 pending steps
            assert np.array_equal(a.get(f), b.get(f), equal_nan=True), (case, f)
        a.compute_virial()
        b.compute_virial()
        for f in ["VirialStressAtParticle", "VirialPressureAtParticle"]:
            assert np.array_equal(a.get(f), b.get(f), equal_nan=True), (case, f)
        a.step(3)
        for _ in range(3):
            b.step(1)
        b.step_batching(False)   # flushes
        b.step(2)
        a.step(2)
        for f in ["Position", "Velocity", "Force", "PressureP"]:
            assert np.array_equal(a.get(f), b.get(f), equal_nan=True), (case, f)


def test_gpu_step_batching_reports_errors():
    """With step batching a diverged state is still MPH_ERR_NONFINITE: from a later mph_step once
    the launched batch's flags have landed, or at the latest from mph_synchronize."""
    from particlemethod_fsi_amd.solver import MphError
    cfg, parts = cases.get("dam2d").build()
    with MphSolver(cfg, parts) as s:
        s.step(2)
        pos = s.get("Position")
        pos[100, 0] = np.nan
        s.set("Position", pos)
        s.step_batching(True)
        with pytest.raises(MphError) as e:
            for _ in range(24):
                s.step(1)
            s.synchronize()
        assert e.value.code == -9


def test_gpu_nonfinite_state_is_an_error_not_a_fault():
    """A diverged state (NaN position) is reported as MPH_ERR_NONFINITE by the next step; every
    index the kernels derive from it stays in range (no device fault)."""
    from particlemethod_fsi_amd.solver import MphError
    cfg, parts = cases.get("dam2d").build()
    with MphSolver(cfg, parts) as s:
        s.step(2)
        pos = s.get("Position")
        pos[100, 0] = np.nan
        pos[200, 1] = np.inf
        s.set("Position", pos)
        with pytest.raises(MphError) as e:
            s.step(1)
        assert e.value.code == -9


def test_gpu_vtk_async_equals_sync(tmp_path):
    """mph_write_vtk_async snapshots the state when called: its file equals mph_write_vtk's of the
    same step even though the solver has advanced while the background thread writes."""
    cfg, parts = cases.get("gate2d").build()
    with MphSolver(cfg, parts) as s:
        s.step(3)
        a, b = str(tmp_path / "sync.vtk"), str(tmp_path / "async.vtk")
        s.write_vtk(a)
        s.write_vtk_async(b)
        s.step(5)
        s.output_wait()
        assert open(a, "rb").read() == open(b, "rb").read()


def test_gpu_vtu_matches_state(tmp_path):
    """mph_write_vtu of a stepped FSI context: the binary file holds exactly the float32 values of
    the state mph_get returns (the fields of the ASCII writer)."""
    from particlemethod_fsi_amd.solver import read_vtu
    cfg, parts = cases.get("gate2d").build()
    with MphSolver(cfg, parts) as s:
        s.step(5)
        path = str(tmp_path / "g.vtu")
        s.write_vtu(path)
        d = read_vtu(path)
        f32 = lambda a: np.asarray(a).astype(np.float32)  # noqa: E731
        np.testing.assert_array_equal(d["Points"], f32(s.get("Position")))
        np.testing.assert_array_equal(d["displacement"], f32(s.get("Position") - s.get("InitialPosition")))
        np.testing.assert_array_equal(d["stress"], f32(s.get("Stress").reshape(-1, 9)))
        np.testing.assert_array_equal(d["velocity"], f32(s.get("Velocity")))
        np.testing.assert_array_equal(d["force"], f32(s.get("Force")))
        np.testing.assert_array_equal(d["neighbor"], s.get("NeighborCount"))
        np.testing.assert_array_equal(d["label"], parts.property)


@pytest.mark.parametrize("case", ["bar2d", "bar3d", "gate3d_sub", "gate2d_sub", "hydro2d", "turek2d"])
def test_gpu_structure_init_equals_host_build(case, monkeypatch):
    """calculateInitialNeighbor + calculateNormalizer run on the device (launch_struct_init) for a
    single context: the counts, Normalizer and Lame constants equal the host build
    (mph_structure_init, pinned to the reference by the s0 goldens) bit for bit, and the lists
    (sorted like the host's) give bitwise the same steps as a context built on the host."""
    check_structure_init_equals_host_build(case, monkeypatch)


def check_structure_init_equals_host_build(case, monkeypatch):
    from particlemethod_fsi_amd import solver
    import ctypes
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


CASES_3D = [c for c in CASES if cases.get(c).dim == 3]


@pytest.mark.parametrize("perm", [1, 2, 3, 4])
@pytest.mark.parametrize("case", CASES_3D)
def test_gpu_cell_orders_match_golden(case, perm, monkeypatch):
    """Every cell order of the z-slab contexts (DevParams.perm, forced on a single context through
    MPH_SLAB_PERM) gives the reference's neighbour counts and fields within the same tolerances:
    the order changes which cells are contiguous and the order of each neighbour list, nothing
    else."""
    monkeypatch.setenv("MPH_SLAB_PERM", str(perm))
    g = Golden(case)
    cfg, parts = cases.get(case).build()
    with MphSolver(cfg, parts) as s:
        for fn in cases.get(case).init_calls:
            s.set_initial_velocity_profile()
        compare(g, s, 0)
        done = 0
        for step in g.steps[:2]:
            s.step(step - done)
            done = step
            compare(g, s, step)


@pytest.mark.parametrize("case", ["box3d", "box3d_st", "gate2d", "dam2d", "seam3d", "gate3d_sub"])
def test_gpu_xcd_balanced_map_bitwise(case, monkeypatch):
    """The work-balanced XCD block map of passes A and B (xcd_split_block in the next step's
    k_rank_scatter, then list_block), which by default runs only from 2^20 particles, forced on
    small cases (MPH_XCD_BAL_MIN=0; their few blocks also
    trip the map's fallback to equal ranges when a range exceeds its slack): it only changes which
    block handles which wave, so every field equals the default run bit for bit."""
    cfg, parts = cases.get(case).build()
    fields = ["Position", "Velocity", "PressureP", "PressureA", "NeighborCount", "Force", "Acceleration",
              "DensityA", "VolStrainP", "DivergenceP", "GravityCenter"]
    out = {}
    for mode in ("0", None):
        if mode is None:
            monkeypatch.delenv("MPH_XCD_BAL_MIN", raising=False)
        else:
            monkeypatch.setenv("MPH_XCD_BAL_MIN", mode)
        with MphSolver(cfg, parts) as s:
            s.step(3)
            s.step(4)
            out[mode] = {f: s.get(f) for f in fields}
    for f in fields:
        assert np.array_equal(out["0"][f], out[None][f]), (f, float(np.max(np.abs(out["0"][f] - out[None][f]))))


@pytest.mark.parametrize("lanes", ["1", "2", "4", "8"])
@pytest.mark.parametrize("case", ["bar2d", "gate3d_sub"])
def test_gpu_struct_lanes_match_oracle(case, lanes, monkeypatch):
    """The elastic kernels with 1, 2, 4 or 8 lanes per structure slot (MPH_STRUCT_LANES; by
    default the count follows the slot count): each lane sums every G-th list entry, the group adds
    the shares in a butterfly -- reassociation only, within the solid bounds above.  Two batches of
    5 steps, so that the output tensors F, E, S (stored on a batch's last step only) are checked
    after a batch whose earlier steps skipped them."""
    from oracle_bindings import OracleSolver
    monkeypatch.setenv("MPH_STRUCT_LANES", lanes)
    cfg, parts = cases.get(case).build()
    o = OracleSolver(cfg, parts)
    o.init()
    solid = (parts.property >= 2) & (parts.property < 4)
    with MphSolver(cfg, parts) as s:
        for k in (5, 10):
            s.step(5)
            o.step(5)
            for f in ["Position", "Velocity"]:
                t = {"Position": 1e-12, "Velocity": 1e-9}[f]
                assert float(np.max(np.abs(s.get(f) - o.get(f)))) <= t, (k, f)
            for f in ["DeformGradient", "Stress", "Strain"]:
                a, b = s.get(f)[solid], o.get(f)[solid]
                t = 1e-8 * float(np.max(np.abs(b))) + FLOOR[f]
                assert float(np.max(np.abs(a - b))) <= t, (k, f, float(np.max(np.abs(a - b))), t)
