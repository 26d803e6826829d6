"""GPU parity: the HIP path (libmph_gpu.so through the C ABI) against the reference's golden
vectors and against the CPU oracle on the same inputs.

Tolerances -- the numbers, and the reasons for them, live in tests/parity.py, which every parity
test asserts through.  In short (FP64; the GPU sums neighbours in its own order with FMA, so results
differ from the reference by reassociation only):
  * NeighborCount / InitialStructureNeighborCount:  bit-exact (integer).
  * positions:   |dx|_inf <= 1e-12 m up to 100 steps, <= 1e-10 m at 1000 steps (dx = 1e-3 m).
  * velocities:  |dv|_inf <= 1e-9 m/s up to 100 steps, <= 1e-7 m/s at 1000 steps.
  * pressures / other per-step sums (one step): |d|_inf <= 1e-9 * max|ref| + the field's floor;
    PressureP at 10/100 steps <= 1e-8 * max|P| + 1e-9, at 1000 steps <= 1e-6 * max|P|.
  * elastic tensors (DeformGradient, Strain, Stress): <= 1e-9 * max|ref| + floor.
"""
import numpy as np
import pytest

from golden_utils import CASES, Golden
from parity import (CHUNK_FIELDS, REL_STEPS, assert_close, check_structure_init_equals_host_build, compare,
                    run_against_oracle_every_step)
from particlemethod_fsi_amd import MphSolver, cases

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("case", ["bar2d", "bar3d", "gate3d_sub", "gate2d_sub", "hydro2d", "turek2d", "mix2d",
                                  "mix3d"])
def test_gpu_structure_init_equals_host_build(case, monkeypatch):
    """calculateInitialNeighbor + calculateNormalizer run on the device (launch_struct_init) for a
    single context: the counts, Normalizer and Lame constants equal the host build
    (mph_structure_init, pinned to the reference by the s0 goldens) bit for bit, and the lists
    (sorted like the host's) give bitwise the same steps as a context built on the host."""
    check_structure_init_equals_host_build(case, monkeypatch)


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
@pytest.mark.parametrize("case", ["bar2d", "gate3d_sub", "mix2d", "mix3d"])
def test_gpu_struct_lanes_match_oracle(case, lanes, monkeypatch):
    """The elastic kernels with 1, 2, 4 or 8 lanes per structure slot (MPH_STRUCT_LANES; by
    default the count follows the slot count): each lane sums every G-th list entry, the group adds
    the shares in a butterfly -- reassociation only, within the tensor bound of the per-step oracle check.  Two batches of
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
                assert_close(f, s.get(f), o.get(f), REL_STEPS, context=(k,))
            for f in ["DeformGradient", "Stress", "Strain"]:
                assert_close(f, s.get(f), o.get(f), REL_STEPS, rows=solid, context=(k,))
