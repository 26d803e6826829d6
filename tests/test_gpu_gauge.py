"""GPU: the free-surface gauges (include/mph_gpu.h mph_gauge_configure / mph_gauge_grid, kernels in
csrc/mph_gauge.hip).

A gauge's record {COUNT, TOP, BOTTOM, WET} is an integer count, a maximum, a minimum and the
population of a bit set, so every value here is compared with == against numpy on mph_get data
(tests/gauge_ref.py): the positions from before the sampled step, wrapped like a particle.  Each
definition test first asserts, on the initial state its first sample reads, that no fluid particle
lies within 1e-9 of a gauge's cylinder.  The later steps are compared with == whatever the
distances: the kernel evaluates the reference's expression for r operation by operation in FP64
(subtraction, Mod, product, sum, square root, each correctly rounded on both sides), so r has the
same bits and r < h falls the same way.  It does come close: before step 3 of box3d_jit a fluid
particle lies 6.7e-11 from the cylinder of the first gauge along axis 0 (the CPU oracle's
positions), 1e7 times the rounding error of r, and the records agree there too.
"""
import numpy as np
import pytest

import gauge_ref
from particlemethod_fsi_amd import MphSolver, cases
from particlemethod_fsi_amd.mphio import Cuboid
from particlemethod_fsi_amd.solver import GAUGE_CHANNELS as C, MphError, Slab, monitor_gauges, monitor_split

pytestmark = pytest.mark.gpu

BOX_GAUGES = [(0.00613, 0.01021, 0.00587), (0.00071, 0.00813, 0.00493), (0.0353, 0.0421, 0.0061)]
DAM_GAUGES = [(0.0213, 0.0117, 0.0), (0.0871, 0.0313, 0.0)]
SEAM_GAUGE = (0.01531, 0.03931, 0.01013)
GATE_GAUGES = [(0.00613, 0.01021, 0.00387), (0.00587, 0.01957, 0.00411), (0.0303, 0.0401, 0.0041)]


def _run(case, gauges, axis, steps, ref_axis=None):
    """`steps` single steps with the gauges along `axis`, every sample checked against numpy (along
    ref_axis where the configured axis is -1) -> (records [steps, ngauge, 4], the last step's
    contributing particles per gauge)."""
    cfg, parts = cases.get(case).build()
    h = cfg.radius_ratio_p * cfg.particle_spacing
    ra = axis if ref_axis is None else ref_axis
    out, contrib = [], None
    with MphSolver(cfg, parts) as s:
        s.monitor(stride=1, capacity=2, gauges=gauges, gauge_axis=axis)
        T = s.get("Property")
        for k in range(steps):
            before = s.get("Position")
            s.step(1)
            rows, lost = s.monitor_read()
            assert rows.shape == (1, 32 + 4 * len(gauges)) and lost == 0
            assert rows[0, 0] == k + 1
            rec = s.monitor_gauges(rows[0])
            x, lo, w = gauge_ref.wrapped(cfg, before)
            contrib = []
            for q, g in enumerate(gauges):
                ref, xs = gauge_ref.record(cfg, x, lo, w, T, g, ra, h, guard=k == 0)
                print("%s axis %d step %d gauge %d: %r numpy %r" % (case, axis, k + 1, q, tuple(rec[q]), ref))
                assert tuple(rec[q]) == ref, (case, axis, k, q, tuple(rec[q]), ref)
                contrib.append(xs)
            out.append(rec)
    return np.array(out), contrib


# ---- 1. definition, 3-D ------------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_definition_3d(axis):
    # box3d: fluid over x, z in (0, 0.012), y in (0.003, 0.02).  In the fluid, against the x = 0
    # wall, in empty space; the three axes take both cell forms whatever the case's cell order
    rec, _ = _run("box3d_jit", BOX_GAUGES, axis, 5)
    assert (rec[:, :2, C["COUNT"]] >= 100).all()
    assert (rec[:, :2, C["WET"]] >= 10).all()
    for k in range(5):
        assert tuple(rec[k, 2]) == (0.0, -np.inf, np.inf, 0.0)
    if axis == 1:
        # at rest (the first sample reads the initial state): 326 / 219 particles, 17 wet bins
        assert list(rec[0, :, C["COUNT"]]) == [326.0, 219.0, 0.0] and list(rec[0, :, C["WET"]]) == [17.0, 17.0, 0.0]
        # not vacuous: the surface moves (gravity is (0, -1, 0))
        assert len(set(rec[:, 0, C["TOP"]])) > 1, rec[:, 0, C["TOP"]]
    if axis == 0:
        assert list(rec[0, :, C["COUNT"]]) == [230.0, 229.0, 0.0] and list(rec[0, :2, C["WET"]]) == [12.0, 12.0]


def test_default_axis_is_gravitys():
    a, _ = _run("box3d_jit", BOX_GAUGES, -1, 3, ref_axis=1)
    b, _ = _run("box3d_jit", BOX_GAUGES, 1, 3)
    assert a.tobytes() == b.tobytes()


# ---- 2. definition, 2-D ------------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1])
def test_definition_2d(axis):
    rec, _ = _run("dam2d", DAM_GAUGES, axis, 5)
    if axis == 1:
        assert tuple(rec[0, 0, [C["COUNT"], C["WET"]]]) == (485.0, 97.0)
        assert all(tuple(rec[k, 1]) == (0.0, -np.inf, np.inf, 0.0) for k in range(5))
    else:
        assert list(rec[0, :, C["COUNT"]]) == [250.0, 250.0] and list(rec[0, :, C["WET"]]) == [50.0, 50.0]


def test_axis_2_is_an_error_in_2d():
    cfg, parts = cases.get("dam2d").build()
    with MphSolver(cfg, parts) as s:
        with pytest.raises(MphError) as e:
            s.monitor(gauges=DAM_GAUGES, gauge_axis=2)
        assert e.value.code == -1 and "gauges" in str(e.value)


# ---- 3. periodic faces -------------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_gauge_across_the_periodic_face(axis):
    # seam3d: fluid at y < 0.006 and y > 0.034 of a domain periodic at y = 0.04; the line 0.7 mm
    # below the face
    rec, contrib = _run("seam3d", [SEAM_GAUGE], axis, 3)
    if axis != 1:
        y = contrib[0][:, 1]
        assert (y < 0.01).any() and (y > 0.03).any()
    else:
        cfg = cases.get("seam3d").build()[0]
        assert gauge_ref.nbins(cfg, 1) == 40
        assert rec[0, 0, C["WET"]] == 12.0
        for k in range(3):
            assert rec[k, 0, C["TOP"]] > 0.034 and rec[k, 0, C["BOTTOM"]] < 0.006
            assert rec[k, 0, C["WET"]] < 40     # the wetted length is not (TOP - BOTTOM) / dx


# ---- 4. batch shapes ---------------------------------------------------------------------------

def _gate_monitor(s, parts, gauges=GATE_GAUGES):
    st = np.nonzero(parts.property == 2)[0]
    s.monitor(stride=1, capacity=64, track=[int(st[-1]), 5, int(st[0]), 5], probes=GATE_GAUGES, gauges=gauges)


def test_batch_shapes_give_the_same_gauge_samples():
    cfg, parts = cases.get("gate3d_jit").build()
    out = []
    with MphSolver(cfg, parts) as s:        # 29 single steps
        _gate_monitor(s, parts)
        for _ in range(29):
            s.step(1)
        out.append(s.monitor_read())
    with MphSolver(cfg, parts) as s:        # three 8-step batches, then single steps
        _gate_monitor(s, parts)
        s.step(24)
        s.step(5)
        out.append(s.monitor_read())
    with MphSolver(cfg, parts) as s:        # step batching: the steps run at the read's flush
        _gate_monitor(s, parts)
        s.step_batching(True)
        for _ in range(29):
            s.step(1)
        out.append(s.monitor_read())
    with MphSolver(cfg, parts) as s:        # phase timing: direct launches
        _gate_monitor(s, parts)
        s.phase_timing(True)
        s.step(29)
        out.append(s.monitor_read())
    ref, lost = out[0]
    assert ref.shape == (29, 32 + 6 * 4 + 2 * 3 + 4 * 3) and lost == 0
    assert np.array_equal(ref[:, 0], np.arange(1, 30))
    gau = monitor_gauges(ref, 4, 3, 3)
    assert (gau[:, :2, C["COUNT"]] >= 100).all() and (gau[:, 2, C["COUNT"]] == 0).all()
    assert len(set(gau[:, 0, C["TOP"]])) > 1
    for rows, lo in out[1:]:
        assert lo == 0
        assert rows.shape == ref.shape
        assert rows.tobytes() == ref.tobytes()


# ---- 5. no side effect -------------------------------------------------------------------------

def test_gauges_do_not_change_the_run():
    cfg, parts = cases.get("gate3d_jit").build()
    fields = ("Position", "Velocity", "Force", "NeighborCount")
    with MphSolver(cfg, parts) as a, MphSolver(cfg, parts) as b, MphSolver(cfg, parts) as c:
        _gate_monitor(a, parts, gauges=())
        _gate_monitor(b, parts)
        _gate_monitor(c, parts)
        assert a._L.mph_monitor_sample_doubles(a._h) == 32 + 6 * 4 + 2 * 3
        assert b._L.mph_monitor_sample_doubles(b._h) == 32 + 6 * 4 + 2 * 3 + 4 * 3
        a.step(16)
        b.step(16)
        c.step(8)
        _gate_monitor(c, parts, gauges=())     # mph_monitor_configure alone: the gauges are gone
        assert c._L.mph_monitor_sample_doubles(c._h) == 32 + 6 * 4 + 2 * 3
        c.step(8)
        ra, rb, rc = a.monitor_read()[0], b.monitor_read()[0], c.monitor_read()[0]
        assert ra.shape == (16, 62) and rb.shape == (16, 74) and rc.shape == (8, 62)
        # the rest of a sample is what it is without gauges
        assert rb[:, :62].tobytes() == ra.tobytes()
        assert rc[:, 1:].tobytes() == ra[8:, 1:].tobytes()
        for t in monitor_split(rc, 4, 3):
            assert t.shape[0] == 8
        for f in fields:
            ref = a.get(f)
            assert np.array_equal(ref, b.get(f)), f
            assert np.array_equal(ref, c.get(f)), f
        assert a.time == b.time == c.time
    with MphSolver(cfg, parts) as a, MphSolver(cfg, parts) as b:    # and against no monitors at all
        _gate_monitor(b, parts)
        a.step(16)
        b.step(16)
        for f in fields:
            assert np.array_equal(a.get(f), b.get(f)), f


# ---- 6. the map --------------------------------------------------------------------------------

MAP_LATTICES = [(1, 1), (5, 13), (65, 3), (257, 1)]
MAP_ORIGIN = {"box3d_jit": (-0.00213, -0.00111, -0.00217), "dam2d": (-0.01713, -0.00611, 0.0)}


def map_lattice(case, dim, axis, n0, n1):
    """(origin, spacing, count) of a lattice of n0 x n1 lines along `axis` (2-D: n0 n1 lines in a
    row) that starts beside the fluid, off the particles' lattice; a long row runs past the domain
    and wraps."""
    across = [d for d in range(dim) if d != axis]
    n = [n0, n1] if dim == 3 else [n0 * n1]
    count, spacing = [1, 1, 1], [0.0, 0.0, 0.0]
    for k, d in enumerate(across):
        count[d] = n[k]
        spacing[d] = 0.0173119 / n[k] if 1 < n[k] <= 13 else 0.00113719 + 1.1e-5 * k
    return MAP_ORIGIN[case], tuple(spacing), tuple(count)


def map_reference(cfg, x, lo, w, T, origin, spacing, count, axis, h):
    ref = np.zeros((count[2], count[1], count[0], 4))
    for k in range(count[2]):
        for j in range(count[1]):
            for i in range(count[0]):
                pt = [origin[0] + i * spacing[0], origin[1] + j * spacing[1], origin[2] + k * spacing[2]]
                ref[k, j, i] = gauge_ref.record(cfg, x, lo, w, T, pt, axis, h)[0]
    return ref


@pytest.mark.parametrize("case", ["box3d_jit", "dam2d"])
def test_map_against_numpy(case):
    cfg, parts = cases.get(case).build()
    h = cfg.radius_ratio_p * cfg.particle_spacing
    gauges = BOX_GAUGES if case == "box3d_jit" else DAM_GAUGES
    with MphSolver(cfg, parts) as s:
        s.monitor(stride=1, capacity=4, gauges=gauges, gauge_axis=1)
        T = s.get("Property")
        s.step(2)
        before = s.get("Position")
        s.step(1)
        x, lo, w = gauge_ref.wrapped(cfg, before)
        mon = s.monitor_gauges(s.monitor_read()[0][-1])
        # a line at a monitor gauge's point is that step's monitor record
        for q, g in enumerate(gauges):
            one = s.gauge_grid(g, (0.0, 0.0, 0.0), (1, 1, 1), axis=1)
            assert one.shape == (1, 1, 1, 4)
            assert one.reshape(4).tobytes() == mon[q].tobytes(), (q, one, mon[q])
        wet = dry = 0
        for axis in range(cfg.dim):
            for n0, n1 in MAP_LATTICES:
                origin, spacing, count = map_lattice(case, cfg.dim, axis, n0, n1)
                out = s.gauge_grid(origin, spacing, count, axis=axis)
                assert out.shape == (count[2], count[1], count[0], 4)
                ref = map_reference(cfg, x, lo, w, T, origin, spacing, count, axis, h)
                bad = np.nonzero((out != ref).any(axis=-1))
                assert out.tobytes() == ref.tobytes(), (case, axis, count, bad, out[bad][:4], ref[bad][:4])
                assert s.gauge_grid(origin, spacing, count, axis=axis).tobytes() == out.tobytes()
                wet += int((out[..., C["COUNT"]] > 0).sum())
                dry += int((out[..., C["COUNT"]] == 0).sum())
                if n0 == 257:
                    # the row begins or ends outside the domain: the lines out there wrap
                    d = [a for a in range(cfg.dim) if a != axis][0]
                    assert origin[d] < cfg.domain_min[d] or origin[d] + 256 * spacing[d] > cfg.domain_max[d]
        assert wet > 100 and dry > 100     # lines through the fluid and lines in empty space
        # the map changed no state: the monitors go on as they were
        s.step(1)
        assert s.monitor_read()[0][-1, 0] == 4.0


# ---- 7. profile names --------------------------------------------------------------------------

def test_gauge_kernel_in_the_profile():
    cfg, parts = cases.get("box3d_jit").build()
    with MphSolver(cfg, parts) as s:
        s.monitor(stride=2, capacity=8, track=[3], probes=[BOX_GAUGES[0]])
        assert "monitor_gauge" not in s.profile(4)
        s.monitor(stride=2, capacity=8, track=[3], probes=[BOX_GAUGES[0]], gauges=BOX_GAUGES)
        prof = s.profile(4)
        mon = sorted(k for k in prof if k.startswith("monitor"))
        assert mon == ["monitor_final", "monitor_gauge", "monitor_partial", "monitor_probe"], prof.keys()
        assert all(prof[k]["launches"] == 4 for k in mon), prof
        rows, lost = s.monitor_read()
        assert list(rows[:, 0]) == [2.0, 4.0] and lost == 0
        assert (s.monitor_gauges(rows)[:, 0, C["COUNT"]] >= 100).all()


# ---- 8. errors ---------------------------------------------------------------------------------

def test_gauge_argument_errors():
    cfg, parts = cases.get("dam2d").build()
    reach = (2.5 + 0.1) * cfg.particle_spacing   # MaxRadius + MARGIN
    pt = (0.0213, 0.0117, 0.0)
    with MphSolver(cfg, parts) as s:
        bad = [dict(gauges=[pt] * 65), dict(gauges=[pt], gauge_axis=3), dict(gauges=[pt], gauge_axis=-2),
               dict(gauges=[pt], gauge_radius=1.01 * reach), dict(gauges=[pt], gauge_radius=-1e-3)]
        for kw in bad:
            with pytest.raises(MphError) as e:
                s.monitor(**kw)
            assert e.value.code == -1, kw
            assert "gauges" in str(e.value), kw
        # monitors off
        s.monitor(None)
        g = np.array(pt)
        from particlemethod_fsi_amd.solver import MphGaugeConfig
        import ctypes
        gc = MphGaugeConfig(1, 1, g.ctypes.data, 0.0)
        assert s._L.mph_gauge_configure(s._h, ctypes.byref(gc)) == -1
        assert b"gauges" in s._L.mph_last_error(s._h)
        # the map: before any step, along its own axis, too many lines
        with pytest.raises(MphError) as e:
            s.gauge_grid(pt, (0.001, 0.0, 0.0), (4, 1, 1), axis=1)
        assert e.value.code == -1
        s.monitor(gauges=[pt] * 64, gauge_radius=0.999 * reach, capacity=2)
        s.step(1)
        assert s.monitor_read()[0].shape == (1, 32 + 4 * 64)
        assert s.gauge_grid(pt, (0.001, 0.0, 0.0), (4, 1, 1), axis=1).shape == (1, 1, 4, 4)
        for kw in (dict(count=(4, 2, 1), axis=1), dict(count=(2 ** 20 + 1, 1, 1), axis=1), dict(count=(4, 1, 2), axis=1),
                   dict(count=(4, 1, 1), axis=2), dict(count=(0, 1, 1), axis=1), dict(count=(4, 1, 1), axis=1, radius=1.01 * reach)):
            with pytest.raises(MphError) as e:
                s.gauge_grid(pt, (0.001, 0.001, 0.0), **kw)
            assert e.value.code == -1, kw
        # after mph_set the sorted set is no longer the state's
        s.set("Velocity", s.get("Velocity"))
        with pytest.raises(MphError) as e:
            s.gauge_grid(pt, (0.001, 0.0, 0.0), (4, 1, 1), axis=1)
        assert e.value.code == -1


def test_too_many_bins():
    c = cases.Case("gauge_bins", 2, "dam", 0.001, (0, 0, 0), (0.05, 9.0, 0.001),
                   [Cuboid(1, (0.01, 0.01, 0), (0.02, 0.02, 0.001), 0.001, (0, 0, 0))])
    cfg, parts = c.build()
    pt = (0.0153, 0.0147, 0.0)
    with MphSolver(cfg, parts) as s:
        with pytest.raises(MphError) as e:      # 9,000 bins along y
            s.monitor(gauges=[pt], gauge_axis=1)
        assert e.value.code == -1 and "gauges" in str(e.value)
        s.monitor(gauges=[pt], gauge_axis=0, capacity=2)
        s.step(1)
        rec = s.monitor_gauges(s.monitor_read()[0][0])
        assert rec[0, C["COUNT"]] == 50.0 and rec[0, C["WET"]] == 10.0
        with pytest.raises(MphError) as e:
            s.gauge_grid(pt, (0.001, 0.0, 0.0), (4, 1, 1), axis=1)
        assert e.value.code == -1
        assert s.gauge_grid(pt, (0.0, 0.001, 0.0), (1, 4, 1), axis=0)[0, 0, 0, C["COUNT"]] == 50.0


def test_gauges_on_a_slab_context_are_unsupported():
    """Two slab ranks of channel3d in two threads of this process (host-staged transport: each
    rank's messages go to the other through a queue); both entry points are MPH_ERR_UNSUPPORTED."""
    import ctypes
    import queue
    import threading
    from particlemethod_fsi_amd.solver import MphGaugeConfig
    cfg, parts = cases.get("channel3d").build()
    box = [queue.Queue(), queue.Queue()]
    codes, errors = [None, None], []

    def rank(r):
        def exchange(sl, sr, rl, rr):
            # both neighbours are the other rank: its send_l is my recv_r, its send_r my recv_l
            box[1 - r].put((bytes(sl), bytes(sr)))
            a, b = box[r].get(timeout=120)
            rr[:len(a)] = a
            rl[:len(b)] = b
        try:
            with MphSolver(cfg, parts, slab=Slab(r, 2, 2, exchange=exchange)) as s:
                g = np.array((0.005, 0.01, 0.01))
                gc = MphGaugeConfig(1, 1, g.ctypes.data, 0.0)
                rc = [s._L.mph_gauge_configure(s._h, ctypes.byref(gc))]
                try:
                    s.gauge_grid((0.005, 0.01, 0.01), (0.001, 0.0, 0.001), (2, 1, 2), axis=1)
                    rc.append(0)
                except MphError as e:
                    rc.append(e.code)
                codes[r] = rc
        except Exception as e:   # noqa: BLE001 -- reported by the asserting thread
            errors.append(repr(e))

    t = threading.Thread(target=rank, args=(1,))
    t.start()
    rank(0)
    t.join()
    assert not errors, errors
    assert codes == [[-8, -8], [-8, -8]]


def test_map_on_an_empty_context():
    c = cases.Case("gauge_empty", 2, "dam", 0.001, (0.0, 0.0, 0.0), (0.05, 0.05, 0.001), [])
    cfg, parts = c.build()
    assert parts.n == 0
    with MphSolver(cfg, parts) as s:
        s.step(1)
        out = s.gauge_grid((0.01, 0.01, 0.0), (0.001, 0.0, 0.0), (5, 1, 1), axis=1)
        assert out.shape == (1, 1, 5, 4)
        for i in range(5):
            assert tuple(out[0, 0, i]) == (0.0, -np.inf, np.inf, 0.0)
