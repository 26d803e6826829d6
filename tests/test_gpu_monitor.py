"""GPU: the per-step monitors (include/mph_gpu.h mph_monitor_*, kernels in csrc/mph_monitor.hip).

A sample is specified against what mph_get returns right after the sampled step, so every test
here recomputes it with numpy from get("Position" / "Velocity" / "PressureP" / "Mass" / "Property"):
counts, extrema, STEP, TIME and the tracked rows bit for bit; the sums within
2 (n_c + 4) 2^-53 sum |term_i| -- the bound of a sum of n_c terms taken in any order on both sides
(each side errs by at most (n_c - 1) 2^-53 sum |term| to first order) plus the terms' own few
roundings.  Probes use the positions before the step (the sorted set PressureP was computed at).
"""
import math

import numpy as np
import pytest

from particlemethod_fsi_amd import MphSolver, cases, mphio
from particlemethod_fsi_amd.mphio import Cuboid
from particlemethod_fsi_amd.solver import MONITOR_SLOTS as S, MphError, Slab, monitor_split

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
CLASSES = ("FLUID", "STRUCT", "WALL")


def _terms(s, cfg):
    """numpy form of a sample's head from the solver's current state: {slot: value} for the exact
    slots, {slot: (sum, sum |term|, n_c)} for the sums."""
    X, V, P, M, T = (s.get(k) for k in ("Position", "Velocity", "PressureP", "Mass", "Property"))
    cls = T >> 1
    v2 = V[:, 0] * V[:, 0] + V[:, 1] * V[:, 1] + V[:, 2] * V[:, 2]
    exact, sums = {}, {}
    for c, name in enumerate(CLASSES):
        sel = cls == c
        n = int(sel.sum())
        exact[name + "_COUNT"] = float(n)
        exact[name + "_VMAX2"] = float(v2[sel].max()) if n else 0.0
        for q, t in (("KE", 0.5 * M * v2), ("PX", M * V[:, 0]), ("PY", M * V[:, 1]), ("PZ", M * V[:, 2])):
            sums["%s_%s" % (name, q)] = (math.fsum(t[sel]), math.fsum(np.abs(t[sel])), n)
    f = cls == 0
    for d, ax in enumerate("XYZ"):
        exact[ax + "MIN"] = float(X[f, d].min()) if f.any() else np.inf
        exact[ax + "MAX"] = float(X[f, d].max()) if f.any() else -np.inf
    exact["FLUID_PMIN"] = float(P[f].min()) if f.any() else np.inf
    exact["FLUID_PMAX"] = float(P[f].max()) if f.any() else -np.inf
    exact["WALL_PMAX"] = float(P[cls == 2].max()) if (cls == 2).any() else -np.inf
    g = cfg.gravity
    e = M * (g[0] * X[:, 0] + g[1] * X[:, 1] + g[2] * X[:, 2])
    fs = cls < 2
    sums["EPOT"] = (-math.fsum(e[fs]), math.fsum(np.abs(e[fs])), int(fs.sum()))
    exact["RESERVED0"] = exact["RESERVED1"] = 0.0
    return exact, sums, X, V


def _check_head(head, s, cfg, step):
    exact, sums, X, V = _terms(s, cfg)
    assert head[S["STEP"]] == float(step)
    assert head[S["TIME"]] == s.time
    for k, v in exact.items():
        assert head[S[k]] == v, (k, head[S[k]], v, step)
    for k, (v, a, n) in sums.items():
        tol = 2.0 * (n + 4) * EPS * a
        print("step %d %s: sample %.17g numpy %.17g |diff| %.3g bound %.3g" % (step, k, head[S[k]], v,
                                                                              abs(head[S[k]] - v), tol))
        assert abs(head[S[k]] - v) <= tol, (k, head[S[k]], v, tol, step)
    return X, V


# ---- 1. definition ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["dam2d", "gate3d_jit"])
def test_definition_against_get(case):
    cfg, parts = cases.get(case).build()
    T = parts.property
    track = [int(np.nonzero(T < 2)[0][7]), int(np.nonzero(T >= 4)[0][-3])]
    if case == "gate3d_jit":
        st = np.nonzero((T == 2) | (T == 3))[0]
        tip = st[np.argsort(parts.position[st, 1])[-3:]]   # the gate's free end (it is clamped at y0 < 0.002)
        track = [int(i) for i in tip] + track
        assert cfg.dt / cfg.elastic_dt > 3.5   # 4 elastic substeps
    with MphSolver(cfg, parts) as s:
        s.monitor(stride=1, capacity=4, track=track)
        ke = []
        for k in range(1, 13):
            s.step(1)
            rows, lost = s.monitor_read()
            assert rows.shape == (1, 32 + 6 * len(track)) and lost == 0
            head, trk, prb = s.monitor_split(rows[0])
            X, V = _check_head(head, s, cfg, k)
            for r, i in zip(trk, track):
                assert np.array_equal(r[:3], X[i]) and np.array_equal(r[3:], V[i]), (i, r, X[i], V[i])
            ke.append(head[S["FLUID_KE"]])
        # not vacuous: the fluid's kinetic energy is there and grows over the steps -- every step
        # for the column falling from rest on its lattice; the off-lattice gate case first relaxes
        # its +-0.3 dx offsets (its KE peaks at step 10 and eases off, in numpy as in the samples),
        # so there the growth is from the first step to the last
        assert ke[0] > 0.0 and ke[-1] > 10.0 * ke[0], ke
        if case == "dam2d":
            assert all(b > a for a, b in zip(ke, ke[1:])), ke
        if case == "gate3d_jit":
            assert head[S["STRUCT_COUNT"]] > 0 and head[S["WALL_COUNT"]] > 0


# ---- 2. reduction edges ------------------------------------------------------------------------

def _fluid_block(nx, ny, vel=(0.03, -0.02, 0.0)):
    """nx x ny fluid particles (2-D, dx = 1 mm) alone in a periodic box."""
    c = cases.Case("mon_edge", 2, "dam", 0.001, (-0.01, 0.0, 0.0), (0.001 * nx + 0.02, 0.001 * ny + 0.03, 0.001),
                   [Cuboid(1, (0.0, 0.01, 0.0), (0.001 * nx, 0.01 + 0.001 * ny, 0.001), 0.001, vel)])
    return c.build()


# the partial stage gives each block 1024 particles; the final stage is one block whose 32 thread
# groups take 8 records each per pass: 520 x 512 particles make 260 partial records, more than the
# 256 of one pass (and more than a 256-thread block has threads)
@pytest.mark.parametrize("nx,ny", [(1, 1), (8, 8), (5, 13), (257, 1), (520, 512)])
def test_reduction_edges(nx, ny):
    cfg, parts = _fluid_block(nx, ny)
    assert parts.n == nx * ny
    with MphSolver(cfg, parts) as s:
        s.monitor(stride=1, capacity=2, track=[0, parts.n - 1])
        for k in (1, 2):
            s.step(1)
            rows, lost = s.monitor_read()
            assert len(rows) == 1 and lost == 0
            head, trk, _ = s.monitor_split(rows[0])
            X, V = _check_head(head, s, cfg, k)
            assert head[S["FLUID_COUNT"]] == parts.n and head[S["WALL_COUNT"]] == 0
            assert head[S["WALL_PMAX"]] == -np.inf and head[S["STRUCT_VMAX2"]] == 0.0
            assert np.array_equal(trk[0], np.concatenate([X[0], V[0]]))
            assert np.array_equal(trk[1], np.concatenate([X[-1], V[-1]]))
        if parts.n == 1:
            # the closed form of test_single_fluid_particle_falls_bitwise: F = m g; v += F / m Dt
            m = cfg.density[1] * cfg.particle_spacing * cfg.particle_spacing
            vr = parts.velocity[0].copy()
            for _ in range(2):
                for d in range(3):
                    vr[d] = vr[d] + m * cfg.gravity[d] / m * cfg.dt
            assert head[S["FLUID_KE"]] == 0.5 * m * (vr[0] * vr[0] + vr[1] * vr[1] + vr[2] * vr[2])
            assert [head[S["FLUID_P" + a]] for a in "XYZ"] == [m * vr[0], m * vr[1], m * vr[2]]
            assert head[S["FLUID_KE"]] > 0.0


# ---- 3. batch shapes ---------------------------------------------------------------------------

GATE_PROBES = [(0.00613, 0.01021, 0.00387), (0.00587, 0.01957, 0.00411), (0.0303, 0.0401, 0.0041)]


def _gate_monitor(s, parts):
    st = np.nonzero(parts.property == 2)[0]
    s.monitor(stride=1, capacity=64, track=[int(st[-1]), 5, int(st[0]), 5], probes=GATE_PROBES)


def test_batch_shapes_give_the_same_samples():
    cfg, parts = cases.get("gate3d_jit").build()
    out = []
    with MphSolver(cfg, parts) as s:        # 29 single steps (kSeq1)
        _gate_monitor(s, parts)
        for _ in range(29):
            s.step(1)
        out.append(s.monitor_read())
    with MphSolver(cfg, parts) as s:        # kSeq8 x 3, kSeq1t x 4, kSeq1
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
    assert ref.shape == (29, 32 + 6 * 4 + 2 * 3) and lost == 0
    assert np.array_equal(ref[:, 0], np.arange(1, 30))
    head, trk, prb = monitor_split(ref, 4, 3)
    assert (prb[:, 0, 1] >= 10).all() and (prb[:, 2, 1] == 0).all()   # in the fluid / in empty space
    assert np.array_equal(trk[:, 1], trk[:, 3])   # the id listed twice
    for rows, lo in out[1:]:
        assert lo == 0
        assert rows.shape == ref.shape
        assert rows.tobytes() == ref.tobytes()


# ---- 4. no side effect -------------------------------------------------------------------------

def test_monitors_do_not_change_the_run():
    cfg, parts = cases.get("gate3d_jit").build()
    fields = ("Position", "Velocity", "Force", "NeighborCount")
    with MphSolver(cfg, parts) as a, MphSolver(cfg, parts) as b, MphSolver(cfg, parts) as c:
        _gate_monitor(b, parts)
        _gate_monitor(c, parts)
        a.step(16)
        b.step(16)
        c.step(8)
        c.monitor(None)
        c.step(8)
        assert len(b.monitor_read()[0]) == 16
        assert c.monitor_read()[0].shape[0] == 0
        for f in fields:
            ref = a.get(f)
            assert np.array_equal(ref, b.get(f)), f
            assert np.array_equal(ref, c.get(f)), f
        assert a.time == b.time == c.time


# ---- 5. stride and ring ------------------------------------------------------------------------

def test_stride_ring_and_reconfigure():
    cfg, parts = cases.get("dam2d").build()
    with MphSolver(cfg, parts) as s:
        s.monitor(stride=3, capacity=16)
        s.step(10)
        rows, lost = s.monitor_read()
        assert lost == 0 and list(rows[:, 0]) == [3.0, 6.0, 9.0]
        t = cfg.time
        ts = []
        for k in range(1, 10):
            t += cfg.dt
            if k % 3 == 0:
                ts.append(t)
        assert list(rows[:, 1]) == ts
        s.monitor(stride=1, capacity=4)            # STEP counts from here again
        s.step(11)
        rows, lost = s.monitor_read()
        assert list(rows[:, 0]) == [8.0, 9.0, 10.0, 11.0] and lost == 7
        assert rows[-1, 1] == s.time
        rows, lost = s.monitor_read()
        assert rows.shape[0] == 0 and lost == 0
        s.step(2)
        rows, lost = s.monitor_read(max_samples=1)   # the rest stays unread
        assert list(rows[:, 0]) == [12.0] and lost == 0
        rows, lost = s.monitor_read()
        assert list(rows[:, 0]) == [13.0] and lost == 0
        s.monitor(stride=2, capacity=4)
        s.step(4)
        rows, lost = s.monitor_read()
        assert list(rows[:, 0]) == [2.0, 4.0] and lost == 0


# ---- 6. probes ---------------------------------------------------------------------------------

def _mod(x, w):
    return x - w * np.floor(x / w)   # the reference's Mod (main.cpp:98)


def _probe_reference(cfg, pos_before, T, P, probe, h):
    lo = np.array([cfg.domain_min[d] for d in range(3)])
    w = np.array([cfg.domain_max[d] - cfg.domain_min[d] for d in range(3)])
    x = _mod(pos_before - lo, w) + lo
    p = _mod(np.asarray(probe) - lo, w) + lo
    d = _mod(x - p + 0.5 * w, w) - 0.5 * w
    r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    fl = T < 2
    assert not (fl & (np.abs(r - h) < 1e-9)).any(), "a fluid particle on the probe's sphere"
    sel = fl & (r < h)
    wt = (1.0 - r[sel] / h) ** 2
    val = float((wt * P[sel]).sum() / wt.sum()) if sel.any() else 0.0
    return val, int(sel.sum()), (float(np.abs(P[sel]).max()) if sel.any() else 0.0), x[sel]


def _run_probes(case, probes, steps, in_fluid):
    cfg, parts = cases.get(case).build()
    h = cfg.radius_ratio_p * cfg.particle_spacing
    seen_value = False
    with MphSolver(cfg, parts) as s:
        s.monitor(stride=1, capacity=2, probes=probes)
        T = s.get("Property")
        contrib = None
        for _ in range(steps):
            before = s.get("Position")
            s.step(1)
            P = s.get("PressureP")
            rows, lost = s.monitor_read()
            prb = s.monitor_split(rows[0])[2]
            pmax = float(np.abs(P[T < 2]).max())
            for q, probe in enumerate(probes):
                val, cnt, pj, contrib = _probe_reference(cfg, before, T, P, probe, h)
                print("probe %d: value %.17g numpy %.17g count %d" % (q, prb[q, 0], val, cnt))
                assert prb[q, 1] == cnt, (q, prb[q], cnt)
                assert abs(prb[q, 0] - val) <= 1e-12 * pj, (q, prb[q, 0], val, pj)
                if q in in_fluid:
                    assert cnt >= 10, (q, cnt)
                    seen_value = seen_value or abs(val) > 1e-3 * pmax
        assert seen_value
    return contrib


def test_probes_in_a_tank():
    # box3d: fluid over x, z in (0, 0.012), y in (0.003, 0.02); walls around; the domain reaches
    # x = 0.04, y = 0.05.  In the fluid, at the free surface, against the x = 0 wall, in empty space
    probes = [(0.00613, 0.01021, 0.00587), (0.00587, 0.01957, 0.00611), (0.00071, 0.00813, 0.00493),
              (0.0353, 0.0421, 0.0061)]
    _run_probes("box3d_jit", probes, 5, in_fluid=(0, 1, 2))


def test_probe_across_the_periodic_face():
    # seam3d: fluid at y < 0.006 and y > 0.034 of a domain periodic at y = 0.04; the probe 0.7 mm
    # below the face takes particles from both sides of it
    contrib = _run_probes("seam3d", [(0.01531, 0.03931, 0.01013)], 3, in_fluid=(0,))
    assert (contrib[:, 1] < 0.01).any() and (contrib[:, 1] > 0.03).any()


# ---- 7. profiler names -------------------------------------------------------------------------

def test_monitor_kernels_in_the_profile():
    cfg, parts = cases.get("box3d_jit").build()
    with MphSolver(cfg, parts) as s:
        prof = s.profile(4)
        assert not [k for k in prof if k.startswith("monitor")], prof.keys()
        s.monitor(stride=2, capacity=8, track=[3], probes=[(0.00613, 0.01021, 0.00587)])
        prof = s.profile(4)
        mon = sorted(k for k in prof if k.startswith("monitor"))
        assert mon == ["monitor_final", "monitor_partial", "monitor_probe"], prof.keys()
        assert all(prof[k]["launches"] == 4 for k in mon), prof
        rows, lost = s.monitor_read()
        assert list(rows[:, 0]) == [2.0, 4.0] and lost == 0
        assert rows[-1, 1] == s.time
        s.monitor(None)
        assert not [k for k in s.profile(2) if k.startswith("monitor")]


# ---- 8. errors ---------------------------------------------------------------------------------

def test_monitor_argument_errors():
    cfg, parts = cases.get("dam2d").build()
    reach = (2.5 + 0.1) * cfg.particle_spacing   # MaxRadius + MARGIN
    with MphSolver(cfg, parts) as s:
        bad = [dict(stride=0), dict(capacity=0), dict(track=list(range(65))), dict(probes=[(0.0, 0.0, 0.0)] * 65),
               dict(track=[parts.n]), dict(track=[-1]), dict(probes=[(0.01, 0.01, 0.0)], probe_radius=1.01 * reach)]
        for kw in bad:
            with pytest.raises(MphError) as e:
                s.monitor(**kw)
            assert e.value.code == -1, kw
            assert "monitors" in str(e.value), kw
        s.monitor(track=list(range(64)), probes=[(0.01, 0.01, 0.0)] * 64, probe_radius=0.999 * reach, capacity=2)
        s.step(1)
        assert s.monitor_read()[0].shape == (1, 32 + 6 * 64 + 2 * 64)


def test_monitor_on_a_slab_context_is_unsupported():
    """Two slab ranks of channel3d in two threads of this process (host-staged transport: each
    rank's messages go to the other through a queue); mph_monitor_configure is MPH_ERR_UNSUPPORTED."""
    import queue
    import threading
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
                try:
                    s.monitor()
                except MphError as e:
                    codes[r] = e.code
                assert s._L.mph_monitor_sample_doubles(s._h) == 0
        except Exception as e:   # noqa: BLE001 -- reported by the asserting thread
            errors.append(repr(e))

    t = threading.Thread(target=rank, args=(1,))
    t.start()
    rank(0)
    t.join()
    assert not errors, errors
    assert codes == [-8, -8]


def test_monitor_on_an_empty_context():
    c = cases.Case("mon_empty", 2, "dam", 0.001, (0.0, 0.0, 0.0), (0.05, 0.05, 0.001), [])
    cfg, parts = c.build()
    assert parts.n == 0
    with MphSolver(cfg, parts) as s:
        s.monitor(stride=1, capacity=4)
        s.step(3)
        rows, lost = s.monitor_read()
        assert rows.shape[0] == 0 and lost == 0
        with pytest.raises(MphError):
            s.monitor(track=[0])
