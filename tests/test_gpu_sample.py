"""GPU: lattice sampling (include/mph_gpu.h mph_sample_grid, kernel in csrc/mph_sample.hip).

The definition is the monitors' probe at every lattice point, so the numpy reference is
test_gpu_monitor._probe_reference applied to every point -- the positions and velocities mph_get
returns before the step, PressureP after it, the reference's Mod for the wrap and the minimum image
-- evaluated in blocks of 8 x 8 x 8 points against the particles of a box around each block.
Tolerances are the probes': COUNT exact; P, VX, VY, VZ within 1e-12 x the largest |f_j| among the
point's contributors; WSUM within 1e-12 x COUNT (a sum of <= ~100 terms in any order errs by ~1e-14
relative).  A point with a selected particle within 1e-12 m of its sphere is left out, and such
points must be at most 0.1 % of the non-empty ones.

The kernel has two ways through a wave (csrc/mph_sample.hip): lanes that share their stencil columns
-- a run of points along the contiguous cell axis (z in 3-D unless MPH_SLAB_PERM says otherwise, y
in 2-D), or many points in one cell -- test records staged in LDS 64 at a time; other lanes walk
their stencils through global memory.  The lattices below take both: the volumes mostly walk, the
lines along z, the 0.05 mm lattice and dam2d's runs along y (windows of more than 64 records in the
water column) are staged, 63 / 65 / 129 points leave lanes without a point in either.
"""
import numpy as np
import pytest

from particlemethod_fsi_amd import MphSolver, cases
from particlemethod_fsi_amd.solver import SAMPLE_CHANNELS as C, MphError, Slab

pytestmark = pytest.mark.gpu

DX = 0.001
REACH = 2.6 * DX          # MaxRadius + MARGIN of every case here (radius ratios 2.5, MARGIN 0.1 dx)
H = 2.4137 * DX

#         case        origin                           spacing                       count         radii
LATTICES = {
    "box3d_jit": ((-0.00372, 0.00041, -0.00408), (0.00113, 0.00107, 0.00109), (18, 23, 19), (0.0, 0.999 * REACH)),
    "seam3d": ((0.00213, 0.03107, 0.00171), (0.00093, 0.00097, 0.00089), (20, 19, 18), (H,)),
    "channel3d": ((-0.0137, 0.00049, -0.0041), (0.00127, 0.00119, 0.00123), (33, 30, 12), (H,)),
    "dam2d": ((-0.00871, 0.00053, 0.0), (0.00137, 0.00131, 0.001), (158, 90, 1), (H,)),
}


def _mod(x, w):
    return x - w * np.floor(x / w)   # the reference's Mod (main.cpp:98)


def _axes(origin, spacing, count):
    return [origin[d] + np.arange(count[d], dtype=np.float64) * spacing[d] for d in range(3)]


def _reference(cfg, X, V, T, P, origin, spacing, count, h, mask=1):
    """(ref [nz, ny, nx, 6], big [nz, ny, nx, 4]: max |f_j| of the contributors for P, VX, VY, VZ,
    near [nz, ny, nx]: a selected particle within 1e-12 m of the sphere, facts)."""
    lo = np.array([cfg.domain_min[d] for d in range(3)])
    w = np.array([cfg.domain_max[d] - cfg.domain_min[d] for d in range(3)])
    nd = int(cfg.dim)
    sel = ((mask >> (T >> 1)) & 1).astype(bool)
    x = _mod(X[sel] - lo, w) + lo
    f = np.concatenate([P[sel, None], V[sel]], axis=1)            # the four averaged fields
    q = _axes(origin, spacing, count)
    nx, ny, nz = count
    ref = np.zeros((nz, ny, nx, 6))
    big = np.zeros((nz, ny, nx, 4))
    near = np.zeros((nz, ny, nx), bool)
    # pairs: (point, particle) within h; across[d]: those reaching across the periodic face of axis d
    facts = {"pairs": 0, "across": np.zeros(3, int), "wrapped": 0, "closest": np.inf}
    B = 8
    for k0 in range(0, nz, B):
        for j0 in range(0, ny, B):
            for i0 in range(0, nx, B):
                sl = (slice(k0, min(k0 + B, nz)), slice(j0, min(j0 + B, ny)), slice(i0, min(i0 + B, nx)))
                sub = [q[0][sl[2]], q[1][sl[1]], q[2][sl[0]]]
                mid = np.array([0.5 * (a[0] + a[-1]) for a in sub])
                half = np.array([0.5 * (a[-1] - a[0]) for a in sub])
                dc = np.abs(_mod(x - mid + 0.5 * w, w) - 0.5 * w)
                keep = (dc[:, :nd] <= half[:nd] + h + 1e-6).all(axis=1)
                xc, fc = x[keep], f[keep]
                kk, jj, ii = np.meshgrid(sub[2], sub[1], sub[0], indexing="ij")
                pts = np.stack([ii.ravel(), jj.ravel(), kk.ravel()], axis=1)
                pw = _mod(pts - lo, w) + lo
                facts["wrapped"] += int((np.abs(pw[:, :nd] - pts[:, :nd]) > 0.5 * w[:nd]).any(axis=1).sum())
                shape = kk.shape
                if len(xc) == 0:
                    continue
                raw = xc[None, :, :] - pw[:, None, :]
                d = _mod(raw + 0.5 * w, w) - 0.5 * w
                if nd == 2:
                    d[..., 2] = 0.0
                r = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
                ins = r < h
                facts["pairs"] += int(ins.sum())
                facts["across"] += (ins[..., None] & (np.abs(raw) > 0.5 * w)).sum(axis=(0, 1))
                facts["closest"] = min(facts["closest"], float(np.abs(r - h).min()))
                near[sl] = (np.abs(r - h) < 1e-12).any(axis=1).reshape(shape)
                wt = np.where(ins, (1.0 - r / h) ** 2, 0.0)
                ws = wt.sum(axis=1)
                ok = ws > 0.0
                out = np.zeros((len(pts), 6))
                out[:, C["COUNT"]] = ins.sum(axis=1)
                out[:, C["WSUM"]] = ws
                for c in range(4):
                    s = (wt * fc[None, :, c]).sum(axis=1)
                    out[ok, 2 + c] = s[ok] / ws[ok]
                    big[sl + (c,)] = np.where(ins, np.abs(fc[None, :, c]), 0.0).max(axis=1).reshape(shape)
                ref[sl] = out.reshape(shape + (6,))
    return ref, big, near, facts


def _compare(got, ref, big, near, what):
    """The issue's tolerances on every point not `near`; returns the non-empty mask."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    use = ~near
    nonempty = ref[..., C["COUNT"]] > 0
    n_near = int((near & nonempty).sum())
    cnt = ref[..., C["COUNT"]]
    dw = np.abs(got[..., C["WSUM"]] - ref[..., C["WSUM"]])
    worst = {"WSUM": float((dw[use] / np.maximum(cnt[use], 1.0)).max())}
    for c, name in enumerate(("P", "VX", "VY", "VZ")):
        df = np.abs(got[..., C[name]] - ref[..., C[name]])
        rel = df[use & nonempty] / np.maximum(big[..., c][use & nonempty], 1e-300)
        worst[name] = float(rel.max()) if rel.size else 0.0
    print("%s: %d points, %d non-empty, %d near a sphere; worst error / scale: %s" % (
        what, cnt.size, int(nonempty.sum()), n_near, {k: "%.2e" % v for k, v in worst.items()}))
    assert np.array_equal(got[..., C["COUNT"]][use], cnt[use]), what
    assert (dw[use] <= 1e-12 * cnt[use]).all(), (what, worst)
    for c, name in enumerate(("P", "VX", "VY", "VZ")):
        df = np.abs(got[..., C[name]] - ref[..., C[name]])
        assert (df[use] <= 1e-12 * big[..., c][use]).all(), (what, name, worst)
    assert n_near <= 0.001 * int(nonempty.sum()), (what, n_near, int(nonempty.sum()))
    return nonempty


class _Run:
    """A solver stepped one step at a time, keeping what the reference needs: Property, the
    Position and Velocity before the last step, PressureP after it."""

    def __init__(self, case):
        self.cfg, self.parts = cases.get(case).build()
        self.s = MphSolver(self.cfg, self.parts)
        self.T = self.s.get("Property")
        self.seen_pressure = False
        self.refs = {}

    def step(self, k=1):
        if k > 1:
            self.s.step(k - 1)
        self.X, self.V = self.s.get("Position"), self.s.get("Velocity")
        self.s.step(1)
        self.P = self.s.get("PressureP")
        self.refs = {}

    def check(self, origin, spacing, count, radius=0.0, mask=0, what=""):
        h = radius if radius > 0.0 else self.cfg.radius_ratio_p * self.cfg.particle_spacing
        got = self.s.sample_grid(origin, spacing, count, radius=radius, classes=mask)
        key = (tuple(origin), tuple(spacing), tuple(count), h, mask)
        if key not in self.refs:   # one reference per lattice and state, shared by the checks on it
            self.refs[key] = _reference(self.cfg, self.X, self.V, self.T, self.P, origin, spacing, count, h,
                                        mask if mask else 1)
        ref, big, near, facts = self.refs[key]
        nonempty = _compare(got, ref, big, near, what)
        fl = self.T < 2
        pmax = float(np.abs(self.P[fl]).max()) if fl.any() else 0.0
        if nonempty.any() and pmax > 0.0 and (np.abs(got[..., C["P"]][nonempty]) > 1e-3 * pmax).any():
            self.seen_pressure = True
        return got, ref, nonempty, facts

    def close(self):
        self.s.close()


# ---- 1. definition ------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sorted(LATTICES))
def test_definition(case):
    origin, spacing, count, radii = LATTICES[case]
    r = _Run(case)
    try:
        for step, k in ((1, 1), (5, 4)):
            r.step(k)
            for radius in radii:
                got, ref, nonempty, facts = r.check(origin, spacing, count, radius, 0,
                                                    "%s step %d radius %g" % (case, step, radius))
                print(facts)
                assert nonempty.sum() > 1000, case
                if case == "seam3d":      # points beyond the periodic y face, pairs across it
                    assert facts["wrapped"] > 0 and facts["across"][1] > 0, facts
                if case == "channel3d":   # points beyond the x and z faces, pairs across the z face
                    assert facts["wrapped"] > 0 and facts["across"][2] > 0, facts
                assert (got[..., C["WSUM"]][~nonempty] == 0.0).all()
        assert r.seen_pressure
    finally:
        r.close()


# ---- 2. every cell order ------------------------------------------------------------------------

def test_every_cell_order(monkeypatch):
    origin, spacing, count, _ = LATTICES["box3d_jit"]
    counts = []
    for perm in range(5):
        monkeypatch.setenv("MPH_SLAB_PERM", str(perm))
        r = _Run("box3d_jit")
        try:
            r.step(2)
            got, ref, nonempty, _ = r.check(origin, spacing, count, 0.0, 0, "perm %d" % perm)
            assert r.seen_pressure
            counts.append(got[..., C["COUNT"]].copy())
        finally:
            r.close()
    assert counts[0].sum() > 0
    for k in range(1, 5):
        assert np.array_equal(counts[0], counts[k]), k


# ---- 3. independence of the lattice ----------------------------------------------------------------

def test_a_point_does_not_depend_on_its_lattice():
    origin, spacing, count, _ = LATTICES["box3d_jit"]
    r = _Run("box3d_jit")
    try:
        r.step(2)
        vol, ref, nonempty, _ = r.check(origin, spacing, count, 0.0, 0, "volume")
        again = r.s.sample_grid(origin, spacing, count)
        assert again.tobytes() == vol.tobytes()
        cnt = vol[..., C["COUNT"]]
        # (i, j, k): in the fluid, at the free surface, beside the x = 0 wall, in empty space
        picks = [(8, 9, 9), (10, 6, 7), (9, 18, 9), (7, 19, 8), (4, 8, 9), (3, 10, 6), (17, 22, 18), (16, 21, 2)]
        full = cnt.max()
        kinds = []
        for (i, j, k) in picks:
            o = tuple(a[m] for a, m in zip(_axes(origin, spacing, count), (i, j, k)))
            one = r.s.sample_grid(o, spacing, (1, 1, 1))
            assert one.shape == (1, 1, 1, 6)
            assert one[0, 0, 0].tobytes() == vol[k, j, i].tobytes(), ((i, j, k), one[0, 0, 0], vol[k, j, i])
            kinds.append(0 if cnt[k, j, i] == 0 else (2 if cnt[k, j, i] > 0.8 * full else 1))
        print("counts at the picks:", [int(cnt[k, j, i]) for (i, j, k) in picks], "largest", int(full))
        assert set(kinds) == {0, 1, 2}, kinds   # empty space, partly filled spheres, full ones
        assert r.seen_pressure
    finally:
        r.close()


# ---- 4. wave edges ------------------------------------------------------------------------------

def test_wave_edges():
    r = _Run("box3d_jit")
    try:
        r.step(3)
        inside = (0.00213, 0.00507, 0.00311)
        fine = (0.00019, 0.00019, 0.00019)
        for axis in range(3):
            for m in (63, 64, 65, 129):
                count = [1, 1, 1]
                count[axis] = m
                _, _, nonempty, _ = r.check(inside, fine, tuple(count), H, 0, "%d points along axis %d" % (m, axis))
                assert nonempty.any()
        _, _, nonempty, _ = r.check(inside, (0.00113, 0.00107, 0.00109), (5, 3, 7), H, 0, "5 x 3 x 7")
        assert nonempty.any()
        # 7 mm apart: every point in another region of the grid (cells are ~1 mm), most of them wrapped
        _, _, nonempty, facts = r.check((-0.009, 0.001, -0.009), (0.007, 0.007, 0.007), (9, 8, 6), H, 0, "7 mm apart")
        assert nonempty.any() and not nonempty.all() and facts["wrapped"] > 0
        # 0.05 mm apart: 80 points in one cell
        _, _, nonempty, _ = r.check((0.00601, 0.01003, 0.00502), (0.00005, 0.00005, 0.00005), (5, 4, 4), H, 0,
                                    "0.05 mm apart")
        assert nonempty.all()
        assert r.seen_pressure
    finally:
        r.close()


# ---- 5. against the probes ----------------------------------------------------------------------

def test_against_the_probes():
    probes = [(0.00613, 0.01021, 0.00587), (0.00587, 0.01957, 0.00611), (0.00071, 0.00813, 0.00493),
              (0.0353, 0.0421, 0.0061)]   # test_gpu_monitor.test_probes_in_a_tank
    r = _Run("box3d_jit")
    try:
        s = r.s
        s.monitor(stride=1, capacity=2, probes=probes)
        h = r.cfg.radius_ratio_p * r.cfg.particle_spacing
        for _ in range(5):
            r.step(1)
            rows, lost = s.monitor_read()
            prb = s.monitor_split(rows[0])[2]
            for q, probe in enumerate(probes):
                one, _, _, _ = r.check(probe, (DX, DX, DX), (1, 1, 1), 0.0, 0, "probe %d" % q)
                one = one[0, 0, 0]
                pj = r.refs[(tuple(probe), (DX, DX, DX), (1, 1, 1), h, 0)][1][0, 0, 0, 0]   # max |P_j|
                print("probe %d: %.17g (%d)  sample %.17g (%d)" % (q, prb[q, 0], prb[q, 1], one[C["P"]], one[C["COUNT"]]))
                assert one[C["COUNT"]] == prb[q, 1]
                assert abs(one[C["P"]] - prb[q, 0]) <= 1e-12 * pj
            assert prb[0, 1] >= 10 and prb[3, 1] == 0
        assert r.seen_pressure
    finally:
        r.close()


# ---- 6. classes ---------------------------------------------------------------------------------

def test_classes():
    origin, spacing, count = (-0.00871, 0.00053, -0.00913), (0.00213, 0.00197, 0.00209), (28, 25, 13)
    r = _Run("gate3d_jit")
    try:
        r.step(3)
        assert ((r.T >> 1) == 1).any() and ((r.T >> 1) == 2).any()
        got2, _, ne2, _ = r.check(origin, spacing, count, H, 2, "structure")
        got7, _, ne7, _ = r.check(origin, spacing, count, H, 7, "every class")
        got1, _, ne1, _ = r.check(origin, spacing, count, H, 1, "fluid")
        got0 = r.s.sample_grid(origin, spacing, count, radius=H, classes=0)
        assert got0.tobytes() == got1.tobytes()          # 0 means fluid only
        assert ne2.any() and ne7.sum() > ne1.sum() > 0 and ne7.sum() > ne2.sum()
        assert (got7[..., C["COUNT"]] >= got1[..., C["COUNT"]] + got2[..., C["COUNT"]]).all()
        assert r.seen_pressure
    finally:
        r.close()


# ---- 7. no side effects ---------------------------------------------------------------------------

@pytest.mark.parametrize("batching", [False, True])
def test_sampling_does_not_change_the_run(batching):
    origin, spacing, count = (-0.00871, 0.00053, -0.00913), (0.00213, 0.00197, 0.00209), (28, 25, 13)
    cfg, parts = cases.get("gate3d_jit").build()
    with MphSolver(cfg, parts) as a, MphSolver(cfg, parts) as b:
        for s in (a, b):
            s.step_batching(batching)
        filled = 0
        for _ in range(12):
            a.step(1)
            b.step(1)
            filled += int((b.sample_grid(origin, spacing, count, classes=7)[..., C["COUNT"]] > 0).sum())
        assert filled > 12 * 100
        for f in ("Position", "Velocity"):
            assert a.get(f).tobytes() == b.get(f).tobytes(), f
        assert a.time == b.time


# ---- 8. errors and edges ------------------------------------------------------------------------

def test_argument_errors():
    cfg, parts = cases.get("box3d_jit").build()
    o, sp, n = (0.001, 0.004, 0.001), (DX, DX, DX), (4, 4, 4)
    with MphSolver(cfg, parts) as s:
        def refused(*a, **kw):
            with pytest.raises(MphError) as e:
                s.sample_grid(*a, **kw)
            assert e.value.code == -1, (a, kw)
        refused(o, sp, n)                                   # before the first step
        s.step(1)
        assert s.sample_grid(o, sp, n)[..., C["COUNT"]].max() > 0
        for bad in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
            refused(o, sp, bad)
        for bad in ((0.0, DX, DX), (DX, -DX, DX), (DX, DX, 0.0)):
            refused(o, bad, n)
        refused(o, sp, (1 << 12, 1 << 12, 2))               # 2^25 points
        refused(o, sp, (1 << 24, 1, 2))
        refused(o, sp, (1 << 16, 1 << 16, 1 << 16))         # (a product past 2^31)
        refused(o, sp, n, radius=1.01 * REACH)
        refused(o, sp, n, radius=-DX)
        refused(o, sp, n, classes=8)
        refused(o, sp, n, classes=-1)
        assert s.sample_grid(o, sp, n, radius=0.999 * REACH, classes=7)[..., C["COUNT"]].max() > 0
        s.set("Velocity", s.get("Velocity"))
        refused(o, sp, n)                                   # right after mph_set
        s.step(1)
        assert s.sample_grid(o, sp, n)[..., C["COUNT"]].max() > 0
    cfg2, parts2 = cases.get("dam2d").build()
    with MphSolver(cfg2, parts2) as s:
        s.step(1)
        with pytest.raises(MphError) as e:
            s.sample_grid((0.0, 0.0, 0.0), sp, (4, 4, 2))   # count[2] != 1 in 2-D
        assert e.value.code == -1
        assert s.sample_grid((0.001, 0.004, 0.0), sp, (4, 4, 1))[..., C["COUNT"]].max() > 0


def test_largest_lattice_is_accepted():
    """MPH_SAMPLE_MAX_POINTS points (a 768 MiB result) pass the argument check; a line of them far
    out in empty space costs the kernel next to nothing."""
    cfg, parts = cases.get("box3d_jit").build()
    with MphSolver(cfg, parts) as s:
        s.step(1)
        out = s.sample_grid((0.036, 0.04, 0.02), (1e-9, 1e-9, 1e-9), (1 << 12, 1 << 12, 1))
        assert out.shape == (1, 1 << 12, 1 << 12, 6) and not out.any()


def test_sampling_a_slab_context_is_unsupported():
    """The two-thread slab pair of test_gpu_monitor.test_monitor_on_a_slab_context_is_unsupported."""
    import queue
    import threading
    cfg, parts = cases.get("channel3d").build()
    box = [queue.Queue(), queue.Queue()]
    codes, errors = [None, None], []

    def rank(r):
        def exchange(sl, sr, rl, rr):
            box[1 - r].put((bytes(sl), bytes(sr)))
            a, b = box[r].get(timeout=120)
            rr[:len(a)] = a
            rl[:len(b)] = b
        try:
            with MphSolver(cfg, parts, slab=Slab(r, 2, 2, exchange=exchange)) as s:
                try:
                    s.sample_grid((0.0, 0.004, 0.001), (DX, DX, DX), (2, 2, 2))
                except MphError as e:
                    codes[r] = e.code
        except Exception as e:   # noqa: BLE001 -- reported by the asserting thread
            errors.append(repr(e))

    t = threading.Thread(target=rank, args=(1,))
    t.start()
    rank(0)
    t.join()
    assert not errors, errors
    assert codes == [-8, -8]


def test_an_empty_context_gives_zeros():
    c = cases.Case("sample_empty", 2, "dam", 0.001, (0.0, 0.0, 0.0), (0.05, 0.05, 0.001), [])
    cfg, parts = c.build()
    assert parts.n == 0
    with MphSolver(cfg, parts) as s:
        s.step(2)
        out = s.sample_grid((0.001, 0.001, 0.0), (DX, DX, DX), (7, 5, 1))
        assert out.shape == (1, 5, 7, 6) and not out.any()
        with pytest.raises(MphError):
            s.sample_grid((0.001, 0.001, 0.0), (DX, DX, DX), (7, 5, 2))


def test_the_kernel_has_a_profiler_name():
    cfg, parts = cases.get("box3d_jit").build()
    origin, spacing, count, _ = LATTICES["box3d_jit"]
    with MphSolver(cfg, parts) as s:
        s.step(1)
        plain = s.sample_grid(origin, spacing, count)
        timed, ms, name = s.sample_grid(origin, spacing, count, timed=True)
        assert name == "sample_grid"
        assert 0.0 < ms < 1000.0
        assert timed.tobytes() == plain.tobytes()
        assert "sample_grid" not in s.profile(2)   # no step runs it
