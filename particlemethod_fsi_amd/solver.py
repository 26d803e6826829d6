"""Python mirror of the reference driver over the C ABI of ``include/mph_gpu.h``.

``MphSolver`` plays the role of the reference's ``main()`` (src/main.cpp:490-727) for tests,
benchmarks and scripting: construct it from a ``.data``/``.grid`` pair (or an in-memory case),
advance with ``step(k)`` (each step = main.cpp:597-686) and read any per-particle array with
``get(<reference array name>)`` in the reference's layout and original particle order.

All compute runs in libmph_gpu.so (HIP kernels for gfx950).  There is no CPU fallback: if the
library is missing or no HIP device is present the constructor raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

from . import mphio

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(PKG_DIR, "lib")
LIB_PATH = os.environ.get("MPH_GPU_LIB") or os.path.join(LIB_DIR, "libmph_gpu.so")   # env: A/B builds
CSRC_DIR = os.path.join(PKG_DIR, "csrc")

# MphField (include/mph_gpu.h) keyed by the reference's array names (main.cpp:102-197)
FIELDS = {
    "Position": (0, 3, np.float64), "InitialPosition": (1, 3, np.float64),
    "Velocity": (2, 3, np.float64), "Force": (3, 3, np.float64),
    "Acceleration": (4, 3, np.float64), "GravityCenter": (5, 3, np.float64),
    "PressureP": (6, 1, np.float64), "PressureA": (7, 1, np.float64),
    "DensityA": (8, 1, np.float64), "VolStrainP": (9, 1, np.float64),
    "DivergenceP": (10, 1, np.float64), "Mass": (11, 1, np.float64), "Kappa": (12, 1, np.float64),
    "Lambda": (13, 1, np.float64), "Mu": (14, 1, np.float64),
    "NeighborCount": (15, 1, np.int32), "InitialStructureNeighborCount": (16, 1, np.int32),
    "Property": (17, 1, np.int32), "DeformGradient": (18, 9, np.float64),
    "Strain": (19, 9, np.float64), "Stress": (20, 9, np.float64),
    "Normalizer": (21, 9, np.float64), "LambdaLames": (22, 1, np.float64),
    "MuLames": (23, 1, np.float64),
    "VirialStressAtParticle": (24, 9, np.float64), "VirialPressureAtParticle": (25, 1, np.float64),
}

STATUS = {0: "MPH_OK", -1: "MPH_ERR_ARG", -2: "MPH_ERR_IO", -3: "MPH_ERR_NEIGHBOR_OVERFLOW",
          -4: "MPH_ERR_DEVICE_OOM", -5: "MPH_ERR_HIP", -6: "MPH_ERR_RCCL", -7: "MPH_ERR_DOMAIN",
          -8: "MPH_ERR_UNSUPPORTED", -9: "MPH_ERR_NONFINITE", -10: "MPH_ERR_TRANSPORT",
          -11: "MPH_ERR_CAPACITY"}

EXPORTED_SYMBOLS = [
    "mph_config_default", "mph_read_data_file", "mph_read_grid_header", "mph_read_grid_particles",
    "mph_write_prof_arrays", "mph_write_vtk_arrays", "mph_create", "mph_step", "mph_synchronize",
    "mph_get", "mph_set", "mph_particle_count", "mph_time", "mph_get_scalars", "mph_write_prof",
    "mph_write_vtk", "mph_last_error", "mph_destroy", "mph_profile_steps", "mph_profile_graphs", "mph_neighbor_stats",
    "mph_dist_unique_id", "mph_create_dist", "mph_owned_count", "mph_derive_scalars",
    "mph_structure_init", "mph_create_dist_host", "mph_owned_ids", "mph_slab_bounds",
    "mph_slab_owner", "mph_dist_selftest", "mph_compute_virial",
    "mph_config_sizeof", "mph_write_vtk_async", "mph_output_wait", "mph_write_grid_binary",
    "mph_write_vtu_arrays", "mph_write_vtu", "mph_velocity_profile_arrays",
    "mph_set_initial_velocity_profile", "mph_dist_info", "mph_create_slab", "mph_slab_window",
    "mph_list_stats", "mph_abi_version", "mph_phase_timing", "mph_phase_times",
    "mph_set_step_batching", "mph_neighbor_rows", "mph_dist_overlap", "mph_list_layout",
    "mph_monitor_configure", "mph_monitor_sample_doubles", "mph_monitor_read",
    "mph_sample_grid", "mph_sample_grid_timed", "mph_write_vti_arrays", "mph_idle_wall_stats",
    "mph_lean_step_stats", "mph_key_fold_stats", "mph_gauge_configure", "mph_gauge_grid",
    "mph_list_format_stats", "mph_list_span_misses", "mph_list_wave_formats",
    "mph_selection_parse", "mph_selection_accepts", "mph_selection_layout", "mph_select",
    "mph_selected_ids", "mph_get_selected", "mph_selection_totals", "mph_write_vtk_selected",
    "mph_write_vtu_selected", "mph_select_profile",
    "mph_kinematics_layout", "mph_kinematics_parse", "mph_kinematics_n0", "mph_kinematics_arrays",
    "mph_write_vtu_kinematics_arrays", "mph_compute_kinematics", "mph_compute_kinematics_timed",
    "mph_get_kinematics", "mph_get_kinematics_selected", "mph_write_vtu_kinematics",
    "mph_write_vtu_kinematics_selected",
    "mph_dist_monitor_configure", "mph_dist_monitor_record_doubles", "mph_dist_monitor_read_partial",
    "mph_monitor_combine", "mph_dist_monitor_read",
    "mph_slab_lattice_owner", "mph_dist_sample_grid_partial", "mph_dist_sample_grid",
    "mph_dist_gauge_grid_partial", "mph_gauge_combine", "mph_dist_gauge_grid",
    "mph_dist_select", "mph_dist_selected_ids", "mph_dist_get_selected", "mph_dist_selection_totals_partial",
    "mph_totals_combine", "mph_dist_selection_totals", "mph_dist_gather_selected", "mph_dist_write_vtk_selected",
    "mph_dist_write_vtu_selected",
]

ABI_VERSION = 6   # MPH_ABI_VERSION of include/mph_gpu.h that these bindings follow

# mph_host_exchange_fn (include/mph_gpu.h): (user, send_l, n, send_r, n, recv_l, n, recv_r, n)
HOST_EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                    ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                    ctypes.c_void_p, ctypes.c_size_t)


class MphSlabOptions(ctypes.Structure):
    """include/mph_gpu.h MphSlabOptions."""
    _fields_ = [("rank", ctypes.c_int), ("nranks", ctypes.c_int), ("axis", ctypes.c_int),
                ("unique_id128", ctypes.c_char_p), ("host_fn", HOST_EXCHANGE_FN),
                ("host_user", ctypes.c_void_p), ("n_glob", ctypes.c_int), ("ids", ctypes.c_void_p),
                ("cuts", ctypes.c_void_p)]


class MphMonitorConfig(ctypes.Structure):
    """include/mph_gpu.h MphMonitorConfig."""
    _fields_ = [("stride", ctypes.c_int), ("capacity", ctypes.c_int), ("ntrack", ctypes.c_int),
                ("track", ctypes.c_void_p), ("nprobe", ctypes.c_int), ("probes", ctypes.c_void_p),
                ("probe_radius", ctypes.c_double)]


class MphSampleGrid(ctypes.Structure):
    """include/mph_gpu.h MphSampleGrid."""
    _fields_ = [("origin", ctypes.c_double * 3), ("spacing", ctypes.c_double * 3), ("count", ctypes.c_int * 3),
                ("classes", ctypes.c_int), ("radius", ctypes.c_double)]


# MphSampleChannel (include/mph_gpu.h): name -> index into a lattice point's record
SAMPLE_CHANNELS = {"COUNT": 0, "WSUM": 1, "P": 2, "VX": 3, "VY": 4, "VZ": 5}
SAMPLE_MAX_POINTS = 1 << 24
SAMPLE_CLASSES = {"fluid": 1, "structure": 2, "walls": 4}


def _sample_grid(origin, spacing, count, radius=0.0, classes=0) -> MphSampleGrid:
    g = MphSampleGrid()
    for d in range(3):
        g.origin[d], g.spacing[d], g.count[d] = float(origin[d]), float(spacing[d]), int(count[d])
    g.classes, g.radius = int(classes), float(radius)
    return g


class MphGaugeConfig(ctypes.Structure):
    """include/mph_gpu.h MphGaugeConfig."""
    _fields_ = [("axis", ctypes.c_int), ("ngauge", ctypes.c_int), ("points", ctypes.c_void_p),
                ("radius", ctypes.c_double)]


class MphGaugeGrid(ctypes.Structure):
    """include/mph_gpu.h MphGaugeGrid."""
    _fields_ = [("origin", ctypes.c_double * 3), ("spacing", ctypes.c_double * 3), ("count", ctypes.c_int * 3),
                ("axis", ctypes.c_int), ("radius", ctypes.c_double)]


# MphGaugeChannel (include/mph_gpu.h): name -> index into a gauge's (a line's) record
GAUGE_CHANNELS = {"COUNT": 0, "TOP": 1, "BOTTOM": 2, "WET": 3}
GAUGE_MAX = 64
GAUGE_MAX_BINS = 8192
GAUGE_GRID_MAX_LINES = 1 << 20
# a slab rank's record of a line (MPH_DIST_GAUGE_RECORD): the four channels, then the lowest and highest
# occupied bin
DIST_GAUGE_RECORD = {"COUNT": 0, "TOP": 1, "BOTTOM": 2, "WET": 3, "LOBIN": 4, "HIBIN": 5}


class MphSelection(ctypes.Structure):
    """include/mph_gpu.h MphSelection."""
    _fields_ = [("type_mask", ctypes.c_int), ("box", ctypes.c_int), ("every", ctypes.c_int),
                ("phase", ctypes.c_int), ("lo", ctypes.c_double * 3), ("hi", ctypes.c_double * 3)]


# MphTotalSlot (include/mph_gpu.h): name -> index into the record of mph_selection_totals
TOTALS = 24
TOTAL_SLOTS = {"COUNT": 0, "MASS": 1, "PX": 2, "PY": 3, "PZ": 4, "KE": 5, "FX": 6, "FY": 7, "FZ": 8,
               "TX": 9, "TY": 10, "TZ": 11, "MX": 12, "MY": 13, "MZ": 14, "XMIN": 15, "XMAX": 16,
               "YMIN": 17, "YMAX": 18, "ZMIN": 19, "ZMAX": 20, "VMAX2": 21, "RESERVED0": 22, "RESERVED1": 23}
SELECTION_BOX = {"position": 1, "initial": 2}


def parse_selection(spec: str) -> MphSelection:
    """mph_selection_parse: "types=0,1;box=x0,y0,z0,x1,y1,z1;on=initial;every=4;phase=1" (any subset
    of the keys, any order) -> MphSelection; MphError(MPH_ERR_ARG) on anything else.  Host only."""
    s = MphSelection()
    _check(load_library().mph_selection_parse(spec.encode(), ctypes.byref(s)))
    return s


def make_selection(types=None, box=None, on: str = "position", every: int = 1, phase: int = 0) -> MphSelection:
    """An MphSelection from Python values: types an iterable of particle types (None: every type),
    box ((x0, y0, z0), (x1, y1, z1)) or six numbers (None: no box) tested on Position or, with
    on="initial", on InitialPosition."""
    s = MphSelection()
    for t in (types if types is not None else ()):
        if not 0 <= int(t) < 6:
            raise ValueError("selection: particle types are 0..5")
        s.type_mask |= 1 << int(t)
    if box is not None:
        b = np.asarray(box, np.float64).reshape(6)
        for d in range(3):
            s.lo[d], s.hi[d] = b[d], b[3 + d]
        s.box = SELECTION_BOX[on]
    elif on not in SELECTION_BOX:
        raise ValueError("selection: on is 'position' or 'initial'")
    s.every, s.phase = int(every), int(phase)
    return s


def selection_accepts(sel: MphSelection, dim: int, index: int, ptype: int, pos=None, pos0=None) -> int:
    """mph_selection_accepts: 1 / 0 for one particle (the function the device evaluates); host only."""
    p = None if pos is None else np.ascontiguousarray(pos, np.float64)
    p0 = None if pos0 is None else np.ascontiguousarray(pos0, np.float64)
    return _check(load_library().mph_selection_accepts(ctypes.byref(sel), int(dim), int(index), int(ptype),
                                                       None if p is None else p.ctypes.data,
                                                       None if p0 is None else p0.ctypes.data))


def totals_combine(records) -> np.ndarray:
    """mph_totals_combine: the ranks' records of dist_selection_totals(partial=True) ([nranks, 24], rank
    order) made one record [24] -- rank 0's combined with ranks 1, 2, ... in order: the sums add, the
    minima take the minimum, the maxima and VMAX2 the maximum.  Host only."""
    recs = [np.ascontiguousarray(r, np.float64).reshape(TOTALS) for r in records]
    ptrs = (ctypes.c_void_p * max(len(recs), 1))(*[r.ctypes.data for r in recs])
    out = np.zeros(TOTALS)
    _check(load_library().mph_totals_combine(len(recs), ptrs, out.ctypes.data))
    return out


class MphKinematics(ctypes.Structure):
    """include/mph_gpu.h MphKinematics."""
    _fields_ = [("radius", ctypes.c_double), ("surface_beta", ctypes.c_double), ("det_floor", ctypes.c_double),
                ("classes", ctypes.c_int), ("reserved", ctypes.c_int)]


# MphKinChannel (include/mph_gpu.h): name -> column of a particle's kinematics record; L is the first
# of the nine columns of the velocity gradient, L[a][b] at KIN["L"] + 3 a + b
KIN_CHANNELS = 24
KIN = {"COUNT": 0, "WSUM": 1, "FILL": 2, "CX": 3, "CY": 4, "CZ": 5, "L": 6, "DIV": 15, "WX": 16, "WY": 17,
       "WZ": 18, "SHEAR": 19, "FLAGS": 20, "RESERVED0": 21, "RESERVED1": 22, "RESERVED2": 23}
KIN_FLAGS = {"DEGENERATE": 1, "SURFACE": 2, "ALONE": 4}


def make_kinematics(radius: float = 0.0, classes: int = 0, beta: float = 0.0, det_floor: float = 0.0) -> MphKinematics:
    k = MphKinematics()
    k.radius, k.surface_beta, k.det_floor = float(radius), float(beta), float(det_floor)
    k.classes, k.reserved = int(classes), 0
    return k


def parse_kinematics(spec: str) -> MphKinematics:
    """mph_kinematics_parse: "radius=..;classes=..;beta=..;det=.." (any subset of the keys; empty: the
    defaults) -> MphKinematics; MphError(MPH_ERR_ARG) on anything else.  Host only."""
    k = MphKinematics()
    _check(load_library().mph_kinematics_parse(spec.encode(), ctypes.byref(k)))
    return k


def kinematics_n0(cfg: "mphio.MphConfig", radius: float = 0.0) -> float:
    """mph_kinematics_n0: the weight sum of a full lattice within `radius` (0: RadiusRatioV dx), the
    denominator of the FILL channel.  Host only."""
    out = ctypes.c_double(0.0)
    _check(load_library().mph_kinematics_n0(ctypes.byref(cfg), float(radius), ctypes.byref(out)))
    return out.value


def kinematics_arrays(cfg: "mphio.MphConfig", prop, pos, vel, radius: float = 0.0, classes: int = 0,
                      beta: float = 0.0, det_floor: float = 0.0, kin: "MphKinematics | None" = None) -> np.ndarray:
    """mph_kinematics_arrays: the [n, 24] records from arrays by the host's O(n^2) loop (j ascending),
    the reference of MphSolver.kinematics.  Host only; at most 65,536 particles."""
    k = kin if kin is not None else make_kinematics(radius, classes, beta, det_floor)
    prop = np.ascontiguousarray(prop, np.int32)
    pos, vel = np.ascontiguousarray(pos, np.float64), np.ascontiguousarray(vel, np.float64)
    n = prop.shape[0]
    if pos.shape != (n, 3) or vel.shape != (n, 3):
        raise ValueError("kinematics_arrays: pos and vel must have shape (n, 3)")
    out = np.zeros((n, KIN_CHANNELS))
    _check(load_library().mph_kinematics_arrays(ctypes.byref(cfg), ctypes.byref(k), n, prop.ctypes.data,
                                                pos.ctypes.data, vel.ctypes.data, out.ctypes.data))
    return out


def write_vtu_kinematics(path: str, prop, pos, kin):
    """mph_write_vtu_kinematics_arrays: a .vtu of the records kin [n, 24] at pos [n, 3] (read_vtu reads
    it back).  Host only."""
    prop = np.ascontiguousarray(prop, np.int32)
    pos, kin = np.ascontiguousarray(pos, np.float64), np.ascontiguousarray(kin, np.float64)
    n = prop.shape[0]
    if pos.shape != (n, 3) or kin.shape != (n, KIN_CHANNELS):
        raise ValueError("write_vtu_kinematics: pos (n, 3) and kin (n, %d) expected" % KIN_CHANNELS)
    _check(load_library().mph_write_vtu_kinematics_arrays(path.encode(), n, prop.ctypes.data, pos.ctypes.data,
                                                          kin.ctypes.data))


# MphMonitorSlot (include/mph_gpu.h): name -> index into a sample's head
MONITOR_HEAD = 32
MONITOR_MAX_TRACK = 64
MONITOR_MAX_PROBES = 64
MONITOR_CLASSES = ("FLUID", "STRUCT", "WALL")
MONITOR_SLOTS = {"STEP": 0, "TIME": 1}
for _c, _cls in enumerate(MONITOR_CLASSES):
    for _k, _q in enumerate(("COUNT", "KE", "PX", "PY", "PZ", "VMAX2")):
        MONITOR_SLOTS["%s_%s" % (_cls, _q)] = 2 + 6 * _c + _k
MONITOR_SLOTS.update({"XMIN": 20, "XMAX": 21, "YMIN": 22, "YMAX": 23, "ZMIN": 24, "ZMAX": 25,
                      "FLUID_PMIN": 26, "FLUID_PMAX": 27, "WALL_PMAX": 28, "EPOT": 29,
                      "RESERVED0": 30, "RESERVED1": 31})


def monitor_split(row: np.ndarray, ntrack: int, nprobe: int):
    """One sample (or [k, width] samples) -> (head [.., 32], tracked [.., ntrack, 6] rows
    {x, y, z, vx, vy, vz}, probes [.., nprobe, 2] rows {value, count})."""
    row = np.asarray(row)
    lead = row.shape[:-1]
    a, b = MONITOR_HEAD, MONITOR_HEAD + 6 * ntrack
    if row.shape[-1] != b + 2 * nprobe:
        raise ValueError("a sample of %d tracked particles and %d probes has %d doubles, not %d"
                         % (ntrack, nprobe, b + 2 * nprobe, row.shape[-1]))
    return (row[..., :a], row[..., a:b].reshape(lead + (ntrack, 6)),
            row[..., b:].reshape(lead + (nprobe, 2)))


def monitor_gauges(row: np.ndarray, ntrack: int, nprobe: int, ngauge: int):
    """The gauge tail of one sample (or of [k, width] samples) of a configuration with gauges
    (mph_gauge_configure) -> [.., ngauge, 4] rows {COUNT, TOP, BOTTOM, WET} (GAUGE_CHANNELS)."""
    row = np.asarray(row)
    b = MONITOR_HEAD + 6 * ntrack + 2 * nprobe
    if row.shape[-1] != b + len(GAUGE_CHANNELS) * ngauge:
        raise ValueError("a sample of %d tracked particles, %d probes and %d gauges has %d doubles, not %d"
                         % (ntrack, nprobe, ngauge, b + len(GAUGE_CHANNELS) * ngauge, row.shape[-1]))
    return row[..., b:].reshape(row.shape[:-1] + (ngauge, len(GAUGE_CHANNELS)))


def monitor_combine(records, ntrack: int, nprobe: int) -> np.ndarray:
    """mph_monitor_combine: the slab ranks' records (records[r]: rank r's [k, 32 + 7 ntrack + 2 nprobe],
    MphSolver.dist_monitor_read_partial) -> the samples [k, 32 + 6 ntrack + 2 nprobe] that
    monitor_split reads.  Host only; a function of the records and of the rank order, bit for bit."""
    recs = [np.ascontiguousarray(r, np.float64) for r in records]
    w = MONITOR_HEAD + 7 * ntrack + 2 * nprobe
    if not recs or any(r.ndim != 2 or r.shape != (recs[0].shape[0], w) for r in recs):
        raise ValueError("every rank's records must be [k, %d] with the same k" % w)
    k = recs[0].shape[0]
    out = np.zeros((k, MONITOR_HEAD + 6 * ntrack + 2 * nprobe))
    ptrs = (ctypes.c_void_p * len(recs))(*[r.ctypes.data for r in recs])
    _check(load_library().mph_monitor_combine(len(recs), int(ntrack), int(nprobe), k, ptrs, out.ctypes.data))
    return out


def gauge_combine(records) -> np.ndarray:
    """mph_gauge_combine: the slab ranks' line records (records[r]: rank r's [..., 6],
    MphSolver.dist_gauge_grid(partial=True)) -> the map [..., 4] that MphSolver.gauge_grid gives on a
    single context.  Host only; every channel is a count, an extremum or a population, so the map is a
    bit-exact function of the state."""
    recs = [np.ascontiguousarray(r, np.float64) for r in records]
    w = len(DIST_GAUGE_RECORD)
    if not recs or any(r.ndim < 1 or r.shape != recs[0].shape or r.shape[-1] != w for r in recs):
        raise ValueError("every rank's records must have the same shape [..., %d]" % w)
    out = np.zeros(recs[0].shape[:-1] + (len(GAUGE_CHANNELS),))
    ptrs = (ctypes.c_void_p * len(recs))(*[r.ctypes.data for r in recs])
    _check(load_library().mph_gauge_combine(len(recs), recs[0].size // w, ptrs, out.ctypes.data))
    return out


class MphError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("%s (%d): %s" % (STATUS.get(code, "?"), code, msg))
        self.code = code


def build(verbose: bool = False) -> str:
    """Compile libmph_gpu.so and mph_explicit for gfx950 (hipcc, in-tree)."""
    r = subprocess.run(["make", "-C", CSRC_DIR, "-j8"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libmph_gpu.so failed:\n" + r.stdout + r.stderr)
    if verbose:
        print(r.stdout)
    return LIB_PATH


_lib = None


def load_library() -> ctypes.CDLL:
    """Load libmph_gpu.so (fails loudly when it is missing -- there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libmph_gpu.so not built (run particlemethod_fsi_amd.solver.build())")
    L = ctypes.CDLL(LIB_PATH)
    vp, ip, dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    cfgp = ctypes.POINTER(mphio.MphConfig)
    sig = {
        "mph_config_default": (ip, [cfgp, ip, ip]),
        "mph_read_data_file": (ip, [ctypes.c_char_p, cfgp]),
        "mph_read_grid_header": (ip, [ctypes.c_char_p, cfgp, ctypes.POINTER(ctypes.c_int)]),
        "mph_read_grid_particles": (ip, [ctypes.c_char_p, ip, vp, vp, vp, vp]),
        "mph_write_prof_arrays": (ip, [ctypes.c_char_p, cfgp, dp, ip, vp, vp, vp, vp]),
        "mph_write_vtk_arrays": (ip, [ctypes.c_char_p, ip] + [vp] * 10),
        "mph_create": (ip, [ctypes.POINTER(vp), cfgp, ip, vp, vp, vp, vp, ip]),
        "mph_step": (ip, [vp, ip]),
        "mph_synchronize": (ip, [vp]),
        "mph_get": (ip, [vp, ip, vp]),
        "mph_set": (ip, [vp, ip, vp]),
        "mph_particle_count": (ip, [vp]),
        "mph_time": (dp, [vp]),
        "mph_get_scalars": (ip, [vp, vp]),
        "mph_write_prof": (ip, [vp, ctypes.c_char_p]),
        "mph_write_vtk": (ip, [vp, ctypes.c_char_p]),
        "mph_last_error": (ctypes.c_char_p, [vp]),
        "mph_destroy": (None, [vp]),
        "mph_profile_steps": (ip, [vp, ip, vp, vp, vp]),
        "mph_profile_graphs": (ip, [vp, ip, vp]),
        "mph_neighbor_stats": (ip, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]),
        "mph_dist_unique_id": (ip, [vp]),
        "mph_create_dist": (ip, [ctypes.POINTER(vp), cfgp, ip, vp, vp, vp, vp, ip, ip, ip, vp, ip]),
        "mph_owned_count": (ip, [vp]),
        "mph_create_dist_host": (ip, [ctypes.POINTER(vp), cfgp, ip, vp, vp, vp, vp, ip, ip, ip, ip,
                                      HOST_EXCHANGE_FN, vp]),
        "mph_owned_ids": (ip, [vp, vp]),
        "mph_slab_bounds": (ip, [cfgp, ip, ip, ip, vp, vp]),
        "mph_slab_owner": (ip, [cfgp, ip, ip, vp, dp]),
        "mph_dist_selftest": (ip, [ip]),
        "mph_derive_scalars": (ip, [cfgp, vp]),
        "mph_structure_init": (ip, [cfgp, ip, vp, vp, vp, vp, vp, vp]),
        "mph_compute_virial": (ip, [vp]),
        "mph_config_sizeof": (ip, []),
        "mph_abi_version": (ip, []),
        "mph_write_grid_binary": (ip, [ctypes.c_char_p, cfgp, ip, vp, vp, vp, vp]),
        "mph_write_vtk_async": (ip, [vp, ctypes.c_char_p]),
        "mph_write_vtu_arrays": (ip, [ctypes.c_char_p, ip] + [vp] * 10),
        "mph_write_vtu": (ip, [vp, ctypes.c_char_p]),
        "mph_output_wait": (ip, [vp]),
        "mph_velocity_profile_arrays": (ip, [cfgp, dp, ip, vp, vp, vp, vp]),
        "mph_set_initial_velocity_profile": (ip, [vp]),
        "mph_dist_info": (ip, [vp, vp]),
        "mph_list_stats": (ip, [vp, vp, vp]),
        "mph_create_slab": (ip, [ctypes.POINTER(vp), cfgp, ip, vp, vp, vp, vp, ip, ctypes.POINTER(MphSlabOptions)]),
        "mph_slab_window": (ip, [cfgp, ip, ip, ip, vp, vp]),
        "mph_phase_timing": (ip, [vp, ip]),
        "mph_phase_times": (ip, [vp, vp]),
        "mph_set_step_batching": (ip, [vp, ip]),
        "mph_neighbor_rows": (ip, [vp, ip, ip, vp, vp, ctypes.c_longlong]),
        "mph_dist_overlap": (ip, [vp, vp]),
        "mph_list_layout": (ip, [vp, vp]),
        "mph_monitor_configure": (ip, [vp, ctypes.POINTER(MphMonitorConfig)]),
        "mph_monitor_sample_doubles": (ip, [vp]),
        "mph_monitor_read": (ctypes.c_longlong, [vp, vp, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]),
        "mph_sample_grid": (ip, [vp, ctypes.POINTER(MphSampleGrid), vp]),
        "mph_sample_grid_timed": (ip, [vp, ctypes.POINTER(MphSampleGrid), vp, ctypes.POINTER(ctypes.c_double), vp]),
        "mph_write_vti_arrays": (ip, [ctypes.c_char_p, ctypes.POINTER(MphSampleGrid), vp]),
        "mph_idle_wall_stats": (ip, [vp, vp]),
        "mph_lean_step_stats": (ip, [vp, vp]),
        "mph_key_fold_stats": (ip, [vp, vp]),
        "mph_list_format_stats": (ip, [vp, vp]),
        "mph_list_span_misses": (ip, [vp, vp]),
        "mph_list_wave_formats": (ip, [vp, vp]),
        "mph_gauge_configure": (ip, [vp, ctypes.POINTER(MphGaugeConfig)]),
        "mph_gauge_grid": (ip, [vp, ctypes.POINTER(MphGaugeGrid), vp]),
        "mph_selection_parse": (ip, [ctypes.c_char_p, ctypes.POINTER(MphSelection)]),
        "mph_selection_accepts": (ip, [ctypes.POINTER(MphSelection), ip, ip, ip, vp, vp]),
        "mph_selection_layout": (ip, [vp]),
        "mph_select": (ip, [vp, ctypes.POINTER(MphSelection), ctypes.POINTER(ctypes.c_int)]),
        "mph_selected_ids": (ip, [vp, vp]),
        "mph_get_selected": (ip, [vp, ip, vp]),
        "mph_selection_totals": (ip, [vp, vp, vp]),
        "mph_write_vtk_selected": (ip, [vp, ctypes.c_char_p]),
        "mph_write_vtu_selected": (ip, [vp, ctypes.c_char_p]),
        "mph_select_profile": (ip, [vp, ctypes.POINTER(MphSelection), vp, ip, vp, vp]),
        "mph_kinematics_layout": (ip, [vp]),
        "mph_kinematics_parse": (ip, [ctypes.c_char_p, ctypes.POINTER(MphKinematics)]),
        "mph_kinematics_n0": (ip, [cfgp, dp, ctypes.POINTER(ctypes.c_double)]),
        "mph_kinematics_arrays": (ip, [cfgp, ctypes.POINTER(MphKinematics), ip, vp, vp, vp, vp]),
        "mph_write_vtu_kinematics_arrays": (ip, [ctypes.c_char_p, ip, vp, vp, vp]),
        "mph_compute_kinematics": (ip, [vp, ctypes.POINTER(MphKinematics)]),
        "mph_compute_kinematics_timed": (ip, [vp, ctypes.POINTER(MphKinematics), ctypes.POINTER(ctypes.c_double), vp]),
        "mph_get_kinematics": (ip, [vp, vp]),
        "mph_get_kinematics_selected": (ip, [vp, vp]),
        "mph_write_vtu_kinematics": (ip, [vp, ctypes.c_char_p]),
        "mph_write_vtu_kinematics_selected": (ip, [vp, ctypes.c_char_p]),
        "mph_dist_monitor_configure": (ip, [vp, ctypes.POINTER(MphMonitorConfig)]),
        "mph_dist_monitor_record_doubles": (ip, [vp]),
        "mph_dist_monitor_read_partial": (ctypes.c_longlong, [vp, vp, ctypes.c_longlong,
                                                              ctypes.POINTER(ctypes.c_longlong)]),
        "mph_monitor_combine": (ip, [ip, ip, ip, ctypes.c_longlong, vp, vp]),
        "mph_dist_monitor_read": (ctypes.c_longlong, [vp, vp, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]),
        "mph_slab_lattice_owner": (ip, [cfgp, ip, ip, vp, dp, dp, ip, vp]),
        "mph_dist_sample_grid_partial": (ip, [vp, ctypes.POINTER(MphSampleGrid), vp, ctypes.POINTER(ctypes.c_longlong)]),
        "mph_dist_sample_grid": (ip, [vp, ctypes.POINTER(MphSampleGrid), vp]),
        "mph_dist_gauge_grid_partial": (ip, [vp, ctypes.POINTER(MphGaugeGrid), vp]),
        "mph_gauge_combine": (ip, [ip, ctypes.c_longlong, vp, vp]),
        "mph_dist_gauge_grid": (ip, [vp, ctypes.POINTER(MphGaugeGrid), vp]),
        "mph_dist_select": (ip, [vp, ctypes.POINTER(MphSelection), ctypes.POINTER(ctypes.c_int)]),
        "mph_dist_selected_ids": (ip, [vp, vp]),
        "mph_dist_get_selected": (ip, [vp, ip, vp]),
        "mph_dist_selection_totals_partial": (ip, [vp, vp, vp]),
        "mph_totals_combine": (ip, [ip, vp, vp]),
        "mph_dist_selection_totals": (ip, [vp, vp, vp]),
        "mph_dist_gather_selected": (ctypes.c_longlong, [vp, ip, vp, vp, ctypes.c_longlong]),
        "mph_dist_write_vtk_selected": (ip, [vp, ctypes.c_char_p]),
        "mph_dist_write_vtu_selected": (ip, [vp, ctypes.c_char_p]),
    }
    # entry points an older library may lack (A/B runs against earlier builds)
    optional = {"mph_phase_timing", "mph_phase_times", "mph_set_step_batching", "mph_neighbor_rows",
                "mph_dist_overlap", "mph_profile_graphs", "mph_list_stats", "mph_list_layout",
                "mph_monitor_configure", "mph_monitor_sample_doubles", "mph_monitor_read",
                "mph_sample_grid", "mph_sample_grid_timed", "mph_write_vti_arrays", "mph_idle_wall_stats",
                "mph_lean_step_stats", "mph_key_fold_stats", "mph_gauge_configure", "mph_gauge_grid",
                "mph_list_format_stats", "mph_list_span_misses", "mph_list_wave_formats",
                "mph_selection_parse", "mph_selection_accepts", "mph_selection_layout", "mph_select",
                "mph_selected_ids", "mph_get_selected", "mph_selection_totals", "mph_write_vtk_selected",
                "mph_write_vtu_selected", "mph_select_profile",
                "mph_kinematics_layout", "mph_kinematics_parse", "mph_kinematics_n0", "mph_kinematics_arrays",
                "mph_write_vtu_kinematics_arrays", "mph_compute_kinematics", "mph_compute_kinematics_timed",
                "mph_get_kinematics", "mph_get_kinematics_selected", "mph_write_vtu_kinematics",
                "mph_write_vtu_kinematics_selected",
                "mph_dist_monitor_configure", "mph_dist_monitor_record_doubles", "mph_dist_monitor_read_partial",
                "mph_monitor_combine", "mph_dist_monitor_read",
                "mph_slab_lattice_owner", "mph_dist_sample_grid_partial", "mph_dist_sample_grid",
                "mph_dist_gauge_grid_partial", "mph_gauge_combine", "mph_dist_gauge_grid",
                "mph_dist_select", "mph_dist_selected_ids", "mph_dist_get_selected",
                "mph_dist_selection_totals_partial", "mph_totals_combine", "mph_dist_selection_totals",
                "mph_dist_gather_selected", "mph_dist_write_vtk_selected", "mph_dist_write_vtu_selected"}
    for name, (res, args) in sig.items():
        if name in optional and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    # MPH_ABI_ACCEPT=3: an A/B run against a round-5 build (ABI 3 differs only by mph_list_formats,
    # replaced by mph_list_stats in 4; MPH_ABI_ACCEPT=4: a build before mph_list_layout, the only
    # change of 5; MPH_ABI_ACCEPT=5: a build before the monitors, the only change of 6;
    # tools/lib_bitwise.py)
    accept = {ABI_VERSION} | {int(v) for v in os.environ.get("MPH_ABI_ACCEPT", "").split(",") if v.strip()}
    if L.mph_abi_version() not in accept:
        raise ImportError("%s has C ABI version %d, these bindings expect %d (rebuild the library)"
                          % (LIB_PATH, L.mph_abi_version(), ABI_VERSION))
    if L.mph_config_sizeof() != ctypes.sizeof(mphio.MphConfig):
        raise ImportError("MphConfig layout mismatch between %s and mphio.MphConfig" % LIB_PATH)
    _lib = L
    return L


def read_case_files(data_path: str, grid_path: str, dim: int, module: str | int = "bar"):
    """readDataFile + readGridFile through the C++ host layer -> (MphConfig, Particles)."""
    L = load_library()
    cfg = mphio.MphConfig()
    mod = mphio.MODULES[module] if isinstance(module, str) else int(module)
    _check(L.mph_config_default(ctypes.byref(cfg), int(dim), mod))
    _check(L.mph_read_data_file(data_path.encode(), ctypes.byref(cfg)))
    n = ctypes.c_int(0)
    _check(L.mph_read_grid_header(grid_path.encode(), ctypes.byref(cfg), ctypes.byref(n)))
    N = n.value
    prop = np.zeros(N, np.int32)
    pos, pos0, vel = (np.zeros((N, 3)) for _ in range(3))
    _check(L.mph_read_grid_particles(grid_path.encode(), N, prop.ctypes.data, pos.ctypes.data,
                                     pos0.ctypes.data, vel.ctypes.data))
    return cfg, mphio.Particles(prop, pos, pos0, vel)


def write_grid_binary(path: str, cfg: mphio.MphConfig, parts: "mphio.Particles"):
    """Binary grid (include/mph_gpu.h mph_write_grid_binary); read_case_files reads it back."""
    p = [np.ascontiguousarray(a, np.float64) for a in (parts.position, parts.initial_position, parts.velocity)]
    prop = np.ascontiguousarray(parts.property, np.int32)
    _check(load_library().mph_write_grid_binary(path.encode(), ctypes.byref(cfg), parts.n, prop.ctypes.data,
                                                p[0].ctypes.data, p[1].ctypes.data, p[2].ctypes.data))


def read_vtu(path: str) -> dict:
    """Arrays of a .vtu written by mph_write_vtu(_arrays): {name: ndarray}, 'Points' for the
    coordinates (raw appended data, UInt64 block headers)."""
    import re
    raw = open(path, "rb").read()
    head, _, data = raw.partition(b'<AppendedData encoding="raw">')
    data = data[data.index(b"_") + 1:]
    dt = {"Float32": np.float32, "Float64": np.float64, "Int32": np.int32, "UInt8": np.uint8}
    out = {}
    for m in re.finditer(rb"<DataArray ([^>]*)/>", head):
        attrs = dict(re.findall(rb'(\w+)="([^"]*)"', m.group(1)))
        off = int(attrs[b"offset"])
        nb = int(np.frombuffer(data[off:off + 8], np.uint64)[0])
        a = np.frombuffer(data[off + 8:off + 8 + nb], dt[attrs[b"type"].decode()])
        k = int(attrs.get(b"NumberOfComponents", b"1"))
        out[attrs.get(b"Name", b"Points").decode()] = a.reshape(-1, k) if k > 1 else a
    return out


def write_vti(path: str, out: np.ndarray, origin, spacing, radius: float = 0.0, classes: int = 0):
    """VTK ImageData (.vti) of a sampled lattice (mph_write_vti_arrays): `out` as MphSolver.sample_grid
    returns it, shape (nz, ny, nx, 6), with the lattice's origin and spacing."""
    a = np.ascontiguousarray(out, np.float64)
    if a.ndim != 4 or a.shape[3] != len(SAMPLE_CHANNELS):
        raise ValueError("write_vti: an array of shape (nz, ny, nx, %d) expected" % len(SAMPLE_CHANNELS))
    g = _sample_grid(origin, spacing, a.shape[2::-1], radius, classes)
    _check(load_library().mph_write_vti_arrays(path.encode(), ctypes.byref(g), a.ctypes.data))


def read_vti(path: str) -> dict:
    """A .vti written by mph_write_vti_arrays: {name: ndarray of shape (nz, ny, nx) or (nz, ny, nx, 3)}
    plus 'origin', 'spacing' (3 floats each) and 'extent' (6 ints)."""
    import re
    raw = open(path, "rb").read()
    head, _, data = raw.partition(b'<AppendedData encoding="raw">')
    data = data[data.index(b"_") + 1:]
    img = dict(re.findall(rb'(\w+)="([^"]*)"', re.search(rb"<ImageData ([^>]*)>", head).group(1)))
    ext = [int(v) for v in img[b"WholeExtent"].split()]
    out = {"origin": [float(v) for v in img[b"Origin"].split()], "spacing": [float(v) for v in img[b"Spacing"].split()],
           "extent": ext}
    shape = (ext[5] - ext[4] + 1, ext[3] - ext[2] + 1, ext[1] - ext[0] + 1)
    for m in re.finditer(rb"<DataArray ([^>]*)/>", head):
        attrs = dict(re.findall(rb'(\w+)="([^"]*)"', m.group(1)))
        off = int(attrs[b"offset"])
        nb = int(np.frombuffer(data[off:off + 8], np.uint64)[0])
        a = np.frombuffer(data[off + 8:off + 8 + nb], {"Float64": np.float64}[attrs[b"type"].decode()])
        k = int(attrs.get(b"NumberOfComponents", b"1"))
        out[attrs[b"Name"].decode()] = a.reshape(shape + (k,)) if k > 1 else a.reshape(shape)
    return out


def derive_scalars(cfg: mphio.MphConfig) -> np.ndarray:
    """Derived constants of initializeWeight/Fluid/Wall/Domain, host only (no device needed)."""
    out = np.zeros(36)
    _check(load_library().mph_derive_scalars(ctypes.byref(cfg), out.ctypes.data))
    return out


def _check(rc, ctx=None):
    if rc < 0:
        msg = ""
        if ctx is not None:
            msg = (load_library().mph_last_error(ctx) or b"").decode()
        raise MphError(rc, msg)
    return rc


def _cuts(cuts, nranks: int):
    """(array kept alive, pointer or None) for MphSlabOptions.cuts / the host helpers."""
    if cuts is None:
        return None, None
    c = np.ascontiguousarray(cuts, np.float64)
    if c.shape != (nranks - 1,):
        raise ValueError("cuts: %d interior boundaries expected for %d slabs" % (nranks - 1, nranks))
    return c, c.ctypes.data


def slab_bounds(cfg: mphio.MphConfig, rank: int, nranks: int, axis: int, cuts=None):
    """(lo, hi, halo) of a rank's slab, as a slab context computes them (host only)."""
    out = np.zeros(3)
    c, p = _cuts(cuts, nranks)
    _check(load_library().mph_slab_bounds(ctypes.byref(cfg), rank, nranks, axis, p, out.ctypes.data))
    return float(out[0]), float(out[1]), float(out[2])


def slab_window(cfg: mphio.MphConfig, rank: int, nranks: int, axis: int, cuts=None):
    """(lo, hi): the periodic window of particles a rank needs for slab-local creation."""
    out = np.zeros(2)
    c, p = _cuts(cuts, nranks)
    _check(load_library().mph_slab_window(ctypes.byref(cfg), rank, nranks, axis, p, out.ctypes.data))
    return float(out[0]), float(out[1])


def slab_owner(cfg: mphio.MphConfig, nranks: int, axis: int, x: float, cuts=None) -> int:
    c, p = _cuts(cuts, nranks)
    return _check(load_library().mph_slab_owner(ctypes.byref(cfg), nranks, axis, p, float(x)))


def slab_lattice_owner(cfg: mphio.MphConfig, nranks: int, axis: int, origin_a: float, spacing_a: float,
                       count_a: int, cuts=None) -> np.ndarray:
    """mph_slab_lattice_owner: the rank that owns each of the count_a planes of an axis-aligned lattice
    along the slab axis -- slab_owner of origin_a + i spacing_a, the kernels' expression -> int32 [count_a]."""
    c, p = _cuts(cuts, nranks)
    owner = np.zeros(max(int(count_a), 1), np.int32)
    _check(load_library().mph_slab_lattice_owner(ctypes.byref(cfg), nranks, axis, p, float(origin_a), float(spacing_a),
                                                 int(count_a), owner.ctypes.data))
    return owner


class Slab:
    """Slab-mode options of MphSolver: this process is `rank` of `nranks`, slabs along `axis`.
    Transport: RCCL with the 128-byte unique id `uid` (mph_create_dist), or a host callback
    `exchange(send_l, send_r, recv_l, recv_r)` over memoryviews (mph_create_dist_host)."""

    def __init__(self, rank: int, nranks: int, axis: int, uid: bytes | None = None, exchange=None,
                 ids: np.ndarray | None = None, n_glob: int = 0, cuts=None):
        """ids/n_glob: slab-local creation -- the particles handed to MphSolver are only this
        rank's window (slab_window), with their original indices ids among n_glob.
        cuts: the nranks - 1 interior slab boundaries (None: equal slabs), the same on every rank
        (dist.balanced_cuts)."""
        if (uid is None) == (exchange is None):
            raise ValueError("Slab needs exactly one of uid (RCCL) or exchange (host transport)")
        self.rank, self.nranks, self.axis, self.uid, self.exchange = rank, nranks, axis, uid, exchange
        self.ids = None if ids is None else np.ascontiguousarray(ids, np.int32)
        self.n_glob = int(n_glob) if ids is not None else 0
        self.cuts = _cuts(cuts, nranks)[0]


def unique_id() -> bytes:
    """A fresh RCCL unique id (rank 0 calls this and shares it with the other ranks)."""
    buf = ctypes.create_string_buffer(128)
    _check(load_library().mph_dist_unique_id(buf))
    return buf.raw


class MphSolver:
    """One MI355X context running the reference hot path (see module docstring).  With
    `slab=Slab(...)` the context is one rank of the multi-GPU slab decomposition: get() then fills
    only the entries of the particles this rank owns (see owned_ids())."""

    def __init__(self, cfg: mphio.MphConfig, parts: mphio.Particles, device: int = 0,
                 slab: Slab | None = None):
        L = load_library()
        self._L = L
        self.cfg = cfg.copy()
        self.n = parts.n
        self.slab = slab
        self._arrays = [np.ascontiguousarray(parts.property, np.int32),
                        np.ascontiguousarray(parts.position, np.float64),
                        np.ascontiguousarray(parts.initial_position, np.float64),
                        np.ascontiguousarray(parts.velocity, np.float64)]
        h = ctypes.c_void_p()
        ptrs = [a.ctypes.data for a in self._arrays]
        if slab is None:
            rc = L.mph_create(ctypes.byref(h), ctypes.byref(self.cfg), self.n, *ptrs, int(device))
        else:
            opt = MphSlabOptions()
            opt.rank, opt.nranks, opt.axis = slab.rank, slab.nranks, slab.axis
            if slab.uid is not None:
                self._uid = ctypes.create_string_buffer(bytes(slab.uid), 128)
                opt.unique_id128 = ctypes.cast(self._uid, ctypes.c_char_p)
            else:
                self._cb = HOST_EXCHANGE_FN(_host_exchange_adapter(slab.exchange))
                opt.host_fn = self._cb
            if slab.ids is not None:
                if len(slab.ids) != parts.n:
                    raise ValueError("Slab.ids must index the particles passed in")
                opt.n_glob = slab.n_glob
                opt.ids = slab.ids.ctypes.data
                self._keep_ids = slab.ids
                self.n = slab.n_glob
            if slab.cuts is not None:
                opt.cuts = slab.cuts.ctypes.data
            rc = L.mph_create_slab(ctypes.byref(h), ctypes.byref(self.cfg), parts.n, *ptrs, int(device),
                                   ctypes.byref(opt))
        if rc < 0:
            msg = (L.mph_last_error(None) or b"").decode()
            raise MphError(rc, msg or "mph_create failed")
        self._h = h

    @classmethod
    def from_files(cls, data_path: str, grid_path: str, dim: int, module="bar", device: int = 0):
        cfg, parts = read_case_files(data_path, grid_path, dim, module)
        return cls(cfg, parts, device)

    # -- lifecycle -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.mph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- stepping ----------------------------------------------------------------------------
    def step(self, k: int = 1):
        _check(self._L.mph_step(self._h, int(k)), self._h)

    def synchronize(self):
        _check(self._L.mph_synchronize(self._h), self._h)

    @property
    def time(self) -> float:
        return self._L.mph_time(self._h)

    # -- data ----------------------------------------------------------------------------------
    def get(self, name: str) -> np.ndarray:
        fid, w, dt = FIELDS[name]
        shape = (self.n,) if w == 1 else ((self.n, 3) if w == 3 else (self.n, 3, 3))
        out = np.zeros(shape, dt)
        _check(self._L.mph_get(self._h, fid, out.ctypes.data), self._h)
        return out

    def set(self, name: str, values: np.ndarray):
        fid, _, _ = FIELDS[name]
        arr = np.ascontiguousarray(values, np.float64)
        _check(self._L.mph_set(self._h, fid, arr.ctypes.data), self._h)

    def set_initial_velocity_profile(self):
        """setInitialVelocityProfile (main.cpp:395-441) once on the current state: Bar beam mode or
        Turek_Hron inlet, by the configured module (the Turek inlet also runs every step)."""
        _check(self._L.mph_set_initial_velocity_profile(self._h), self._h)

    def scalars(self) -> np.ndarray:
        out = np.zeros(36)
        _check(self._L.mph_get_scalars(self._h, out.ctypes.data), self._h)
        return out

    def write_vtk(self, path: str):
        _check(self._L.mph_write_vtk(self._h, path.encode()), self._h)

    def write_vtu(self, path: str):
        """Binary VTK XML (.vtu) of the same fields as write_vtk (Float32, appended raw data)."""
        _check(self._L.mph_write_vtu(self._h, path.encode()), self._h)

    def write_vtk_async(self, path: str):
        """Snapshot now, format and write in the background (wait with output_wait())."""
        _check(self._L.mph_write_vtk_async(self._h, path.encode()), self._h)

    def output_wait(self):
        _check(self._L.mph_output_wait(self._h), self._h)

    def write_prof(self, path: str):
        _check(self._L.mph_write_prof(self._h, path.encode()), self._h)

    # -- measurement ----------------------------------------------------------------------------
    def profile(self, nsteps: int) -> dict:
        """Per-kernel average duration (ms) over nsteps, HIP events around every launch."""
        avg = np.zeros(24)
        cnt = np.zeros(24, np.int32)
        names = ctypes.create_string_buffer(24 * 32)
        k = _check(self._L.mph_profile_steps(self._h, int(nsteps), avg.ctypes.data, cnt.ctypes.data,
                                             ctypes.addressof(names)), self._h)
        raw = names.raw
        out = {}
        for i in range(k):
            nm = raw[32 * i:32 * (i + 1)].split(b"\0", 1)[0].decode()
            out[nm] = {"avg_ms": float(avg[i]), "launches": int(cnt[i])}
        return out

    def profile_graphs(self, reps: int = 16) -> dict:
        """The list kernels timed as graph replays (mph_profile_graphs): ms per launch of the search
        (with the XCD split), pass A and pass B; None where not measured."""
        out = np.zeros(3)
        _check(self._L.mph_profile_graphs(self._h, int(reps), out.ctypes.data), self._h)
        return {k: (float(v) if v >= 0 else None) for k, v in zip(("neighbors", "pass_a", "pass_b"), out)}

    def step_batching(self, on: bool = True):
        """mph_set_step_batching: step(1) per time-loop iteration costs what step(8) does; pending
        steps run (and their errors surface) at the next synchronize/get/write."""
        _check(self._L.mph_set_step_batching(self._h, 1 if on else 0), self._h)

    def phase_timing(self, on: bool = True):
        """Time the reference's clock() buckets (main.cpp:695-700) with HIP events at every step's
        phase boundaries; read the sums with phase_times().  While on, mph_step launches the steps'
        kernels directly instead of replaying the captured graphs (HIP cannot time events inside a
        graph) and waits for the events after every batch of up to 8 steps, so it is slower."""
        _check(self._L.mph_phase_timing(self._h, 1 if on else 0), self._h)

    def phase_times(self) -> dict:
        """Accumulated GPU milliseconds: neighbour search (sort + search), explicit calculation
        (sums, integration, elastic substeps), virial."""
        a = np.zeros(3)
        _check(self._L.mph_phase_times(self._h, a.ctypes.data), self._h)
        return {"neighbor_ms": float(a[0]), "explicit_ms": float(a[1]), "virial_ms": float(a[2])}

    # -- monitors ---------------------------------------------------------------------------------
    def monitor(self, stride=1, capacity: int = 4096, track=(), probes=(), probe_radius: float = 0.0,
                gauges=(), gauge_axis: int = -1, gauge_radius: float = 0.0):
        """mph_monitor_configure: from the next step on, every `stride`-th step leaves a sample
        (MONITOR_SLOTS, then the tracked particles `track` (original indices), then the pressure
        probes `probes` ([k][3] points)) in a device ring of `capacity` samples, computed inside the
        step graphs -- stepping stays batched, monitor_read() fetches.  monitor(None): off.
        gauges: free-surface gauges ([k][3] points, mph_gauge_configure), lines along `gauge_axis`
        (-1: gravity's) of radius `gauge_radius` (0: RadiusRatioP dx); each adds {COUNT, TOP, BOTTOM,
        WET} (GAUGE_CHANNELS) behind the probes, read with monitor_gauges()."""
        self._mon_gauges = 0
        if stride is None:
            _check(self._L.mph_monitor_configure(self._h, None), self._h)
            self._mon_shape = None
            return
        tr = np.ascontiguousarray(track, np.int32).reshape(-1)
        pr = np.ascontiguousarray(probes, np.float64).reshape(-1, 3)
        m = MphMonitorConfig(int(stride), int(capacity), len(tr), tr.ctypes.data if len(tr) else None,
                             len(pr), pr.ctypes.data if len(pr) else None, float(probe_radius))
        _check(self._L.mph_monitor_configure(self._h, ctypes.byref(m)), self._h)
        self._mon_shape = (len(tr), len(pr))
        self._mon_cap = int(capacity)
        ga = np.ascontiguousarray(gauges, np.float64).reshape(-1, 3)
        if len(ga):
            g = MphGaugeConfig(int(gauge_axis), len(ga), ga.ctypes.data, float(gauge_radius))
            _check(self._L.mph_gauge_configure(self._h, ctypes.byref(g)), self._h)
            self._mon_gauges = len(ga)

    def monitor_read(self, max_samples: int | None = None):
        """(samples [k, width], lost): the unread samples, oldest first, and how many unread ones the
        ring overwrote since the last read.  A flush point like get()."""
        w = self._L.mph_monitor_sample_doubles(self._h)
        if w == 0:
            return np.zeros((0, 0)), 0
        cap = int(max_samples) if max_samples is not None else self._mon_cap
        out = np.zeros((max(cap, 1), w))
        lost = ctypes.c_longlong(0)
        k = _check(self._L.mph_monitor_read(self._h, out.ctypes.data, cap, ctypes.byref(lost)), self._h)
        return out[:k].copy(), int(lost.value)

    # -- monitors on a slab rank --------------------------------------------------------------------
    def dist_monitor(self, stride=1, capacity: int = 4096, track=(), probes=(), probe_radius: float = 0.0):
        """mph_dist_monitor_configure: monitor() for a slab context, with the same configuration on
        every rank.  From the next step on every `stride`-th step leaves this rank's record -- the head
        over its owned particles, {present, x, y, z, vx, vy, vz} per tracked particle (original indices
        of the whole problem), {value, count} per probe its slab holds and {0, -1} per other probe --
        in its device ring; dist_monitor_read() makes samples of the ranks' records.
        dist_monitor(None): off."""
        self._mon_gauges = 0
        if stride is None:
            _check(self._L.mph_dist_monitor_configure(self._h, None), self._h)
            self._mon_shape = None
            return
        tr = np.ascontiguousarray(track, np.int32).reshape(-1)
        pr = np.ascontiguousarray(probes, np.float64).reshape(-1, 3)
        m = MphMonitorConfig(int(stride), int(capacity), len(tr), tr.ctypes.data if len(tr) else None,
                             len(pr), pr.ctypes.data if len(pr) else None, float(probe_radius))
        _check(self._L.mph_dist_monitor_configure(self._h, ctypes.byref(m)), self._h)
        self._mon_shape = (len(tr), len(pr))
        self._mon_cap = int(capacity)

    def _dist_monitor_read(self, fn, width, max_samples):
        if self._L.mph_dist_monitor_record_doubles(self._h) == 0:
            return np.zeros((0, 0)), 0
        cap = int(max_samples) if max_samples is not None else self._mon_cap
        out = np.zeros((max(cap, 1), width))
        lost = ctypes.c_longlong(0)
        k = _check(fn(self._h, out.ctypes.data, cap, ctypes.byref(lost)), self._h)
        return out[:k].copy(), int(lost.value)

    def dist_monitor_read_partial(self, max_samples: int | None = None):
        """(records [k, 32 + 7 ntrack + 2 nprobe], lost): this rank's unread records, oldest first; no
        communication.  monitor_combine() makes samples of all ranks' records."""
        return self._dist_monitor_read(self._L.mph_dist_monitor_read_partial,
                                       self._L.mph_dist_monitor_record_doubles(self._h), max_samples)

    def dist_monitor_read(self, max_samples: int | None = None):
        """(samples [k, 32 + 6 ntrack + 2 nprobe], lost), collective: every rank calls it with the same
        max_samples; rank 0 receives the combined samples (monitor_split reads them), every other
        rank none; lost is the rank's own."""
        nt, npr = self._mon_shape if self._mon_shape else (0, 0)
        return self._dist_monitor_read(self._L.mph_dist_monitor_read, MONITOR_HEAD + 6 * nt + 2 * npr, max_samples)

    def monitor_split(self, rows: np.ndarray):
        """monitor_split(rows, ...) with this solver's tracked-particle and probe counts."""
        nt, npr = self._mon_shape
        rows = np.asarray(rows)
        return monitor_split(rows[..., :rows.shape[-1] - len(GAUGE_CHANNELS) * self._mon_gauges], nt, npr)

    def monitor_gauges(self, rows: np.ndarray):
        """monitor_gauges(rows, ...) with this solver's counts: the gauges' records [.., ngauge, 4]."""
        nt, npr = self._mon_shape
        return monitor_gauges(rows, nt, npr, self._mon_gauges)

    # -- elevation map ----------------------------------------------------------------------------
    def gauge_grid(self, origin, spacing, count, axis: int = -1, radius: float = 0.0):
        """mph_gauge_grid: the gauge record of every line of a lattice of count = (nx, ny, nz) lines
        along `axis` (-1: gravity's; count[axis] must be 1) through origin + (i sx, j sy, k sz) ->
        array of shape (nz, ny, nx, 4), the channels GAUGE_CHANNELS (COUNT, TOP, BOTTOM, WET) over the
        fluid particles within `radius` (0: RadiusRatioP dx) of each line.  Needs a step since
        creation / the last set(); a flush point."""
        g = MphGaugeGrid()
        for d in range(3):
            g.origin[d], g.spacing[d], g.count[d] = float(origin[d]), float(spacing[d]), int(count[d])
        g.axis, g.radius = int(axis), float(radius)
        shape = (max(int(count[2]), 0), max(int(count[1]), 0), max(int(count[0]), 0), len(GAUGE_CHANNELS))
        n = shape[0] * shape[1] * shape[2]
        out = np.zeros(shape if 0 < n <= GAUGE_GRID_MAX_LINES else (1, 1, 1, len(GAUGE_CHANNELS)))
        _check(self._L.mph_gauge_grid(self._h, ctypes.byref(g), out.ctypes.data), self._h)
        return out

    # -- lattice sampling -------------------------------------------------------------------------
    def sample_grid(self, origin, spacing, count, radius: float = 0.0, classes: int = 0, timed: bool = False,
                    out: np.ndarray | None = None):
        """mph_sample_grid: the fields at the points origin + (i sx, j sy, k sz) of a lattice of
        count = (nx, ny, nz) points, evaluated on the device -> array of shape (nz, ny, nx, 6), the
        channels SAMPLE_CHANNELS (COUNT, WSUM = the fill level, P, VX, VY, VZ): Shepard averages over
        the particles of `classes` (bit mask SAMPLE_CLASSES, 0: fluid) within `radius` (0:
        RadiusRatioP dx) of each point.  Needs a step since creation / the last set(); a flush point.
        timed: (array, kernel milliseconds from HIP events, the kernel's profiler name).
        out: a C-contiguous float64 array of that shape to fill instead of a new one."""
        g = _sample_grid(origin, spacing, count, radius, classes)
        shape = (max(int(count[2]), 0), max(int(count[1]), 0), max(int(count[0]), 0), len(SAMPLE_CHANNELS))
        n = shape[0] * shape[1] * shape[2]
        if out is None:
            out = np.zeros(shape if 0 < n <= SAMPLE_MAX_POINTS else (1, 1, 1, len(SAMPLE_CHANNELS)))
        elif out.shape != shape or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("sample_grid: out must be a C-contiguous float64 array of shape %r" % (shape,))
        if not timed:
            _check(self._L.mph_sample_grid(self._h, ctypes.byref(g), out.ctypes.data), self._h)
            return out
        ms = ctypes.c_double(0.0)
        name = ctypes.create_string_buffer(32)
        _check(self._L.mph_sample_grid_timed(self._h, ctypes.byref(g), out.ctypes.data, ctypes.byref(ms),
                                             ctypes.addressof(name)), self._h)
        return out, ms.value, name.value.decode()

    # -- lattice sampling and elevation maps on slab ranks ------------------------------------------
    def dist_sample_grid(self, origin, spacing, count, radius: float = 0.0, classes: int = 0, partial: bool = False,
                         out: np.ndarray | None = None):
        """mph_dist_sample_grid: sample_grid() for a slab context, collective -- every rank calls it with
        the same lattice; rank 0 returns the whole lattice (nz, ny, nx, 6), every other rank None.
        partial (mph_dist_sample_grid_partial, no communication): (array, owned points) -- the rows of
        the lattice planes this rank owns (slab_lattice_owner) written into `out`, or into a new array
        filled with NaN, every other row left as it is."""
        g = _sample_grid(origin, spacing, count, radius, classes)
        shape = (max(int(count[2]), 0), max(int(count[1]), 0), max(int(count[0]), 0), len(SAMPLE_CHANNELS))
        n = shape[0] * shape[1] * shape[2]
        if out is None:
            out = np.full(shape if 0 < n <= SAMPLE_MAX_POINTS else (1, 1, 1, len(SAMPLE_CHANNELS)),
                          np.nan if partial else 0.0)
        elif out.shape != shape or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("dist_sample_grid: out must be a C-contiguous float64 array of shape %r" % (shape,))
        if partial:
            owned = ctypes.c_longlong(0)
            _check(self._L.mph_dist_sample_grid_partial(self._h, ctypes.byref(g), out.ctypes.data, ctypes.byref(owned)),
                   self._h)
            return out, owned.value
        _check(self._L.mph_dist_sample_grid(self._h, ctypes.byref(g), out.ctypes.data), self._h)
        return out if self.dist_info()["rank"] == 0 else None

    def dist_gauge_grid(self, origin, spacing, count, axis: int = -1, radius: float = 0.0, partial: bool = False):
        """mph_dist_gauge_grid: gauge_grid() for a slab context, collective -- rank 0 returns the map
        (nz, ny, nx, 4), every other rank None.  partial (mph_dist_gauge_grid_partial, no
        communication): this rank's records (nz, ny, nx, 6), the channels DIST_GAUGE_RECORD;
        gauge_combine() makes the map of all ranks' records."""
        g = MphGaugeGrid()
        for d in range(3):
            g.origin[d], g.spacing[d], g.count[d] = float(origin[d]), float(spacing[d]), int(count[d])
        g.axis, g.radius = int(axis), float(radius)
        w = len(DIST_GAUGE_RECORD) if partial else len(GAUGE_CHANNELS)
        shape = (max(int(count[2]), 0), max(int(count[1]), 0), max(int(count[0]), 0), w)
        n = shape[0] * shape[1] * shape[2]
        out = np.zeros(shape if 0 < n <= GAUGE_GRID_MAX_LINES else (1, 1, 1, w))
        if partial:
            _check(self._L.mph_dist_gauge_grid_partial(self._h, ctypes.byref(g), out.ctypes.data), self._h)
            return out
        _check(self._L.mph_dist_gauge_grid(self._h, ctypes.byref(g), out.ctypes.data), self._h)
        return out if self.dist_info()["rank"] == 0 else None

    # -- particle selections ----------------------------------------------------------------------
    def select(self, types=None, box=None, on: str = "position", every: int = 1, phase: int = 0, spec=None) -> int:
        """mph_select: make the particles of `types` (None: every type) with original index
        i % every == phase inside `box` ((x0, y0, z0), (x1, y1, z1): lo <= x < hi, tested on Position
        or, with on="initial", on InitialPosition; None: no box) the context's selection and return
        its size.  spec: a text spec (parse_selection) or an MphSelection instead of the other
        arguments.  A snapshot of the current state: the next step() or set() makes it stale, and
        the consumers below then raise MPH_ERR_ARG.  A flush point like get()."""
        if spec is None:
            sel = make_selection(types, box, on, every, phase)
        else:
            sel = spec if isinstance(spec, MphSelection) else parse_selection(spec)
        cnt = ctypes.c_int(0)
        _check(self._L.mph_select(self._h, ctypes.byref(sel), ctypes.byref(cnt)), self._h)
        self._sel_count = cnt.value
        return cnt.value

    def selected_ids(self) -> np.ndarray:
        """The selected original indices, ascending."""
        out = np.zeros(getattr(self, "_sel_count", 0), np.int32)
        _check(self._L.mph_selected_ids(self._h, out.ctypes.data), self._h)
        return out

    def get_selected(self, name: str) -> np.ndarray:
        """get(name)[selected_ids()], bit for bit, gathered on the device: only the selected rows
        are copied."""
        fid, w, dt = FIELDS[name]
        m = getattr(self, "_sel_count", 0)
        out = np.zeros((m,) if w == 1 else ((m, 3) if w == 3 else (m, 3, 3)), dt)
        _check(self._L.mph_get_selected(self._h, fid, out.ctypes.data), self._h)
        return out

    def selection_totals(self, center=(0.0, 0.0, 0.0)) -> dict:
        """mph_selection_totals: {TOTAL_SLOTS name: value} over the selection -- COUNT, MASS, momentum
        P*, KE, the summed Force F*, its torque T* about `center` (plain differences, no minimum
        image), the mass moment M*, the extent and VMAX2 -- reduced on the device in a fixed order."""
        c = np.ascontiguousarray(center, np.float64).reshape(3)
        out = np.zeros(TOTALS)
        _check(self._L.mph_selection_totals(self._h, c.ctypes.data, out.ctypes.data), self._h)
        return {k: float(out[i]) for k, i in TOTAL_SLOTS.items()}

    def write_vtk_selected(self, path: str):
        """write_vtk of the selection alone: the array writer's file for get(...)[selected_ids()]."""
        _check(self._L.mph_write_vtk_selected(self._h, path.encode()), self._h)

    def write_vtu_selected(self, path: str):
        _check(self._L.mph_write_vtu_selected(self._h, path.encode()), self._h)

    def select_profile(self, sel: MphSelection, center=(0.0, 0.0, 0.0)) -> list:
        """mph_select_profile: [(kernel name, ms)] of every launch of select(spec=sel), get_selected
        of Position, Velocity and PressureP, and selection_totals(center), from HIP events."""
        c = np.ascontiguousarray(center, np.float64).reshape(3)
        ms = np.zeros(64)
        names = ctypes.create_string_buffer(64 * 32)
        k = _check(self._L.mph_select_profile(self._h, ctypes.byref(sel), c.ctypes.data, 64, ms.ctypes.data,
                                              ctypes.addressof(names)), self._h)
        raw = names.raw
        return [(raw[32 * i:32 * (i + 1)].split(b"\0", 1)[0].decode(), float(ms[i])) for i in range(min(k, 64))]

    # -- particle selections on slab ranks ----------------------------------------------------------
    def dist_select(self, types=None, box=None, on: str = "position", every: int = 1, phase: int = 0, spec=None) -> int:
        """mph_dist_select: select() for a slab context, no communication -- among the particles this
        rank owns now (owned_ids()); returns this rank's count.  The ranks' selections partition the
        whole problem's.  Stale after step() / set() like a single context's."""
        if spec is None:
            sel = make_selection(types, box, on, every, phase)
        else:
            sel = spec if isinstance(spec, MphSelection) else parse_selection(spec)
        cnt = ctypes.c_int(0)
        _check(self._L.mph_dist_select(self._h, ctypes.byref(sel), ctypes.byref(cnt)), self._h)
        self._sel_count = cnt.value
        return cnt.value

    def dist_selected_ids(self) -> np.ndarray:
        """This rank's selected original indices (of the whole problem), ascending."""
        out = np.zeros(getattr(self, "_sel_count", 0), np.int32)
        _check(self._L.mph_dist_selected_ids(self._h, out.ctypes.data), self._h)
        return out

    def dist_get_selected(self, name: str) -> np.ndarray:
        """get(name)[dist_selected_ids()] of this rank, bit for bit, gathered on the device; no
        communication."""
        fid, w, dt = FIELDS[name]
        m = getattr(self, "_sel_count", 0)
        out = np.zeros((m,) if w == 1 else ((m, 3) if w == 3 else (m, 3, 3)), dt)
        _check(self._L.mph_dist_get_selected(self._h, fid, out.ctypes.data), self._h)
        return out

    def dist_selection_totals(self, center=(0.0, 0.0, 0.0), partial: bool = False):
        """mph_dist_selection_totals, collective: rank 0 returns {TOTAL_SLOTS name: value} over the
        whole problem's selection -- totals_combine of the ranks' records -- every other rank None.
        partial (mph_dist_selection_totals_partial, no communication): this rank's record [24]."""
        c = np.ascontiguousarray(center, np.float64).reshape(3)
        out = np.zeros(TOTALS)
        if partial:
            _check(self._L.mph_dist_selection_totals_partial(self._h, c.ctypes.data, out.ctypes.data), self._h)
            return out
        _check(self._L.mph_dist_selection_totals(self._h, c.ctypes.data, out.ctypes.data), self._h)
        if self.dist_info()["rank"] != 0:
            return None
        return {k: float(out[i]) for k, i in TOTAL_SLOTS.items()}

    def dist_gather_selected(self, name: str):
        """mph_dist_gather_selected, collective: rank 0 returns (ids, rows) -- every rank's selected
        rows of `name` merged by ascending original index -- every other rank None.  Only selected
        rows travel."""
        fid, w, dt = FIELDS[name]
        if self.dist_info()["rank"] != 0:
            _check(self._L.mph_dist_gather_selected(self._h, fid, None, None, 0), self._h)
            return None
        cap = self.n
        ids = np.zeros(max(cap, 1), np.int32)
        out = np.zeros((max(cap, 1),) if w == 1 else ((max(cap, 1), 3) if w == 3 else (max(cap, 1), 3, 3)), dt)
        k = _check(self._L.mph_dist_gather_selected(self._h, fid, out.ctypes.data, ids.ctypes.data, cap), self._h)
        return ids[:k].copy(), out[:k].copy()

    def dist_write_vtk_selected(self, path: str):
        """mph_dist_write_vtk_selected, collective: rank 0 writes the array writer's file of the merged
        selected rows."""
        _check(self._L.mph_dist_write_vtk_selected(self._h, path.encode()), self._h)

    def dist_write_vtu_selected(self, path: str):
        _check(self._L.mph_dist_write_vtu_selected(self._h, path.encode()), self._h)

    # -- velocity gradient, vorticity and free-surface fields ---------------------------------------
    def kinematics(self, radius: float = 0.0, classes: int = 0, beta: float = 0.0, det_floor: float = 0.0,
                   selected: bool = False, timed: bool = False):
        """mph_compute_kinematics + mph_get_kinematics: the [n, 24] array of per-particle records
        (columns KIN: COUNT, WSUM, FILL, the centroid offset C*, the velocity gradient L, DIV, the
        vorticity W*, SHEAR, FLAGS with the bits KIN_FLAGS) from one pass over the step's neighbour
        lists, over the neighbours of `classes` (SAMPLE_CLASSES mask, 0: all) within `radius` (0:
        RadiusRatioV dx, at most MaxRadius); beta: the FILL below which a particle is marked surface
        (0: 0.97); det_floor: the conditioning floor (0: 1e-6).  Legal before the first step, not
        between set() and the next step.  selected: the rows of the current selection only, gathered
        on the device.  timed: (array, kernel milliseconds from HIP events, the kernel's name)."""
        k = make_kinematics(radius, classes, beta, det_floor)
        ms = ctypes.c_double(0.0)
        name = ctypes.create_string_buffer(32)
        if timed:
            _check(self._L.mph_compute_kinematics_timed(self._h, ctypes.byref(k), ctypes.byref(ms),
                                                        ctypes.addressof(name)), self._h)
        else:
            _check(self._L.mph_compute_kinematics(self._h, ctypes.byref(k)), self._h)
        out = self.get_kinematics(selected)
        return (out, ms.value, name.value.decode()) if timed else out

    def get_kinematics(self, selected: bool = False) -> np.ndarray:
        """The records of the last kinematics() again (MPH_ERR_ARG once a step or set() made them
        stale): every particle in original order, or the current selection's rows."""
        if selected:
            out = np.zeros((getattr(self, "_sel_count", 0), KIN_CHANNELS))
            _check(self._L.mph_get_kinematics_selected(self._h, out.ctypes.data), self._h)
        else:
            out = np.zeros((self.n, KIN_CHANNELS))
            _check(self._L.mph_get_kinematics(self._h, out.ctypes.data), self._h)
        return out

    def write_vtu_kinematics(self, path: str, selected: bool = False):
        """The last kinematics() as a .vtu (mph_write_vtu_kinematics): every particle, or the current
        selection's rows."""
        f = self._L.mph_write_vtu_kinematics_selected if selected else self._L.mph_write_vtu_kinematics
        _check(f(self._h, path.encode()), self._h)

    def owned_ids(self) -> np.ndarray:
        """Original indices of the particles this context owns (all of them without a slab)."""
        k = self._L.mph_owned_count(self._h)
        out = np.zeros(max(self.n, 1), np.int32)
        _check(self._L.mph_owned_ids(self._h, out.ctypes.data), self._h)
        return out[:k].copy()

    def list_stats(self):
        """(mean, max) length of the stored neighbour lists of the last search (mph_list_stats: the
        pairs the passes walk; every neighbour with MPH_LIST_FULL=1)."""
        m = ctypes.c_double()
        x = ctypes.c_int()
        _check(self._L.mph_list_stats(self._h, ctypes.byref(m), ctypes.byref(x)), self._h)
        return m.value, x.value

    def list_layout(self) -> dict:
        """How the last search laid the stored lists out in rows (mph_list_layout): waves, the waves
        that jumped rows, the jumps in all and the most of one wave, the gap rows in all, and the most
        rows (entries + gaps) of one lane.  Single contexts only."""
        a = np.zeros(6, np.int64)
        _check(self._L.mph_list_layout(self._h, a.ctypes.data), self._h)
        keys = ["waves", "waves_jumped", "jumps", "max_jumps", "gap_rows", "max_rows"]
        return {k: int(v) for k, v in zip(keys, a)}

    def _counter_pair(self, entry: str, keys) -> dict:
        """Two step counters of the device state through `entry`; zeros from a library built before it."""
        a = np.zeros(2, np.int64)
        if hasattr(self._L, entry):
            _check(getattr(self._L, entry)(self._h, a.ctypes.data), self._h)
        return {k: int(v) for k, v in zip(keys, a)}

    def idle_wall_stats(self) -> dict:
        """Lazy wall steps since the creation (mph_idle_wall_stats): the wall waves the search skipped
        ("idle_wave_steps") over the steps that store no output-only field ("lazy_steps"); both 0
        in slab mode, with monitors, with MPH_LAZY_WALLS=0 at creation, or from a library built
        before the entry point."""
        return self._counter_pair("mph_idle_wall_stats", ("idle_wave_steps", "lazy_steps"))

    def lean_step_stats(self) -> dict:
        """Lean steps since the creation (mph_lean_step_stats): the lazy steps whose search ran its
        lean form ("search_steps") and those whose pass A did ("pass_a_steps"); both 0 wherever no
        step is lazy, with MPH_LEAN_STEPS=0 at creation, or from a library built before the entry
        point."""
        return self._counter_pair("mph_lean_step_stats", ("search_steps", "pass_a_steps"))

    def key_fold_stats(self) -> dict:
        """The key fold since the creation (mph_key_fold_stats): the steps whose pass B left the next
        step's cell keys ("folded_steps") and the steps that opened with a k_prep launch
        ("prep_launches"); the first 0 with structure particles, monitors, in slab mode or with
        MPH_KEY_FOLD=0 at creation, both 0 from a library built before the entry point."""
        return self._counter_pair("mph_key_fold_stats", ("folded_steps", "prep_launches"))

    def list_format_stats(self) -> dict:
        """The list formats of the last search (mph_list_format_stats): the waves with 16-bit rows
        ("short_waves"), those with 32-bit rows ("wide_waves") and, among the latter, the waves that
        began in the 16-bit format and started over ("restarted_waves"); zeros from a library built
        before the entry point."""
        a = np.zeros(3, np.int64)
        if hasattr(self._L, "mph_list_format_stats"):
            _check(self._L.mph_list_format_stats(self._h, a.ctypes.data), self._h)
        out = {k: int(v) for k, v in zip(("short_waves", "wide_waves", "restarted_waves"), a)}
        # of the wide waves, the interior ones the span limit alone turned away (mph_list_span_misses)
        m = np.zeros(1, np.int64)
        if hasattr(self._L, "mph_list_span_misses"):
            _check(self._L.mph_list_span_misses(self._h, m.ctypes.data), self._h)
        out["span_miss_waves"] = int(m[0])
        return out

    def list_wave_formats(self):
        """The last search's format decision wave by wave (mph_list_wave_formats): (codes, bases), one
        code per wave of 64 sorted particles -- 0 never decided, 1 16-bit rows, 2 began in the 16-bit
        format and started over, 3 turned away by the span limit -- and the seven group bases of
        every wave with 16-bit rows (zeros elsewhere)."""
        a = np.zeros(((self.n + 63) // 64, 8), np.int32)
        _check(self._L.mph_list_wave_formats(self._h, a.ctypes.data), self._h)
        return a[:, 0].copy(), a[:, 1:].copy()

    def neighbor_rows(self, first: int = 0, count: int | None = None):
        """(counts, offsets, ids): the neighbour sets of the particles [first, first + count) from
        the last search (mph_neighbor_rows; calculateNeighbor's Neighbor[i][k], main.cpp:1764-1772),
        each row as ascending original indices, row k = ids[offsets[k]:offsets[k + 1]]."""
        if count is None:
            count = self.n - first
        counts = np.zeros(count, np.int32)
        cap = max(1, count * 128)
        while True:
            ids = np.zeros(cap, np.int32)
            r = self._L.mph_neighbor_rows(self._h, int(first), int(count), counts.ctypes.data, ids.ctypes.data, cap)
            need = int(np.minimum(counts, 512).sum()) if r == -1 else 0
            if r == -1 and need > cap:
                cap = need
                continue
            _check(r, self._h)
            break
        offsets = np.concatenate([[0], np.cumsum(np.minimum(counts, 512))]).astype(np.int64)
        return counts, offsets, ids[:r].copy()

    def dist_info(self) -> dict:
        """Slab-mode facts (mph_dist_info): slab ranks, RCCL communicator size (0: host-staged),
        graph replay, capacities."""
        a = np.zeros(8, np.int32)
        _check(self._L.mph_dist_info(self._h, a.ctypes.data), self._h)
        keys = ["nranks", "rank", "rccl_ranks", "graphs", "cap", "cap_send", "cap_recv", "held"]
        return {k: int(v) for k, v in zip(keys, a)}

    def dist_overlap(self) -> dict:
        """Pass-B mode of a slab context (mph_dist_overlap): overlap on/off, whether MPH_SLAB_OVERLAP
        forced it or the creation probe chose it, and the probe's maxima over ranks (ms)."""
        a = np.zeros(5)
        _check(self._L.mph_dist_overlap(self._h, a.ctypes.data), self._h)
        return {"overlap": bool(a[0] == 1.0), "chosen_by": {-1: "probe", 0: "forced", 1: "forced"}.get(int(a[1]), "none"),
                "halo_exchange_ms": float(a[2]), "redistribution_exchange_ms": float(a[3]),
                "split_pass_b_cost_ms": float(a[4])}

    def compute_virial(self):
        """calculateVirialStressAtParticle (main.cpp:3077-3318) on the current state; read the result
        with get("VirialStressAtParticle") / get("VirialPressureAtParticle")."""
        _check(self._L.mph_compute_virial(self._h), self._h)

    def neighbor_stats(self):
        m = ctypes.c_double()
        x = ctypes.c_int()
        _check(self._L.mph_neighbor_stats(self._h, ctypes.byref(m), ctypes.byref(x)), self._h)
        return m.value, x.value


def _host_exchange_adapter(fn):
    """Wrap a Python exchange(send_l, send_r, recv_l, recv_r) over writable memoryviews as an
    mph_host_exchange_fn; exceptions become a nonzero return (MPH_ERR_TRANSPORT)."""
    def view(ptr, n):
        if not n:
            return memoryview(bytearray(0))
        return memoryview((ctypes.c_uint8 * n).from_address(ptr)).cast("B")

    def cb(user, sl, nsl, sr, nsr, rl, nrl, rr, nrr):
        try:
            fn(view(sl, nsl), view(sr, nsr), view(rl, nrl), view(rr, nrr))
            return 0
        except Exception as e:  # reported through the status code
            import sys
            print("mph host exchange failed: %r" % (e,), file=sys.stderr)
            return 1
    return cb
