"""The long-row geometry of the 16-bit list rows' tests and a plain model of the format decision
(DESIGN.md section 3.3), shared by test_list16_long_model.py (CPU) and test_gpu_list16_long.py.

The geometry: a strip 10 dx wide and up to 1,800 dx long on the contiguous cell axis -- a floor
(type 4), four fluid slabs of stepped lengths (1,250 to 1,800 dx), a short ledge of type 0 on top
with a cap of type 5 -- 283,500 particles, 4,430 waves.  A cell row along the long axis holds five
to six lattice lines, so a stencil group (seven cell rows) spans 3,000 to 9,300 sorted indices:
waves on both sides of the 8191 limit, offsets with every one of the 13 bits set.  The ledge's
lines are 12 particles long three cell rows above lines of 1,800: its waves cover several cell
rows, and their candidates in the columns below are short runs a whole long line apart -- windows
thousands of records wide that no two-run split fits.

The model is numpy from the definitions: each particle's cell from the grid (choose_grid,
choose_grid_origin) and the cell order (DevParams.perm), the sorted keys, start[] by searchsorted,
and per wave of 64 sorted particles the seven group spans start[hi_g] - start[lo_g] and the
untrimmed window of each of the 49 stencil columns.  Order inside a cell does not matter to any of
it; a case with a particle within 1e-9 cell widths of a cell face is refused.
"""
from __future__ import annotations

import functools
import os
import re
from dataclasses import dataclass

import numpy as np

from particlemethod_fsi_amd import cases, mphio
from particlemethod_fsi_amd.mphio import Cuboid

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "particlemethod_fsi_amd", "csrc")


def _define(path, name):
    m = re.search(r"^\s*(?:#define\s+%s\s+|constexpr int %s = )(\d+)" % (name, name), open(os.path.join(CSRC, path)).read(), re.M)
    assert m, (path, name)
    return int(m.group(1))


K_REACH = _define("mph_params.h", "MPH_R")        # stencil reach across the two column axes, cells
SA = _define("mph_params.h", "MPH_SA")            # and along the contiguous axis
OFF_BITS = _define("mph_params.h", "kOff16Bits")
SPAN_LIMIT = (1 << OFF_BITS) - 1                  # kList16Span: 8191
GROUPS = 2 * K_REACH + 1
WAVE = 64
_CAP, _SB = _define("mph_search.hip", "MPH_LDS_CAP"), _define("mph_search.hip", "MPH_SB")
# the staging area in 16-byte records, less the SB + 1 past a window's end (mph_search.hip stage_words, kCap32)
CAP32 = (3 * ((_CAP + _SB + 3) & ~1) + ((_CAP + _SB + 11) & ~3) // 2) // 2 - _SB - 1

DX = 0.001
AXES = {"x": 0, "y": 1, "z": 2}
# (type, lower, upper) with the long axis last
_BLOCKS = [
    (4, (0.0, 0.0, 0.0), (0.010, 0.003, 1.25)),
    (1, (0.0, 0.003, 0.0), (0.010, 0.007, 1.25)),
    (1, (0.0, 0.007, 0.0), (0.010, 0.011, 1.45)),
    (1, (0.0, 0.011, 0.0), (0.010, 0.015, 1.62)),
    (1, (0.0, 0.015, 0.0), (0.010, 0.019, 1.80)),
    (0, (0.0, 0.019, 0.0), (0.010, 0.027, 0.012)),
    (5, (0.0, 0.027, 0.0), (0.010, 0.029, 0.012)),
]
_LOWER, _UPPER = (-0.01, -0.01, -0.01), (0.02, 0.039, 1.81)
N_PARTICLES = 283500
# The seed of mphio.jitter (amplitude 0.3 dx).  The cells across the strip are 0.875 dx wide, so a
# coordinate printed with seven digits can lie exactly on a cell face, which the model refuses: 22 %
# of the seeds leave no such particle, and of the first 300 this one also puts two waves' widest
# span at exactly 8191 and one at 8192.
SEED = 253


def order_axis(perm, k):
    """Axis of cell order `perm` at position k (0 slowest, 2 contiguous): DevParams.perm."""
    return {0: (0, 1, 2), 1: (2, 0, 1), 2: (2, 1, 0), 3: (1, 2, 0), 4: (0, 2, 1)}[perm][k]


def perm_axis(perm):
    """The name of the contiguous axis of cell order `perm`: the long axis to build for it."""
    return "xyz"[order_axis(perm, 2)]


@functools.lru_cache(maxsize=None)
def _base_particles(seed):
    parts = mphio.generate([Cuboid(t, lo, up, DX) for t, lo, up in _BLOCKS])
    with np.errstate(over="ignore"):   # (the seed's multiple wraps in 64 bits)
        parts = mphio.jitter(parts, DX, 0.3, 3, seed=seed)
    assert parts.n == N_PARTICLES
    return parts


def build(axis="z", solid=False, data_changes=None, seed=SEED):
    """-> (MphConfig, Particles): the geometry with its long axis along `axis` (the coordinates
    rotated cyclically); solid: the second fluid slab as type 2 with four elastic substeps per step;
    data_changes: further parameter changes (cases._ST).  The positions are the same in every form."""
    r = (AXES[axis] + 1) % 3                          # column c of the built set goes to axis (c + r) % 3
    rot = lambda v: tuple(v[(d - r) % 3] for d in range(3))
    changes = dict(data_changes or {})
    if solid:
        changes["ElasticDt"] = [2.5e-5]
    cfg, _ = cases.Case("list16_long", 3, "dam", DX, rot(_LOWER), rot(_UPPER), [], data_changes=changes)._config()
    b = _base_particles(seed)
    src = [(d - r) % 3 for d in range(3)]
    prop = b.property.copy()
    if solid:
        lo, up = _BLOCKS[2][1], _BLOCKS[2][2]
        n0 = sum(int(round((u[0] - l[0]) / DX)) * int(round((u[1] - l[1]) / DX)) * int(round((u[2] - l[2]) / DX))
                 for _, l, u in _BLOCKS[:2])
        n1 = n0 + int(round((up[0] - lo[0]) / DX)) * int(round((up[1] - lo[1]) / DX)) * int(round((up[2] - lo[2]) / DX))
        assert (prop[n0:n1] == 1).all() and n1 - n0 == 58000
        prop[n0:n1] = 2
    # the reference takes each class (fluid, structure, wall) as one range of indices, first to last
    # particle of the class: the blocks, generated and moved off the lattice in the table's order, are
    # put in that order of classes
    idx = np.argsort(np.where(prop < 2, 0, np.where(prop < 4, 1, 2)), kind="stable")
    pos = np.ascontiguousarray(b.position[idx][:, src])
    return cfg, mphio.Particles(prop[idx], pos, pos.copy(), np.ascontiguousarray(b.velocity[idx][:, src]))


# ---------------------------------------------------------------------------------- the model ----

@dataclass
class Model:
    perm: int
    gc: tuple            # cells per axis (x, y, z)
    order: np.ndarray    # sorted position -> original index (any order inside a cell)
    key: np.ndarray      # sorted cell keys
    start: np.ndarray    # start[c]: the first sorted index of cell c; ncell + 1 entries
    lmin: np.ndarray     # per wave: the lowest and the highest cell
    lmax: np.ndarray
    base: np.ndarray     # [waves, 7]: start[lo_g]
    span: np.ndarray     # [waves, 7]: start[hi_g] - start[lo_g]
    interior: np.ndarray  # per particle: at least reach + 1 cells from every face of the grid
    window: np.ndarray   # [waves]: the widest untrimmed column window
    wide: np.ndarray     # waves with a window > CAP32, ascending
    unsplit: np.ndarray  # those of `wide` with a window > CAP32 that the widest-gap split cannot fit

    @property
    def waves(self):
        return len(self.lmin)

    @property
    def widest(self):
        return self.span.max(axis=1)

    def fits(self, limit=SPAN_LIMIT):
        return (self.span <= limit).all(axis=1)

    def wave_cells_particles(self, w):
        """Original indices of every particle in a cell that wave w touches: the wave's own particles
        and, where it begins or ends inside a cell, that cell's others."""
        a, b = self.start[self.lmin[w]], self.start[self.lmax[w] + 1]
        return np.sort(self.order[a:b])


def _grid(cfg, perm):
    dmin = np.array(cfg.domain_min[:])
    dw = np.array(cfg.domain_max[:]) - dmin
    rc = max(cfg.radius_ratio_a, cfg.radius_ratio_p, cfg.radius_ratio_v) * cfg.particle_spacing + 0.1 * cfg.particle_spacing
    ca = order_axis(perm, 2)
    reach = [SA if d == ca else K_REACH for d in range(3)]
    gc = [int(np.floor(dw[d] / (rc / reach[d] * (1.0 + 1e-6)))) for d in range(3)]
    return dmin, dw, gc, reach


def _origin(occupied, m):
    """choose_grid_origin: the grid's first cell, in whole cells from the domain's lower face: 0
    unless particles lie within m cells of a face, then the middle of the longest circular run of
    empty cells when that run is at least 2 m + 2 long."""
    gc = len(occupied)
    if not (occupied[:m].any() or occupied[gc - m:].any()):
        return 0
    first = int(np.argmax(occupied))
    best, best_start, run = 0, 0, 0
    for k in range(1, gc + 1):
        c = (first + k) % gc
        if not occupied[c]:
            if run == 0:
                run_start = c
            run += 1
        else:
            if run > best:
                best, best_start = run, run_start
            run = 0
    return (best_start + best // 2) % gc if best >= 2 * m + 2 else 0


def model(cfg, parts, perm=0, windows=True) -> Model:
    dmin, dw, gc, reach = _grid(cfg, perm)
    n = parts.n
    cell = np.zeros((n, 3), np.int64)
    interior = np.ones(n, bool)
    for d in range(3):
        u = (parts.position[:, d] - dmin[d]) * (gc[d] / dw[d])
        occ = np.zeros(gc[d], bool)
        occ[np.clip(np.floor(u).astype(np.int64), 0, gc[d] - 1)] = True
        s0 = _origin(occ, reach[d] + 1)
        u = np.mod(u - s0, gc[d])
        f = u - np.floor(u)
        if (np.minimum(f, 1.0 - f) < 1e-9).any():
            raise ValueError("a particle within 1e-9 cell widths of a cell face along axis %d" % d)
        cell[:, d] = np.floor(u).astype(np.int64)
        interior &= (u >= reach[d] + 1 + 1e-6) & (u <= gc[d] - reach[d] - 1 - 1e-6)
    a0, a1, a2 = (order_axis(perm, k) for k in range(3))
    g1, g2 = gc[a1], gc[a2]
    ncell = gc[0] * gc[1] * gc[2]
    lin = (cell[:, a0] * g1 + cell[:, a1]) * g2 + cell[:, a2]
    order = np.argsort(lin, kind="stable")
    key = lin[order]
    start = np.searchsorted(key, np.arange(ncell + 1)).astype(np.int64)
    waves = (n + WAVE - 1) // WAVE
    first = np.arange(waves) * WAVE
    lmin, lmax = key[first], key[np.minimum(first + WAVE - 1, n - 1)]
    # a group: the stencil columns of one slowest-axis offset dg.  Its candidates begin at the first
    # cell of its first column as the wave's lowest cell sees it and end before the cell past its last
    # column's last cell as the highest cell sees it.
    dg = np.arange(-K_REACH, K_REACH + 1)
    lo = np.clip(lmin[:, None] + (dg[None, :] * g1 - K_REACH) * g2 - SA, 0, ncell)
    hi = np.clip(lmax[:, None] + (dg[None, :] * g1 + K_REACH) * g2 + SA + 1, 0, ncell)
    base = start[lo]
    span = start[hi] - base
    m = Model(perm, tuple(gc), order, key, start, lmin, lmax, base, span, interior[order],
              np.zeros(waves, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64))
    if windows:
        _windows(m, g1, g2, ncell)
    return m


def _windows(m, g1, g2, ncell):
    """Per wave and stencil column the untrimmed window: the union of the lanes' ranges of +-SA
    cells in the column's row, [lowest begin, highest end) over the lanes with a candidate."""
    n, waves = len(m.key), m.waves
    first = np.arange(waves) * WAVE
    widest = np.zeros(waves, np.int64)
    cols = [(a, b) for a in range(-K_REACH, K_REACH + 1) for b in range(-K_REACH, K_REACH + 1)]
    big = np.iinfo(np.int64).max
    wide_cols = []
    for a, b in cols:
        c = m.key + (a * g1 + b) * g2
        jb = m.start[np.clip(c - SA, 0, ncell)]
        je = m.start[np.clip(c + SA + 1, 0, ncell)]
        has = je > jb
        mn = np.minimum.reduceat(np.where(has, jb, big), first)
        mx = np.maximum.reduceat(np.where(has, je, -1), first)
        w = np.where(mx >= 0, mx - mn, 0)
        widest = np.maximum(widest, w)
        for wv in np.nonzero(w > CAP32)[0]:
            s = slice(wv * WAVE, min(n, (wv + 1) * WAVE))
            wide_cols.append((int(wv), jb[s][has[s]], je[s][has[s]]))
    m.window = widest
    m.wide = np.unique(np.array([w for w, _, _ in wide_cols], np.int64))
    # the split at the widest gap: a lane whose range begins past every earlier lane's end; the two
    # runs' windows together are the whole window less that gap
    unsplit = set()
    for wv, jb, je in wide_cols:
        gaps = jb[1:] - np.maximum.accumulate(je)[:-1]
        gmax = int(gaps.max()) if len(gaps) else 0
        if gmax <= 0 or (je.max() - jb.min()) - gmax > CAP32:
            unsplit.add(wv)
    m.unsplit = np.array(sorted(unsplit), np.int64)


def high_offset_types(m, parts, limit=SPAN_LIMIT, half=1 << (OFF_BITS - 1)):
    """The particle types that occur as neighbours at an offset >= `half` from their group's base
    in some wave with every span <= limit (the entries of a 16-bit wave with bit 12 set)."""
    x = parts.position[m.order]
    t = parts.property[m.order]
    rc = 2.6 * DX
    a0 = order_axis(m.perm, 0)
    a1, a2 = order_axis(m.perm, 1), order_axis(m.perm, 2)
    g1, g2 = m.gc[a1], m.gc[a2]
    found = set()
    want = set(np.unique(t).tolist())
    ok = m.fits(limit)
    for w in np.nonzero(ok & (m.widest >= half))[0]:
        s = slice(w * WAVE, min(len(x), (w + 1) * WAVE))
        c0 = m.key[s] // (g1 * g2)                 # the lanes' cells along the slowest axis
        for g in np.nonzero(m.span[w] > half)[0]:
            j = np.arange(m.base[w, g] + half, m.base[w, g] + m.span[w, g])
            j = j[~np.isin(t[j], list(found))]
            if not len(j):
                continue
            cj = m.key[j] // (g1 * g2)
            for c in np.unique(c0):
                lanes = x[s][c0 == c]
                cand = j[cj == c + g - K_REACH]
                if not len(cand):
                    continue
                box = ((x[cand] >= lanes.min(axis=0) - rc) & (x[cand] <= lanes.max(axis=0) + rc)).all(axis=1)
                cand = cand[box]
                if not len(cand):
                    continue
                d2 = ((x[cand][None, :, :] - lanes[:, None, :]) ** 2).sum(axis=2)
                found |= set(t[cand[(d2 <= rc * rc).any(axis=0)]].tolist())
        if found >= want:
            break
    return found
