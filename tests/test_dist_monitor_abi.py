"""CPU: the slab monitors' part of the C ABI (include/mph_gpu.h mph_dist_monitor_*, mph_monitor_combine)
and the combine rule itself, which is host code: rank records [k][32 + 7 ntrack + 2 nprobe] in, samples
[k][32 + 6 ntrack + 2 nprobe] out; every head slot from rank 0's value through ranks 1, 2, ... in order,
a tracked entry from the one rank with present == 1, a probe from the one rank with count >= 0.
"""
import os
import re

import numpy as np
import pytest

from particlemethod_fsi_amd import solver
from particlemethod_fsi_amd.solver import MONITOR_SLOTS as S, MphError, monitor_combine, monitor_split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mph_gpu.h")
NEW = ("mph_dist_monitor_configure", "mph_dist_monitor_record_doubles", "mph_dist_monitor_read_partial",
       "mph_monitor_combine", "mph_dist_monitor_read")

SUMS = [k for k in S if k.split("_")[-1] in ("COUNT", "KE", "PX", "PY", "PZ")] + ["EPOT"]
MINS = ["XMIN", "YMIN", "ZMIN", "FLUID_PMIN"]
MAXS = ["XMAX", "YMAX", "ZMAX", "FLUID_PMAX", "WALL_PMAX", "FLUID_VMAX2", "STRUCT_VMAX2", "WALL_VMAX2"]


def test_symbols_in_header_bindings_and_library():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = solver.load_library()
    for name in NEW:
        assert name in solver.EXPORTED_SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(L, name), name
    assert sorted(SUMS + MINS + MAXS + ["STEP", "TIME", "RESERVED0", "RESERVED1"]) == sorted(S)


def _empty_rank(k, ntrack, nprobe, step0=1):
    """k records of a rank that holds nothing: the reductions' identities, no tracked row, no probe."""
    r = np.zeros((k, 32 + 7 * ntrack + 2 * nprobe))
    r[:, S["STEP"]] = np.arange(step0, step0 + k)
    r[:, S["TIME"]] = 1e-3 * np.arange(step0, step0 + k)
    for name in MINS:
        r[:, S[name]] = np.inf
    for name in MAXS:
        r[:, S[name]] = 0.0 if name.endswith("VMAX2") else -np.inf
    r[:, 32 + 7 * ntrack + 1::2] = -1.0   # every probe's count: not owned
    return r


@pytest.mark.parametrize("nranks", [1, 2, 5])
def test_sums_in_rank_order_bit_for_bit(nranks):
    # 1.0 + 2^-53 + 2^-53: left to right the small terms are lost one by one, the other way they add up
    base = [1.0, 2.0 ** -53, 2.0 ** -53, -0.75, 3.0e-17]
    assert (base[0] + base[1]) + base[2] != base[0] + (base[1] + base[2])
    recs = [_empty_rank(3, 0, 0) for _ in range(nranks)]
    for r in range(nranks):
        for j, name in enumerate(SUMS):
            # every slot its own rotation of the values, scaled per sample
            recs[r][:, S[name]] = [base[(r + j) % len(base)] * (1.0 + s) for s in range(3)]
    out = monitor_combine(recs, 0, 0)
    assert out.shape == (3, 32)
    differs = False
    for s in range(3):
        for name in SUMS:
            v = recs[0][s, S[name]]
            for r in range(1, nranks):
                v = v + recs[r][s, S[name]]
            assert out[s, S[name]] == v, (name, s)
            if nranks >= 3:
                back = recs[nranks - 1][s, S[name]]
                for r in range(nranks - 2, -1, -1):
                    back = back + recs[r][s, S[name]]
                differs = differs or back != v
        assert out[s, S["STEP"]] == s + 1 and out[s, S["TIME"]] == recs[0][s, S["TIME"]]
        assert out[s, S["RESERVED0"]] == 0.0 and out[s, S["RESERVED1"]] == 0.0
    if nranks >= 3:
        assert differs   # the rank order is visible in the bits: another order gives another sum
    if nranks == 1:
        assert np.array_equal(out, recs[0])


@pytest.mark.parametrize("nranks", [1, 2, 5])
def test_extrema_across_ranks_and_an_empty_rank(nranks):
    recs = [_empty_rank(2, 0, 0) for _ in range(nranks)]
    holds = [r for r in range(nranks) if r != 1]   # rank 1 (where there is one) holds no particle
    for r in holds:
        for j, name in enumerate(MINS):
            recs[r][:, S[name]] = [0.1 * (r + 1) - 0.01 * j, -0.2 * (r + 1) + j]
        for j, name in enumerate(MAXS):
            recs[r][:, S[name]] = [0.3 * (nranks - r) + j, 7.0 * (r + 1) + j * j]
    out = monitor_combine(recs, 0, 0)
    for s in range(2):
        for name in MINS:
            assert out[s, S[name]] == min(recs[r][s, S[name]] for r in holds), name
        for name in MAXS:
            assert out[s, S[name]] == max(recs[r][s, S[name]] for r in holds), name
        assert np.isfinite(out[s, 2:30]).all()
    # nothing anywhere: the identities stay
    none = monitor_combine([_empty_rank(1, 0, 0) for _ in range(nranks)], 0, 0)
    assert none[0, S["XMIN"]] == np.inf and none[0, S["WALL_PMAX"]] == -np.inf and none[0, S["FLUID_VMAX2"]] == 0.0


def _row(present, seed):
    return [1.0] + [seed + 0.125 * e for e in range(6)] if present else [0.0] * 7


def test_tracked_row_moves_between_ranks_and_probes():
    nt, npr = 2, 2
    recs = [_empty_rank(2, nt, npr) for _ in range(3)]
    # entry 0: on rank 0 in the first sample, on rank 2 in the second; entry 1 stays on rank 1
    recs[0][0, 32:39] = _row(True, 10.0)
    recs[2][1, 32:39] = _row(True, 20.0)
    recs[1][:, 39:46] = [_row(True, 30.0), _row(True, 40.0)]
    # probe 0 on rank 2 (in the fluid), probe 1 on rank 0 (in empty space: count 0 is an owner's count)
    recs[2][:, 46:48] = [[101.5, 17.0], [99.25, 16.0]]
    recs[0][:, 48:50] = [[0.0, 0.0], [0.0, 0.0]]
    out = monitor_combine(recs, nt, npr)
    assert out.shape == (2, 32 + 6 * nt + 2 * npr)
    head, trk, prb = monitor_split(out, nt, npr)
    assert list(trk[0, 0]) == _row(True, 10.0)[1:] and list(trk[1, 0]) == _row(True, 20.0)[1:]
    assert list(trk[0, 1]) == _row(True, 30.0)[1:] and list(trk[1, 1]) == _row(True, 40.0)[1:]
    assert prb[:, 0].tolist() == [[101.5, 17.0], [99.25, 16.0]]
    assert prb[:, 1].tolist() == [[0.0, 0.0], [0.0, 0.0]]


def _combine_code(recs, nt, npr):
    with pytest.raises(MphError) as e:
        monitor_combine(recs, nt, npr)
    return e.value.code


def test_records_that_do_not_combine():
    def good():
        recs = [_empty_rank(2, 1, 1) for _ in range(3)]
        recs[1][:, 32:39] = _row(True, 5.0)
        recs[2][:, 39:41] = [3.5, 4.0]
        return recs
    assert monitor_combine(good(), 1, 1).shape == (2, 40)
    recs = good()
    recs[2][1, 32:39] = _row(True, 6.0)        # the tracked particle on two ranks
    assert _combine_code(recs, 1, 1) == -1
    recs = good()
    recs[1][0, 32:39] = 0.0                    # on none
    assert _combine_code(recs, 1, 1) == -1
    recs = good()
    recs[0][1, 39:41] = [0.0, 0.0]             # the probe owned twice
    assert _combine_code(recs, 1, 1) == -1
    recs = good()
    recs[2][:, 40] = -1.0                      # and by no rank
    assert _combine_code(recs, 1, 1) == -1
    recs = good()
    recs[1][1, S["STEP"]] += 1.0               # unequal STEP
    assert _combine_code(recs, 1, 1) == -1
    with pytest.raises(ValueError):
        monitor_combine([np.zeros((2, 40)), np.zeros((3, 40))], 1, 1)
