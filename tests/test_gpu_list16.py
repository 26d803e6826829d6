"""16-bit neighbour-list rows: a 3-D interior wave whose stencil groups'
candidates lie within 8191 indices of a wave-uniform base stores its list as rows of 64 uint16
(offset | type << 13) in the first half of its tile; every other wave keeps the 32-bit rows.  The
format changes no value a caller can read: every comparison here is bitwise, between a context
created with the default and one created with MPH_LIST16=0 (every wave wide), after mph_step(11)
-- one 8-step batch and three remainder steps, so lean, lazy and full steps all run.

The goldens' small boxes have qualifying interior waves (the counters are printed and asserted per
case): no larger case was needed.
"""
import numpy as np
import pytest

from parity import assert_same, snapshot
from particlemethod_fsi_amd import MphSolver, cases, mphio
from particlemethod_fsi_amd.solver import MphError

pytestmark = pytest.mark.gpu

STEPS = 11
SPAN = 200   # MPH_LIST16_SPAN of test_fallback_by_span: 143 of box3d_jit's 154 waves short at the creation


def run(cfg, parts, monkeypatch, steps=STEPS, **env):
    """One context created under `env`, stepped by one mph_step(steps): (snapshot, format counters)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        with MphSolver(cfg, parts) as s:
            if steps:
                s.step(steps)
            snap = snapshot(s)
            stats = s.list_format_stats()
    finally:
        for k in env:
            monkeypatch.delenv(k)
    return snap, stats


def compare(name, cfg, parts, monkeypatch, **env):
    wide, w = run(cfg, parts, monkeypatch, MPH_LIST16="0", **env)
    short, s = run(cfg, parts, monkeypatch, **env)
    print(name, "default", s, "MPH_LIST16=0", w)
    assert w["short_waves"] == 0 and w["restarted_waves"] == 0, w
    assert w["wide_waves"] == s["short_waves"] + s["wide_waves"] == (parts.n + 63) // 64
    assert_same(short, wide, name)
    return s


# box3d: on the lattice, plain rows; box3d_jit: off it, jumps and gaps; box3d_st: surface tension,
# pass B reads the entry's type; gate3d: structure particles
@pytest.mark.parametrize("case", ["box3d", "box3d_jit", "box3d_st", "gate3d"])
def test_short_rows_equal_wide_rows(case, monkeypatch):
    cfg, parts = cases.get(case).build()
    s = compare(case, cfg, parts, monkeypatch)
    assert s["short_waves"] > 0, s


def test_fallback_by_span(monkeypatch):
    """MPH_LIST16_SPAN (read at creation into DevParams.list16_span) lowered until box3d_jit's
    interior waves split between the formats: a wave's widest group span there is the seven cell
    rows of the group plus the wave's own extent, several hundred indices."""
    cfg, parts = cases.get("box3d_jit").build()
    _, full = run(cfg, parts, monkeypatch)
    s = compare("box3d_jit span %d" % SPAN, cfg, parts, monkeypatch, MPH_LIST16_SPAN=str(SPAN))
    # some of the waves that qualify at the default limit are short, some wide
    assert 0 < s["short_waves"] < full["short_waves"], (s, full)
    assert s["wide_waves"] > full["wide_waves"], (s, full)
    # every wave of this case is interior, so a wide wave is either a restarted one or one the limit
    # turned away, counted as a span miss; none is at the default limit
    assert full["span_miss_waves"] == 0 and s["span_miss_waves"] == s["wide_waves"] - s["restarted_waves"] > 0, (s, full)


def _cluster(extra):
    """The hub cluster of test_gpu_edge.py's test_exactly_512_neighbors_is_accepted, built again
    here: 511 particles of an 8 x 8 x 8 block at 0.18 dx (every pair within MaxRadius) and two hubs
    0.75 dx beyond its two x faces, so every block particle has exactly 512 neighbours, all of them
    stored entries; `extra` adds a particle at the block's centre (513).  The block's waves are
    interior and their group spans tiny, so they begin in the 16-bit format -- and pass kAlignRows
    rows long before their last group end."""
    c = cases.Case("cluster16", 3, "dam", 0.001, (0.0, 0.0, 0.0), (0.02, 0.02, 0.02), [])
    cfg, _ = c._config()
    s, a = 0.00018, 0.00075
    g = np.arange(8) * s
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:511] + 0.01
    yc = 0.01 + 3.5 * s
    hubs = [[0.01 - a, yc, yc], [0.01 + 7 * s + a, yc, yc], [0.01 + 3.5 * s, yc + 1e-6, yc]]
    pos = np.concatenate([pos, np.array(hubs[:2 + extra])])
    n = len(pos)
    return cfg, mphio.Particles(np.ones(n, np.int32), pos.copy(), pos.copy(), np.zeros((n, 3)))


def test_restart(monkeypatch):
    """A short wave whose highest row reaches kAlignRows at a group end starts over in the wide
    format inside the same launch: counted, equal to the MPH_LIST16=0 run in every field, and
    NeighborCount equal to the oracle's.  With one neighbour more the creation reports
    MPH_ERR_NEIGHBOR_OVERFLOW, as with the wide rows."""
    from oracle_bindings import OracleSolver
    cfg, parts = _cluster(0)
    o = OracleSolver(cfg, parts)
    o.init()
    wide, w = run(cfg, parts, monkeypatch, steps=1, MPH_LIST16="0")
    short, s = run(cfg, parts, monkeypatch, steps=1)
    print("cluster", s, w)
    assert w["short_waves"] == 0 and w["restarted_waves"] == 0, w
    assert s["restarted_waves"] >= 1, s
    assert_same(short, wide, "cluster")
    o.step(1)
    assert np.array_equal(short["NeighborCount"], o.get("NeighborCount"))
    # the initial search (the creation's) restarts too
    _, s0 = run(cfg, parts, monkeypatch, steps=0)
    assert s0["restarted_waves"] >= 1, s0
    cfg, parts = _cluster(1)
    with pytest.raises(MphError) as e:
        MphSolver(cfg, parts)
    assert e.value.code == -3


def test_2d_is_untouched(monkeypatch):
    cfg, parts = cases.get("dam2d").build()
    s = compare("dam2d", cfg, parts, monkeypatch)
    assert s["short_waves"] == 0 and s["restarted_waves"] == 0, s
