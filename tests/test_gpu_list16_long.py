"""The 16-bit list rows with long cell rows: offsets that use all 13 bits,
the span limit at 8191 / 8192, short waves that start over because a column's window does not fit
the search's staging area, the wide form's per-lane gather loop for such a window and the two-run
split of a window wider than the staging area.

The geometry and the plain model of the decision are tests/list16_ref.py's (283,500 particles,
4,430 waves; test_list16_long_model.py checks the model's side on the CPU: every wave interior,
waves on both sides of the limit and exactly at it, wide windows of both kinds, every type at
offsets >= 4096).  The device's decision is read wave by wave (mph_list_wave_formats) and compared
with the model's; the values are compared bit for bit with MPH_LIST16=0 (parity.assert_same) and
within the one tolerance table with the oracle (parity.check_fields_against_oracle), which shares
no search path with the device.

Measured on an MI355X (profiles/list16_long/README.md has the table).  Waves short / restarted /
span misses / most rows of one lane, at the creation and after mph_step(11); the model has 3,127
waves with every span <= 8191 (2,815 in cell orders 2 and 4), 12 of them with a window no split fits:
  fluid    3115 / 12 / 1303 / 115    3145 / 13 / 1272
  rotated  3115 / 12 / 1303 / 115    3146 / 13 / 1271
  solid    3115 / 12 / 1303 / 115    3144 / 12 / 1274
  st       3115 / 12 / 1303 / 115    3150 / 11 / 1269
  floor    2815 /  0 / 1615 / 120    2832 /  0 / 1598
Wall times: test_decision_matches_model 0.18 s per cell order (0.65 s the first, which builds the
particles), test_short_equals_wide 0.38 to 0.49 s per variant, test_against_oracle 1.1 s,
test_neighbor_sets_of_far_waves 1.0 s (2,709 particles of 12 restarted and 30 short waves).
"""
import functools

import numpy as np
import pytest

import list16_ref as ref
from parity import run_against_oracle_every_step
from particlemethod_fsi_amd import MphSolver, cases
from test_gpu_list16 import compare

pytestmark = pytest.mark.gpu

@functools.lru_cache(maxsize=None)
def _model(perm):
    cfg, parts = ref.build(axis=ref.perm_axis(perm))
    return ref.model(cfg, parts, perm)


def _formats(cfg, parts, monkeypatch, steps=0, **env):
    """One context created under `env`: (codes, bases) of mph_list_wave_formats, the format counters
    and mph_list_layout of the last search."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        with MphSolver(cfg, parts) as s:
            if steps:
                s.step(steps)
            codes, bases = s.list_wave_formats()
            return codes, bases, s.list_format_stats(), s.list_layout()
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _check_decision(m, codes, bases, stats, limit, context):
    fits = m.fits(limit)
    assert len(codes) == m.waves
    assert not (codes == 0).any(), (context, "undecided", np.nonzero(codes == 0)[0][:10])
    decided_short = (codes == 1) | (codes == 2)
    assert np.array_equal(decided_short, fits), (context, "short or restarted where every span <= limit",
                                                np.nonzero(decided_short != fits)[0][:10])
    assert np.array_equal(codes == 3, ~fits), (context, "span miss", np.nonzero((codes == 3) == fits)[0][:10])
    short = codes == 1
    assert np.array_equal(bases[short], m.base[short]), (context, "bases")
    assert not bases[~short].any(), (context, "bases of a wave without 16-bit rows")
    # a wave starts over only for a window wider than the staging area (the rows stay below
    # kAlignRows here); trimming only narrows a window, so the model's untrimmed ones bound them
    assert np.isin(np.nonzero(codes == 2)[0], m.wide).all(), (context, "restarted", np.nonzero(codes == 2)[0])
    assert stats == {"short_waves": int(short.sum()), "wide_waves": int((~short).sum()),
                     "restarted_waves": int((codes == 2).sum()), "span_miss_waves": int((codes == 3).sum())}, (context, stats)


@pytest.mark.parametrize("perm", [0, 1, 2, 3, 4])
def test_decision_matches_model(perm, monkeypatch):
    """The creation's search in every cell order, the long axis along the order's contiguous one:
    each wave's format code and the seven bases of each short wave equal the model's, at the
    default limit, at a limit S that is some wave's widest span and at S - 1 (exactly the waves
    whose widest span is S change sides), and at 4095."""
    m = _model(perm)
    cfg, parts = ref.build(axis=ref.perm_axis(perm))
    widest = m.widest
    # S: a widest span that occurs, the one nearest to three quarters of the limit
    vals = np.unique(widest[(widest > 4096) & (widest < ref.SPAN_LIMIT)])
    S = int(vals[np.argmin(np.abs(vals - 6144))])
    got = {}
    for limit in (None, S, S - 1, 4095):
        env = {"MPH_SLAB_PERM": str(perm)}
        if limit is not None:
            env["MPH_LIST16_SPAN"] = str(limit)
        codes, bases, stats, layout = _formats(cfg, parts, monkeypatch, **env)
        print("perm", perm, "limit", limit, stats, "model fits", int(m.fits(limit or ref.SPAN_LIMIT).sum()),
              "max rows", layout["max_rows"])
        assert layout["waves"] == m.waves and layout["max_rows"] < 128
        _check_decision(m, codes, bases, stats, limit or ref.SPAN_LIMIT, (perm, limit))
        got[limit] = codes
    moved = np.nonzero((got[S] == 3) != (got[S - 1] == 3))[0]
    assert len(moved) >= 1 and np.array_equal(moved, np.nonzero(widest == S)[0]), (S, moved)
    assert (got[S - 1][moved] == 3).all()
    if perm == 0:
        # the waves at the limit itself: 8191 stays, 8192 is turned away
        at, past = widest == ref.SPAN_LIMIT, widest == ref.SPAN_LIMIT + 1
        assert at.any() and past.any()
        assert (got[None][at] != 3).all() and (got[None][past] == 3).all()


# rotated: another cell order with the same rows; solid: type bit 14 with high offsets; st: pass B
# reads the entry's type.  floor: cell order 2, whose groups are seven cell rows of one level -- the one
# form in which the floor's entries (type 4) lie 4096 and more past their base; none of its short
# waves has a window that no split fits (test_list16_long_model.py), so no restart is asked of it.
VARIANTS = {
    "fluid": dict(perm=0),
    "rotated": dict(perm=1),
    "solid": dict(perm=0, solid=True),
    "st": dict(perm=0, data_changes=cases._ST),
    "floor": dict(perm=2, restarts=False),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_short_equals_wide(variant, monkeypatch):
    """Every field and both virial fields after mph_step(11), bit for bit equal to MPH_LIST16=0, with
    all three kinds of waves present: short, turned away by the limit, restarted.  No lane has 128
    rows, so the restarts are the window ones -- and in the MPH_LIST16=0 run those waves, and the
    span misses with such a window, took the wide form's gather loop or its two-run split."""
    v = dict(VARIANTS[variant])
    perm, restarts = v.pop("perm"), v.pop("restarts", True)
    m = _model(perm)
    cfg, parts = ref.build(axis=ref.perm_axis(perm), **v)
    env = {"MPH_SLAB_PERM": str(perm)}
    if variant == "solid":
        assert (parts.property == 2).sum() == 58000
    s = compare("list16_long " + variant, cfg, parts, monkeypatch, **env)
    assert s["short_waves"] > 0 and s["span_miss_waves"] > 0 and s["restarted_waves"] >= restarts, s
    # the creation's search, whose positions are the model's: wave by wave
    codes, bases, stats, layout = _formats(cfg, parts, monkeypatch, **env)
    print(variant, "creation", stats, layout)
    assert layout["max_rows"] < 128, layout
    _check_decision(m, codes, bases, stats, ref.SPAN_LIMIT, variant)
    assert stats["restarted_waves"] >= restarts, stats
    # and after the steps (the particles have moved by less than 1e-3 dx): the same layout bound
    codes, bases, stats, layout = _formats(cfg, parts, monkeypatch, steps=11, **env)
    assert layout["max_rows"] < 128, layout
    assert stats == s, (stats, s)


def test_against_oracle():
    """Two steps of the fluid / walls form against the oracle, every field after every step and the
    virial after the last: a reference that shares neither format nor the wide path."""
    from oracle_bindings import use_oracle_threads
    use_oracle_threads()
    cfg, parts = ref.build()
    run_against_oracle_every_step(cfg, parts, 2)


def test_neighbor_sets_of_far_waves(monkeypatch):
    """The neighbour sets themselves (mph_neighbor_rows, MPH_LIST_FULL=1) after one step against the
    oracle's lists, as sorted original indices: NeighborCount of every particle, and the rows of
    every particle in a cell of a restarted wave and of up to 30 short waves whose widest span
    exceeds 4096 -- the waves at exactly 8191 among them."""
    from oracle_bindings import OracleSolver, use_oracle_threads
    use_oracle_threads()
    monkeypatch.setenv("MPH_LIST_FULL", "1")
    m = _model(0)
    cfg, parts = ref.build()
    o = OracleSolver(cfg, parts)
    o.init()
    o.step(1)
    with MphSolver(cfg, parts) as s:
        s.step(1)
        codes, _ = s.list_wave_formats()
        counts, offsets, ids = s.neighbor_rows()
    assert np.array_equal(counts, o.get("NeighborCount"))
    restarted = np.nonzero(codes == 2)[0]
    assert len(restarted) >= 1
    far = np.nonzero((codes == 1) & (m.widest > 4096))[0]
    at = far[m.widest[far] == ref.SPAN_LIMIT]
    assert len(far) >= 30 and len(at) >= 1
    pick = np.unique(np.concatenate([at, far[np.linspace(0, len(far) - 1, 30 - len(at)).astype(int)]]))
    rows = np.unique(np.concatenate([m.wave_cells_particles(w) for w in np.concatenate([restarted, pick])]))
    print("restarted", len(restarted), "short far waves", len(pick), "particles", len(rows))
    for i in rows:
        assert np.array_equal(ids[offsets[i]:offsets[i + 1]], np.sort(o.neighbors(int(i)))), i
