"""The inputs of test_gpu_list16_long.py, checked on the model alone (tests/list16_ref.py; no
library, no device): the conditions that keep the GPU tests from passing vacuously.  Every wave is
interior, the waves lie on both sides of the 8191 limit with waves exactly at 8191 and at 8192,
windows wider than the search's staging area occur both in the form the two-run split fits and in
the form it cannot, and entries of every type occur at offsets with bit 12 set (those of the floor's
type in the rotated form of cell order 2, see test_every_type_at_high_offsets).
"""
import numpy as np
import pytest

import list16_ref as ref


@pytest.fixture(scope="module")
def base():
    cfg, parts = ref.build()
    return cfg, parts, ref.model(cfg, parts, 0)


def test_constants():
    assert ref.SPAN_LIMIT == 8191 and ref.GROUPS == 7 and ref.K_REACH == 3 and ref.SA == 2
    # 176 FP64 candidates' staging holds 317 16-byte records, 3 of them past a window's end
    assert ref.CAP32 == 314


def test_geometry(base):
    cfg, parts, m = base
    assert parts.n == ref.N_PARTICLES and m.waves == 4430
    assert m.gc == (34, 56, 1399)
    assert sorted(np.unique(parts.property)) == [0, 1, 4, 5]
    # every particle at least reach + 1 cells from every face of the grid: every wave is interior
    assert m.interior.all()


def test_waves_on_both_sides_of_the_limit(base):
    _, _, m = base
    widest = m.widest
    print("waves", m.waves, "fit", int(m.fits().sum()), "widest span min/max", widest.min(), widest.max(),
          "at 8191:", int((widest == 8191).sum()), "at 8192:", int((widest == 8192).sum()))
    assert m.fits().sum() >= 0.25 * m.waves and (~m.fits()).sum() >= 0.25 * m.waves
    assert (widest == ref.SPAN_LIMIT).sum() >= 1 and (widest == ref.SPAN_LIMIT + 1).sum() >= 1
    assert (m.span >= 0).all()


def test_wide_windows_of_both_kinds(base):
    _, _, m = base
    fits = m.fits()
    unsplit = [w for w in m.unsplit if fits[w]]
    split = [w for w in m.wide if w not in set(m.unsplit.tolist())]
    print("windows >", ref.CAP32, ":", len(m.wide), "waves;", len(m.unsplit), "no split fits (", len(unsplit),
          "of them with every span <= 8191 );", len(split), "the split fits; widest window", int(m.window.max()))
    assert len(unsplit) >= 5
    assert len(split) >= 5


# Where the floor (type 4) is the lowest block along the middle axis of the cell order, its cell rows
# lead every group's index range that holds them, at most some 3,300 floor particles per column of
# cells: no floor entry can lie 4096 past a base.  In the cell orders whose middle axis runs across
# the strip (2 and 4) a group is seven cell rows of one level, and the floor's entries reach 5,800.
@pytest.mark.parametrize("perm,solid,want", [(0, False, {0, 1, 5}), (0, True, {0, 1, 2, 5}), (2, False, {1, 4})])
def test_every_type_at_high_offsets(base, perm, solid, want):
    if perm == 0 and not solid:
        cfg, parts, m = base
    else:
        cfg, parts = ref.build(axis=ref.perm_axis(perm), solid=solid)
        m = ref.model(cfg, parts, perm, windows=False)
    found = ref.high_offset_types(m, parts)
    print("perm", perm, "solid", solid, "types at offsets >= 4096:", sorted(found))
    assert found >= want


@pytest.mark.parametrize("perm", [1, 2, 3, 4])
def test_rotated_forms(base, perm):
    """The rotated forms hold the same particles with the long axis along the cell order's contiguous
    one: every wave interior, waves on both sides of the limit."""
    cfg, parts = ref.build(axis=ref.perm_axis(perm))
    m = ref.model(cfg, parts, perm, windows=False)
    assert np.array_equal(np.sort(parts.position, axis=1), np.sort(base[1].position, axis=1))
    assert m.interior.all() and max(m.gc) == 1399 and m.gc[ref.order_axis(perm, 2)] == 1399
    print("perm", perm, "grid", m.gc, "fit", int(m.fits().sum()), "of", m.waves)
    assert m.fits().sum() >= 0.1 * m.waves and (~m.fits()).sum() >= 0.1 * m.waves
