"""rv_gi_relight_box (host only): the GI-cell box to relight after an edit -- the
bounding box of the edit boxes' voxels in GI cells (cell = voxel >> 2), grown by a
margin per axis and clipped to the grid -- against a numpy restatement."""
import numpy as np
import pytest

from gpu_world import rv

WORLDS = [(7, 7, 7), (8, 6, 7), (4, 4, 4)]
MARGINS = [0, 1, 5, 1000]   # 1000 cells: larger than every grid here


def restated(lg, boxes, margin):
    if not boxes:
        return (0,) * 6
    b = np.asarray(boxes, np.int64)
    lo = b[:, 0:3].min(axis=0) // 4
    hi = (b[:, 3:6].max(axis=0) - 1) // 4 + 1
    G = np.array([1 << (l - 2) for l in lg], np.int64)
    lo = np.maximum(0, lo - margin)
    hi = np.minimum(G, hi + margin)
    return tuple(int(v) for v in lo) + tuple(int(v) for v in hi)


def box_lists(lg):
    X, Y, Z = (1 << l for l in lg)
    cx, cy, cz = X // 2, Y // 2, Z // 2
    out = {
        "one voxel": [(cx, cy, cz, cx + 1, cy + 1, cz + 1, 1)],
        "one voxel, last of its cell": [(cx + 3, cy + 3, cz + 3, cx + 4, cy + 4, cz + 4, 0)],
        "straddles cell boundaries": [(cx - 1, cy - 5, cz + 3, cx + 1, cy + 1, cz + 5, 1)],
        "ends on a cell boundary": [(cx - 4, cy - 4, cz - 4, cx, cy, cz, 1)],
        "several": [(1, 2, 3, 3, 5, 4, 1), (cx + 1, cy - 2, cz, cx + 6, cy + 3, cz + 2, 0), (X - 5, 0, 6, X - 2, 2, 9, 1)],
        "whole world": [(0, 0, 0, X, Y, Z, 0)],
    }
    # a box touching each world face
    for a in range(3):
        D = (X, Y, Z)
        lo = [cx - 1, cy - 1, cz - 1]
        hi = [cx + 2, cy + 2, cz + 2]
        lo[a], hi[a] = 0, 2
        out[f"face {a}-"] = [tuple(lo) + tuple(hi) + (1,)]
        lo[a], hi[a] = D[a] - 1, D[a]
        out[f"face {a}+"] = [tuple(lo) + tuple(hi) + (0,)]
    return out


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("lg", WORLDS)
def test_box_equals_the_restatement(rv, lg, margin):
    G = tuple(1 << (l - 2) for l in lg)
    for name, boxes in box_lists(lg).items():
        got = rv.relight_box(lg, boxes, margin)
        assert got == restated(lg, boxes, margin), (name, margin)
        assert all(0 <= got[a] < got[a + 3] <= G[a] for a in range(3)), (name, got)
        if margin == 1000:
            assert got == (0, 0, 0) + G, name   # clips to the whole grid


def test_known_boxes(rv):
    # voxels 37..45 -> cells 9..11, 30..51 -> 7..12, 21..27 -> 5..6
    assert rv.relight_box((7, 7, 7), [(37, 30, 21, 46, 52, 28, 1)], 0) == (9, 7, 5, 12, 13, 7)
    assert rv.relight_box((7, 7, 7), [(37, 30, 21, 46, 52, 28, 1)], 2) == (7, 5, 3, 14, 15, 9)
    # the one-block edit at the centre of a 1024^3 world with margin 16: 33^3 cells
    b = rv.relight_box((10, 10, 10), [(512, 512, 512, 513, 513, 513, 1)], 16)
    assert b == (112, 112, 112, 145, 145, 145)
    assert rv.relight_box((4, 4, 4), [(0, 0, 0, 1, 1, 1, 1)], 0) == (0, 0, 0, 1, 1, 1)
    assert rv.relight_box((4, 4, 4), [(15, 15, 15, 16, 16, 16, 1)], 1) == (2, 2, 2, 4, 4, 4)


@pytest.mark.parametrize("lg", WORLDS)
def test_no_boxes_gives_zeros(rv, lg):
    for margin in MARGINS:
        assert rv.relight_box(lg, [], margin) == (0,) * 6


def test_invalid_arguments_rejected(rv):
    lg = (7, 6, 8)
    X, Y, Z = 128, 64, 256
    bad = [(4, 4, 4, 4, 5, 5, 1), (4, 4, 4, 5, 4, 5, 1), (4, 4, 4, 5, 5, 3, 1),      # empty / reversed
           (-1, 0, 0, 1, 1, 1, 1), (0, -1, 0, 1, 1, 1, 0), (0, 0, -1, 1, 1, 1, 0),   # below the world
           (0, 0, 0, X + 1, 1, 1, 1), (0, 0, 0, 1, Y + 1, 1, 1), (0, 0, 0, 1, 1, Z + 1, 1),
           (0, 0, 0, 1, 1, 1, 2), (0, 0, 0, 1, 1, 1, -1)]                              # solid not 0 / 1
    good = (0, 0, 0, X, Y, Z, 1)
    assert rv.relight_box(lg, [good], 0) == (0, 0, 0, 32, 16, 64)
    for b in bad:   # exactly what rv_world_edit_region rejects
        with pytest.raises(rv.RvError):
            rv.edit_region(lg, [b])
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            rv.relight_box(lg, [b], 1)
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            rv.relight_box(lg, [good, b], 1)   # every box is validated
    with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
        rv.relight_box(lg, [good] * (rv._lib.RV_EDIT_MAX_BOXES + 1), 0)
    rv.relight_box(lg, [good] * rv._lib.RV_EDIT_MAX_BOXES, 0)
    for dims in ((3, 6, 6), (6, 14, 6), (12, 12, 12)):   # rv_create's limits
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            rv.relight_box(dims, [(0, 0, 0, 1, 1, 1, 1)], 0)
    for margin in (-1, -(2 ** 31)):
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            rv.relight_box(lg, [good], margin)
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            rv.relight_box(lg, [], margin)
    assert rv.relight_box(lg, [good], 2 ** 31 - 1) == (0, 0, 0, 32, 16, 64)
    L = rv._lib.load()
    out = rv._lib.rv_gi_box()
    assert L.rv_gi_relight_box(6, 6, 6, None, 1, 0, out) == rv._lib.RV_ERR_INVALID
    assert L.rv_gi_relight_box(6, 6, 6, None, 0, 0, None) == rv._lib.RV_ERR_INVALID
    assert L.rv_gi_relight(None, None, 0, 0, 0) == rv._lib.RV_ERR_INVALID
    assert L.rv_gi_relight_info(None, None, None, None) == rv._lib.RV_ERR_INVALID
