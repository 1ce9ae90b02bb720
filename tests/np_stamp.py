"""rv_world_stamp restated in numpy from the comment in include/rvgrt.h, not from the C: dense [z, y, x] bools,
np.flip and swapaxes for the orientation, slices for the clip.  A pattern is a bool array [z, y, x]; a stamp is
(pattern index, op, orient, (x, y, z))."""
import numpy as np

SET, CLEAR, COPY = range(3)
SWAP_XZ, FLIP_X, FLIP_Z = 1, 2, 4
MAX_DIM, MAX_PATTERNS, MAX_STAMPS, MAX_AT = 256, 256, 1024, 1 << 20
ZERO = (0,) * 6


def oriented(pat, orient):
    """The oriented pattern o[w, v, u] = pat[sz, v, sx]: with u' and w' the flipped u and w, (sx, sz) is (w', u')
    under SWAP_XZ and (u', w') without -- the swap comes last, so it is applied to the array first."""
    o = pat.swapaxes(0, 2) if orient & SWAP_XZ else pat      # o[w', v, u']
    if orient & FLIP_X:
        o = np.flip(o, 2)
    if orient & FLIP_Z:
        o = np.flip(o, 0)
    return o


def box(lg, pats, stamp):
    """The clipped box (x0, y0, z0, x1, y1, z1) of one stamp, all zero when empty.  pats: arrays or dims."""
    p = pats[stamp[0]]
    nx, ny, nz = p.shape[::-1] if isinstance(p, np.ndarray) else p
    o = (nz, ny, nx) if stamp[2] & SWAP_XZ else (nx, ny, nz)
    lo = [max(0, int(stamp[3][a])) for a in range(3)]
    hi = [min(1 << lg[a], int(stamp[3][a]) + o[a]) for a in range(3)]
    if any(h <= l for l, h in zip(lo, hi)):
        return ZERO
    return tuple(lo) + tuple(hi)


def boxes(lg, pats, stamps):
    """(each, all): every stamp's clipped box and their union (all zero when every box is empty)."""
    each = [box(lg, pats, s) for s in stamps]
    live = [b for b in each if b != ZERO]
    if not live:
        return each, ZERO
    return each, tuple(min(b[a] for b in live) for a in range(3)) + tuple(max(b[3 + a] for b in live) for a in range(3))


def apply(vox, pats, stamps):
    """(vox', n_set, n_cleared): the stamps in list order, a later one winning voxel by voxel; the counts compare
    the world before the call with the world after it."""
    out = vox.copy()
    lg = tuple(int(n).bit_length() - 1 for n in vox.shape[::-1])
    for s in stamps:
        b = box(lg, pats, s)
        if b == ZERO:
            continue
        o = oriented(pats[s[0]], s[2])
        ax, ay, az = (int(v) for v in s[3])
        m = o[b[2] - az:b[5] - az, b[1] - ay:b[4] - ay, b[0] - ax:b[3] - ax]
        dst = out[b[2]:b[5], b[1]:b[4], b[0]:b[3]]     # a view
        if s[1] == SET:
            dst[m] = True
        elif s[1] == CLEAR:
            dst[m] = False
        else:
            dst[...] = m
    return out, int((out & ~vox).sum()), int((vox & ~out).sum())


def move(vox, b, delta):
    """StateRender.world_move: the box's voxels cleared at the old place, the box copied to box + delta."""
    pat = vox[b[2]:b[5], b[1]:b[4], b[0]:b[3]].copy()
    at = tuple(b[:3])
    return apply(vox, [pat], [(0, CLEAR, 0, at), (0, COPY, 0, tuple(at[a] + int(delta[a]) for a in range(3)))])
