"""Host-side mirror of the reference's StateRender interface over the C ABI.

Reference: class StateRender (include/StateRender.cuh:11-47), its
drawCUDA (src/StateRender.cu:289-346), CoarseArray::InitializeGIData /
UpdateGIData (src/CoarseArray.cu:357-395) and the init sequence of
State::Create (src/State.cpp:24-56).  Every method forwards to
librvgrt_hip.so; errors raise RvError with rv_last_error().
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import (RvError, rv_camera, rv_config, rv_edit_box, rv_edit_shape, rv_frame_desc, rv_gi_box, rv_hit,
                   rv_stats, rv_voxel_box)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def camera_from_pose(pos, yaw, pitch, width, height):
    """Character::Update basis + unjittered VP (src/Character.cpp:18-126)."""
    L = _lib.load()
    cam = rv_camera()
    vp = np.zeros(16, np.float32)
    st = L.rv_camera_from_pose(float(pos[0]), float(pos[1]), float(pos[2]), float(yaw),
                               float(pitch), int(width), int(height), C.byref(cam), _ptr(vp))
    if st != 0:
        raise RvError(f"rv_camera_from_pose: {_lib.STATUS_NAMES.get(st, st)}")
    return cam, vp


def frame_desc(cam: rv_camera, vp, prev_vp=None, time=0.0, jx=0.0, jy=0.0) -> rv_frame_desc:
    """One frame's inputs (rv_frame_desc): camera, unjittered VP and the
    previous frame's, effective time and jitter."""
    d = rv_frame_desc()
    d.cam = cam
    vp = np.ascontiguousarray(vp, np.float32)
    pvp = vp if prev_vp is None else np.ascontiguousarray(prev_vp, np.float32)
    for i in range(16):
        d.vp[i] = float(vp[i])
        d.prev_vp[i] = float(pvp[i])
    d.time, d.jitter_x, d.jitter_y = float(time), float(jx), float(jy)
    return d


def camera_dict(cam: rv_camera, vp):
    return {"pos": np.array(cam.pos[:], np.float32), "fo": np.array(cam.forward[:], np.float32),
            "ri": np.array(cam.right[:], np.float32), "up": np.array(cam.up[:], np.float32),
            "vp": np.asarray(vp, np.float32)}


def _edit_boxes(boxes):
    """ctypes array of rv_edit_box from tuples (x0, y0, z0, x1, y1, z1, solid)."""
    arr = (rv_edit_box * max(len(boxes), 1))()
    for i, b in enumerate(boxes):
        if len(b) != 7:
            raise ValueError("an edit box is (x0, y0, z0, x1, y1, z1, solid)")
        arr[i] = rv_edit_box(*(int(v) for v in b))
    return arr


def edit_region(log2_dims, boxes):
    """rv_world_edit_region (host only): the coarse-cell box (cx0, cx1, cy0, cy1,
    cz0, cz1) whose CSDF bytes world_edit(boxes) recomputes locally in a world
    of these log2 dims, and its volume."""
    L = _lib.load()
    boxes = list(boxes)
    region = (C.c_int32 * 6)()
    cells = C.c_uint64()
    st = L.rv_world_edit_region(int(log2_dims[0]), int(log2_dims[1]), int(log2_dims[2]), _edit_boxes(boxes),
                                len(boxes), region, C.byref(cells))
    if st != 0:
        raise RvError(f"rv_world_edit_region: {_lib.STATUS_NAMES.get(st, st)}")
    return tuple(region), int(cells.value)


def _edit_shapes(shapes):
    """ctypes array of rv_edit_shape from tuples (kind, solid, c2, r2), c2 and r2 being three half-voxel
    values each."""
    arr = (rv_edit_shape * max(len(shapes), 1))()
    for i, s in enumerate(shapes):
        if len(s) != 4 or len(s[2]) != 3 or len(s[3]) != 3:
            raise ValueError("an edit shape is (kind, solid, (cx2, cy2, cz2), (rx2, ry2, rz2))")
        arr[i] = rv_edit_shape(int(s[0]), int(s[1]), (C.c_int32 * 3)(*(int(v) for v in s[2])),
                               (C.c_int32 * 3)(*(int(v) for v in s[3])))
    return arr


def edit_shapes_at(log2_dims, bits, shapes):
    """rv_world_edit_shapes_at (host only): StateRender.world_edit_shapes evaluated on the CPU by the
    row function the kernel calls, over a copy of `bits` (RV_WORLD_BITS layout, log2_x >= 5).  Returns
    (bits_after, n_set, n_cleared)."""
    L = _lib.load()
    out = np.array(bits, np.uint32, copy=True).reshape(-1)
    if out.size != (1 << sum(int(v) for v in log2_dims)) // 32:
        raise ValueError("bits does not match log2_dims")
    shapes = list(shapes)
    lg = [int(v) for v in log2_dims]
    a, b = C.c_uint64(), C.c_uint64()
    st = L.rv_world_edit_shapes_at(lg[0], lg[1], lg[2], _ptr(out), _edit_shapes(shapes), len(shapes), C.byref(a),
                                   C.byref(b))
    if st != 0:
        raise RvError(f"rv_world_edit_shapes_at: {_lib.STATUS_NAMES.get(st, st)}")
    return out, int(a.value), int(b.value)


def edit_shapes_box(log2_dims, shapes):
    """rv_world_edit_shapes_box (host only): (each, all) -- the clipped voxel box (x0, y0, z0, x1, y1,
    z1) of every shape in a world of these log2 dims (all zero for an empty one) and their union."""
    L = _lib.load()
    shapes = list(shapes)
    lg = [int(v) for v in log2_dims]
    each = (rv_voxel_box * max(len(shapes), 1))()
    u = rv_voxel_box()
    st = L.rv_world_edit_shapes_box(lg[0], lg[1], lg[2], _edit_shapes(shapes), len(shapes), each, C.byref(u))
    if st != 0:
        raise RvError(f"rv_world_edit_shapes_box: {_lib.STATUS_NAMES.get(st, st)}")
    return [_box_tuple(each[i]) for i in range(len(shapes))], _box_tuple(u)


def settle_parts(box, dims, cap=_lib.RV_DETACHED_MAX_VOXELS):
    """The voxel boxes world_blast settles after clearing a shape whose clipped box is `box` in a window
    of `dims` voxels: the box grown by 1 voxel per side and clipped to the window, halved along its
    longest axis (the lower half getting the smaller share of an odd length) until no part holds more
    than `cap` voxels, which is what rv_world_detached and rv_world_fall take.  The parts tile the grown
    box without overlap.  Settling in parts is not settling the whole: each part is judged on its own,
    and whatever reaches solid matter beyond a part stays, so a loose piece that straddles a cut holds
    itself up from the other side and does not fall.  An empty box gives no parts."""
    if _box_volume(_voxel_box(box)) == 0:
        return []
    parts = [tuple(max(int(box[a]) - 1, 0) for a in range(3)) +
             tuple(min(int(box[3 + a]) + 1, int(dims[a])) for a in range(3))]
    while any(_box_volume(_voxel_box(p)) > cap for p in parts):
        nxt = []
        for p in parts:
            if _box_volume(_voxel_box(p)) <= cap:
                nxt.append(p)
                continue
            a = max(range(3), key=lambda k: p[3 + k] - p[k])
            mid = (p[a] + p[3 + a]) // 2
            nxt.append(p[:3 + a] + (mid,) + p[4 + a:])
            nxt.append(p[:a] + (mid,) + p[a + 1:])
        parts = nxt
    return parts


def relight_box(log2_dims, boxes, margin=0):
    """rv_gi_relight_box (host only): the GI-cell box (x0, y0, z0, x1, y1, z1) around
    the edit boxes' voxels, grown by `margin` cells per axis and clipped to the
    grid of a world of these log2 dims -- what to hand to gi_relight after
    world_edit(boxes)."""
    L = _lib.load()
    boxes = list(boxes)
    out = rv_gi_box()
    st = L.rv_gi_relight_box(int(log2_dims[0]), int(log2_dims[1]), int(log2_dims[2]), _edit_boxes(boxes),
                             len(boxes), int(margin), C.byref(out))
    if st != 0:
        raise RvError(f"rv_gi_relight_box: {_lib.STATUS_NAMES.get(st, st)}")
    return (out.x0, out.y0, out.z0, out.x1, out.y1, out.z1)


def scroll_region(log2_dims, axis, d):
    """rv_world_scroll_region (host only): (trailing, leading, cells, full) for a
    one-axis scroll by d voxels (axis 0 = x, 2 = z) of a world of these log2
    dims -- the two coarse-cell boxes (cx0, cx1, cy0, cy1, cz0, cz1) whose CSDF
    bytes world_scroll recomputes, their volume, and whether it runs the
    whole-grid build instead (then trailing is the whole grid, leading empty)."""
    L = _lib.load()
    region = (C.c_int32 * 12)()
    cells, full = C.c_uint64(), C.c_int32()
    st = L.rv_world_scroll_region(int(log2_dims[0]), int(log2_dims[1]), int(log2_dims[2]), int(axis), int(d),
                                  region, C.byref(cells), C.byref(full))
    if st != 0:
        raise RvError(f"rv_world_scroll_region: {_lib.STATUS_NAMES.get(st, st)}")
    return tuple(region[:6]), tuple(region[6:]), int(cells.value), bool(full.value)


def scroll_view(dx, dz, cam: rv_camera = None, vp=None, prev_vp=None):
    """rv_scroll_view (host only): (cam, vp, prev_vp) re-expressed in the grid after
    world_scroll(dx, dz) -- copies; the arguments are left alone, None stays None."""
    L = _lib.load()
    c2 = None
    if cam is not None:
        c2 = rv_camera()
        C.memmove(C.byref(c2), C.byref(cam), C.sizeof(rv_camera))
    m = [None if a is None else np.array(a, np.float32).reshape(16) for a in (vp, prev_vp)]
    st = L.rv_scroll_view(int(dx), int(dz), None if c2 is None else C.byref(c2),
                          *[None if a is None else _ptr(a) for a in m])
    if st != 0:
        raise RvError(f"rv_scroll_view: {_lib.STATUS_NAMES.get(st, st)}")
    return c2, m[0], m[1]


def persist_column_map(log2_dims, bx, bz):
    """rv_persist_column_map (host only): for each of the 2 Y words of brick column
    (bx, bz)'s column bits in a world of these log2 dims, the dword index into the
    brick array that the persistence kernels read or write."""
    L = _lib.load()
    out = np.zeros(2 << int(log2_dims[1]), np.uint32)
    st = L.rv_persist_column_map(int(log2_dims[0]), int(log2_dims[1]), int(log2_dims[2]), int(bx), int(bz), _ptr(out))
    if st != 0:
        raise RvError(f"rv_persist_column_map: {_lib.STATUS_NAMES.get(st, st)}")
    return out


def texture_tile_at(ox, oz, pos):
    """rv_texture_tile_at (host only): sampleTexture's atlas tile, a uint8 0xYX per
    position (n, 3) float32, evaluated on the CPU from the noise at texture origin
    (ox, oz) -- the function the kernels call."""
    L = _lib.load()
    p = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    out = np.zeros(len(p), np.uint8)
    st = L.rv_texture_tile_at(int(ox), int(oz), _ptr(p), len(p), _ptr(out))
    if st != 0:
        raise RvError(f"rv_texture_tile_at: {_lib.STATUS_NAMES.get(st, st)}")
    return out


def _bodies(lo, size, delta):
    """(n, 9) float32 rows lo | size | delta: an array of rv_body.  size and delta broadcast."""
    lo = np.asarray(lo, np.float32).reshape(-1, 3)
    b = np.empty((len(lo), 9), np.float32)
    b[:, 0:3] = lo
    b[:, 3:6] = np.asarray(size, np.float32)
    b[:, 6:9] = np.asarray(delta, np.float32)
    return b


def _bodies_out(out):
    """An array of rv_body_out as (lo (n, 3) float32, flags (n,) uint32)."""
    return np.ascontiguousarray(out[:, :3]).view(np.float32), out[:, 3].copy()


def bodies_move_at(log2_dims, bits, lo, size, delta, flags=0):
    """rv_world_bodies_move_at (host only): the swept box collision the kernel evaluates,
    on the CPU over `bits` (RV_WORLD_BITS layout, log2_x >= 5).  Returns (lo, flags)."""
    L = _lib.load()
    bits = np.ascontiguousarray(bits, np.uint32)
    if bits.size != (1 << sum(int(v) for v in log2_dims)) // 32:
        raise ValueError("bits does not match log2_dims")
    b = _bodies(lo, size, delta)
    out = np.zeros((len(b), 4), np.uint32)
    st = L.rv_world_bodies_move_at(int(log2_dims[0]), int(log2_dims[1]), int(log2_dims[2]), _ptr(bits), _ptr(b),
                                   len(b), int(flags), _ptr(out))
    if st != 0:
        raise RvError(f"rv_world_bodies_move_at: {_lib.STATUS_NAMES.get(st, st)}")
    return _bodies_out(out)


# an array of rv_component
COMPONENT_DTYPE = np.dtype([("lo", np.int32, 3), ("hi", np.int32, 3), ("seed", np.int32, 3), ("voxels", np.uint32)])


def _voxel_box(box):
    if len(box) != 6:
        raise ValueError("a voxel box is (x0, y0, z0, x1, y1, z1)")
    return rv_voxel_box(*(int(v) for v in box))


def _box_volume(b):
    return max(b.x1 - b.x0, 0) * max(b.y1 - b.y0, 0) * max(b.z1 - b.z0, 0)


def detached_at(log2_dims, bits, box, cap=None, want_mask=True):
    """rv_world_detached_at (host only): the query of StateRender.world_detached evaluated on the
    CPU over `bits` (RV_WORLD_BITS layout, log2_x >= 5) by the functions the kernels call.  Returns
    (components, n_comps, n_voxels, mask) like it; cap None = every component."""
    L = _lib.load()
    bits = np.ascontiguousarray(bits, np.uint32)
    if bits.size != (1 << sum(int(v) for v in log2_dims)) // 32:
        raise ValueError("bits does not match log2_dims")
    b = _voxel_box(box)
    lg = [int(v) for v in log2_dims]
    if cap is None:
        cap = (_box_volume(b) + 1) // 2
    comps = np.zeros(max(int(cap), 1), COMPONENT_DTYPE)
    mask = np.zeros(max((_box_volume(b) + 31) // 32, 1), np.uint32) if want_mask else None
    n, v = C.c_int64(), C.c_uint64()
    st = L.rv_world_detached_at(lg[0], lg[1], lg[2], _ptr(bits), C.byref(b), _ptr(comps) if cap else None, int(cap),
                                C.byref(n), C.byref(v), None if mask is None else _ptr(mask),
                                0 if mask is None else mask.nbytes)
    if st != 0:
        raise RvError(f"rv_world_detached_at: {_lib.STATUS_NAMES.get(st, st)}")
    return comps[:min(int(cap), int(n.value))].copy(), int(n.value), int(v.value), mask


# an array of rv_fallen
FALLEN_DTYPE = np.dtype([("comp", COMPONENT_DTYPE), ("fall", np.int32), ("flags", np.uint32)])


def _box_tuple(b):
    return (b.x0, b.y0, b.z0, b.x1, b.y1, b.z1)


def fall_at(log2_dims, bits, box, max_fall=0, cap=None, want_bits=True, in_place=False):
    """rv_world_fall_at (host only): the move of StateRender.world_fall evaluated on the CPU over
    `bits` (RV_WORLD_BITS layout, log2_x >= 5) by the functions the kernels call.  Returns
    (components, n_comps, n_voxels, changed, bits_out): FALLEN_DTYPE records (cap None = every
    component), the totals, the changed voxel box as a tuple and the world after the move (None
    unless want_bits; in_place writes it over `bits`, which must then be a contiguous uint32 array)."""
    L = _lib.load()
    src = np.ascontiguousarray(bits, np.uint32)
    if src.size != (1 << sum(int(v) for v in log2_dims)) // 32:
        raise ValueError("bits does not match log2_dims")
    if in_place and src is not bits:
        raise ValueError("in_place needs a contiguous uint32 array")
    b = _voxel_box(box)
    lg = [int(v) for v in log2_dims]
    if cap is None:
        cap = (_box_volume(b) + 1) // 2
    comps = np.zeros(max(int(cap), 1), FALLEN_DTYPE)
    out = src if in_place else (np.zeros_like(src) if want_bits else None)
    n, v, ch = C.c_int64(), C.c_uint64(), rv_voxel_box()
    st = L.rv_world_fall_at(lg[0], lg[1], lg[2], _ptr(src), C.byref(b), int(max_fall), _ptr(comps) if cap else None,
                            int(cap), C.byref(n), C.byref(v), C.byref(ch), None if out is None else _ptr(out),
                            0 if out is None else out.nbytes)
    if st != 0:
        raise RvError(f"rv_world_fall_at: {_lib.STATUS_NAMES.get(st, st)}")
    return comps[:min(int(cap), int(n.value))].copy(), int(n.value), int(v.value), _box_tuple(ch), out


def pattern_bits(vox):
    """A pattern in the ABI's layout from a bool array vox[z, y, x]: (dims (nx, ny, nz), uint32 words), rows
    along x padded to 32-bit words, voxel (x, y, z) being bit x & 31 of word (x >> 5) + nwx * (y + ny * z)."""
    vox = np.asarray(vox, bool)
    if vox.ndim != 3 or 0 in vox.shape:
        raise ValueError("a pattern is a non-empty bool array [z, y, x]")
    nz, ny, nx = vox.shape
    padded = np.zeros((nz, ny, 32 * ((nx + 31) // 32)), bool)
    padded[:, :, :nx] = vox
    return (nx, ny, nz), np.packbits(padded.ravel(), bitorder="little").view(np.uint32)


def pattern_voxels(dims, words):
    """The inverse of pattern_bits: the bool array [z, y, x] of a pattern of dims (nx, ny, nz)."""
    nx, ny, nz = (int(v) for v in dims)
    nwx = (nx + 31) // 32
    w = np.ascontiguousarray(words, np.uint32)[:nwx * ny * nz]
    return np.unpackbits(w.view(np.uint8), bitorder="little").reshape(nz, ny, 32 * nwx)[:, :, :nx].astype(bool)


def _stamps(stamps):
    """ctypes array of rv_stamp from tuples (pattern, op, orient, (x, y, z))."""
    arr = (_lib.rv_stamp * max(len(stamps), 1))()
    for i, s in enumerate(stamps):
        if len(s) != 4 or len(s[3]) != 3:
            raise ValueError("a stamp is (pattern, op, orient, (x, y, z))")
        arr[i] = _lib.rv_stamp(int(s[0]), int(s[1]), int(s[2]), (C.c_int32 * 3)(*(int(v) for v in s[3])))
    return arr


def _patterns_host(patterns, need_bits):
    """ctypes array of rv_pattern_host from bool arrays [z, y, x] (or, where only boxes are wanted, dims
    (nx, ny, nz)); the second value keeps the words alive."""
    arr = (_lib.rv_pattern_host * max(len(patterns), 1))()
    keep = []
    for i, p in enumerate(patterns):
        if need_bits or isinstance(p, np.ndarray):
            (nx, ny, nz), words = pattern_bits(p)
            keep.append(words)
            arr[i] = _lib.rv_pattern_host(nx, ny, nz, words.ctypes.data)
        else:
            arr[i] = _lib.rv_pattern_host(int(p[0]), int(p[1]), int(p[2]), None)
    return arr, keep


def stamp_at(log2_dims, bits, patterns, stamps):
    """rv_world_stamp_at (host only): StateRender.world_stamp evaluated on the CPU by the row function the
    kernel calls, over a copy of `bits` (RV_WORLD_BITS layout, log2_x >= 5).  patterns: bool arrays
    [z, y, x] that stamp.pattern indexes.  Returns (bits_after, n_set, n_cleared)."""
    L = _lib.load()
    out = np.array(bits, np.uint32, copy=True).reshape(-1)
    if out.size != (1 << sum(int(v) for v in log2_dims)) // 32:
        raise ValueError("bits does not match log2_dims")
    stamps, patterns = list(stamps), list(patterns)
    lg = [int(v) for v in log2_dims]
    pats, keep = _patterns_host(patterns, True)
    a, b = C.c_uint64(), C.c_uint64()
    st = L.rv_world_stamp_at(lg[0], lg[1], lg[2], _ptr(out), pats, len(patterns), _stamps(stamps), len(stamps),
                             C.byref(a), C.byref(b))
    if st != 0:
        raise RvError(f"rv_world_stamp_at: {_lib.STATUS_NAMES.get(st, st)}")
    return out, int(a.value), int(b.value)


def stamp_box(log2_dims, patterns, stamps):
    """rv_world_stamp_box (host only): (each, all) -- the clipped voxel box (x0, y0, z0, x1, y1, z1) of every
    stamp in a world of these log2 dims (all zero for an empty one) and their union, world_stamp's
    `changed`.  patterns: bool arrays [z, y, x] or dims (nx, ny, nz)."""
    L = _lib.load()
    stamps, patterns = list(stamps), list(patterns)
    lg = [int(v) for v in log2_dims]
    pats, keep = _patterns_host(patterns, False)
    each = (rv_voxel_box * max(len(stamps), 1))()
    u = rv_voxel_box()
    st = L.rv_world_stamp_box(lg[0], lg[1], lg[2], pats, len(patterns), _stamps(stamps), len(stamps), each, C.byref(u))
    if st != 0:
        raise RvError(f"rv_world_stamp_box: {_lib.STATUS_NAMES.get(st, st)}")
    return [_box_tuple(each[i]) for i in range(len(stamps))], _box_tuple(u)


def rccl_path():
    """The RCCL of the HIP runtime this process uses: torch's bundled librccl
    when torch is already imported (the library then shares torch's runtime),
    else None (the library loads the system librccl.so.1 next to the system
    HIP runtime it was linked with)."""
    import sys
    torch = sys.modules.get("torch")
    if torch is None:
        return None
    p = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
    return p if os.path.exists(p) else None


class Comm:
    """RCCL communicator of one rank (rv_comm_*): rank 0 makes the unique id,
    the caller broadcasts its 128 bytes, every rank creates its side."""

    ID_BYTES = 128

    @staticmethod
    def unique_id(path=None) -> bytes:
        L = _lib.load()
        buf = (C.c_ubyte * Comm.ID_BYTES)()
        p = path if path is not None else rccl_path()
        st = L.rv_comm_unique_id(p.encode() if p else None, C.cast(buf, C.c_void_p), Comm.ID_BYTES)
        if st != 0:
            raise RvError(f"rv_comm_unique_id: {_lib.STATUS_NAMES.get(st, st)}")
        return bytes(buf)

    def __init__(self, render: "StateRender", uid: bytes, nranks: int, rank: int, path=None):
        self._L = _lib.load()
        buf = (C.c_ubyte * Comm.ID_BYTES).from_buffer_copy(uid)
        h = C.c_void_p()
        p = path if path is not None else rccl_path()
        render._check(self._L.rv_comm_create(render._h, p.encode() if p else None, C.cast(buf, C.c_void_p),
                                             Comm.ID_BYTES, int(nranks), int(rank), C.byref(h)), "rv_comm_create")
        self._h = h
        self.rank, self.nranks = int(rank), int(nranks)

    @classmethod
    def loopback(cls, render: "StateRender", group: "LoopbackGroup", rank: int):
        """Rank `rank` of an in-process loopback group (rv_comm_create_loopback)."""
        self = cls.__new__(cls)
        self._L = _lib.load()
        h = C.c_void_p()
        render._check(self._L.rv_comm_create_loopback(render._h, group._h, group.nranks, int(rank), C.byref(h)),
                      "rv_comm_create_loopback")
        self._h = h
        self.rank, self.nranks = int(rank), group.nranks
        return self

    def wait(self, timeout_ms=0):
        """rv_comm_wait: bounded wait for this rank's loop; raises on a stalled peer."""
        st = self._L.rv_comm_wait(self._h, int(timeout_ms))
        if st != 0:
            raise RvError(f"rv_comm_wait: {_lib.STATUS_NAMES.get(st, st)}")

    def close(self):
        if getattr(self, "_h", None):
            self._L.rv_comm_destroy(self._h)
            self._h = None


class LoopbackGroup:
    """N in-process ranks on one GPU (rv_loopback_group_create)."""

    def __init__(self, nranks, timeout_ms=0):
        self._L = _lib.load()
        h = C.c_void_p()
        st = self._L.rv_loopback_group_create(int(nranks), int(timeout_ms), C.byref(h))
        if st != 0:
            raise RvError(f"rv_loopback_group_create: {_lib.STATUS_NAMES.get(st, st)}")
        self._h = h
        self.nranks = int(nranks)

    def close(self):
        if getattr(self, "_h", None):
            self._L.rv_loopback_group_destroy(self._h)
            self._h = None


class StateRender:
    """One render context on one GPU (reference: StateRender + its arrays)."""

    def __init__(self, log2_dims=(9, 9, 9), width=1920, height=1080, flags=_lib.RV_FLAGS_REFERENCE,
                 atlas=None, device=0, seed=(0, 0), ref_compat=True, ref_oob_jy=0.0,
                 gi_rays_per_frame=0, gi_init_saturate=False, tex_table=0, exits_off=0):
        self._L = _lib.load()
        self.width, self.height = int(width), int(height)
        self.log2_dims = tuple(int(v) for v in log2_dims)
        self.flags = int(flags)
        self._atlas = None if atlas is None else np.ascontiguousarray(atlas, np.uint8)
        cfg = rv_config()
        cfg.log2_x, cfg.log2_y, cfg.log2_z = self.log2_dims
        cfg.width, cfg.height, cfg.flags = self.width, self.height, self.flags
        cfg.seed_x, cfg.seed_z = int(seed[0]), int(seed[1])
        cfg.ref_compat, cfg.ref_oob_jy = int(bool(ref_compat)), float(ref_oob_jy)
        if self._atlas is not None:
            cfg.atlas_rgba8 = self._atlas.ctypes.data
            cfg.atlas_h, cfg.atlas_w = self._atlas.shape[0], self._atlas.shape[1]
        cfg.gi_rays_per_frame = int(gi_rays_per_frame)
        cfg.gi_init_saturate = int(bool(gi_init_saturate))
        cfg.tex_table, cfg.exits_off = int(tex_table), int(exits_off)
        h = C.c_void_p()
        st = self._L.rv_create(C.byref(cfg), int(device), C.byref(h))
        if st != 0:
            raise RvError(f"rv_create failed: {_lib.STATUS_NAMES.get(st, st)} "
                          "(needs a gfx950 GPU and a valid config)")
        self._h = h
        X, Y, Z = (1 << d for d in self.log2_dims)
        self.dims = (X, Y, Z)

    # ------------------------------------------------------------ plumbing
    def _check(self, st, what):
        if st != 0:
            msg = self._L.rv_last_error(self._h)
            raise RvError(f"{what}: {_lib.STATUS_NAMES.get(st, st)}: "
                          f"{msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "_h", None):
            self._L.rv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, option, value):
        """rv_set_option (include/rvgrt.h): RV_OPT_* run-time options."""
        self._check(self._L.rv_set_option(self._h, int(option), int(value)), "rv_set_option")

    def get_option(self, option) -> int:
        v = C.c_int64()
        self._check(self._L.rv_get_option(self._h, int(option), C.byref(v)), "rv_get_option")
        return int(v.value)

    def set_stream(self, stream_handle: int):
        self._check(self._L.rv_set_stream(self._h, C.c_void_p(stream_handle)), "rv_set_stream")

    def set_frame_path(self, path):
        """RV_PATH_FUSED (per-pixel megakernels) or RV_PATH_WAVEFRONT (stage kernels)."""
        p = {"fused": _lib.RV_PATH_FUSED, "wavefront": _lib.RV_PATH_WAVEFRONT}.get(path, path)
        self._check(self._L.rv_set_frame_path(self._h, int(p)), "rv_set_frame_path")

    def set_frames_in_flight(self, n):
        """Frame slots for concurrent frames on alternating streams (fused path)."""
        self._check(self._L.rv_set_frames_in_flight(self._h, int(n)), "rv_set_frames_in_flight")

    def set_gi_async(self, on):
        self._check(self._L.rv_set_gi_async(self._h, int(bool(on))), "rv_set_gi_async")

    def set_pipeline(self, on):
        """rv_set_pipeline: pipelined reference frames in render_frames."""
        self._check(self._L.rv_set_pipeline(self._h, int(bool(on))), "rv_set_pipeline")

    def set_frame_group(self, n):
        """rv_set_frame_group: reference frames rendered n per launch (0 = off)."""
        self._check(self._L.rv_set_frame_group(self._h, int(n)), "rv_set_frame_group")

    def frame_group_effective(self):
        """The group size render_frames will use (0: per-frame pipeline)."""
        v = C.c_int32(0)
        self._check(self._L.rv_get_frame_group(self._h, C.byref(v)), "rv_get_frame_group")
        return int(v.value)

    def set_flow(self, on):
        """rv_set_flow: drop-in frames as one launch (pre-pass | next GI window | render)."""
        self._check(self._L.rv_set_flow(self._h, int(bool(on))), "rv_set_flow")

    def flow_info(self):
        """(active, launches, fallbacks) of the flow frames (rv_flow_info; synchronises)."""
        a, n, fb = C.c_int32(), C.c_uint64(), C.c_uint64()
        self._check(self._L.rv_flow_info(self._h, C.byref(a), C.byref(n), C.byref(fb)), "rv_flow_info")
        return bool(a.value), int(n.value), int(fb.value)

    def tex_table_info(self):
        """(active, bytes) of sampleTexture's tile table (rv_tex_table_info)."""
        a, n = C.c_int32(), C.c_uint64()
        self._check(self._L.rv_tex_table_info(self._h, C.byref(a), C.byref(n)), "rv_tex_table_info")
        return bool(a.value), int(n.value)

    def set_gi_stats(self, on):
        """rv_set_gi_stats: count the GI update's traversal steps (stage 'gi')."""
        self._check(self._L.rv_set_gi_stats(self._h, int(bool(on))), "rv_set_gi_stats")

    def sync(self):
        self._check(self._L.rv_sync(self._h), "rv_sync")

    # ------------------------------------------------------------ world
    def world_build(self):
        """State::Create: CArray::fill -> GenerateSDF -> InitializeGIData."""
        self._check(self._L.rv_world_build(self._h), "rv_world_build")

    def csdf_build(self):
        self._check(self._L.rv_csdf_build(self._h), "rv_csdf_build")

    def gi_init(self):
        self._check(self._L.rv_gi_init(self._h), "rv_gi_init")

    def gi_update(self, frame, first=0, count=None):
        if count is None:
            X, Y, Z = self.dims
            count = (X // 4) * (Y // 4) * (Z // 4)
        self._check(self._L.rv_gi_update(self._h, int(frame), int(first), int(count)), "rv_gi_update")

    def gi_sweeps(self, n):
        for s in range(n):
            self.gi_update(s)

    def update_gi_data(self):
        """CoarseArray::UpdateGIData: RAYPS cells, rolling offset."""
        self._check(self._L.rv_update_gi_data(self._h), "rv_update_gi_data")

    def world_import(self, kind, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        self._check(self._L.rv_world_import(self._h, kind, _ptr(a), a.nbytes), "rv_world_import")

    def world_export(self, kind) -> np.ndarray:
        X, Y, Z = self.dims
        if kind == _lib.RV_WORLD_BITS:
            a = np.zeros(X * Y * Z // 32, np.uint32)
        elif kind == _lib.RV_WORLD_CSDF:
            a = np.zeros(X * Y * Z // 8, np.uint8)
        elif kind in (_lib.RV_WORLD_COLTOP, _lib.RV_WORLD_HORIZON):   # test hooks: [z / 2, x / 2]
            a = np.zeros((Z // 2, X // 2), np.uint32)
        elif kind == _lib.RV_WORLD_DTOP:                              # [z / 8, x / 8]
            a = np.zeros((Z // 8, X // 8), np.int32)
        else:
            a = np.zeros((X // 4) * (Y // 4) * (Z // 4) * 4, np.uint8)
        self._check(self._L.rv_world_export(self._h, kind, _ptr(a), a.nbytes), "rv_world_export")
        return a

    def world_top_info(self) -> int:
        """rv_world_top_info (test hook): the sky exit in effect, World::ytop."""
        y = C.c_uint32()
        self._check(self._L.rv_world_top_info(self._h, C.byref(y)), "rv_world_top_info")
        return int(y.value)

    def world_edit(self, boxes):
        """rv_world_edit: set / clear voxel boxes (x0, y0, z0, x1, y1, z1, solid) in
        place, in order; bits, CSDF and exits end as a bits import + csdf_build
        of the edited world would leave them."""
        boxes = list(boxes)
        self._check(self._L.rv_world_edit(self._h, _edit_boxes(boxes), len(boxes)), "rv_world_edit")

    def world_edit_shapes(self, shapes):
        """rv_world_edit_shapes: set / clear ellipsoids and axis-aligned elliptic cylinders (kind, solid,
        c2, r2) -- centre and radii in half-voxels, voxel x having its centre at 2 x + 1 -- in place, in
        order, by one launch; shapes are clipped to the window.  Ends like world_edit over the union of
        their boxes (edit_shapes_box).  Returns (n_set, n_cleared): the voxels that turned solid and the
        voxels that turned empty, world before against world after."""
        shapes = list(shapes)
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self._L.rv_world_edit_shapes(self._h, _edit_shapes(shapes), len(shapes), C.byref(a), C.byref(b)),
                    "rv_world_edit_shapes")
        return int(a.value), int(b.value)

    def world_blast(self, centre_voxel, radius_voxels, settle=True, relight=0):
        """An explosion, composed of existing calls: world_edit_shapes clears the sphere of
        `radius_voxels` around the centre of voxel `centre_voxel`; with `settle`, world_settle lets what
        it cut loose come down, over the parts settle_parts makes of the sphere's clipped box -- the box
        grown by 1 voxel, whole up to a radius of about 62 voxels, in halves above that, where a loose
        piece that straddles a cut stays up (see there); with relight > 0, gi_relight runs
        that many steps (frame0 = 0, INIT) over relight_box (margin 1) of everything that changed.
        Returns a dict: "edit" (n_set, n_cleared), "box" the sphere's clipped box, "settle" a list of
        world_settle's (rounds, box) per part (None without settle), "relight" the GI box (or None)."""
        r2 = 2 * int(radius_voxels)
        shape = (_lib.RV_SHAPE_ELLIPSOID, 0, tuple(2 * int(v) + 1 for v in centre_voxel), (r2, r2, r2))
        edit = self.world_edit_shapes([shape])
        _, box = edit_shapes_box(self.log2_dims, [shape])
        out = {"edit": edit, "box": box, "settle": None, "relight": None}
        changed = [box] if edit[1] else []
        if settle and _box_volume(_voxel_box(box)) > 0:
            parts = settle_parts(box, self.dims)
            out["settle"] = [self.world_settle(p) for p in parts]
            changed += [b for rounds, b in out["settle"] if rounds]
        if relight > 0 and changed:
            gbox = relight_box(self.log2_dims, [b + (0,) for b in changed], margin=1)
            cells = (gbox[3] - gbox[0]) * (gbox[4] - gbox[1]) * (gbox[5] - gbox[2])
            step = max(_lib.RV_RELIGHT_MAX_RECORDS // max(cells, 1), 1)   # k1 then k2 steps equal k1 + k2
            done = 0
            while done < int(relight):
                k = min(step, int(relight) - done)
                self.gi_relight(gbox, done, k, init=done == 0)
                done += k
            out["relight"] = gbox
        return out

    def pattern_create(self, vox) -> int:
        """rv_pattern_create: a bool array vox[z, y, x] (at most 256 per axis) becomes a pattern kept on the
        device; returns its id, the lowest free slot."""
        (nx, ny, nz), words = pattern_bits(vox)
        pid = C.c_int32(-1)
        self._check(self._L.rv_pattern_create(self._h, nx, ny, nz, _ptr(words), words.nbytes, C.byref(pid)),
                    "rv_pattern_create")
        return int(pid.value)

    def pattern_capture(self, box) -> int:
        """rv_pattern_capture: the voxels of the box (x0, y0, z0, x1, y1, z1) of the world become a new
        pattern without leaving the device; a query, like world_detached.  Returns the id."""
        b = _voxel_box(box)
        pid = C.c_int32(-1)
        self._check(self._L.rv_pattern_capture(self._h, C.byref(b), C.byref(pid)), "rv_pattern_capture")
        return int(pid.value)

    def pattern_read(self, pid) -> np.ndarray:
        """rv_pattern_read: the pattern as a bool array [z, y, x]."""
        dims = (C.c_int32 * 3)()
        self._check(self._L.rv_pattern_read(self._h, int(pid), dims, None, 0), "rv_pattern_read")
        nx, ny, nz = dims[:]
        words = np.zeros(((nx + 31) // 32) * ny * nz, np.uint32)
        self._check(self._L.rv_pattern_read(self._h, int(pid), dims, _ptr(words), words.nbytes), "rv_pattern_read")
        return pattern_voxels((nx, ny, nz), words)

    def pattern_destroy(self, pid):
        """rv_pattern_destroy: the id is free again."""
        self._check(self._L.rv_pattern_destroy(self._h, int(pid)), "rv_pattern_destroy")

    def world_stamp(self, stamps):
        """rv_world_stamp: patterns pasted into the world by one launch, in list order, a later stamp winning
        voxel by voxel.  A stamp is (pattern id, op, orient, (x, y, z)): op RV_STAMP_SET / CLEAR / COPY,
        orient any OR of RV_ORIENT_SWAP_XZ / FLIP_X / FLIP_Z (the 8 symmetries that keep y up), (x, y, z) the
        world voxel of the oriented pattern's low corner; stamps are clipped to the window.  Ends like
        world_edit over the union of their boxes.  Returns (n_set, n_cleared, changed): the voxels that turned
        solid and empty, world before against world after, and that union box (relight over it)."""
        stamps = list(stamps)
        a, b, ch = C.c_uint64(), C.c_uint64(), rv_voxel_box()
        self._check(self._L.rv_world_stamp(self._h, _stamps(stamps), len(stamps), C.byref(a), C.byref(b), C.byref(ch)),
                    "rv_world_stamp")
        return int(a.value), int(b.value), _box_tuple(ch)

    def world_stamp_info(self):
        """(calls, stamps, patterns_live, pattern_bytes): the world_stamp calls that launched, the stamps
        they applied, the live patterns and their bytes."""
        n, s, p, by = C.c_uint64(), C.c_uint64(), C.c_int32(), C.c_uint64()
        self._check(self._L.rv_world_stamp_info(self._h, C.byref(n), C.byref(s), C.byref(p), C.byref(by)),
                    "rv_world_stamp_info")
        return int(n.value), int(s.value), int(p.value), int(by.value)

    def world_move(self, box, delta):
        """Matter moved sideways, up or down, composed of existing calls: pattern_capture of the voxel box,
        then one world_stamp that clears the box's solid voxels at the old place and copies the box to
        box + delta (the copy wins where the two overlap; what reaches beyond the window is lost), then
        pattern_destroy.  The horizontal counterpart of world_fall.  Returns world_stamp's result."""
        pid = self.pattern_capture(box)
        try:
            at = tuple(int(box[a]) for a in range(3))
            to = tuple(int(box[a]) + int(delta[a]) for a in range(3))
            return self.world_stamp([(pid, _lib.RV_STAMP_CLEAR, 0, at), (pid, _lib.RV_STAMP_COPY, 0, to)])
        finally:
            self.pattern_destroy(pid)

    def world_edit_info(self):
        """(edits, csdf_cells, last_full): calls that changed a voxel, the coarse
        cells the last call recomputed, whether it ran the whole-grid build."""
        e, n, f = C.c_uint64(), C.c_uint64(), C.c_int32()
        self._check(self._L.rv_world_edit_info(self._h, C.byref(e), C.byref(n), C.byref(f)), "rv_world_edit_info")
        return int(e.value), int(n.value), bool(f.value)

    def world_scroll(self, dx, dz):
        """rv_world_scroll: the window moves by (dx, 0, dz) voxels (multiples of 8) over
        the generated terrain; retained voxels, CSDF bytes and GI cells move to their
        new index, the entering slab is generated at the new origin, the CSDF slabs
        the move can change and the exits are rebuilt, entering GI cells take
        gi_init's value.  Synchronous."""
        self._check(self._L.rv_world_scroll(self._h, int(dx), int(dz)), "rv_world_scroll")

    def world_scroll_info(self):
        """(scrolls, csdf_cells, last_full, (origin_x, origin_z)): calls that moved the
        window, the coarse cells the last one recomputed, whether a step of it ran
        the whole-grid build, the window's origin."""
        n, c, f, ox, oz = C.c_uint64(), C.c_uint64(), C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._L.rv_world_scroll_info(self._h, C.byref(n), C.byref(c), C.byref(f), C.byref(ox),
                                                 C.byref(oz)), "rv_world_scroll_info")
        return int(n.value), int(c.value), bool(f.value), (int(ox.value), int(oz.value))

    def world_persist(self, on):
        """rv_world_persist: edited columns survive scrolling away and back -- the dirty
        columns that leave the window are kept in a host store and put back when the
        library generates them again (world_scroll, world_build).  Default off."""
        self._check(self._L.rv_world_persist(self._h, int(bool(on))), "rv_world_persist")

    def world_persist_info(self) -> dict:
        """rv_world_persist_info: {on, dirty_columns, stored_columns, stored_bytes,
        captured_total, restored_total}."""
        on = C.c_int32()
        v = [C.c_uint64() for _ in range(5)]
        self._check(self._L.rv_world_persist_info(self._h, C.byref(on), *[C.byref(x) for x in v]),
                    "rv_world_persist_info")
        names = ("dirty_columns", "stored_columns", "stored_bytes", "captured_total", "restored_total")
        return {"on": bool(on.value), **{k: int(x.value) for k, x in zip(names, v)}}

    def world_persist_flush(self):
        """rv_world_persist_flush ("save game"): every dirty column of the window is copied
        into the store; the columns stay dirty.  Synchronous."""
        self._check(self._L.rv_world_persist_flush(self._h), "rv_world_persist_flush")

    def world_store_list(self) -> np.ndarray:
        """rv_world_store_list: the store's keys, (n, 2) int32 rows (wx, wz) sorted by (wz, wx)."""
        n = C.c_int64()
        self._check(self._L.rv_world_store_list(self._h, None, 0, C.byref(n)), "rv_world_store_list")
        keys = np.zeros((int(n.value), 2), np.int32)
        self._check(self._L.rv_world_store_list(self._h, _ptr(keys), len(keys), C.byref(n)), "rv_world_store_list")
        return keys

    def world_store_get(self, wx, wz) -> np.ndarray:
        """rv_world_store_get: the stored column bits (2 Y uint32) of key (wx, wz)."""
        bits = np.zeros(2 * self.dims[1], np.uint32)
        self._check(self._L.rv_world_store_get(self._h, int(wx), int(wz), _ptr(bits), bits.nbytes), "rv_world_store_get")
        return bits

    def world_store_put(self, wx, wz, bits):
        """rv_world_store_put: column bits (2 Y uint32) into the store under key (wx, wz);
        used the next time the library generates that column."""
        a = np.ascontiguousarray(bits, np.uint32)
        self._check(self._L.rv_world_store_put(self._h, int(wx), int(wz), _ptr(a), a.nbytes), "rv_world_store_put")

    def world_store_clear(self):
        """rv_world_store_clear: empties the store and the dirty set."""
        self._check(self._L.rv_world_store_clear(self._h), "rv_world_store_clear")

    def world_columns_read(self, bxz) -> np.ndarray:
        """rv_world_columns_read: the column bits of the grid brick columns (bx, bz) of
        the list, (n, 2 Y) uint32 in list order (repeats allowed).  Synchronous."""
        cols = np.ascontiguousarray(bxz, np.int32).reshape(-1, 2)
        bits = np.zeros((len(cols), 2 * self.dims[1]), np.uint32)
        self._check(self._L.rv_world_columns_read(self._h, _ptr(cols), len(cols), _ptr(bits), bits.nbytes),
                    "rv_world_columns_read")
        return bits

    def texture_origin_set(self, ox, oz):
        """rv_texture_origin_set: sampleTexture's lattice points are shifted by (ox, 0, oz)
        as integers; the tile table is rebuilt at the new origin.  Synchronous; discards
        work computed ahead (unless the origin is the one the context has)."""
        self._check(self._L.rv_texture_origin_set(self._h, int(ox), int(oz)), "rv_texture_origin_set")

    def texture_follow_scroll(self, on):
        """rv_texture_follow_scroll: world_scroll(dx, dz) also adds (dx, dz) to the texture
        origin, so the textures stay anchored to the terrain."""
        self._check(self._L.rv_texture_follow_scroll(self._h, int(bool(on))), "rv_texture_follow_scroll")

    def texture_origin(self):
        """((ox, oz), follow): the texture origin and whether it follows scrolls."""
        ox, oz, f = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._L.rv_texture_origin_get(self._h, C.byref(ox), C.byref(oz), C.byref(f)),
                    "rv_texture_origin_get")
        return (int(ox.value), int(oz.value)), bool(f.value)

    def texture_tiles(self, pos):
        """rv_texture_tiles (test hook): the kernels' atlas tile, a uint8 0xYX per position
        (n, 3) float32, against this context's tile table and texture origin."""
        p = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        out = np.zeros(len(p), np.uint8)
        self._check(self._L.rv_texture_tiles(self._h, _ptr(p), len(p), _ptr(out)), "rv_texture_tiles")
        return out

    def bodies_move(self, lo, size, delta, flags=0):
        """rv_world_bodies_move: n boxes [lo, lo + size) in grid coordinates moved by delta
        through the voxel bits with per-axis collision (y, x, z).  lo is (n, 3); size and
        delta broadcast against it.  Returns (lo (n, 3) float32, flags (n,) uint32 of
        RV_BODY_*).  Synchronous."""
        b = _bodies(lo, size, delta)
        out = np.zeros((len(b), 4), np.uint32)
        self._check(self._L.rv_world_bodies_move(self._h, _ptr(b), len(b), int(flags), _ptr(out)),
                    "rv_world_bodies_move")
        return _bodies_out(out)

    def bodies_move_device(self, dev_in: int, n: int, dev_out: int, flags=0):
        """rv_world_bodies_move_device: n rv_body at device address dev_in -> n rv_body_out
        at dev_out, enqueued on the context's stream (not synchronous)."""
        self._check(self._L.rv_world_bodies_move_device(self._h, C.c_void_p(dev_in), int(n), int(flags),
                                                        C.c_void_p(dev_out)), "rv_world_bodies_move_device")

    def bodies_info(self):
        """(calls, bodies): sums over the bodies_move calls that did work."""
        n, b = C.c_uint64(), C.c_uint64()
        self._check(self._L.rv_world_bodies_info(self._h, C.byref(n), C.byref(b)), "rv_world_bodies_info")
        return int(n.value), int(b.value)

    def world_detached(self, box, flags=0, cap=None, want_mask=True):
        """rv_world_detached: the solid voxels of the voxel box (x0, y0, z0, x1, y1, z1) that nothing
        holds -- no 6-connected path inside the box to solid matter beyond it, the floor or the window's
        walls.  Returns (components, n_comps, n_voxels, mask): the first min(cap, n_comps) components
        (COMPONENT_DTYPE: lo, hi, seed, voxels; cap None = all of them, by a counting call first), their
        total, the detached voxels, and the mask words (None unless want_mask).
        flags=RV_DETACHED_CLEAR clears them like a world_edit of those voxels; the results are those of
        before the clear.  Synchronous."""
        b = _voxel_box(box)
        nw = (_box_volume(b) + 31) // 32
        n, v = C.c_int64(), C.c_uint64()
        if cap is None and not flags:
            self._check(self._L.rv_world_detached(self._h, C.byref(b), 0, None, 0, C.byref(n), None, None, 0),
                        "rv_world_detached")
            cap = int(n.value)
        elif cap is None:   # a clearing call runs once: room for the most a box can hold
            cap = (_box_volume(b) + 1) // 2
        comps = np.zeros(max(int(cap), 1), COMPONENT_DTYPE)
        mask = np.zeros(max(nw, 1), np.uint32) if want_mask else None
        self._check(self._L.rv_world_detached(self._h, C.byref(b), int(flags), _ptr(comps) if cap else None, int(cap),
                                              C.byref(n), C.byref(v), None if mask is None else _ptr(mask),
                                              0 if mask is None else mask.nbytes), "rv_world_detached")
        return comps[:min(int(cap), int(n.value))].copy(), int(n.value), int(v.value), mask

    def world_detached_info(self):
        """(calls, voxels_scanned, voxels_cleared): sums over the world_detached calls that ran."""
        n, s, k = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._L.rv_world_detached_info(self._h, C.byref(n), C.byref(s), C.byref(k)),
                    "rv_world_detached_info")
        return int(n.value), int(s.value), int(k.value)

    def world_fall(self, box, max_fall=0, cap=None):
        """rv_world_fall: every detached component of the voxel box drops straight down until a voxel
        that does not move with it, or the floor, stops it (max_fall > 0: at most that many rows).
        One call is one round, judged on the world before the call.  Returns (components, n_comps,
        n_voxels, changed): FALLEN_DTYPE records (comp as before the move, fall, flags; cap None =
        room for the most a box can hold), the totals, and the voxel box that bounds every cleared
        and every set voxel (all zero when nothing moved).  Ends like the world_edit of the same
        change; relight over `changed`.  Synchronous."""
        b = _voxel_box(box)
        if cap is None:   # the call runs once
            cap = (_box_volume(b) + 1) // 2
        comps = np.zeros(max(int(cap), 1), FALLEN_DTYPE)
        n, v, ch = C.c_int64(), C.c_uint64(), rv_voxel_box()
        self._check(self._L.rv_world_fall(self._h, C.byref(b), int(max_fall), _ptr(comps) if cap else None, int(cap),
                                          C.byref(n), C.byref(v), C.byref(ch)), "rv_world_fall")
        return comps[:min(int(cap), int(n.value))].copy(), int(n.value), int(v.value), _box_tuple(ch)

    def world_fall_info(self):
        """(calls, components_moved, voxels_moved): sums over the world_fall calls that ran."""
        n, k, v = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._L.rv_world_fall_info(self._h, C.byref(n), C.byref(k), C.byref(v)), "rv_world_fall_info")
        return int(n.value), int(k.value), int(v.value)

    def world_settle(self, box, max_fall=0, max_rounds=64):
        """world_fall repeated, each call over the `changed` box of the one before, until a call finds
        nothing detached (or max_rounds calls have moved something).  Returns (rounds, box): the
        calls that moved something and the union of their changed boxes (all zero for none).  A
        changed box grows downwards with the fall; one above RV_DETACHED_MAX_VOXELS raises RvError."""
        rounds, union = 0, None
        box = tuple(int(v) for v in box)
        while rounds < max_rounds:
            _, n, _, changed = self.world_fall(box, max_fall, cap=0)
            if n == 0:
                break
            rounds += 1
            union = changed if union is None else (tuple(min(a, c) for a, c in zip(union[:3], changed[:3])) +
                                                   tuple(max(a, c) for a, c in zip(union[3:], changed[3:])))
            box = changed
        return rounds, union or (0, 0, 0, 0, 0, 0)

    def gi_relight(self, box, frame0, iterations, init=False):
        """rv_gi_relight: `iterations` update steps (RNG frames frame0, frame0 + 1, ...)
        of the GI cells (x0, y0, z0, x1, y1, z1), each step reading the grid the step
        before left; init=True first gives the box's cells gi_init's values.  The
        GI frame counter and the rolling offset are untouched."""
        if len(box) != 6:
            raise ValueError("a GI box is (x0, y0, z0, x1, y1, z1)")
        b = rv_gi_box(*(int(v) for v in box))
        self._check(self._L.rv_gi_relight(self._h, C.byref(b), int(frame0) & 0xFFFFFFFF, int(iterations),
                                          _lib.RV_RELIGHT_INIT if init else 0), "rv_gi_relight")

    def gi_relight_info(self):
        """(calls, cells, records): sums over the gi_relight calls that did work."""
        n, c, r = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._L.rv_gi_relight_info(self._h, C.byref(n), C.byref(c), C.byref(r)), "rv_gi_relight_info")
        return int(n.value), int(c.value), int(r.value)

    # ------------------------------------------------------------ frames
    def draw_cuda(self, pos, fo, up, ri, vp, prev_vp, jitter_x=0.0, jitter_y=0.0):
        """StateRender::drawCUDA, same argument order."""
        arrs = [np.ascontiguousarray(a, np.float32) for a in (pos, fo, up, ri, vp, prev_vp)]
        self._check(self._L.rv_draw_cuda(self._h, *[_ptr(a) for a in arrs],
                                         float(jitter_x), float(jitter_y)), "rv_draw_cuda")

    def frame(self, cam: rv_camera, vp, prev_vp=None, time=0.0, jx=0.0, jy=0.0, flags=None):
        vp = np.ascontiguousarray(vp, np.float32)
        pvp = vp if prev_vp is None else np.ascontiguousarray(prev_vp, np.float32)
        f = self.flags if flags is None else int(flags)
        self._check(self._L.rv_frame(self._h, C.byref(cam), _ptr(vp), _ptr(pvp), float(time),
                                     float(jx), float(jy), f), "rv_frame")

    def frame_tiles(self, cam, vp, tile_ids, tile_px=64, prev_vp=None, time=0.0, jx=0.0, jy=0.0,
                    flags=None):
        vp = np.ascontiguousarray(vp, np.float32)
        pvp = vp if prev_vp is None else np.ascontiguousarray(prev_vp, np.float32)
        ids = np.ascontiguousarray(tile_ids, np.int32)
        f = self.flags if flags is None else int(flags)
        self._check(self._L.rv_frame_tiles(self._h, C.byref(cam), _ptr(vp), _ptr(pvp), float(time),
                                           float(jx), float(jy), f, _ptr(ids), len(ids),
                                           int(tile_px)), "rv_frame_tiles")

    def set_tile_shard(self, tile_px, rank, nranks, root_weight=None):
        """This rank's interleaved share of T x T tiles for render_frames (0 ranks = full frames);
        root_weight = rank 0's share relative to the others (default 1)."""
        if root_weight is None:
            self._check(self._L.rv_set_tile_shard(self._h, int(tile_px), int(rank), int(nranks)), "rv_set_tile_shard")
        else:
            self._check(self._L.rv_set_tile_shard_weighted(self._h, int(tile_px), int(rank), int(nranks),
                                                           float(root_weight)), "rv_set_tile_shard_weighted")

    def set_gather_bpp(self, bpp):
        """Packed pixel bytes of the loop's tile gather (3 RGB24, 4 RGBA8)."""
        self._check(self._L.rv_set_gather_bpp(self._h, int(bpp)), "rv_set_gather_bpp")

    def render_frames(self, n, cam, vp, prev_vp=None, time=0.0, jx=0.0, jy=0.0, flags=None,
                      gi_per_frame=False, comm=None):
        """Native frame loop (rv_render_frames): n frames over the frame slots'
        streams; with a tile shard, this rank's tiles, the RCCL gather to rank 0
        and rank 0's untile every frame."""
        vp = np.ascontiguousarray(vp, np.float32)
        pvp = vp if prev_vp is None else np.ascontiguousarray(prev_vp, np.float32)
        f = self.flags if flags is None else int(flags)
        self._check(self._L.rv_render_frames(self._h, int(n), C.byref(cam), _ptr(vp), _ptr(pvp), float(time),
                                             float(jx), float(jy), f, int(bool(gi_per_frame)),
                                             comm._h if comm is not None else None), "rv_render_frames")

    def render_frame_seq(self, descs, next_desc=None, flags=None, gi_per_frame=False, comm=None):
        """rv_render_frame_seq: one rv_frame_desc per frame (moving camera,
        jitter/time sequence); next_desc = the frame after the sequence."""
        n = len(descs)
        arr = (rv_frame_desc * max(n, 1))(*descs)
        f = self.flags if flags is None else int(flags)
        nxt = C.byref(next_desc) if next_desc is not None else None
        self._check(self._L.rv_render_frame_seq(self._h, n, arr, nxt, f, int(bool(gi_per_frame)),
                                                comm._h if comm is not None else None), "rv_render_frame_seq")

    def tile_buffer(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.rv_tile_buffer(self._h, C.byref(p), C.byref(n)), "rv_tile_buffer")
        return p.value, n.value

    def bind_tile_buffer(self, dev_ptr, nbytes):
        self._check(self._L.rv_bind_tile_buffer(self._h, C.c_void_p(dev_ptr), int(nbytes)),
                    "rv_bind_tile_buffer")

    def untile(self, dev_ptr: int, tile_ids, tile_px=64):
        ids = np.ascontiguousarray(tile_ids, np.int32)
        self._check(self._L.rv_untile(self._h, C.c_void_p(dev_ptr), _ptr(ids), len(ids), int(tile_px)),
                    "rv_untile")

    def bind_output(self, kind, dev_ptr, pitch):
        self._check(self._L.rv_bind_output(self._h, kind, C.c_void_p(dev_ptr), pitch), "rv_bind_output")

    def image_ptr(self, kind):
        p, pitch = C.c_void_p(), C.c_size_t()
        self._check(self._L.rv_image_ptr(self._h, kind, C.byref(p), C.byref(pitch)), "rv_image_ptr")
        return p.value, pitch.value

    def readback(self, kind=_lib.RV_IMAGE_COLOR) -> np.ndarray:
        W, H = self.width, self.height
        if kind == _lib.RV_IMAGE_COLOR:
            a = np.zeros((H, W, 4), np.uint8)
        elif kind == _lib.RV_IMAGE_MOTION:
            a = np.zeros((H, W, 2), np.uint16)
        elif kind == _lib.RV_IMAGE_DEPTH:
            a = np.zeros((H, W), np.uint16)
        else:
            a = np.zeros((H // 2, W // 2), np.float32)
        self._check(self._L.rv_readback(self._h, kind, _ptr(a), 0), "rv_readback")
        return a

    # ------------------------------------------------------------ test surface
    def trace_rays(self, org, dirs, dist, variant=None) -> np.ndarray:
        """rv_trace_rays, or with `variant` (look-ahead group 1 / 4 / 8 | RV_TRACE_SKY / SUN / COL)
        rv_trace_rays_variant: one of the frame kernels' traversals on the world's own exit
        tables; `pad` then counts the look-ahead groups the ray's lane knew empty."""
        org = np.ascontiguousarray(org, np.float32)
        dirs = np.ascontiguousarray(dirs, np.float32)
        dist = np.ascontiguousarray(dist, np.float32)
        n = len(dist)
        dt = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("u", "<f4"), ("v", "<f4"),
                       ("hit", "<i4"), ("undef", "<i4"), ("sphere_steps", "<i4"),
                       ("dda_steps", "<i4"), ("csdf_checks", "<i4"), ("pad", "<i4")])
        assert dt.itemsize == C.sizeof(rv_hit)
        out = np.zeros(max(n, 1), dt)
        if variant is None:
            self._check(self._L.rv_trace_rays(self._h, _ptr(org), _ptr(dirs), _ptr(dist), n, _ptr(out)),
                        "rv_trace_rays")
        else:
            self._check(self._L.rv_trace_rays_variant(self._h, int(variant), _ptr(org), _ptr(dirs), _ptr(dist), n,
                                                      _ptr(out)), "rv_trace_rays_variant")
        return out[:n]

    def stats(self, stage=-1) -> dict:
        """Counters (RV_F_STATS frames) of one RV_STAGE_* (-1 = all stages)."""
        s = rv_stats()
        self._check(self._L.rv_stats_stage(self._h, int(stage), C.byref(s)), "rv_stats_stage")
        return s.as_dict()

    def timing_enable(self, max_frames):
        self._check(self._L.rv_timing_enable(self._h, int(max_frames)), "rv_timing_enable")

    def timing_get(self):
        """(ms per stage [gi, prepass, render] summed over frames, frames)."""
        ms = (C.c_double * 3)()
        n = C.c_int32()
        self._check(self._L.rv_timing_get(self._h, ms, C.byref(n)), "rv_timing_get")
        return list(ms), n.value

    def timing_stages(self):
        """({stage name: summed ms}, frames) for the RV_STAGE_* slots."""
        n = len(_lib.STAGES)
        ms = (C.c_double * n)()
        k = C.c_int32()
        self._check(self._L.rv_timing_stages(self._h, ms, n, C.byref(k)), "rv_timing_stages")
        return dict(zip(_lib.STAGES, list(ms))), k.value

    def timing_launches(self):
        """{stage name: launches timed} (divide timing_stages' sums by these)."""
        n = len(_lib.STAGES)
        k = (C.c_int32 * n)()
        self._check(self._L.rv_timing_launches(self._h, k, n), "rv_timing_launches")
        return dict(zip(_lib.STAGES, list(k)))

    def stats_reset(self):
        self._check(self._L.rv_stats_reset(self._h), "rv_stats_reset")
