"""Who owns what on the device: one context taken through every site that reshapes or regrows a buffer it
keeps -- frame slots, the tile order arrays, the loops' frame sets and exchange buffers, the scratch of edit,
relight, scroll and bodies -- must go on producing exactly what a fresh context of the same configuration
produces, and contexts must come and go without disturbing each other.  Everything is compared for equality:
frames as their colour, motion-vector and depth images, worlds as their exported bits, CSDF and GI grid."""
import numpy as np
import pytest

from gpu_world import gi, images, pack, run_ranks, rv, synthetic_voxels, world
import np_bodies as B

pytestmark = pytest.mark.gpu

LG, W, H, T = (5, 5, 5), 48, 32, 16          # a 32^3 world, 3 x 2 tiles of 16 px
RAYS = 64                                    # GI cells per update: 1/8 of the 8^3 grid, so a frame group of 4 holds


def _blocks(n, seed):
    """A floor and 4^3 blocks, with the air around the camera kept free."""
    vox = synthetic_voxels("blocks", n, n, n, np.random.default_rng(seed))
    c = n // 2
    vox[c - 3:c + 3, n - 12:n, c - 3:c + 3] = False
    return vox


def _context(rv, atlas, n=32, w=W, h=H, **kw):
    lg = (n.bit_length() - 1,) * 3
    r = rv.StateRender(lg, w, h, flags=rv.RV_FLAGS_REFERENCE, atlas=atlas, **kw)
    r.world_import(rv.RV_WORLD_BITS, pack(_blocks(n, 7)))
    r.csdf_build()
    r.gi_init()
    r.gi_update(0)
    return r


def _view(rv, n=32, w=W, h=H):
    """From under the top of the world, steeply down onto the blocks and the floor."""
    return rv.camera_from_pose((0.5 * n + 0.5, n - 6.5, 0.5 * n + 0.5), 2.44, -np.pi - 0.9, w, h)


def _same(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (what, k)


# ---------------------------------------------------------------- 1. slots
def test_slot_reshaping(rv, atlas):
    """Frame A with 1 slot, with 3 slots and with 1 again equals the fresh context's, and so does every slot
    after 3 -> 1 -> 3.  In between, tile frames whose list grows from 1 tile to all 6, to all 6 twice (12 ids
    take a second block of 8 order entries: the order arrays regrow, also while slot 1 or 2 is active)
    and shrinks to 2: their tiles, assembled, equal the fresh frame's pixels under them."""
    cam, vp = _view(rv)
    fresh = _context(rv, atlas)
    fresh.frame(cam, vp)
    want = images(rv, fresh)
    fresh.close()
    assert len(np.unique(want[0].reshape(-1, 4), axis=0)) > 8, "the view shows more than sky"
    every = np.arange(6, dtype=np.int32)
    lists = {"1": every[:1], "6": every, "12": np.concatenate([every, every]), "2": every[[1, 4]]}

    r = _context(rv, atlas)

    def frame_a(what):
        r.frame(cam, vp)
        _same(images(rv, r), want, what)

    def tiles(name):
        ids = lists[name]
        r.frame_tiles(cam, vp, ids, tile_px=T)
        r.untile(r.tile_buffer()[0], ids, tile_px=T)
        got = r.readback(rv.RV_IMAGE_COLOR)
        for t in set(int(i) for i in ids):
            y, x = (t // 3) * T, (t % 3) * T
            assert np.array_equal(got[y:y + T, x:x + T], want[0][y:y + T, x:x + T]), (name, t)

    frame_a("1 slot")
    for name in ("1", "6", "12", "2"):
        tiles(name)
    frame_a("1 slot, after tiles")
    r.set_frames_in_flight(3)
    for k in range(3):
        frame_a(("3 slots", k))
    for name in ("1", "1", "1", "6", "12", "12", "2"):     # slots 0 1 2 0 1 2 0: slots 1 and 2 regrow at "12"
        tiles(name)
    for k in range(3):
        frame_a(("3 slots, after tiles", k))
    r.set_frames_in_flight(1)
    frame_a("1 slot again")
    for name in ("12", "2"):                                # slot 0 regrows here
        tiles(name)
    frame_a("1 slot again, after tiles")
    for n in (3, 1, 3):
        r.set_frames_in_flight(n)
    for k in range(3):
        frame_a(("3 -> 1 -> 3", k))
    r.close()


# ---------------------------------------------------------------- 2. loops
def test_loop_reshaping(rv, atlas):
    """rv_render_frames on the two ranks of a loopback group: a tile shard of 16 px, of 32 px (the library's
    tile sizes are multiples of 16), no shard, then frame groups of 4, groups off again, and groups of 4 with
    the 16 px shard.  Each shape runs the loops that keep buffers of that shape -- pipelined or grouped with a
    GI update per frame, one frame at a time, batched over 2 slots -- so every reshape-on-mismatch site of
    rv_loops.cpp meets a new shape at least twice.  The fresh context renders the same frames one at a time; the
    last frame of each run equals its same frame, and every rank's GI grid equals its grid.  Whole frames are
    compared in colour, motion vectors and depth on both ranks; a shard gathers colour only, to rank 0."""
    cam, vp = _view(rv)
    flags = rv.RV_FLAGS_REFERENCE
    fresh = _context(rv, atlas, gi_rays_per_frame=RAYS)
    rs = [_context(rv, atlas, gi_rays_per_frame=RAYS) for _ in range(2)]
    group = rv.LoopbackGroup(2, timeout_ms=60000)
    comms = [rv.Comm.loopback(r, group, q) for q, r in enumerate(rs)]

    def run(n, with_gi, sharded, what):
        run_ranks([lambda q=q: rs[q].render_frames(n, cam, vp, flags=flags, gi_per_frame=with_gi,
                                                   comm=comms[q] if sharded else None) for q in range(2)])
        for q in range(2):
            comms[q].wait(60000) if sharded else rs[q].sync()
        for _ in range(n if with_gi else 1):
            if with_gi:
                fresh.update_gi_data()
            fresh.frame(cam, vp, flags=flags)
        want = images(rv, fresh)
        if sharded:
            assert np.array_equal(rs[0].readback(rv.RV_IMAGE_COLOR), want[0]), what
        else:
            for q in range(2):
                _same(images(rv, rs[q]), want, (what, q))
        for q in range(2):
            assert np.array_equal(gi(rv, rs[q]), gi(rv, fresh)), (what, q)

    def shape(px, grp, what):
        for q, r in enumerate(rs):
            r.set_tile_shard(px, q, 2 if px else 0)
            r.set_frame_group(grp)
        assert rs[0].frame_group_effective() == grp
        run(9 if grp else 3, True, px > 0, (what, "gi per frame"))      # pipelined, or two groups and a part
        run(2, False, px > 0, (what, "frame by frame"))
        for r in rs:
            r.set_frames_in_flight(2)
        run(5, False, px > 0, (what, "batched"))
        for r in rs:
            r.set_frames_in_flight(1)

    shape(16, 0, "shard 16")
    shape(32, 0, "shard 32")
    shape(0, 0, "no shard")
    shape(0, 4, "groups of 4")
    shape(0, 0, "groups off")
    shape(16, 4, "groups of 4, shard 16")
    for c in comms:
        c.close()
    for r in rs:
        r.close()
    group.close()
    fresh.close()


# ---------------------------------------------------------------- 3. scratch
def test_scratch_regrowth(rv):
    """Every scratch buffer a context keeps between calls, first small, then at its largest: an edit of 1 box
    and one of RV_EDIT_MAX_BOXES, relights of 1 cell and of the whole grid, scrolls by 8 along x and by 16 along
    z, 1 body and 300.  The fresh context gets each call at its final size only (the first box is in the long
    list too, and the whole-grid relight starts from gi_init's values, so the small calls leave nothing behind);
    both worlds -- bits, CSDF, GI -- and the 300 bodies end up equal."""
    rng = np.random.default_rng(5)
    lo = rng.integers(0, 29, (rv._lib.RV_EDIT_MAX_BOXES, 3))
    size = rng.integers(1, 4, lo.shape)
    boxes = [(int(a[0]), int(a[1]), int(a[2]), int(a[0] + s[0]), int(a[1] + s[1]), int(a[2] + s[2]), int(i & 1))
             for i, (a, s) in enumerate(zip(lo, size))]
    bodies = B.random_bodies(np.random.default_rng(6), 300, (32, 32, 32))

    def ends(grown):
        r = rv.StateRender(LG, W, H, gi_rays_per_frame=RAYS)
        r.world_import(rv.RV_WORLD_BITS, pack(_blocks(32, 7)))   # (the generated window is solid up to row 32)
        r.csdf_build()
        r.gi_init()
        if grown:
            r.world_edit(boxes[:1])
        r.world_edit(boxes)
        if grown:
            r.gi_relight((3, 3, 3, 4, 4, 4), 11, 2)
        r.gi_relight((0, 0, 0, 8, 8, 8), 11, 2, init=True)
        r.world_scroll(8, 0)
        r.world_scroll(0, 16)
        if grown:
            r.bodies_move(bodies[0][:1], bodies[1][:1], bodies[2][:1])
        moved = r.bodies_move(*bodies)
        out = world(rv, r) + (gi(rv, r), moved[0].view(np.uint32), moved[1])
        r.close()
        return out

    want = ends(False)
    assert want[0].any() and not want[0].all() and len(np.unique(want[2])) > 1, "a world with something in it"
    _same(ends(True), want, "bits, csdf, gi, bodies' lo, bodies' flags")


# ---------------------------------------------------------------- 4. contexts come and go
def test_create_destroy(rv, atlas):
    """20 contexts of a 16^3 world with a 16 x 16 frame, one after the other, each rendering one frame: all
    20 frames are the same.  (Nothing is asserted about free device memory: the card is shared.)"""
    cam, vp = _view(rv, 16, 16, 16)
    first = None
    for k in range(20):
        r = _context(rv, atlas, 16, 16, 16)
        r.frame(cam, vp)
        got = images(rv, r)
        r.close()
        if first is None:
            first = got
        _same(got, first, k)
