// rv_scroll.cpp -- host side of librvgrt_hip.so, part 6 of the C ABI (include/rvgrt.h): the world window
// moved over the generated terrain in place (rv_world_scroll, rv_world_scroll_info), the host-only plan of
// the CSDF cells a one-axis step rebuilds (rv_world_scroll_region) and the camera / VP matrices re-expressed
// in the moved grid (rv_scroll_view), and the texture origin that can follow the window (rv_texture_origin_set,
// rv_texture_follow_scroll, rv_texture_origin_get, the test hooks rv_texture_tiles and rv_texture_tile_at).
// The kernels are in rv_scroll.hip.
#include "rv_host.h"

namespace {

// What a one-axis step by d voxels (a multiple of 8, d != 0) rebuilds of the CSDF.
//
// With k = |d| / 2 coarse cells and d > 0 along x: the shifted old bytes were built with the solidity known
// on the new coordinates [-k, SX - k) and none outside; a whole-grid build of the new window knows it on
// [0, SX) (the passes skip a cell outside the world, which is the same as a non-solid one).  So the
// solidity "changes" in [-k, 0), the planes that left, and in [SX - k, SX), the planes that entered, and by
// the argument of rv_edit.cpp the final byte can differ only within 64 cells of either:
//   trailing  [0, 64)             E = the empty range at the face the old planes left through
//   leading   [SX - k - 64, SX)   E = the entering planes
// each over all of y and z, with the nested input boxes of csdf_boxes.  d < 0 mirrors the two.  Along z the
// boxes are the same with z for x, except that dx and dy, which the scratch never keeps, are needed over the
// whole 128-plane input slab of the final pass (csdf_boxes' ry, rx).
//
// full: the two slabs touch or overlap, or the local passes would visit at least as many cells as the four
// whole-grid passes, counted by the x axis' figure for either axis: (640 + 4k) planes against 4 S (at
// equality the proven path).  A z step's passes visit (896 + 4k) planes -- the wider dx / dy boxes -- so
// between k = S - 224 and the crossover it visits up to a quarter more than the whole build would; the
// bytes are the same either way.  |d| >= the axis: every voxel enters, full.
struct ScrollPlan {
    int k = 0;             // coarse cells of the step
    bool all = false;      // |d| >= the axis: nothing is retained
    bool full = false;
    CsdfBoxes slab[2];     // trailing, leading (local path)
    uint64_t cells = 0;    // final bytes recomputed
};

ScrollPlan scroll_plan(int lx, int ly, int lz, int axis, int64_t d) {
    ScrollPlan p;
    const int S[3] = {1 << (lx - 1), 1 << (ly - 1), 1 << (lz - 1)};
    const int64_t ad = d < 0 ? -d : d;
    const uint64_t whole = (uint64_t)S[0] * (uint64_t)S[1] * (uint64_t)S[2];
    p.all = ad >= 2 * (int64_t)S[axis];
    p.k = p.all ? S[axis] : (int)(ad / 2);
    p.full = p.all;
    if (!p.full) {
        int t0[3] = {0, 0, 0}, t1[3] = {S[0], S[1], S[2]}, l0[3] = {0, 0, 0}, l1[3] = {S[0], S[1], S[2]};
        if (d > 0) {
            t0[axis] = t1[axis] = 0;
            l0[axis] = S[axis] - p.k;
        } else {
            t0[axis] = t1[axis] = S[axis];
            l1[axis] = p.k;
        }
        p.slab[0] = csdf_boxes(t0, t1, S);
        p.slab[1] = csdf_boxes(l0, l1, S);
        const CellBox &a = p.slab[0].rf, &b = p.slab[1].rf;
        const int a0 = axis == 0 ? a.x0 : a.z0, a1 = a0 + (axis == 0 ? a.nx : a.nz);
        const int b0 = axis == 0 ? b.x0 : b.z0, b1 = b0 + (axis == 0 ? b.nx : b.nz);
        const bool touch = d > 0 ? b0 <= a1 : a0 <= b1;
        p.full = touch || 640 + 4 * (int64_t)p.k >= 4 * (int64_t)S[axis];
        p.cells = a.cells() + b.cells();
    }
    if (p.full) p.cells = whole;
    return p;
}

void box_out(const CellBox& b, int32_t r[6]) {
    r[0] = b.x0; r[1] = b.x0 + b.nx;
    r[2] = b.y0; r[3] = b.y0 + b.ny;
    r[4] = b.z0; r[5] = b.z0 + b.nz;
}

bool origin_ok(int64_t o, int64_t d, int64_t dim) {
    return o + d >= INT32_MIN && o + d + dim <= INT32_MAX;
}
// A texture origin (o + d along an axis of dim voxels) whose every lattice point fits an int: the second
// point of sampleTexture lies up to `reach` (1322 along x, 722 along z: the offset + the carry) further on
bool tex_origin_ok(int64_t o, int64_t d, int64_t dim, int64_t reach) {
    return o + d >= INT32_MIN && o + d + dim + reach <= INT32_MAX;
}
constexpr int64_t TEX_REACH_X = 1322, TEX_REACH_Z = 722;

// One step: the window moves by d voxels along `axis` (validated: a multiple of 8, not 0, no overflow).
rv_status scroll_axis(rv_ctx* c, int axis, int d, uint64_t* cells, int* full) {
    const World& w = c->w;
    const int dim = axis == 0 ? w.X : w.Z;
    const ScrollPlan p = scroll_plan(c->lx, c->ly, c->lz, axis, d);
    const int nb = d / 8, NB = dim / 8, ab = p.all ? NB : (nb < 0 ? -nb : nb);   // bricks that enter: ab of NB
    const int NBX = w.X / 8, NBY = w.Y / 8, NBZ = w.Z / 8;

    // the scratch copy of the retained brick records (128 B each; the GI cells' 32 B per brick reuse it),
    // before anything is written: a failed allocation leaves the world as it was
    const size_t kept = (size_t)(NB - ab) * (size_t)(axis == 0 ? NBZ : NBX) * (size_t)NBY;
    if (rv_status s = c->scroll_tmp.reserve(c, kept * 128)) return s;
    // persistence: the brick columns that leave (old window) and those that enter (new window), and the
    // staging for the dirty ones among the former and the stored ones among the latter, reserved here too
    ColumnRange col_leave{0, NBX, 0, NBZ}, col_enter = col_leave;
    (axis == 0 ? col_leave.bx0 : col_leave.bz0) = d > 0 ? 0 : NB - ab;
    (axis == 0 ? col_leave.bx1 : col_leave.bz1) = d > 0 ? ab : NB;
    (axis == 0 ? col_enter.bx0 : col_enter.bz0) = d > 0 ? NB - ab : 0;
    (axis == 0 ? col_enter.bx1 : col_enter.bz1) = d > 0 ? NB : ab;
    if (c->persist) {
        const int32_t ox = c->cfg.seed_x, oz = c->cfg.seed_z;
        const size_t nl = persist_dirty_in(c, col_leave, ox, oz);
        const size_t ne = persist_stored_in(c, col_enter, ox + (axis == 0 ? d : 0), oz + (axis == 2 ? d : 0));
        if (rv_status s = persist_reserve(c, std::max(nl, ne))) return s;
    }

    c->geom_ver++;
    if (rv_status s = persist_capture(c, col_leave, false)) return s;   // before the retained bricks move
    if (!p.all) {
        launch_scroll_bricks(c->stream, c->brick, current_world(c), axis, nb, c->scroll_tmp);
        LAUNCH_CHECK(c);
    }
    // the entering slab, generated at the new origin
    (axis == 0 ? c->cfg.seed_x : c->cfg.seed_z) += d;
    CellBox slab{0, 0, 0, NBX, NBY, NBZ};
    (axis == 0 ? slab.nx : slab.nz) = ab;
    if (d > 0) (axis == 0 ? slab.x0 : slab.z0) = NB - ab;
    launch_fill_box(c->stream, c->brick, current_world(c), slab, c->cfg.seed_x, c->cfg.seed_z);
    LAUNCH_CHECK(c);
    // persistence: the stored columns of the slab take their saved bits; the exits, the CSDF slabs, the
    // entering GI cells and the tile table below all see the final bits
    if (rv_status s = persist_restore(c, col_enter)) return s;
    if (rv_status ts = world_top(c)) return ts;   // the exits, from the bits
    if (p.full) {
        if (rv_status s = rv_csdf_build(c)) return s;
    } else {
        if (rv_status s = csdf_rebuild_boxes(c, p.slab, 2)) return s;
    }

    // the GI grid: retained cells to their new index, then the entering cells against the final voxels and CSDF
    const int g = d / 4, G = dim / 4, ag = p.all ? G : (g < 0 ? -g : g);
    CellBox keep{0, 0, 0, w.GX, w.GY, w.GZ}, enter = keep;
    (axis == 0 ? keep.nx : keep.nz) = G - ag;
    (axis == 0 ? enter.nx : enter.nz) = ag;
    if (d > 0) (axis == 0 ? enter.x0 : enter.z0) = G - ag;
    else (axis == 0 ? keep.x0 : keep.z0) = ag;
    if (!p.all) {
        launch_scroll_gi(c->stream, c->gi, current_world(c), keep, axis == 0 ? g : 0, axis == 2 ? g : 0, c->scroll_tmp);
        LAUNCH_CHECK(c);
    }
    launch_scroll_gi_init(c->stream, c->gi, current_world(c), sun_dir(), enter,
                          c->cfg.gi_init_saturate ? RV_GI_LIT_SATURATE : RV_GI_LIT_REFERENCE,
                          c->counters + ST_GI * NCNT);
    LAUNCH_CHECK(c);
    // the texture origin follows the window: the retained table entries to their new index, the entering
    // ones at the new origin (rows below tex_ny, which a scroll keeps); without a table only the origin moves
    if (c->tex_follow) {
        (axis == 0 ? c->w.tex_ox : c->w.tex_oz) += d;
        if (c->tex) {
            if (p.all) {
                launch_tex_table(c->stream, c->tex, c->w);
            } else {
                launch_scroll_tex(c->stream, c->tex, c->w, axis, nb);
                slab.ny = (int)(w.tex_ny >> 3);
                launch_tex_box(c->stream, c->tex, c->w, slab);
            }
            LAUNCH_CHECK(c);
        }
    }
    if (rv_status ms = mark_world(c)) return ms;
    *cells += p.cells;
    *full |= p.full ? 1 : 0;
    return RV_OK;
}

}  // namespace

extern "C" {

rv_status rv_world_scroll_region(int32_t log2_x, int32_t log2_y, int32_t log2_z, int32_t axis, int32_t d,
                                 int32_t region[2][6], uint64_t* cells, int32_t* full) {
    if (!region || !dims_ok(log2_x, log2_y, log2_z) || (axis != 0 && axis != 2) || d % 8 != 0) return RV_ERR_INVALID;
    for (int i = 0; i < 6; i++) region[0][i] = region[1][i] = 0;
    if (cells) *cells = 0;
    if (full) *full = 0;
    if (d == 0) return RV_OK;
    const ScrollPlan p = scroll_plan(log2_x, log2_y, log2_z, axis, d);
    if (p.full) {
        box_out(CellBox{0, 0, 0, 1 << (log2_x - 1), 1 << (log2_y - 1), 1 << (log2_z - 1)}, region[0]);
    } else {
        box_out(p.slab[0].rf, region[0]);
        box_out(p.slab[1].rf, region[1]);
    }
    if (cells) *cells = p.cells;
    if (full) *full = p.full ? 1 : 0;
    return RV_OK;
}

rv_status rv_world_scroll(rv_ctx* c, int32_t dx, int32_t dz) {
    if (!c) return RV_ERR_INVALID;
    if (dx % 8 != 0 || dz % 8 != 0) return fail(c, RV_ERR_INVALID, "rv_world_scroll: dx, dz must be multiples of 8");
    if (!origin_ok(c->cfg.seed_x, dx, c->w.X) || !origin_ok(c->cfg.seed_z, dz, c->w.Z))
        return fail(c, RV_ERR_INVALID, "rv_world_scroll: the window's origin would leave the int32 range");
    if (c->tex_follow && (!tex_origin_ok(c->w.tex_ox, dx, c->w.X, TEX_REACH_X) ||
                          !tex_origin_ok(c->w.tex_oz, dz, c->w.Z, TEX_REACH_Z)))
        return fail(c, RV_ERR_INVALID, "rv_world_scroll: the texture origin would leave the int32 range");
    if (!c->world_ready) return fail(c, RV_ERR_STATE, "rv_world_scroll before a world build or import");
    if (dx == 0 && dz == 0) return RV_OK;
    if (rv_status ws = wait_all_frames(c)) return ws;
    // work computed ahead read the old window (the version bumps below would also reject it)
    c->spec_gi = false;
    c->carry_gi = c->carry_pp = false;
    uint64_t cells = 0;
    int full = 0;
    rv_status s = RV_OK;
    if (dx != 0) s = scroll_axis(c, 0, dx, &cells, &full);
    if (s == RV_OK && dz != 0) s = scroll_axis(c, 2, dz, &cells, &full);
    const hipError_t se = hipStreamSynchronize(c->stream);
    c->scroll_tmp.trim(EDIT_SCRATCH_KEEP);
    persist_trim(c);
    if (s != RV_OK) return s;
    HIP_TRY(c, se);
    c->scroll_count++;
    c->scroll_cells = cells;
    c->scroll_full = full;
    return RV_OK;
}

rv_status rv_world_scroll_info(rv_ctx* c, uint64_t* scrolls, uint64_t* csdf_cells, int32_t* last_full,
                               int32_t* origin_x, int32_t* origin_z) {
    if (!c) return RV_ERR_INVALID;
    if (scrolls) *scrolls = c->scroll_count;
    if (csdf_cells) *csdf_cells = c->scroll_cells;
    if (last_full) *last_full = c->scroll_full;
    if (origin_x) *origin_x = c->cfg.seed_x;
    if (origin_z) *origin_z = c->cfg.seed_z;
    return RV_OK;
}

rv_status rv_texture_origin_set(rv_ctx* c, int32_t ox, int32_t oz) {
    if (!c) return RV_ERR_INVALID;
    if (!tex_origin_ok(ox, 0, c->w.X, TEX_REACH_X) || !tex_origin_ok(oz, 0, c->w.Z, TEX_REACH_Z))
        return fail(c, RV_ERR_INVALID, "rv_texture_origin_set: a lattice point would leave the int32 range");
    if (ox == c->w.tex_ox && oz == c->w.tex_oz) return RV_OK;
    if (rv_status ws = wait_all_frames(c)) return ws;
    // work computed ahead sampled the old textures (the GI update multiplies a bounce hit's colour by them)
    c->spec_gi = false;
    c->carry_gi = c->carry_pp = false;
    c->w.tex_ox = ox;
    c->w.tex_oz = oz;
    if (c->tex) {   // (not built yet: tex_table builds it at this origin)
        launch_tex_table(c->stream, c->tex, c->w);
        LAUNCH_CHECK(c);
    }
    if (rv_status ms = mark_world(c)) return ms;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RV_OK;
}

rv_status rv_texture_follow_scroll(rv_ctx* c, int32_t on) {
    if (!c) return RV_ERR_INVALID;
    c->tex_follow = on != 0;
    return RV_OK;
}

rv_status rv_texture_origin_get(rv_ctx* c, int32_t* ox, int32_t* oz, int32_t* follow) {
    if (!c) return RV_ERR_INVALID;
    if (ox) *ox = c->w.tex_ox;
    if (oz) *oz = c->w.tex_oz;
    if (follow) *follow = c->tex_follow ? 1 : 0;
    return RV_OK;
}

rv_status rv_texture_tiles(rv_ctx* c, const float* pos, int64_t n, uint8_t* tiles) {
    if (!c || n < 0 || (n > 0 && (!pos || !tiles))) return RV_ERR_INVALID;
    if (!c->world_ready) return fail(c, RV_ERR_STATE, "rv_texture_tiles before a world build or import");
    if (n == 0) return RV_OK;
    if (rv_status ws = wait_all_frames(c)) return ws;
    DevBuf<float> dp;
    DevBuf<uint8_t> dt;
    if (rv_status s = dp.reserve(c, (size_t)n * 12)) return s;
    if (dt.reserve(c, (size_t)n)) return fail(c, RV_ERR_OOM, "rv_texture_tiles: out of device memory");
    hipError_t e = hipMemcpyAsync(dp, pos, (size_t)n * 12, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        launch_texture_tiles(c->stream, current_world(c), dp, n, dt);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(tiles, dt, (size_t)n, hipMemcpyDeviceToHost, c->stream);
    const hipError_t se = hipStreamSynchronize(c->stream);   // before dp and dt go
    HIP_TRY(c, e);
    HIP_TRY(c, se);
    return RV_OK;
}

rv_status rv_texture_tile_at(int32_t ox, int32_t oz, const float* pos, int64_t n, uint8_t* tiles) {
    if (n < 0 || (n > 0 && (!pos || !tiles)) || !tex_origin_ok(ox, 0, 0, TEX_REACH_X) ||
        !tex_origin_ok(oz, 0, 0, TEX_REACH_Z))
        return RV_ERR_INVALID;
    World w{};   // no table: the noise, as a frame kernel evaluates it outside the table
    w.tex_ox = ox;
    w.tex_oz = oz;
    for (int64_t i = 0; i < n; i++)
        tiles[i] = (uint8_t)texture_tile(w, host_v(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]));
    return RV_OK;
}

rv_status rv_scroll_view(int32_t dx, int32_t dz, rv_camera* cam, float* vp16, float* prev_vp16) {
    if (cam) {
        cam->pos[0] = (float)((double)cam->pos[0] - (double)dx);
        cam->pos[2] = (float)((double)cam->pos[2] - (double)dz);
    }
    float* const m[2] = {vp16, prev_vp16};
    for (float* v : m) {
        if (!v) continue;
        for (int i = 0; i < 4; i++)   // VP . T(dx, 0, dz): column 3 += dx column 0 + dz column 2
            v[12 + i] = (float)((double)v[12 + i] + (double)dx * (double)v[i] + (double)dz * (double)v[8 + i]);
    }
    return RV_OK;
}

}  // extern "C"
