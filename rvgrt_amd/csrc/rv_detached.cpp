// rv_detached.cpp -- host side of librvgrt_hip.so, part 9 of the C ABI (include/rvgrt.h): the voxels of a box
// that nothing holds any more, found and optionally cleared (rv_world_detached, rv_world_detached_info), and
// the host-only evaluation of the same query (rv_world_detached_at).  The per-word functions are in
// include/rvgrt/rv_detached.h, the kernels in rv_detached.hip.  The query reads the bits and writes nothing
// the frames read; the clear ends like an rv_world_edit of the same voxels (edit_finish, rv_edit.cpp).
#include "rv_host.h"
#include "../../include/rvgrt/rv_detached.h"

static_assert(sizeof(rv_component) == 40 && sizeof(rv_voxel_box) == 24, "rv_component / rv_voxel_box layout");

// shared with rv_fall.cpp (declared in rv_host.h): the argument check, the records' order and conversion, the
// host form of the query and the device form's opening
bool detach_args_ok(int X, int Y, int Z, const rv_voxel_box* b, int32_t flags, const void* comps, int64_t cap,
                    const uint32_t* mask, size_t mask_bytes) {
    if (!b || (flags & ~RV_DETACHED_CLEAR) || cap < 0 || (cap > 0 && !comps)) return false;
    if (!voxel_box_ok(X, Y, Z, *b)) return false;
    const uint64_t V = (uint64_t)(b->x1 - b->x0) * (uint64_t)(b->y1 - b->y0) * (uint64_t)(b->z1 - b->z0);
    if (V > RV_DETACHED_MAX_VOXELS) return false;
    return !mask || mask_bytes >= 4 * ((V + 31) / 32);
}

// the slots of nc records in ascending order of their seeds
std::vector<uint32_t> detach_seed_order(const DetachRec* rec, uint32_t nc) {
    std::vector<uint32_t> order(nc);
    for (uint32_t i = 0; i < nc; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t p, uint32_t q) { return rec[p].seed < rec[q].seed; });
    return order;
}

// one box-local record as rv_component in window coordinates
rv_component detach_component(const DetachBox& b, const DetachRec& r) {
    const rv_voxel_box v = detach_rec_box(b, r);
    const uint32_t n = r.seed;
    return rv_component{{v.x0, v.y0, v.z0}, {v.x1, v.y1, v.z1},
                        {b.x0 + (int32_t)(n % (uint32_t)b.nx), b.y0 + (int32_t)(n / (uint32_t)b.nx % (uint32_t)b.ny),
                         b.z0 + (int32_t)(n / (uint32_t)b.nx / (uint32_t)b.ny)},
                        r.voxels};
}

// The kernels' passes, word after word: gather, init, merge, flatten (roots take their slots), stats.  mask
// may be NULL.
void detach_host_query(const LinearWorld& w, const DetachBox& b, uint32_t* mask, DetachHost& q) {
    const uint32_t V = b.voxels(), NW = b.words();
    std::vector<uint32_t>&W = q.W, &D = q.D, &L = q.L, &slot = q.slot;
    std::vector<DetachRec>& rec = q.rec;
    W.assign(NW, 0); D.assign(NW, 0); L.assign((size_t)V + 1, 0); slot.assign(V, 0); rec.clear();
    for (uint32_t g = 0; g < NW; g++) W[g] = detach_gather_word(w, b, g);
    L[0] = 0;
    for (uint32_t g = 0; g < NW; g++) detach_init_word(L.data(), detach_word(b, g), W[g]);
    for (uint32_t g = 0; g < NW; g++) detach_merge_word(w, b, W.data(), L.data(), g);
    if (mask) std::memset(mask, 0, (size_t)((V + 31) / 32) * 4);
    q.voxels = 0;
    for (int pass = 0; pass < 2; pass++)   // flatten (roots take their slots), then stats
        for (uint32_t g = 0; g < NW; g++) {
            const DetachWord d = detach_word(b, g);
            uint32_t m = W[g], s, len;
            while (detach_next_run(m, s, len)) {
                const uint32_t p = d.base + s;
                if (pass == 0) {
                    const uint32_t r = detach_find(L.data(), p);
                    for (uint32_t k = 0; k < len; k++) L[p + k] = r;
                    if (r == p) {
                        slot[p - 1] = (uint32_t)rec.size();
                        rec.push_back(DetachRec{0, {~0u, ~0u, ~0u}, {0, 0, 0}, p - 1});
                    }
                    continue;
                }
                const uint32_t r = L[p];
                if (r == 0) continue;
                q.voxels += len;
                D[g] |= detach_low_bits(len) << s;
                if (mask)
                    for (uint32_t k = 0; k < len; k++) mask[(p - 1 + k) >> 5] |= 1u << ((p - 1 + k) & 31u);
                DetachRec& t = rec[slot[r - 1]];
                const uint32_t lo[3] = {32u * (uint32_t)d.wx + s, (uint32_t)d.yl, (uint32_t)d.zl};
                t.voxels += len;
                for (int a = 0; a < 3; a++) {
                    t.lo[a] = std::min(t.lo[a], lo[a]);
                    t.hi[a] = std::max(t.hi[a], a == 0 ? lo[0] + len - 1 : lo[a]);
                }
            }
        }
}

rv_status detach_run_query(rv_ctx* c, const DetachBox& b, size_t extra_dwords, uint32_t cnt[2]) {
    const DetachLayout l = detach_layout(b);
    if (rv_status s = c->detach_scratch.reserve(c, (l.total + extra_dwords) * 4)) return s;
    // the last world write may have been issued on another stream
    if (c->world_stream != c->stream) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_world, 0));
    launch_detach_query(c->stream, current_world(c), b, c->detach_scratch);
    LAUNCH_CHECK(c);
    HIP_TRY(c, hipMemcpyAsync(cnt, c->detach_scratch + l.cnt, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RV_OK;
}

rv_status detach_copy_records(rv_ctx* c, const DetachBox& b, uint32_t nc) {
    c->detach_h.resize(nc);
    if (nc)
        HIP_TRY(c, hipMemcpyAsync(c->detach_h.data(), c->detach_scratch + detach_layout(b).rec, nc * sizeof(DetachRec),
                                  hipMemcpyDeviceToHost, c->stream));
    return RV_OK;
}

namespace {

// The nc records in ascending order of their seeds as rv_component: the first min(cap, nc) of them.
void write_components(const DetachBox& b, const DetachRec* rec, uint32_t nc, rv_component* comps, int64_t cap) {
    const std::vector<uint32_t> order = detach_seed_order(rec, nc);
    for (int64_t i = 0; i < std::min<int64_t>(cap, nc); i++) comps[i] = detach_component(b, rec[order[i]]);
}

}  // namespace

extern "C" {

rv_status rv_world_detached(rv_ctx* c, const rv_voxel_box* box, int32_t flags, rv_component* comps, int64_t cap,
                            int64_t* n_comps, uint64_t* n_voxels, uint32_t* mask, size_t mask_bytes) {
    if (!c) return RV_ERR_INVALID;
    if (!detach_args_ok(1 << c->lx, 1 << c->ly, 1 << c->lz, box, flags, comps, cap, mask, mask_bytes))
        return fail(c, RV_ERR_INVALID, "rv_world_detached: bad box, flags, cap or array");
    if (!c->world_ready) return fail(c, RV_ERR_STATE, "rv_world_detached before a world build or import");
    const DetachBox b = detach_box(*box);
    const DetachLayout l = detach_layout(b);
    const uint32_t V = b.voxels();
    uint32_t cnt[2] = {0, 0};   // components, detached voxels
    if (rv_status s = detach_run_query(c, b, 0, cnt)) return s;
    const uint32_t nc = cnt[0];
    if (rv_status s = detach_copy_records(c, b, nc)) return s;
    if (mask)
        HIP_TRY(c, hipMemcpyAsync(mask, c->detach_scratch + l.mask, (size_t)((V + 31) / 32) * 4, hipMemcpyDeviceToHost,
                                  c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const DetachRec* rec = c->detach_h.data();
    write_components(b, rec, nc, comps, cap);
    if (n_comps) *n_comps = nc;
    if (n_voxels) *n_voxels = cnt[1];
    c->detach_calls++;
    c->detach_scanned += V;

    rv_status st = RV_OK;
    if ((flags & RV_DETACHED_CLEAR) && cnt[1]) {
        // the voxel box of everything detached, and the columns under each component for persistence
        rv_voxel_box all = empty_box();
        for (uint32_t i = 0; i < nc; i++) box_include(all, detach_rec_box(b, rec[i]));
        if (rv_status ws = wait_all_frames(c)) return ws;
        launch_detach_clear(c->stream, c->brick, current_world(c), b, c->detach_scratch + l.D, all);
        LAUNCH_CHECK(c);
        for (uint32_t i = 0; i < nc; i++) persist_mark(c, columns_under(detach_rec_box(b, rec[i])));
        c->detach_cleared += cnt[1];
        st = edit_finish(c, all);   // waits for the clear as well
    }
    c->detach_scratch.trim(EDIT_SCRATCH_KEEP);
    return st;
}

rv_status rv_world_detached_info(rv_ctx* c, uint64_t* calls, uint64_t* voxels_scanned, uint64_t* voxels_cleared) {
    if (!c) return RV_ERR_INVALID;
    if (calls) *calls = c->detach_calls;
    if (voxels_scanned) *voxels_scanned = c->detach_scanned;
    if (voxels_cleared) *voxels_cleared = c->detach_cleared;
    return RV_OK;
}

rv_status rv_world_detached_at(int32_t log2_x, int32_t log2_y, int32_t log2_z, const uint32_t* bits,
                               const rv_voxel_box* box, rv_component* comps, int64_t cap, int64_t* n_comps,
                               uint64_t* n_voxels, uint32_t* mask, size_t mask_bytes) {
    if (!linear_dims_ok(log2_x, log2_y, log2_z) || !bits) return RV_ERR_INVALID;
    if (!detach_args_ok(1 << log2_x, 1 << log2_y, 1 << log2_z, box, 0, comps, cap, mask, mask_bytes)) return RV_ERR_INVALID;
    const LinearWorld w = linear_world(log2_x, log2_y, log2_z, bits, nullptr);
    const DetachBox b = detach_box(*box);
    DetachHost q;
    detach_host_query(w, b, mask, q);
    const uint32_t nc = (uint32_t)q.rec.size();
    write_components(b, q.rec.data(), nc, comps, cap);
    if (n_comps) *n_comps = nc;
    if (n_voxels) *n_voxels = q.voxels;
    return RV_OK;
}

}  // extern "C"
