// rv_fall.cpp -- host side of librvgrt_hip.so, part 10 of the C ABI (include/rvgrt.h): the detached components
// of a box dropped in place as rigid bodies (rv_world_fall, rv_world_fall_info) and the host-only evaluation
// of the same move (rv_world_fall_at).  The query is rv_world_detached's (launch_detach_query, unchanged);
// the clearance scan is in include/rvgrt/rv_fall.h, the kernels in rv_fall.hip.  A call that moves something
// ends like an rv_world_edit of the same voxels (edit_finish, rv_edit.cpp).
#include "rv_host.h"
#include "../../include/rvgrt/rv_fall.h"

static_assert(sizeof(rv_fallen) == 48, "rv_fallen layout");

namespace {

bool args_ok(int X, int Y, int Z, const rv_voxel_box* b, int32_t max_fall, const rv_fallen* comps, int64_t cap) {
    return detach_args_ok(X, Y, Z, b, 0, comps, cap, nullptr, 0) && max_fall >= 0 && max_fall <= Y;
}

// The nc components (records and clearances by slot) in ascending order of their seeds: the first
// min(cap, nc) as rv_fallen.  Returns the voxel box of every cleared and every set voxel (nc > 0).
rv_voxel_box write_fallen(const DetachBox& b, const DetachRec* rec, const uint32_t* clearance, uint32_t nc,
                          int32_t max_fall, rv_fallen* comps, int64_t cap) {
    const std::vector<uint32_t> order = detach_seed_order(rec, nc);
    rv_voxel_box all = empty_box();
    for (uint32_t i = 0; i < nc; i++) {
        const uint32_t sl = order[i];
        const int32_t fall = (int32_t)fall_rows(clearance[sl], max_fall);
        rv_voxel_box v = detach_rec_box(b, rec[sl]);
        v.y0 -= fall;
        box_include(all, v);
        if ((int64_t)i < cap) {
            comps[i].comp = detach_component(b, rec[sl]);
            comps[i].fall = fall;
            comps[i].flags = fall_stopped(clearance[sl], max_fall) ? RV_FALL_STOPPED : 0u;
        }
    }
    return all;
}

}  // namespace

extern "C" {

rv_status rv_world_fall(rv_ctx* c, const rv_voxel_box* box, int32_t max_fall, rv_fallen* comps, int64_t cap,
                        int64_t* n_comps, uint64_t* n_voxels, rv_voxel_box* changed) {
    if (!c) return RV_ERR_INVALID;
    if (!args_ok(1 << c->lx, 1 << c->ly, 1 << c->lz, box, max_fall, comps, cap))
        return fail(c, RV_ERR_INVALID, "rv_world_fall: bad box, max_fall, cap or array");
    if (!c->world_ready) return fail(c, RV_ERR_STATE, "rv_world_fall before a world build or import");
    const DetachBox b = detach_box(*box);
    const DetachLayout l = detach_layout(b);
    // behind the query's scratch, one clearance dword per component: at most ceil(V / 2)
    uint32_t cnt[2] = {0, 0};   // components, detached voxels
    if (rv_status s = detach_run_query(c, b, detach_up64((b.voxels() + 1) / 2), cnt)) return s;
    uint32_t* clearance = c->detach_scratch + l.total;
    const World w = current_world(c);
    const uint32_t nc = cnt[0];
    if (n_comps) *n_comps = nc;
    if (n_voxels) *n_voxels = cnt[1];
    c->fall_calls++;
    if (changed) *changed = rv_voxel_box{0, 0, 0, 0, 0, 0};
    rv_status st = RV_OK;
    if (nc) {
        launch_fall_clearance(c->stream, w, b, c->detach_scratch, nc, max_fall, clearance);
        LAUNCH_CHECK(c);
        c->fall_h.resize(nc);
        if (rv_status s = detach_copy_records(c, b, nc)) return s;
        HIP_TRY(c, hipMemcpyAsync(c->fall_h.data(), clearance, (size_t)nc * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        const DetachRec* rec = c->detach_h.data();
        const rv_voxel_box all = write_fallen(b, rec, c->fall_h.data(), nc, max_fall, comps, cap);
        if (changed) *changed = all;
        // what is cleared lies inside B; what is set may lie below it
        rv_voxel_box cleared = empty_box();
        for (uint32_t i = 0; i < nc; i++) box_include(cleared, detach_rec_box(b, rec[i]));
        if (rv_status ws = wait_all_frames(c)) return ws;
        launch_detach_clear(c->stream, c->brick, w, b, c->detach_scratch + l.D, cleared);
        launch_fall_stamp(c->stream, c->brick, w, b, c->detach_scratch, max_fall, clearance);
        LAUNCH_CHECK(c);
        for (uint32_t i = 0; i < nc; i++)   // x and z do not change in a fall
            persist_mark(c, columns_under(detach_rec_box(b, rec[i])));
        c->fall_comps += nc;
        c->fall_voxels += cnt[1];
        st = edit_finish(c, all);   // waits for the clear and the stamp as well
    }
    c->detach_scratch.trim(EDIT_SCRATCH_KEEP);
    return st;
}

rv_status rv_world_fall_info(rv_ctx* c, uint64_t* calls, uint64_t* components_moved, uint64_t* voxels_moved) {
    if (!c) return RV_ERR_INVALID;
    if (calls) *calls = c->fall_calls;
    if (components_moved) *components_moved = c->fall_comps;
    if (voxels_moved) *voxels_moved = c->fall_voxels;
    return RV_OK;
}

rv_status rv_world_fall_at(int32_t log2_x, int32_t log2_y, int32_t log2_z, const uint32_t* bits, const rv_voxel_box* box,
                           int32_t max_fall, rv_fallen* comps, int64_t cap, int64_t* n_comps, uint64_t* n_voxels,
                           rv_voxel_box* changed, uint32_t* bits_out, size_t bits_bytes) {
    if (!linear_dims_ok(log2_x, log2_y, log2_z) || !bits) return RV_ERR_INVALID;
    if (!args_ok(1 << log2_x, 1 << log2_y, 1 << log2_z, box, max_fall, comps, cap)) return RV_ERR_INVALID;
    const size_t world_bytes = ((size_t)1 << (log2_x + log2_y + log2_z)) / 8;
    if (bits_out && bits_bytes < world_bytes) return RV_ERR_INVALID;
    const LinearWorld w = linear_world(log2_x, log2_y, log2_z, bits, nullptr);
    const DetachBox b = detach_box(*box);
    DetachHost q;
    detach_host_query(w, b, nullptr, q);
    const uint32_t nc = (uint32_t)q.rec.size(), NW = b.words();
    // the clearance kernel's scan, word after word and run after run
    std::vector<uint32_t> clearance(nc, FALL_NONE);
    const uint32_t limit = fall_scan_limit(max_fall);
    for (uint32_t g = 0; g < NW; g++) {
        const DetachWord d = detach_word(b, g);
        uint32_t m = q.D[g], s, len;
        while (detach_next_run(m, s, len)) {
            const uint32_t r = q.L[d.base + s];
            uint32_t* best = clearance.data() + q.slot[r - 1];
            const uint32_t v = fall_run_clearance(w, b, q.W.data(), q.L.data(), d, g, s, len, r, limit, best);
            *best = std::min(*best, v);
        }
    }
    const rv_voxel_box all = write_fallen(b, q.rec.data(), clearance.data(), nc, max_fall, comps, cap);
    if (changed) *changed = nc ? all : rv_voxel_box{0, 0, 0, 0, 0, 0};
    if (n_comps) *n_comps = nc;
    if (n_voxels) *n_voxels = q.voxels;
    if (!bits_out) return RV_OK;
    // everything above read `bits`; from here on bits_out, which may be the same array, is written: the
    // clear of every detached voxel, then the stamp
    if (bits_out != bits) std::memcpy(bits_out, bits, world_bytes);
    auto word_of = [&](int x, int y, int z) { return bits_out + voxel_word_off(w, (uint32_t)x, (uint32_t)y, (uint32_t)z) / 4; };
    for (int pass = 0; pass < 2; pass++)
        for (uint32_t g = 0; g < NW; g++) {
            const DetachWord d = detach_word(b, g);
            uint32_t m = q.D[g], s, len;
            while (detach_next_run(m, s, len)) {
                const int fall = pass ? (int)fall_rows(clearance[q.slot[q.L[d.base + s] - 1]], max_fall) : 0;
                const int y = b.y0 + d.yl - fall, z = b.z0 + d.zl;
                for (uint32_t k = 0; k < len; k++) {
                    const int x = b.x0 + 32 * d.wx + (int)(s + k);
                    if (pass) *word_of(x, y, z) |= 1u << (x & 31);
                    else *word_of(x, y, z) &= ~(1u << (x & 31));
                }
            }
        }
    return RV_OK;
}

}  // extern "C"
