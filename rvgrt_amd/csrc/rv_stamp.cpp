// rv_stamp.cpp -- host side of librvgrt_hip.so, part 12 of the C ABI (include/rvgrt.h): patterns kept on the
// device (rv_pattern_create, rv_pattern_capture, rv_pattern_read, rv_pattern_destroy), their stamps
// (rv_world_stamp, rv_world_stamp_info) and the host-only forms (rv_world_stamp_at, rv_world_stamp_box).  The
// integer functions are in include/rvgrt/rv_stamp.h, the kernels in rv_stamp.hip.  A stamp call ends like an
// rv_world_edit over the union of the clipped boxes (edit_finish, rv_edit.cpp).
#include "rv_host.h"

static_assert(sizeof(rv_stamp) == 24, "rv_stamp layout");

namespace {

// the lowest free slot, or -1
int free_slot(const rv_ctx* c) {
    for (int i = 0; i < RV_PATTERN_MAX; i++)
        if (!c->patterns[i].live()) return i;
    return -1;
}

bool live_id(const rv_ctx* c, int32_t id) { return id >= 0 && id < RV_PATTERN_MAX && c->patterns[id].live(); }

// the slot is free: its allocations go when they are large, or at once (after a failure)
void pattern_release(rv_ctx::Pattern& p, size_t keep) {
    p.on = false;
    p.a.trim(keep);
    p.t.trim(keep);
}

// both layouts of the free slot `id` allocated for these dims (what a destroyed pattern left there is used when
// it is large enough); the slot stays free until pattern_finish
rv_status pattern_alloc(rv_ctx* c, int id, int32_t nx, int32_t ny, int32_t nz) {
    rv_ctx::Pattern& p = c->patterns[id];
    rv_status s = p.a.reserve(c, (size_t)pattern_words(nx, ny, nz) * 4);
    if (!s) s = p.t.reserve(c, (size_t)pattern_words(nz, ny, nx) * 4);
    if (s) { pattern_release(p, 0); return s; }
    p.nx = nx; p.ny = ny; p.nz = nz;
    return RV_OK;
}

// the second layout from the first, then the wait that ends every pattern call; the slot is live after it
rv_status pattern_finish(rv_ctx* c, int id) {
    rv_ctx::Pattern& p = c->patterns[id];
    launch_pattern_transpose(c->stream, p.a, p.nx, p.ny, p.nz, p.t);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        pattern_release(p, 0);
        return fail(c, RV_ERR_HIP, std::string("pattern upload: ") + hipGetErrorString(e));
    }
    p.on = true;
    return RV_OK;
}

// The host form's patterns: dims valid, and bits given where they are read.
bool host_patterns_ok(const rv_pattern_host* pats, int32_t npats, bool need_bits) {
    if (npats < 0 || (npats > 0 && !pats)) return false;
    for (int32_t i = 0; i < npats; i++)
        if (!pattern_dims_ok(pats[i].nx, pats[i].ny, pats[i].nz) || (need_bits && !pats[i].bits)) return false;
    return true;
}

// n stamps as rv_world_stamp takes them; live(id): whether the pattern exists
template <class Live>
bool stamps_ok(const rv_stamp* s, int32_t n, Live live) {
    if (n < 0 || n > RV_STAMP_MAX || (n > 0 && !s)) return false;
    for (int32_t i = 0; i < n; i++)
        if (!stamp_valid(s[i]) || !live(s[i].pattern)) return false;
    return true;
}

// The stamps made ready, those with a non-empty clipped box only, in order; each (n of them, may be NULL) takes
// every stamp's box, all zero for an empty one; the union is all zero when there is none.  pat(id, nx, ny, nz,
// a, t): the pattern's dims and layouts.
template <class Pat>
bool stamps_ready(int lx, int ly, int lz, const rv_stamp* s, int32_t n, Pat pat, std::vector<StampRec>* recs,
                  rv_voxel_box* each, rv_voxel_box* all) {
    const int32_t D[3] = {1 << lx, 1 << ly, 1 << lz};
    rv_voxel_box u = empty_box();
    if (recs) recs->clear();
    for (int32_t i = 0; i < n; i++) {
        int32_t nx, ny, nz;
        const uint32_t *a, *t;
        pat(s[i].pattern, nx, ny, nz, a, t);
        StampRec r;
        const bool ok = stamp_rec(s[i], nx, ny, nz, a, t, D, r);
        if (each) each[i] = r.box;
        if (!ok) continue;
        box_include(u, r.box);
        if (recs) recs->push_back(r);
    }
    const bool any = u.x1 > u.x0;
    *all = any ? u : rv_voxel_box{0, 0, 0, 0, 0, 0};
    return any;
}

}  // namespace

extern "C" {

rv_status rv_pattern_create(rv_ctx* c, int32_t nx, int32_t ny, int32_t nz, const uint32_t* bits, size_t bytes,
                            int32_t* id) {
    if (!c) return RV_ERR_INVALID;
    if (!pattern_dims_ok(nx, ny, nz) || !bits || !id || bytes < (size_t)pattern_words(nx, ny, nz) * 4)
        return fail(c, RV_ERR_INVALID, "rv_pattern_create: bad dims, bits, bytes or id pointer");
    const int slot = free_slot(c);
    if (slot < 0) return fail(c, RV_ERR_INVALID, "rv_pattern_create: RV_PATTERN_MAX patterns are live");
    // the padding bits of every row's last word are ignored: zero in the copy that is uploaded
    const uint32_t nwx = pattern_row_words(nx), nw = pattern_words(nx, ny, nz);
    std::vector<uint32_t> clean(bits, bits + nw);
    const uint32_t last = pattern_word_mask(nx, nwx - 1);
    for (uint32_t g = nwx - 1; g < nw; g += nwx) clean[g] &= last;
    if (rv_status s = pattern_alloc(c, slot, nx, ny, nz)) return s;
    hipError_t e = hipMemcpyAsync(c->patterns[slot].a, clean.data(), (size_t)nw * 4, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) {
        pattern_release(c->patterns[slot], 0);
        return fail(c, RV_ERR_HIP, std::string("rv_pattern_create: ") + hipGetErrorString(e));
    }
    if (rv_status s = pattern_finish(c, slot)) return s;   // waits: `clean` may go
    *id = slot;
    return RV_OK;
}

rv_status rv_pattern_capture(rv_ctx* c, const rv_voxel_box* box, int32_t* id) {
    if (!c) return RV_ERR_INVALID;
    if (!box || !id || !voxel_box_ok(1 << c->lx, 1 << c->ly, 1 << c->lz, *box) ||
        !pattern_dims_ok(box->x1 - box->x0, box->y1 - box->y0, box->z1 - box->z0))
        return fail(c, RV_ERR_INVALID, "rv_pattern_capture: bad box or id pointer");
    if (!c->world_ready) return fail(c, RV_ERR_STATE, "rv_pattern_capture before a world build or import");
    const int slot = free_slot(c);
    if (slot < 0) return fail(c, RV_ERR_INVALID, "rv_pattern_capture: RV_PATTERN_MAX patterns are live");
    if (rv_status s = pattern_alloc(c, slot, box->x1 - box->x0, box->y1 - box->y0, box->z1 - box->z0)) return s;
    // a query: after the last world write, which may have been issued on another stream; nothing the frames read
    // is written, no frame is waited for
    hipError_t e = c->world_stream != c->stream ? hipStreamWaitEvent(c->stream, c->ev_world, 0) : hipSuccess;
    if (e != hipSuccess) {
        pattern_release(c->patterns[slot], 0);
        return fail(c, RV_ERR_HIP, std::string("rv_pattern_capture: ") + hipGetErrorString(e));
    }
    launch_pattern_capture(c->stream, c->brick, current_world(c), *box, c->patterns[slot].a);
    if (rv_status s = pattern_finish(c, slot)) return s;
    *id = slot;
    return RV_OK;
}

rv_status rv_pattern_read(rv_ctx* c, int32_t id, int32_t dims[3], uint32_t* bits, size_t bytes) {
    if (!c) return RV_ERR_INVALID;
    if (!live_id(c, id) || !dims) return fail(c, RV_ERR_INVALID, "rv_pattern_read: no such pattern, or dims NULL");
    const rv_ctx::Pattern& p = c->patterns[id];
    const size_t need = (size_t)pattern_words(p.nx, p.ny, p.nz) * 4;
    if (bits && bytes < need) return fail(c, RV_ERR_INVALID, "rv_pattern_read: bytes below the pattern's size");
    dims[0] = p.nx; dims[1] = p.ny; dims[2] = p.nz;
    if (bits) {
        HIP_TRY(c, hipMemcpyAsync(bits, p.a, need, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return RV_OK;
}

rv_status rv_pattern_destroy(rv_ctx* c, int32_t id) {
    if (!c) return RV_ERR_INVALID;
    if (!live_id(c, id)) return fail(c, RV_ERR_INVALID, "rv_pattern_destroy: no such pattern");
    pattern_release(c->patterns[id], rv_ctx::PATTERN_KEEP);
    return RV_OK;
}

rv_status rv_world_stamp(rv_ctx* c, const rv_stamp* stamps, int32_t n, uint64_t* n_set, uint64_t* n_cleared,
                         rv_voxel_box* changed) {
    if (!c) return RV_ERR_INVALID;
    if (!c->world_ready) return fail(c, RV_ERR_STATE, "rv_world_stamp before a world build or import");
    if (!stamps_ok(stamps, n, [&](int32_t id) { return live_id(c, id); }))
        return fail(c, RV_ERR_INVALID, "rv_world_stamp: bad stamp list");
    if (n_set) *n_set = 0;
    if (n_cleared) *n_cleared = 0;
    if (changed) *changed = rv_voxel_box{0, 0, 0, 0, 0, 0};
    if (n == 0) return RV_OK;
    c->stamp_box_h.resize((size_t)n);
    rv_voxel_box u;
    const bool any = stamps_ready(c->lx, c->ly, c->lz, stamps, n,
                                  [&](int32_t id, int32_t& nx, int32_t& ny, int32_t& nz, const uint32_t*& a, const uint32_t*& t) {
                                      const rv_ctx::Pattern& p = c->patterns[id];
                                      nx = p.nx; ny = p.ny; nz = p.nz; a = p.a; t = p.t;
                                  },
                                  &c->stamp_h, c->stamp_box_h.data(), &u);   // stamp_h: the stable host copy the upload reads
    if (!any) {   // every stamp lies outside the window: nothing is launched, so nothing is waited for
        c->edit_cells = 0;
        c->edit_full = 0;
        return RV_OK;
    }
    if (changed) *changed = u;
    if (rv_status ws = wait_all_frames(c)) return ws;

    // the bits: the made-ready stamps to the device, one lane per word of the union box
    const int nrecs = (int)c->stamp_h.size();
    if (rv_status s = c->stamp_counts.reserve(c, 2 * sizeof(unsigned long long))) return s;
    if (rv_status s = c->stamp_list.reserve(c, (size_t)nrecs * sizeof(StampRec))) return s;
    HIP_TRY(c, hipMemcpyAsync(c->stamp_list, c->stamp_h.data(), (size_t)nrecs * sizeof(StampRec), hipMemcpyHostToDevice,
                              c->stream));
    HIP_TRY(c, hipMemsetAsync(c->stamp_counts, 0, 2 * sizeof(unsigned long long), c->stream));
    launch_stamp(c->stream, c->brick, current_world(c), c->stamp_list, nrecs, u, c->stamp_counts);
    LAUNCH_CHECK(c);
    unsigned long long cnt[2] = {0, 0};   // turned on, turned off
    HIP_TRY(c, hipMemcpyAsync(cnt, c->stamp_counts, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n_set) *n_set = cnt[0];
    if (n_cleared) *n_cleared = cnt[1];
    c->stamp_calls++;
    c->stamp_applied += (uint64_t)nrecs;
    c->edit_cells = 0;
    c->edit_full = 0;
    if (cnt[0] + cnt[1] == 0) return RV_OK;   // every voxel already had its value: nothing to rebuild or invalidate

    for (int i = 0; i < n; i++) {   // persistence: the columns under each non-empty clipped box
        const rv_voxel_box& b = c->stamp_box_h[(size_t)i];
        if (b.x1 > b.x0) persist_mark(c, columns_under(b));
    }
    return edit_finish(c, u);
}

rv_status rv_world_stamp_info(rv_ctx* c, uint64_t* calls, uint64_t* stamps, int32_t* patterns_live,
                              uint64_t* pattern_bytes) {
    if (!c) return RV_ERR_INVALID;
    int32_t live = 0;
    uint64_t bytes = 0;
    for (const rv_ctx::Pattern& p : c->patterns)
        if (p.live()) { live++; bytes += (uint64_t)pattern_words(p.nx, p.ny, p.nz) * 4; }
    if (calls) *calls = c->stamp_calls;
    if (stamps) *stamps = c->stamp_applied;
    if (patterns_live) *patterns_live = live;
    if (pattern_bytes) *pattern_bytes = bytes;
    return RV_OK;
}

rv_status rv_world_stamp_at(int32_t log2_x, int32_t log2_y, int32_t log2_z, uint32_t* bits, const rv_pattern_host* pats,
                            int32_t npats, const rv_stamp* stamps, int32_t n, uint64_t* n_set, uint64_t* n_cleared) {
    if (!linear_dims_ok(log2_x, log2_y, log2_z) || !bits || !host_patterns_ok(pats, npats, true) ||
        !stamps_ok(stamps, n, [&](int32_t id) { return id >= 0 && id < npats; }))
        return RV_ERR_INVALID;
    // the two layouts of every pattern a stamp names, padding bits zero, made as the device makes them
    std::vector<std::vector<uint32_t>> A((size_t)npats), T((size_t)npats);
    for (int32_t i = 0; i < n; i++) {
        const int32_t id = stamps[i].pattern;
        if (!A[(size_t)id].empty()) continue;
        const rv_pattern_host& p = pats[id];
        const uint32_t nwx = pattern_row_words(p.nx), nw = pattern_words(p.nx, p.ny, p.nz);
        std::vector<uint32_t>& a = A[(size_t)id];
        a.assign(p.bits, p.bits + nw);
        for (uint32_t g = nwx - 1; g < nw; g += nwx) a[g] &= pattern_word_mask(p.nx, nwx - 1);
        std::vector<uint32_t>& t = T[(size_t)id];
        t.resize(pattern_words(p.nz, p.ny, p.nx));
        for (uint32_t g = 0; g < (uint32_t)t.size(); g++) t[g] = pattern_transpose_word(a.data(), p.nx, p.ny, p.nz, g);
    }
    std::vector<StampRec> recs;
    rv_voxel_box u;
    stamps_ready(log2_x, log2_y, log2_z, stamps, n,
                 [&](int32_t id, int32_t& nx, int32_t& ny, int32_t& nz, const uint32_t*& a, const uint32_t*& t) {
                     nx = pats[id].nx; ny = pats[id].ny; nz = pats[id].nz;
                     a = A[(size_t)id].data(); t = T[(size_t)id].data();
                 },
                 &recs, nullptr, &u);
    stamps_apply_linear(log2_x, log2_y, bits, recs.data(), (int32_t)recs.size(), u, n_set, n_cleared);
    return RV_OK;
}

rv_status rv_world_stamp_box(int32_t log2_x, int32_t log2_y, int32_t log2_z, const rv_pattern_host* pats, int32_t npats,
                             const rv_stamp* stamps, int32_t n, rv_voxel_box* each, rv_voxel_box* all) {
    if (!linear_dims_ok(log2_x, log2_y, log2_z) || !all || !host_patterns_ok(pats, npats, false) ||
        !stamps_ok(stamps, n, [&](int32_t id) { return id >= 0 && id < npats; }))
        return RV_ERR_INVALID;
    stamps_ready(log2_x, log2_y, log2_z, stamps, n,
                 [&](int32_t id, int32_t& nx, int32_t& ny, int32_t& nz, const uint32_t*& a, const uint32_t*& t) {
                     nx = pats[id].nx; ny = pats[id].ny; nz = pats[id].nz;
                     a = t = nullptr;
                 },
                 nullptr, each, all);
    return RV_OK;
}

}  // extern "C"
