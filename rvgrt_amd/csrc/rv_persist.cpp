// rv_persist.cpp -- host side of librvgrt_hip.so, part 7 of the C ABI (include/rvgrt.h): edited columns that
// survive scrolling away and back (rv_world_persist, rv_world_persist_info, rv_world_persist_flush), the host
// store of column bits (rv_world_store_list / get / put / clear), the column read-back
// (rv_world_columns_read) and the host-only index map of the kernels (rv_persist_column_map).  The dirty
// set and the store live in the context (rv_host.h); rv_world_edit and rv_world_import mark, rv_world_scroll
// captures what leaves and restores what enters, rv_world_build restores, through the helpers below.  The
// kernels are in rv_persist.hip.
#include "rv_host.h"

namespace {

using Key = std::pair<int32_t, int32_t>;   // (wz, wx)

inline Key key_of(int32_t ox, int32_t oz, int bx, int bz) { return Key(oz + 8 * bz, ox + 8 * bx); }
inline const Key& key_in(const Key& k) { return k; }
inline const Key& key_in(const std::pair<const Key, std::vector<uint32_t>>& e) { return e.first; }
inline size_t range_columns(const ColumnRange& r) {
    return r.bx1 > r.bx0 && r.bz1 > r.bz0 ? (size_t)(r.bx1 - r.bx0) * (size_t)(r.bz1 - r.bz0) : 0;
}
inline size_t column_words(const rv_ctx* c) { return (size_t)2 << c->ly; }   // 2 Y
inline ColumnRange window(const rv_ctx* c) { return ColumnRange{0, c->w.X >> 3, 0, c->w.Z >> 3}; }

// fn(key, bx, bz) for every entry of `keys` (the dirty set or the store) that is a column of r when the
// window's origin is (ox, oz), in key order; walks whichever is smaller, the container or the range
template <class Keys, class Fn>
void each_in(const Keys& keys, const ColumnRange& r, int32_t ox, int32_t oz, Fn fn) {
    const size_t n = range_columns(r);
    if (n == 0 || keys.empty()) return;
    if (keys.size() <= n) {
        for (const auto& e : keys) {
            const Key& k = key_in(e);
            const int64_t rx = (int64_t)k.second - ox, rz = (int64_t)k.first - oz;
            if ((rx & 7) || (rz & 7)) continue;
            const int64_t bx = rx >> 3, bz = rz >> 3;
            if (bx >= r.bx0 && bx < r.bx1 && bz >= r.bz0 && bz < r.bz1) fn(k, (int)bx, (int)bz);
        }
    } else {
        for (int bz = r.bz0; bz < r.bz1; bz++)
            for (int bx = r.bx0; bx < r.bx1; bx++) {
                const Key k = key_of(ox, oz, bx, bz);
                if (keys.find(k) != keys.end()) fn(k, bx, bz);
            }
    }
}

// the context's column list -> device, for a launch over its columns
rv_status upload_columns(rv_ctx* c) {
    HIP_TRY(c, hipMemcpyAsync(c->persist_cols, c->persist_cols_h.data(), c->persist_cols_h.size() * sizeof(int2),
                              hipMemcpyHostToDevice, c->stream));
    return RV_OK;
}

// the columns of persist_cols_h gathered into persist_stage_h (reserved by the caller); waits for the stream
rv_status gather_columns(rv_ctx* c) {
    const size_t n = c->persist_cols_h.size(), words = column_words(c);
    if (rv_status s = upload_columns(c)) return s;
    launch_columns_gather(c->stream, c->brick, current_world(c), c->ly, c->persist_cols, (uint32_t)n, c->persist_stage);
    LAUNCH_CHECK(c);
    HIP_TRY(c, hipMemcpyAsync(c->persist_stage_h, c->persist_stage, n * words * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RV_OK;
}

}  // namespace

void persist_mark(rv_ctx* c, const ColumnRange& r) {
    if (!c->persist) return;
    for (int bz = r.bz0; bz < r.bz1; bz++)
        for (int bx = r.bx0; bx < r.bx1; bx++) c->persist_dirty.insert(key_of(c->cfg.seed_x, c->cfg.seed_z, bx, bz));
}

size_t persist_dirty_in(const rv_ctx* c, const ColumnRange& r, int32_t ox, int32_t oz) {
    size_t n = 0;
    if (c->persist) each_in(c->persist_dirty, r, ox, oz, [&](const Key&, int, int) { n++; });
    return n;
}

size_t persist_stored_in(const rv_ctx* c, const ColumnRange& r, int32_t ox, int32_t oz) {
    size_t n = 0;
    if (c->persist) each_in(c->persist_store, r, ox, oz, [&](const Key&, int, int) { n++; });
    return n;
}

rv_status persist_reserve(rv_ctx* c, size_t ncols) {
    if (ncols == 0) return RV_OK;
    const size_t bytes = ncols * column_words(c) * 4;
    if (rv_status s = c->persist_cols.reserve(c, ncols * sizeof(int2))) return s;
    if (rv_status s = c->persist_stage.reserve(c, bytes)) return s;
    return c->persist_stage_h.reserve(c, bytes);
}

void persist_trim(rv_ctx* c) {
    c->persist_stage.trim(EDIT_SCRATCH_KEEP);
    c->persist_stage_h.trim(EDIT_SCRATCH_KEEP);
}

rv_status persist_capture(rv_ctx* c, const ColumnRange& r, bool keep_dirty) {
    if (!c->persist) return RV_OK;
    std::vector<Key> keys;
    c->persist_cols_h.clear();
    each_in(c->persist_dirty, r, c->cfg.seed_x, c->cfg.seed_z, [&](const Key& k, int bx, int bz) {
        keys.push_back(k);
        c->persist_cols_h.push_back(make_int2(bx, bz));
    });
    if (keys.empty()) return RV_OK;
    if (rv_status s = gather_columns(c)) return s;
    const size_t words = column_words(c);
    for (size_t i = 0; i < keys.size(); i++) {
        const uint32_t* src = c->persist_stage_h + i * words;
        c->persist_store[keys[i]].assign(src, src + words);
        if (!keep_dirty) c->persist_dirty.erase(keys[i]);
    }
    c->persist_captured += keys.size();
    return RV_OK;
}

rv_status persist_restore(rv_ctx* c, const ColumnRange& r) {
    if (!c->persist) return RV_OK;
    const size_t words = column_words(c);
    std::vector<Key> keys;
    c->persist_cols_h.clear();
    each_in(c->persist_store, r, c->cfg.seed_x, c->cfg.seed_z, [&](const Key& k, int bx, int bz) {
        keys.push_back(k);
        c->persist_cols_h.push_back(make_int2(bx, bz));
    });
    if (keys.empty()) return RV_OK;
    for (size_t i = 0; i < keys.size(); i++)
        std::memcpy(c->persist_stage_h + i * words, c->persist_store[keys[i]].data(), words * 4);
    if (rv_status s = upload_columns(c)) return s;
    HIP_TRY(c, hipMemcpyAsync(c->persist_stage, c->persist_stage_h, keys.size() * words * 4, hipMemcpyHostToDevice,
                              c->stream));
    launch_columns_scatter(c->stream, c->brick, current_world(c), c->ly, c->persist_cols, (uint32_t)keys.size(),
                           c->persist_stage);
    LAUNCH_CHECK(c);
    // the host copies are free again, and an entry leaves the store only once its bits are in the world
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (const Key& k : keys) {
        c->persist_store.erase(k);
        c->persist_dirty.insert(k);
    }
    c->persist_restored += keys.size();
    return RV_OK;
}

extern "C" {

rv_status rv_world_persist(rv_ctx* c, int32_t on) {
    if (!c) return RV_ERR_INVALID;
    c->persist = on != 0;
    return RV_OK;
}

rv_status rv_world_persist_info(rv_ctx* c, int32_t* on, uint64_t* dirty_columns, uint64_t* stored_columns,
                                uint64_t* stored_bytes, uint64_t* captured_total, uint64_t* restored_total) {
    if (!c) return RV_ERR_INVALID;
    if (on) *on = c->persist ? 1 : 0;
    if (dirty_columns) *dirty_columns = c->persist_dirty.size();
    if (stored_columns) *stored_columns = c->persist_store.size();
    if (stored_bytes) *stored_bytes = (uint64_t)c->persist_store.size() * column_words(c) * 4;
    if (captured_total) *captured_total = c->persist_captured;
    if (restored_total) *restored_total = c->persist_restored;
    return RV_OK;
}

rv_status rv_world_persist_flush(rv_ctx* c) {
    if (!c) return RV_ERR_INVALID;
    if (!c->world_ready) return fail(c, RV_ERR_STATE, "rv_world_persist_flush before a world build or import");
    if (!c->persist || c->persist_dirty.empty()) return RV_OK;
    if (rv_status ws = wait_all_frames(c)) return ws;
    const ColumnRange all = window(c);
    if (rv_status s = persist_reserve(c, persist_dirty_in(c, all, c->cfg.seed_x, c->cfg.seed_z))) return s;
    const rv_status s = persist_capture(c, all, true);
    persist_trim(c);
    return s;
}

rv_status rv_world_store_list(rv_ctx* c, int32_t* keys_xz, int64_t cap, int64_t* n) {
    if (!c || cap < 0 || (cap > 0 && !keys_xz)) return RV_ERR_INVALID;
    int64_t i = 0;
    for (const auto& e : c->persist_store) {
        if (i >= cap) break;
        keys_xz[2 * i] = e.first.second;
        keys_xz[2 * i + 1] = e.first.first;
        i++;
    }
    if (n) *n = (int64_t)c->persist_store.size();
    return RV_OK;
}

rv_status rv_world_store_get(rv_ctx* c, int32_t wx, int32_t wz, uint32_t* bits, size_t bytes) {
    if (!c || !bits) return RV_ERR_INVALID;
    if (bytes != column_words(c) * 4) return fail(c, RV_ERR_INVALID, "rv_world_store_get: a column is 8 Y bytes");
    const auto it = c->persist_store.find(Key(wz, wx));
    if (it == c->persist_store.end()) return fail(c, RV_ERR_INVALID, "rv_world_store_get: no such column in the store");
    std::memcpy(bits, it->second.data(), bytes);
    return RV_OK;
}

rv_status rv_world_store_put(rv_ctx* c, int32_t wx, int32_t wz, const uint32_t* bits, size_t bytes) {
    if (!c || !bits) return RV_ERR_INVALID;
    if (bytes != column_words(c) * 4) return fail(c, RV_ERR_INVALID, "rv_world_store_put: a column is 8 Y bytes");
    // a key the window can never take (its origin moves by multiples of 8) would sit in the store for good
    if ((((int64_t)wx - c->cfg.seed_x) & 7) || (((int64_t)wz - c->cfg.seed_z) & 7))
        return fail(c, RV_ERR_INVALID, "rv_world_store_put: the key is not a multiple of 8 from the window's origin");
    c->persist_store[Key(wz, wx)].assign(bits, bits + column_words(c));
    return RV_OK;
}

rv_status rv_world_store_clear(rv_ctx* c) {
    if (!c) return RV_ERR_INVALID;
    c->persist_store.clear();
    c->persist_dirty.clear();
    return RV_OK;
}

rv_status rv_world_columns_read(rv_ctx* c, const int32_t* bxz, int32_t n, uint32_t* bits, size_t bytes) {
    if (!c || n < 0 || (n > 0 && (!bxz || !bits))) return RV_ERR_INVALID;
    if (!c->world_ready) return fail(c, RV_ERR_STATE, "rv_world_columns_read before a world build or import");
    if (bytes != (size_t)n * column_words(c) * 4)
        return fail(c, RV_ERR_INVALID, "rv_world_columns_read: a column is 8 Y bytes");
    const int NBX = c->w.X >> 3, NBZ = c->w.Z >> 3;
    for (int32_t i = 0; i < n; i++)
        if (bxz[2 * i] < 0 || bxz[2 * i] >= NBX || bxz[2 * i + 1] < 0 || bxz[2 * i + 1] >= NBZ)
            return fail(c, RV_ERR_INVALID, "rv_world_columns_read: a column outside the window");
    if (n == 0) return RV_OK;
    if (rv_status ws = wait_all_frames(c)) return ws;
    if (rv_status s = persist_reserve(c, (size_t)n)) return s;
    c->persist_cols_h.resize((size_t)n);
    for (int32_t i = 0; i < n; i++) c->persist_cols_h[i] = make_int2(bxz[2 * i], bxz[2 * i + 1]);
    const rv_status s = gather_columns(c);
    if (s == RV_OK) std::memcpy(bits, c->persist_stage_h, bytes);
    persist_trim(c);
    return s;
}

rv_status rv_persist_column_map(int32_t log2_x, int32_t log2_y, int32_t log2_z, int32_t bx, int32_t bz,
                                uint32_t* src_dword) {
    if (!src_dword || !dims_ok(log2_x, log2_y, log2_z)) return RV_ERR_INVALID;
    if (bx < 0 || bx >= 1 << (log2_x - 3) || bz < 0 || bz >= 1 << (log2_z - 3)) return RV_ERR_INVALID;
    const ColumnGeom g{log2_z - 3, (log2_z - 3) + (log2_y - 3), log2_y};
    for (uint32_t i = 0; i < 2u << log2_y; i++)
        src_dword[i] = (uint32_t)column_word_dword(g, (uint32_t)bx, (uint32_t)bz, i);
    return RV_OK;
}

}  // extern "C"
