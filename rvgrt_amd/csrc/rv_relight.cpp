// rv_relight.cpp -- host side of librvgrt_hip.so, part 5 of the C ABI (include/rvgrt.h): the GI refresh of
// a box of cells right after an edit (rv_gi_relight, rv_gi_relight_info) and the host-only choice of that
// box from the edit's boxes (rv_gi_relight_box).  The kernels are in rv_kernels.hip beside the GI update's
// functions they reuse (gi_record_cell, gi_combine).
#include "rv_host.h"

extern "C" {

rv_status rv_gi_relight_box(int32_t log2_x, int32_t log2_y, int32_t log2_z, const rv_edit_box* boxes, int32_t n,
                            int32_t margin_cells, rv_gi_box* out) {
    if (!out || margin_cells < 0 || !dims_ok(log2_x, log2_y, log2_z) || !boxes_ok(log2_x, log2_y, log2_z, boxes, n))
        return RV_ERR_INVALID;
    *out = rv_gi_box{0, 0, 0, 0, 0, 0};
    if (n == 0) return RV_OK;
    const int64_t G[3] = {(int64_t)1 << (log2_x - 2), (int64_t)1 << (log2_y - 2), (int64_t)1 << (log2_z - 2)};
    int64_t lo[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, hi[3] = {0, 0, 0};
    for (int i = 0; i < n; i++) {
        const int l[3] = {boxes[i].x0, boxes[i].y0, boxes[i].z0}, h[3] = {boxes[i].x1, boxes[i].y1, boxes[i].z1};
        for (int a = 0; a < 3; a++) {
            lo[a] = std::min<int64_t>(lo[a], l[a] >> 2);
            hi[a] = std::max<int64_t>(hi[a], ((h[a] - 1) >> 2) + 1);
        }
    }
    for (int a = 0; a < 3; a++) {   // 64-bit: any margin_cells clips to the grid without overflow
        lo[a] = std::max<int64_t>(0, lo[a] - margin_cells);
        hi[a] = std::min<int64_t>(G[a], hi[a] + margin_cells);
    }
    *out = rv_gi_box{(int32_t)lo[0], (int32_t)lo[1], (int32_t)lo[2], (int32_t)hi[0], (int32_t)hi[1], (int32_t)hi[2]};
    return RV_OK;
}

rv_status rv_gi_relight(rv_ctx* c, const rv_gi_box* box, uint32_t frame0, int32_t iterations, int32_t flags) {
    if (!c) return RV_ERR_INVALID;
    if (!c->world_ready) return fail(c, RV_ERR_STATE, "rv_gi_relight before a world build or import");
    if (!box) return fail(c, RV_ERR_INVALID, "rv_gi_relight: no box");
    if (box->x0 < 0 || box->y0 < 0 || box->z0 < 0 || box->x1 > c->w.GX || box->y1 > c->w.GY || box->z1 > c->w.GZ ||
        box->x1 <= box->x0 || box->y1 <= box->y0 || box->z1 <= box->z0)
        return fail(c, RV_ERR_INVALID, "rv_gi_relight: box empty or outside the GI grid");
    if (flags & ~RV_RELIGHT_INIT) return fail(c, RV_ERR_INVALID, "rv_gi_relight: unknown flags");
    if (iterations < 0) return fail(c, RV_ERR_INVALID, "rv_gi_relight: negative iterations");
    const CellBox b{box->x0, box->y0, box->z0, box->x1 - box->x0, box->y1 - box->y0, box->z1 - box->z0};
    const uint64_t cells = b.cells(), records = cells * (uint64_t)iterations;
    if (records > RV_RELIGHT_MAX_RECORDS)
        return fail(c, RV_ERR_INVALID, "rv_gi_relight: cells x iterations above RV_RELIGHT_MAX_RECORDS");
    const bool init = (flags & RV_RELIGHT_INIT) != 0;
    if (iterations == 0 && !init) return RV_OK;   // nothing to do: nothing invalidated

    // Scratch (bytes), before anything is enqueued: the records are bounded by RV_RELIGHT_MAX_RECORDS, each
    // dense array by the grid's own size.  An array that has to grow is freed only once the last relight, which
    // ended in mark_world, has finished with it.
    const size_t rec_need = (size_t)records * sizeof(uint2), dense_need = (size_t)cells * 4;
    if (rec_need > c->relight_rec.cap || dense_need > c->relight_dense[0].cap || dense_need > c->relight_dense[1].cap)
        HIP_TRY(c, hipEventSynchronize(c->ev_world));
    if (rv_status s = c->relight_rec.reserve(c, rec_need)) return s;
    for (int k = 0; k < 2; k++)
        if (rv_status s = c->relight_dense[k].reserve(c, dense_need)) return s;
    uint32_t* const dense[2] = {c->relight_dense[0], c->relight_dense[1]};

    // Ordered like rv_gi_update: after the frames in flight and the last world/GI write.  The call reads
    // and writes the grid and its own scratch only (never gi_tmp), on the context's stream.
    if (rv_status ws = wait_all_frames(c)) return ws;
    launch_gi_relight(c->stream, current_world(c), sun_dir(), b, frame0, (uint32_t)iterations, init,
                      c->cfg.gi_init_saturate ? RV_GI_LIT_SATURATE : RV_GI_LIT_REFERENCE, c->gi, c->relight_rec,
                      dense, c->counters + ST_GI * NCNT);
    LAUNCH_CHECK(c);
    c->relight_calls++;
    c->relight_cells += cells;
    c->relight_records += records;
    return mark_world(c);
}

rv_status rv_gi_relight_info(rv_ctx* c, uint64_t* calls, uint64_t* cells, uint64_t* records) {
    if (!c) return RV_ERR_INVALID;
    if (calls) *calls = c->relight_calls;
    if (cells) *cells = c->relight_cells;
    if (records) *records = c->relight_records;
    return RV_OK;
}

}  // extern "C"
