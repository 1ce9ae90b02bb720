// rv_edit.cpp -- host side of librvgrt_hip.so, part 4 of the C ABI (include/rvgrt.h): voxel edits in
// place (rv_world_edit, rv_world_edit_info) and the host-only plan of what an edit rebuilds
// (rv_world_edit_region).  The kernels are in rv_edit.hip.
#include "rv_host.h"

// shared with rv_relight.cpp
bool dims_ok(int lx, int ly, int lz) {   // rv_create's limits
    return lx >= 4 && ly >= 4 && lz >= 4 && lx <= 13 && ly <= 13 && lz <= 13 && lx + ly + lz <= 34;
}

static rv_voxel_box edit_voxels(const rv_edit_box& b) { return rv_voxel_box{b.x0, b.y0, b.z0, b.x1, b.y1, b.z1}; }

bool boxes_ok(int lx, int ly, int lz, const rv_edit_box* b, int n) {
    if (n < 0 || n > RV_EDIT_MAX_BOXES || (n > 0 && !b)) return false;
    const int X = 1 << lx, Y = 1 << ly, Z = 1 << lz;
    for (int i = 0; i < n; i++)
        if (!voxel_box_ok(X, Y, Z, edit_voxels(b[i])) || (b[i].solid != 0 && b[i].solid != 1)) return false;
    return true;
}

static CellBox grown(const int e0[3], const int e1[3], const int S[3], int gx, int gy, int gz) {
    const int g[3] = {gx, gy, gz};
    int a0[3], a1[3];
    for (int a = 0; a < 3; a++) {
        a0[a] = std::max(0, e0[a] - g[a]);
        a1[a] = std::min(S[a], e1[a] + g[a]);
    }
    return CellBox{a0[0], a0[1], a0[2], a1[0] - a0[0], a1[1] - a0[1], a1[2] - a0[2]};
}

CsdfBoxes csdf_boxes(const int e0[3], const int e1[3], const int S[3]) {
    CsdfBoxes b;
    b.rf = grown(e0, e1, S, 64, 64, 64);
    b.ry = grown(e0, e1, S, 64, 64, 128);
    b.rx = grown(e0, e1, S, 64, 128, 128);
    b.rs = grown(e0, e1, S, 128, 128, 128);
    return b;
}

rv_status csdf_rebuild_boxes(rv_ctx* c, const CsdfBoxes* b, int n) {
    size_t n0 = 0, n1 = 0;
    for (int i = 0; i < n; i++) {
        n0 = std::max(n0, (size_t)b[i].rs.cells());
        n1 = std::max(n1, (size_t)b[i].rx.cells());
    }
    if (rv_status s = c->edit_t0.reserve(c, n0)) return s;
    if (rv_status s = c->edit_t1.reserve(c, n1)) return s;
    for (int i = 0; i < n; i++)
        launch_csdf_box(c->stream, c->brick, current_world(c), b[i].rs, b[i].rx, b[i].ry, b[i].rf, c->edit_t0,
                        c->edit_t1);
    LAUNCH_CHECK(c);
    const hipError_t se = hipStreamSynchronize(c->stream);
    if (c->edit_t0.cap + c->edit_t1.cap > EDIT_SCRATCH_KEEP) {
        c->edit_t0.reset();
        c->edit_t1.reset();
    }
    HIP_TRY(c, se);
    return RV_OK;
}

namespace {

// What one rv_world_edit call touches.
//
// The CSDF is three chained 1-D passes over the coarse grid (rv_kernels.hip k_csdf_x, k_csdf_yz):
//   dx(p)    reads the solidity of the cells p.x - 64 .. p.x + 64 of p's x row;
//   dy(p)    reads dx at p.y - 63 .. p.y + 63 of p's y column (the scan stops once off * off >= m, and
//            m <= 64 * 64, so offset 64 is never read);
//   final(p) reads dy at p.z - 63 .. p.z + 63 of p's z column.
// With E the coarse bounding box of the edited voxels: a cell's solidity changes only inside E, so dx can
// change only inside E grown by 64 along x, dy only inside that grown by 63 along y, and the final byte only
// inside that grown by 63 along z.  The rebuild recomputes F = E grown by 64 per axis (rf; the one bound
// serves all three axes) and, reading backwards through the passes, needs
//   dy    over F grown by 64 along z          = E + (64, 64, 128)   (ry)
//   dx    over that grown by 64 along y       = E + (64, 128, 128)  (rx)
//   solid over that grown by 64 along x       = E + (128, 128, 128) (rs)
// each clipped to the world (a neighbour outside the world is skipped by the passes, Appendix R3).
// Everything outside F keeps its byte: it equals what a whole-grid build would write there.
struct EditPlan {
    rv_voxel_box box;        // voxel bounding box of the boxes
    CsdfBoxes b;
    uint64_t local_cells;    // cells the four local passes visit
    uint64_t full_cells;     // cells the four whole-grid passes visit
};

// the plan of an edit whose voxels lie in box
EditPlan edit_plan_box(int lx, int ly, int lz, const rv_voxel_box& box) {
    EditPlan p{};
    p.box = box;
    const int S[3] = {1 << (lx - 1), 1 << (ly - 1), 1 << (lz - 1)};
    const int e0[3] = {box.x0 >> 1, box.y0 >> 1, box.z0 >> 1};
    const int e1[3] = {((box.x1 - 1) >> 1) + 1, ((box.y1 - 1) >> 1) + 1, ((box.z1 - 1) >> 1) + 1};
    p.b = csdf_boxes(e0, e1, S);
    p.local_cells = p.b.passes();
    p.full_cells = 4ull * (uint64_t)S[0] * (uint64_t)S[1] * (uint64_t)S[2];
    return p;
}

// boxes validated, n >= 1
EditPlan edit_plan(int lx, int ly, int lz, const rv_edit_box* b, int n) {
    rv_voxel_box all = empty_box();
    for (int i = 0; i < n; i++) box_include(all, edit_voxels(b[i]));
    return edit_plan_box(lx, ly, lz, all);
}

}  // namespace

// What follows the bit writes of an edit whose changed voxels lie in `changed` (the caller has waited for the
// frames, written the bits and marked the columns for persistence): shared by every in-place voxel write.
rv_status edit_finish(rv_ctx* c, const rv_voxel_box& changed) {
    const EditPlan p = edit_plan_box(c->lx, c->ly, c->lz, changed);
    c->edit_cells = 0;
    c->edit_full = 0;
    c->geom_ver++;
    if (rv_status ts = world_top(c)) return ts;   // the exits, from the bits (a cleared voxel can lower them)
    if (p.local_cells >= p.full_cells) {
        if (rv_status s = rv_csdf_build(c)) return s;
        c->edit_cells = n_csdf(c);
        c->edit_full = 1;
    } else {
        if (rv_status s = csdf_rebuild_boxes(c, &p.b, 1)) return s;
        if (rv_status ms = mark_world(c)) return ms;
        c->edit_cells = p.b.rf.cells();
    }
    c->edit_count++;
    return RV_OK;
}

extern "C" {

rv_status rv_world_edit_region(int32_t log2_x, int32_t log2_y, int32_t log2_z, const rv_edit_box* boxes, int32_t n,
                               int32_t region[6], uint64_t* cells) {
    if (!region || !dims_ok(log2_x, log2_y, log2_z) || !boxes_ok(log2_x, log2_y, log2_z, boxes, n))
        return RV_ERR_INVALID;
    if (n == 0) {
        for (int i = 0; i < 6; i++) region[i] = 0;
        if (cells) *cells = 0;
        return RV_OK;
    }
    const EditPlan p = edit_plan(log2_x, log2_y, log2_z, boxes, n);
    region[0] = p.b.rf.x0; region[1] = p.b.rf.x0 + p.b.rf.nx;
    region[2] = p.b.rf.y0; region[3] = p.b.rf.y0 + p.b.rf.ny;
    region[4] = p.b.rf.z0; region[5] = p.b.rf.z0 + p.b.rf.nz;
    if (cells) *cells = p.b.rf.cells();
    return RV_OK;
}

rv_status rv_world_edit(rv_ctx* c, const rv_edit_box* boxes, int32_t n) {
    if (!c) return RV_ERR_INVALID;
    if (!c->world_ready) return fail(c, RV_ERR_STATE, "rv_world_edit before a world build or import");
    if (!boxes_ok(c->lx, c->ly, c->lz, boxes, n)) return fail(c, RV_ERR_INVALID, "rv_world_edit: bad box list");
    if (n == 0) return RV_OK;
    const EditPlan p = edit_plan(c->lx, c->ly, c->lz, boxes, n);
    if (rv_status ws = wait_all_frames(c)) return ws;

    // the bits: boxes to the device (from a stable host copy), one lane per affected word
    c->edit_h.assign(boxes, boxes + n);
    if (rv_status s = c->edit_flag.reserve(c, 4)) return s;
    if (rv_status s = c->edit_boxes.reserve(c, (size_t)n * sizeof(rv_edit_box))) return s;
    HIP_TRY(c, hipMemcpyAsync(c->edit_boxes, c->edit_h.data(), (size_t)n * sizeof(rv_edit_box), hipMemcpyHostToDevice,
                              c->stream));
    HIP_TRY(c, hipMemsetAsync(c->edit_flag, 0, 4, c->stream));
    launch_edit_bits(c->stream, c->brick, current_world(c), c->edit_boxes, n, p.box, c->edit_flag);
    LAUNCH_CHECK(c);
    uint32_t changed = 0;
    HIP_TRY(c, hipMemcpyAsync(&changed, c->edit_flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->edit_cells = 0;
    c->edit_full = 0;
    if (!changed) return RV_OK;   // every voxel already had its value: nothing to rebuild or invalidate

    for (int i = 0; i < n; i++)   // persistence: the columns under each box may now differ from the generator's
        persist_mark(c, columns_under(edit_voxels(boxes[i])));
    return edit_finish(c, p.box);
}

rv_status rv_world_edit_info(rv_ctx* c, uint64_t* edits, uint64_t* csdf_cells, int32_t* last_full) {
    if (!c) return RV_ERR_INVALID;
    if (edits) *edits = c->edit_count;
    if (csdf_cells) *csdf_cells = c->edit_cells;
    if (last_full) *last_full = c->edit_full;
    return RV_OK;
}

}  // extern "C"
