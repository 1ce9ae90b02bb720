// rv_shapes.cpp -- host side of librvgrt_hip.so, part 11 of the C ABI (include/rvgrt.h): shaped edits in place
// (rv_world_edit_shapes) and the host-only forms (rv_world_edit_shapes_at, rv_world_edit_shapes_box).  The
// integer functions are in include/rvgrt/rv_shapes.h, the kernel in rv_shapes.hip.  The call ends like an
// rv_world_edit over the union of the clipped boxes (edit_finish, rv_edit.cpp).
#include "rv_host.h"
#include "../../include/rvgrt/rv_shapes.h"

static_assert(sizeof(rv_edit_shape) == 32, "rv_edit_shape layout");

extern "C" {

rv_status rv_world_edit_shapes(rv_ctx* c, const rv_edit_shape* shapes, int32_t n, uint64_t* n_set,
                               uint64_t* n_cleared) {
    if (!c) return RV_ERR_INVALID;
    if (!c->world_ready) return fail(c, RV_ERR_STATE, "rv_world_edit_shapes before a world build or import");
    if (!shapes_ok(shapes, n)) return fail(c, RV_ERR_INVALID, "rv_world_edit_shapes: bad shape list");
    if (n_set) *n_set = 0;
    if (n_cleared) *n_cleared = 0;
    if (n == 0) return RV_OK;
    c->shape_h.assign(shapes, shapes + n);   // the stable host copy the upload reads
    c->shape_box_h.resize((size_t)n);
    rv_voxel_box u;
    const bool any = shapes_boxes(c->lx, c->ly, c->lz, c->shape_h.data(), n, c->shape_box_h.data(), &u);
    if (!any) {   // every shape lies outside the window: nothing is launched, so nothing is waited for
        c->edit_cells = 0;
        c->edit_full = 0;
        return RV_OK;
    }
    if (rv_status ws = wait_all_frames(c)) return ws;

    // the bits: shapes to the device, one lane per word of the union box
    if (rv_status s = c->shape_counts.reserve(c, 2 * sizeof(unsigned long long))) return s;
    if (rv_status s = c->shape_list.reserve(c, (size_t)n * sizeof(rv_edit_shape))) return s;
    HIP_TRY(c, hipMemcpyAsync(c->shape_list, c->shape_h.data(), (size_t)n * sizeof(rv_edit_shape), hipMemcpyHostToDevice,
                              c->stream));
    HIP_TRY(c, hipMemsetAsync(c->shape_counts, 0, 2 * sizeof(unsigned long long), c->stream));
    launch_edit_shapes(c->stream, c->brick, current_world(c), c->shape_list, n, u, c->shape_counts);
    LAUNCH_CHECK(c);
    unsigned long long cnt[2] = {0, 0};   // turned on, turned off
    HIP_TRY(c, hipMemcpyAsync(cnt, c->shape_counts, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n_set) *n_set = cnt[0];
    if (n_cleared) *n_cleared = cnt[1];
    c->edit_cells = 0;
    c->edit_full = 0;
    if (cnt[0] + cnt[1] == 0) return RV_OK;   // every voxel already had its value: nothing to rebuild or invalidate

    for (int i = 0; i < n; i++) {   // persistence: the columns under each non-empty clipped box
        const rv_voxel_box& b = c->shape_box_h[(size_t)i];
        if (b.x1 > b.x0) persist_mark(c, columns_under(b));
    }
    return edit_finish(c, u);
}

rv_status rv_world_edit_shapes_at(int32_t log2_x, int32_t log2_y, int32_t log2_z, uint32_t* bits,
                                  const rv_edit_shape* shapes, int32_t n, uint64_t* n_set, uint64_t* n_cleared) {
    if (!linear_dims_ok(log2_x, log2_y, log2_z) || !bits || !shapes_ok(shapes, n)) return RV_ERR_INVALID;
    shapes_apply_linear(log2_x, log2_y, log2_z, bits, shapes, n, n_set, n_cleared);
    return RV_OK;
}

rv_status rv_world_edit_shapes_box(int32_t log2_x, int32_t log2_y, int32_t log2_z, const rv_edit_shape* shapes,
                                   int32_t n, rv_voxel_box* each, rv_voxel_box* all) {
    if (!linear_dims_ok(log2_x, log2_y, log2_z) || !all || !shapes_ok(shapes, n)) return RV_ERR_INVALID;
    shapes_boxes(log2_x, log2_y, log2_z, shapes, n, each, all);
    return RV_OK;
}

}  // extern "C"
