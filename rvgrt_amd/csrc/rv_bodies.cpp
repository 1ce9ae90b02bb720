// rv_bodies.cpp -- host side of librvgrt_hip.so, part 8 of the C ABI (include/rvgrt.h): swept box collision
// against the voxel window (rv_world_bodies_move, rv_world_bodies_move_device, rv_world_bodies_info) and the
// host-only evaluation of the same function (rv_world_bodies_move_at).  The sweep is bodies_move_one of
// include/rvgrt/rv_bodies.h; the kernel is in rv_bodies.hip.  The calls read the bits and write nothing the
// frames read, so they neither wait for frames in flight nor discard work computed ahead.
#include "rv_host.h"
#include "../../include/rvgrt/rv_bodies.h"

static_assert(sizeof(rv_body) == 36 && sizeof(rv_body_out) == 16, "rv_body / rv_body_out layout");

namespace {

bool args_ok(const void* in, int64_t n, int32_t flags, const void* out) {
    return n >= 0 && n <= BODIES_MAX && !(flags & ~RV_BODIES_OPEN_EDGES) && (n == 0 || (in && out));
}

}  // namespace

extern "C" {

rv_status rv_world_bodies_move_device(rv_ctx* c, const void* dev_in, int64_t n, int32_t flags, void* dev_out) {
    if (!c) return RV_ERR_INVALID;
    if (!args_ok(dev_in, n, flags, dev_out)) return fail(c, RV_ERR_INVALID, "rv_world_bodies_move: bad n, flags or array");
    if (n == 0) return RV_OK;
    if (((uintptr_t)dev_in & 3) || ((uintptr_t)dev_out & 15))
        return fail(c, RV_ERR_INVALID, "rv_world_bodies_move_device: dev_in is 4-byte, dev_out 16-byte aligned");
    const uintptr_t a = (uintptr_t)dev_in, b = (uintptr_t)dev_out;
    if (a < b + (uintptr_t)n * sizeof(rv_body_out) && b < a + (uintptr_t)n * sizeof(rv_body))
        return fail(c, RV_ERR_INVALID, "rv_world_bodies_move_device: dev_in and dev_out overlap");
    if (!c->world_ready) return fail(c, RV_ERR_STATE, "rv_world_bodies_move before a world build or import");
    // the last world write may have been issued on another stream
    if (c->world_stream != c->stream) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_world, 0));
    launch_bodies_move(c->stream, current_world(c), dev_in, n, (flags & RV_BODIES_OPEN_EDGES) != 0, dev_out);
    LAUNCH_CHECK(c);
    c->bodies_calls++;
    c->bodies_moved += (uint64_t)n;
    return RV_OK;
}

rv_status rv_world_bodies_move(rv_ctx* c, const rv_body* in, int64_t n, int32_t flags, rv_body_out* out) {
    if (!c) return RV_ERR_INVALID;
    if (!args_ok(in, n, flags, out)) return fail(c, RV_ERR_INVALID, "rv_world_bodies_move: bad n, flags or array");
    if (n == 0) return RV_OK;
    if (!c->world_ready) return fail(c, RV_ERR_STATE, "rv_world_bodies_move before a world build or import");
    if (rv_status s = c->bodies_in.reserve(c, (size_t)n * sizeof(rv_body))) return s;
    if (rv_status s = c->bodies_out.reserve(c, (size_t)n * sizeof(rv_body_out))) return s;
    HIP_TRY(c, hipMemcpyAsync(c->bodies_in, in, (size_t)n * sizeof(rv_body), hipMemcpyHostToDevice, c->stream));
    if (rv_status s = rv_world_bodies_move_device(c, c->bodies_in, n, flags, c->bodies_out)) return s;
    HIP_TRY(c, hipMemcpyAsync(out, c->bodies_out, (size_t)n * sizeof(rv_body_out), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RV_OK;
}

rv_status rv_world_bodies_info(rv_ctx* c, uint64_t* calls, uint64_t* bodies) {
    if (!c) return RV_ERR_INVALID;
    if (calls) *calls = c->bodies_calls;
    if (bodies) *bodies = c->bodies_moved;
    return RV_OK;
}

rv_status rv_world_bodies_move_at(int32_t log2_x, int32_t log2_y, int32_t log2_z, const uint32_t* bits, const rv_body* in,
                                  int64_t n, int32_t flags, rv_body_out* out) {
    if (!linear_dims_ok(log2_x, log2_y, log2_z) || !bits || !args_ok(in, n, flags, out)) return RV_ERR_INVALID;
    const LinearWorld w = linear_world(log2_x, log2_y, log2_z, bits, nullptr);
    const bool open = (flags & RV_BODIES_OPEN_EDGES) != 0;
    for (int64_t i = 0; i < n; i++) {
        uint32_t b[9], r[4];
        std::memcpy(b, &in[i], sizeof(b));
        bodies_move_one(w, open, b, r);
        std::memcpy(&out[i], r, sizeof(r));
    }
    return RV_OK;
}

}  // extern "C"
