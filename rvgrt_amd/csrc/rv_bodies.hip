// rv_bodies.hip -- gfx950 kernel of rv_world_bodies_move (include/rvgrt.h): n axis-aligned boxes swept through
// the voxel bits, one lane per body.  The sweep itself is bodies_move_one of include/rvgrt/rv_bodies.h, the
// function rv_world_bodies_move_at evaluates on the CPU; here it reads the brick records the frames read,
// through load_dword's 32-bit offsets from the SGPR base.  Bodies are independent: no LDS, no atomics, and
// nothing the frames read is written.
#include "../../include/rvgrt/rv_bodies.h"

namespace rv {

__global__ void __launch_bounds__(256) k_bodies_move(World w, const uint32_t* __restrict__ in, uint32_t n, uint32_t open,
                                                     uint4* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t b[9], r[4];
    for (int k = 0; k < 9; k++) b[k] = in[9u * i + (uint32_t)k];   // n <= 2^24: 9 i + 8 < 2^28
    bodies_move_one(w, open != 0, b, r);
    out[i] = make_uint4(r[0], r[1], r[2], r[3]);
}

void launch_bodies_move(hipStream_t s, const World& w, const void* in, int64_t n, bool open, void* out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_bodies_move, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, w,
                       static_cast<const uint32_t*>(in), (uint32_t)n, open ? 1u : 0u, static_cast<uint4*>(out));
}

}  // namespace rv
