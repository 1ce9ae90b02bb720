// rv_edit.hip -- gfx950 kernel of rv_world_edit (include/rvgrt.h): voxel boxes written into the brick bit
// words in place.  The CSDF rebuild that follows is launch_csdf_box (rv_kernels.hip) over the boxes of
// coarse cells the edit can reach: the passes rv_csdf_build runs over the whole world, the same kernels,
// so the bytes equal a whole-grid build's.
#include "../../include/rvgrt/rv_internal.h"

namespace rv {

// ================================================================ bit write
// One lane per 32-bit brick word (8 x, 4 y, 1 z voxels) of the voxel box that bounds all edit boxes.  The
// lane folds every box, in order, into a set mask and a clear mask (a later box overrides an earlier one
// bit by bit) and is the word's only writer: no atomics, no two lanes on one word.
__global__ void __launch_bounds__(256) k_edit_bits(uint32_t* __restrict__ brick, World w,
                                                   const rv_edit_box* __restrict__ boxes, int nboxes, int wx0, int wy0,
                                                   int wz0, int nwy, int nwz, uint64_t nwords,
                                                   uint32_t* __restrict__ changed) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nwords) return;
    const int z = wz0 + (int)(g % (uint64_t)nwz);
    const uint64_t t = g / (uint64_t)nwz;
    const int wy = wy0 + (int)(t % (uint64_t)nwy), wx = wx0 + (int)(t / (uint64_t)nwy);
    const int X0 = wx * 8, Y0 = wy * 4;   // the word's voxels: x X0..X0+7 (bit & 7), y Y0..Y0+3 (bit >> 3)
    uint32_t set = 0, clr = 0;
    for (int i = 0; i < nboxes; i++) {
        const rv_edit_box b = boxes[i];
        if (z < b.z0 || z >= b.z1) continue;
        const int xa = imax(b.x0, X0) - X0, xb = imin(b.x1, X0 + 8) - X0;
        const int ya = imax(b.y0, Y0) - Y0, yb = imin(b.y1, Y0 + 4) - Y0;
        if (xa >= xb || ya >= yb) continue;
        const uint32_t row = ((1u << (xb - xa)) - 1u) << xa;   // xb - xa <= 8
        uint32_t m = 0;
        for (int r = ya; r < yb; r++) m |= row << (8 * r);
        if (b.solid) { set |= m; clr &= ~m; } else { clr |= m; set &= ~m; }
    }
    if ((set | clr) == 0) return;
    // brick (x >> 3, y >> 3, z >> 3), word (y >> 2 & 1) | (z & 7) << 1 (k_fill_bricks' order)
    const uint64_t bi = bits_word_index(brick_of(w, wx, wy >> 1, z >> 3), (uint32_t)(wy & 1) | ((uint32_t)(z & 7) << 1));
    const uint32_t old = brick[bi];
    const uint32_t nw = (old & ~clr) | set;
    if (nw != old) {
        brick[bi] = nw;
        *changed = 1u;   // every writer stores the same value
    }
}

// ================================================================ launchers
static inline uint32_t nblk(uint64_t n) { return (uint32_t)((n + 255) / 256); }

void launch_edit_bits(hipStream_t s, uint32_t* brick, const World& w, const rv_edit_box* boxes, int n,
                      const int lo[3], const int hi[3], uint32_t* changed) {
    const int wx0 = lo[0] >> 3, wy0 = lo[1] >> 2, wz0 = lo[2];
    const int nwx = ((hi[0] - 1) >> 3) - wx0 + 1, nwy = ((hi[1] - 1) >> 2) - wy0 + 1, nwz = hi[2] - wz0;
    const uint64_t nwords = (uint64_t)nwx * (uint64_t)nwy * (uint64_t)nwz;
    hipLaunchKernelGGL(k_edit_bits, dim3(nblk(nwords)), dim3(256), 0, s, brick, w, boxes, n, wx0, wy0, wz0, nwy, nwz,
                       nwords, changed);
}

}  // namespace rv
