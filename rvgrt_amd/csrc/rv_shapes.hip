// rv_shapes.hip -- gfx950 kernel of rv_world_edit_shapes (include/rvgrt.h): ellipsoids and elliptic cylinders
// rasterised into the brick bit words in place.  Which voxels a shape holds is decided by the integer
// functions of include/rvgrt/rv_shapes.h, the ones rv_world_edit_shapes_at runs on the CPU.
#include "../../include/rvgrt/rv_internal.h"
#include "../../include/rvgrt/rv_shapes.h"

namespace rv {

// One lane per word of the grid (WordGrid, rv_words.h) of the voxel box that bounds all clipped shape boxes.
// The lane folds every shape, in order, into a set mask and a clear mask (a later shape overrides an earlier
// one bit by bit) and is the word's only writer.
//   - The shape list is the same for every lane and the loop index is wave-uniform, so a shape, its clipped
//     box and its q products live in SGPRs (scalar loads, scalar multiplies).
//   - A word outside a shape's clipped box skips the shape on integer compares, before any 64-bit multiply.
//   - The z terms are computed once per shape and word, the eight dx^2 K products once for the word's four
//     rows, a row's budget once for its eight bits: 8 + 4 64-bit multiplies per shape that meets the word.
//   - The bits turned on and off are counted against the word before the call, reduced over the wave (of
//     whatever size the device has) and added by one lane with one atomic each to counts[0] / counts[1]
//     (pre-zeroed).  Integer sums do not depend on the order.
// Every word lies inside the window (X a multiple of 8, Y of 4), so the window's clip needs no mask.
__global__ void __launch_bounds__(256) k_edit_shapes(uint32_t* __restrict__ brick, World w,
                                                     const rv_edit_shape* __restrict__ shapes, int nshapes,
                                                     WordGridT<uint64_t> grid, unsigned long long* __restrict__ counts) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = g < grid.nwords;   // no early return: the wave reduction below needs every lane
    uint32_t on = 0, off = 0;
    if (live) {
        int wx, wy, z;
        grid.word(g, wx, wy, z);
        const int X0 = wx * 8, Y0 = wy * 4;
        const int32_t D[3] = {w.X, w.Y, w.Z};
        uint32_t set = 0, clr = 0;
        for (int i = 0; i < nshapes; i++) {
            const rv_edit_shape s = shapes[i];
            int32_t lo[3], hi[3];
            if (!shape_box(s, D, lo, hi)) continue;   // uniform
            if (z < lo[2] || z >= hi[2] || X0 + 8 <= lo[0] || X0 >= hi[0] || Y0 + 4 <= lo[1] || Y0 >= hi[1]) continue;
            ShapeTerms zt;
            if (!shape_z_terms(s, z, zt)) continue;
            int64_t P[8];
            shape_x_products(s, shape_k(s), X0, P);
            uint32_t m = 0;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int64_t T = shape_row_budget(s, zt, Y0 + r);
                if (T >= 0) m |= shape_bits(P, T) << (8 * r);
            }
            if (s.solid) { set |= m; clr &= ~m; } else { clr |= m; set &= ~m; }
        }
        if (set | clr) {
            const uint64_t bi = brick_word_index(w, wx, wy, z);
            const uint32_t old = brick[bi];
            const uint32_t nw = (old & ~clr) | set;
            if (nw != old) {
                brick[bi] = nw;
                on = (uint32_t)__popc(nw & ~old);
                off = (uint32_t)__popc(old & ~nw);
            }
        }
    }
    // one atomic per wave and counter: a butterfly over the wave's real width
    for (int d = warpSize >> 1; d > 0; d >>= 1) {
        on += __shfl_xor(on, d, warpSize);
        off += __shfl_xor(off, d, warpSize);
    }
    if ((threadIdx.x & (warpSize - 1)) == 0) {
        if (on) atomicAdd(&counts[0], (unsigned long long)on);
        if (off) atomicAdd(&counts[1], (unsigned long long)off);
    }
}

void launch_edit_shapes(hipStream_t s, uint32_t* brick, const World& w, const rv_edit_shape* shapes, int n,
                        const rv_voxel_box& box, unsigned long long* counts) {
    const WordGridT<uint64_t> grid = word_grid<uint64_t>(box);
    hipLaunchKernelGGL(k_edit_shapes, dim3(nblk(grid.nwords)), dim3(256), 0, s, brick, w, shapes, n, grid, counts);
}

}  // namespace rv
