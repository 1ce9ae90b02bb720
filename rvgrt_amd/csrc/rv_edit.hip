// rv_edit.hip -- gfx950 kernel of rv_world_edit (include/rvgrt.h): voxel boxes written into the brick bit
// words in place.  The CSDF rebuild that follows is launch_csdf_box (rv_kernels.hip) over the boxes of
// coarse cells the edit can reach: the passes rv_csdf_build runs over the whole world, the same kernels,
// so the bytes equal a whole-grid build's.
#include "../../include/rvgrt/rv_internal.h"

namespace rv {

// ================================================================ bit write
// One lane per word of the grid (WordGrid, rv_words.h) of the voxel box that bounds all edit boxes.  The
// lane folds every box, in order, into a set mask and a clear mask (a later box overrides an earlier one
// bit by bit) and is the word's only writer: no atomics, no two lanes on one word.
__global__ void __launch_bounds__(256) k_edit_bits(uint32_t* __restrict__ brick, World w,
                                                   const rv_edit_box* __restrict__ boxes, int nboxes, WordGrid grid,
                                                   uint32_t* __restrict__ changed) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= grid.nwords) return;
    int wx, wy, z;
    grid.word(g, wx, wy, z);
    const int X0 = wx * 8, Y0 = wy * 4;
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
    const uint64_t bi = brick_word_index(w, wx, wy, z);
    const uint32_t old = brick[bi];
    const uint32_t nw = (old & ~clr) | set;
    if (nw != old) {
        brick[bi] = nw;
        *changed = 1u;   // every writer stores the same value
    }
}

// ================================================================ launcher
void launch_edit_bits(hipStream_t s, uint32_t* brick, const World& w, const rv_edit_box* boxes, int n,
                      const rv_voxel_box& box, uint32_t* changed) {
    const WordGrid grid = word_grid(box);
    hipLaunchKernelGGL(k_edit_bits, dim3(nblk(grid.nwords)), dim3(256), 0, s, brick, w, boxes, n, grid, changed);
}

}  // namespace rv
