// rv_stamp.hip -- gfx950 kernels of rv_world_stamp and the pattern objects (include/rvgrt.h): oriented patterns
// assembled into the brick bit words in place, a box of the world gathered into a pattern, and a pattern's
// second layout.  Which bits a stamp lays over a word is decided by the integer functions of
// include/rvgrt/rv_stamp.h, the ones rv_world_stamp_at runs on the CPU.
#include "../../include/rvgrt/rv_internal.h"
#include "../../include/rvgrt/rv_stamp.h"

namespace rv {

// One lane per word of the grid (WordGrid, rv_words.h) of the voxel box that bounds all clipped stamp boxes, in
// the shape of k_edit_shapes.  The lane folds every stamp, in order, into a set mask and a clear mask (a later
// stamp overrides an earlier one bit by bit) and is the word's only writer.
//   - The list of made-ready stamps (StampRec: the layout to read, its dims, the offset, the clipped box) is the
//     same for every lane and the loop index is wave-uniform, so a record lives in SGPRs (scalar loads).
//   - A word outside a stamp's clipped box skips the stamp on integer compares, before any pattern load.
//   - Each of the word's four rows fetches its 8 bits from the pattern row at x offset X0 - at.x -- unaligned,
//     possibly negative, possibly across two pattern words: two guarded dword loads, a 64-bit shift, a mask.
//     FLIP_Z flips the row index, FLIP_X reads the mirrored run and reverses it, SWAP_XZ reads the transposed
//     layout: one code path.
//   - The bits turned on and off are counted against the word before the call, reduced over the wave (of
//     whatever size the device has) and added by one lane with one atomic each to counts[0] / counts[1]
//     (pre-zeroed).  Integer sums do not depend on the order.
// Every word lies inside the window (X a multiple of 8, Y of 4), so the window's clip needs no mask.
__global__ void __launch_bounds__(256) k_stamp(uint32_t* __restrict__ brick, World w, const StampRec* __restrict__ recs,
                                               int nrecs, WordGrid grid, unsigned long long* __restrict__ counts) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = g < grid.nwords;   // no early return: the wave reduction below needs every lane
    uint32_t on = 0, off = 0;
    if (live) {
        int wx, wy, z;
        grid.word(g, wx, wy, z);
        uint32_t set, clr;
        stamp_word(recs, nrecs, wx * 8, wy * 4, 4, z, set, clr);
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

// One lane per pattern word: the 32 x-voxels x0 + 32 wx .. of row (y0 + y, z0 + z) of the box, the ones below
// x1.  A brick word holds 8 x-voxels of the row in one byte (row y & 3), so the lane shifts together the bytes
// of the up to five brick words the run meets -- five when x0 is no multiple of 8 -- and drops the bits before
// its first voxel.  Only brick words that hold a voxel of the box are read: they lie inside the window.
__global__ void __launch_bounds__(256) k_pattern_capture(const uint32_t* __restrict__ brick, World w, rv_voxel_box box,
                                                         uint32_t nwx, uint32_t nwords, uint32_t* __restrict__ out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nwords) return;
    const uint32_t ny = (uint32_t)(box.y1 - box.y0);
    const uint32_t wx = g % nwx, t = g / nwx;
    const int y = box.y0 + (int)(t % ny), z = box.z0 + (int)(t / ny);
    const int xs = box.x0 + 32 * (int)wx;   // < x1
    const int left = box.x1 - xs;           // >= 1
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const int bwx = (xs >> 3) + k;
        if (8 * bwx < box.x1) {
            const uint32_t word = brick[brick_word_index(w, bwx, y >> 2, z)];
            acc |= (uint64_t)((word >> (8 * (y & 3))) & 0xFFu) << (8 * k);
        }
    }
    const uint32_t v = (uint32_t)(acc >> (xs & 7));
    out[g] = left >= 32 ? v : v & ((1u << left) - 1u);
}

// One lane per word of the transposed layout T of a pattern kept as A (rv_stamp.h).
__global__ void __launch_bounds__(256) k_pattern_transpose(const uint32_t* __restrict__ a, int nx, int ny, int nz,
                                                           uint32_t nwords, uint32_t* __restrict__ t) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < nwords) t[g] = pattern_transpose_word(a, nx, ny, nz, g);
}

void launch_stamp(hipStream_t s, uint32_t* brick, const World& w, const StampRec* recs, int n, const rv_voxel_box& box,
                  unsigned long long* counts) {
    const WordGrid grid = word_grid(box);
    hipLaunchKernelGGL(k_stamp, dim3(nblk(grid.nwords)), dim3(256), 0, s, brick, w, recs, n, grid, counts);
}

void launch_pattern_capture(hipStream_t s, const uint32_t* brick, const World& w, const rv_voxel_box& box, uint32_t* out) {
    const uint32_t nwx = pattern_row_words(box.x1 - box.x0);
    const uint32_t nwords = pattern_words(box.x1 - box.x0, box.y1 - box.y0, box.z1 - box.z0);
    hipLaunchKernelGGL(k_pattern_capture, dim3(nblk(nwords)), dim3(256), 0, s, brick, w, box, nwx, nwords, out);
}

void launch_pattern_transpose(hipStream_t s, const uint32_t* a, int nx, int ny, int nz, uint32_t* t) {
    const uint32_t nwords = pattern_words(nz, ny, nx);
    hipLaunchKernelGGL(k_pattern_transpose, dim3(nblk(nwords)), dim3(256), 0, s, a, nx, ny, nz, nwords, t);
}

}  // namespace rv
