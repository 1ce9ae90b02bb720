// rv_detached.hip -- gfx950 kernels of rv_world_detached (include/rvgrt.h): connected-component labelling of
// the solid voxels of a box by union-find with min-roots, one lane per box-local bit word (32 x-consecutive
// voxels), in a fixed number of launches -- gather, init, merge, flatten, stats -- and the clear of what was
// found.  The per-word functions, the data layout and the argument why no lane can spin are in
// include/rvgrt/rv_detached.h; rv_world_detached_at runs the same functions on the CPU.  A launch boundary
// separates the passes, so a pass reads what the pass before wrote; inside merge and flatten the lanes agree
// through relaxed agent-scope atomics on L alone.
#include "../../include/rvgrt/rv_detached.h"

namespace rv {

// ================================================================ pass 1: gather
__global__ void __launch_bounds__(256) k_detach_gather(World w, DetachBox b, uint32_t nwords, uint32_t* __restrict__ W) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < nwords) W[g] = detach_gather_word(w, b, g);
}

// ================================================================ pass 2: init
__global__ void __launch_bounds__(256) k_detach_init(DetachBox b, uint32_t nwords, const uint32_t* __restrict__ W,
                                                     uint32_t* __restrict__ L) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= nwords) return;
    if (g == 0) L[0] = 0u;   // the virtual anchor
    detach_init_word(L, detach_word(b, g), W[g]);
}

// ================================================================ pass 3: merge
__global__ void __launch_bounds__(256) k_detach_merge(World w, DetachBox b, uint32_t nwords, const uint32_t* __restrict__ W,
                                                      uint32_t* L) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < nwords) detach_merge_word(w, b, W, L, g);
}

// ================================================================ pass 4: flatten
// L[p] = find(p) for every solid voxel (a lane that walks through a node another lane has just flattened reads
// its parent or its root: both are ancestors).  Detached = root != 0.  The word's detached bits go to D in W's
// layout and, by atomic or, to the mask in voxel-index order (a mask word is shared by two rows when nx is no
// multiple of 32).  A root takes a slot from the component counter and starts its record.
__global__ void __launch_bounds__(256) k_detach_flatten(DetachBox b, uint32_t nwords, const uint32_t* __restrict__ W,
                                                        uint32_t* L, uint32_t* __restrict__ D, uint32_t* mask,
                                                        uint32_t* __restrict__ slot, uint32_t* __restrict__ rec,
                                                        uint32_t* cnt) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    uint32_t det = 0;
    if (g < nwords) {
        const DetachWord d = detach_word(b, g);
        uint32_t m = W[g], s, len;
        while (detach_next_run(m, s, len)) {
            const uint32_t p = d.base + s, r = detach_find(L, p);
            for (uint32_t k = 0; k < len; k++) L[p + k] = r;
            if (r == 0u) continue;
            det |= detach_low_bits(len) << s;
            if (r == p) {   // the component's least voxel: its seed
                const uint32_t sl = atomicAdd(cnt, 1u);
                slot[p - 1u] = sl;
                uint32_t* q = rec + (size_t)DETACH_REC * sl;
                q[0] = 0u;
                q[1] = q[2] = q[3] = 0xFFFFFFFFu;
                q[4] = q[5] = q[6] = 0u;
                q[7] = p - 1u;
            }
        }
        D[g] = det;
        if (det) {
            const uint32_t n0 = d.base - 1u, sh = n0 & 31u;
            atomicOr(mask + (n0 >> 5), det << sh);
            if (sh && (det >> (32u - sh))) atomicOr(mask + (n0 >> 5) + 1u, det >> (32u - sh));
        }
    }
    const uint32_t total = wave_add((uint32_t)__popc(det));
    if ((threadIdx.x & 63u) == 0u && total) atomicAdd(cnt + 1, total);
}

// ================================================================ pass 5: stats
// Every detached run adds its length and its bounds to its component's record.  The lanes of a wave that
// hold runs of one component reduce first (the leader loop of rv_device.h's gd_distinct), so a component that
// fills the box costs seven atomics per wave and round, not seven per run; a run alone in its wave goes
// straight to the atomics.  All of it commutes: the record does not depend on the order.
__global__ void __launch_bounds__(256) k_detach_stats(DetachBox b, uint32_t nwords, const uint32_t* __restrict__ D,
                                                      const uint32_t* __restrict__ L, const uint32_t* __restrict__ slot,
                                                      uint32_t* rec) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    const bool valid = g < nwords;
    const DetachWord d = detach_word(b, valid ? g : 0u);
    uint32_t m = valid ? D[g] : 0u;
    const uint32_t lane = threadIdx.x & 63u;
    while (__ballot(m != 0u)) {
        uint32_t s = 0, len = 0;
        bool todo = detach_next_run(m, s, len);
        const uint32_t r = todo ? L[d.base + s] : 0u;   // flattened: the root itself
        const uint32_t xa = 32u * (uint32_t)d.wx + s, xb = xa + len - 1u;
        while (true) {
            const uint64_t act = __ballot(todo);
            if (!act) break;
            const int src = __builtin_ctzll(act);
            const uint32_t rr = (uint32_t)__shfl((int)r, src);
            const bool mine = todo && r == rr;
            const uint64_t same = __ballot(mine);
            uint32_t n = len, x0 = xa, x1 = xb, y0 = (uint32_t)d.yl, y1 = y0, z0 = (uint32_t)d.zl, z1 = z0;
            bool writer = mine;
            if (__popcll(same) > 1) {   // wave-uniform
                n = wave_add(mine ? len : 0u);
                x0 = wave_umin(mine ? xa : 0xFFFFFFFFu); x1 = wave_umax(mine ? xb : 0u);
                y0 = wave_umin(mine ? y0 : 0xFFFFFFFFu); y1 = wave_umax(mine ? y1 : 0u);
                z0 = wave_umin(mine ? z0 : 0xFFFFFFFFu); z1 = wave_umax(mine ? z1 : 0u);
                writer = lane == (uint32_t)src;
            }
            if (writer) {
                uint32_t* q = rec + (size_t)DETACH_REC * slot[rr - 1u];
                atomicAdd(q, n);
                atomicMin(q + 1, x0); atomicMin(q + 2, y0); atomicMin(q + 3, z0);
                atomicMax(q + 4, x1); atomicMax(q + 5, y1); atomicMax(q + 6, z1);
            }
            if (mine) todo = false;
        }
    }
}

// ================================================================ pass 6: clear
// One lane per word of the grid (WordGrid, rv_words.h) of the voxel box that bounds the detached voxels: the
// lane and-nots the word's detached voxels out and is the word's only writer.
__global__ void __launch_bounds__(256) k_detach_clear(uint32_t* __restrict__ brick, World w, DetachBox b,
                                                      const uint32_t* __restrict__ D, WordGrid grid) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= grid.nwords) return;
    int wx, wy, z;
    grid.word(g, wx, wy, z);
    const int xl = wx * 8 - b.x0, zl = z - b.z0;   // xl >= -7; zl inside B
    uint32_t clr = 0;
    for (int r = 0; r < 4; r++) {
        const int yl = wy * 4 + r - b.y0;
        if (yl < 0 || yl >= b.ny) continue;
        const uint32_t* row = D + ((uint32_t)zl * (uint32_t)b.ny + (uint32_t)yl) * (uint32_t)b.nwx;
        uint32_t byte;
        if (xl >= 0) {   // D is zero from nx on, and xl < nx: the word exists
            const int wi = xl >> 5;
            uint64_t win = row[wi];
            if (wi + 1 < b.nwx) win |= (uint64_t)row[wi + 1] << 32;
            byte = (uint32_t)(win >> (xl & 31)) & 0xFFu;
        } else {
            byte = (row[0] << (uint32_t)(-xl)) & 0xFFu;
        }
        clr |= byte << (8 * r);
    }
    if (!clr) return;
    brick[brick_word_index(w, wx, wy, z)] &= ~clr;
}

// ================================================================ launchers

void launch_detach_query(hipStream_t s, const World& w, const DetachBox& b, uint32_t* scratch) {
    const DetachLayout l = detach_layout(b);
    const uint32_t nw = b.words();
    uint32_t *cnt = scratch + l.cnt, *mask = scratch + l.mask, *W = scratch + l.W, *D = scratch + l.D, *L = scratch + l.L,
             *slot = scratch + l.slot, *rec = scratch + l.rec;
    (void)hipMemsetAsync(scratch, 0, l.W * 4, s);   // the counters and the mask
    hipLaunchKernelGGL(k_detach_gather, dim3(nblk(nw)), dim3(256), 0, s, w, b, nw, W);
    hipLaunchKernelGGL(k_detach_init, dim3(nblk(nw)), dim3(256), 0, s, b, nw, W, L);
    hipLaunchKernelGGL(k_detach_merge, dim3(nblk(nw)), dim3(256), 0, s, w, b, nw, W, L);
    hipLaunchKernelGGL(k_detach_flatten, dim3(nblk(nw)), dim3(256), 0, s, b, nw, W, L, D, mask, slot, rec, cnt);
    hipLaunchKernelGGL(k_detach_stats, dim3(nblk(nw)), dim3(256), 0, s, b, nw, D, L, slot, rec);
}

void launch_detach_clear(hipStream_t s, uint32_t* brick, const World& w, const DetachBox& b, const uint32_t* D,
                         const rv_voxel_box& box) {
    const WordGrid grid = word_grid(box);
    hipLaunchKernelGGL(k_detach_clear, dim3(nblk(grid.nwords)), dim3(256), 0, s, brick, w, b, D, grid);
}

}  // namespace rv
