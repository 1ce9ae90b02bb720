// rv_fall.hip -- gfx950 kernels of rv_world_fall (include/rvgrt.h): after the five passes of the detached
// query (rv_detached.hip), the clearance of every component -- one lane per word of D scans down under its
// runs and takes the minimum into the component's dword -- and, after the clear, the stamp that ors every
// run into the brick records `fall` rows lower.  The scan itself is in include/rvgrt/rv_fall.h, where
// rv_world_fall_at runs it on the CPU.  Two launches whatever the data.
#include "../../include/rvgrt/rv_fall.h"

namespace rv {

// ================================================================ the clearance
// Every run of D reports its constraint to its component's dword by a relaxed agent-scope atomic min; the
// lanes of a wave that hold runs of one component reduce first (the leader loop of k_detach_stats), so a
// component that fills the box costs one atomic per wave and round.  A minimum does not depend on the order.
__global__ void __launch_bounds__(256) k_fall_clearance(World w, DetachBox b, uint32_t nwords, const uint32_t* __restrict__ W,
                                                        const uint32_t* __restrict__ D, const uint32_t* __restrict__ L,
                                                        const uint32_t* __restrict__ slot, uint32_t limit,
                                                        uint32_t* clearance) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    const bool valid = g < nwords;
    const DetachWord d = detach_word(b, valid ? g : 0u);
    uint32_t m = valid ? D[g] : 0u;
    const uint32_t lane = threadIdx.x & 63u;
    while (__ballot(m != 0u)) {
        uint32_t s = 0, len = 0, r = 0, sl = 0, v = FALL_NONE;
        if (detach_next_run(m, s, len)) {
            r = L[d.base + s];   // flattened: the root itself
            sl = slot[r - 1u];
            v = fall_run_clearance(w, b, W, L, d, g, s, len, r, limit, clearance + sl);
        }
        bool todo = v != FALL_NONE;
        while (true) {
            const uint64_t act = __ballot(todo);
            if (!act) break;
            const int src = __builtin_ctzll(act);
            const uint32_t ss = (uint32_t)__shfl((int)sl, src);
            const bool mine = todo && sl == ss;
            const uint64_t same = __ballot(mine);
            uint32_t least = v;
            bool writer = mine;
            if (__popcll(same) > 1) {   // wave-uniform
                least = wave_umin(mine ? v : FALL_NONE);
                writer = lane == (uint32_t)src;
            }
            if (writer) __hip_atomic_fetch_min(clearance + ss, least, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (mine) todo = false;
        }
    }
}

// ================================================================ the stamp
// One lane per word of D.  A run of the word lands in row y - fall of its component: byte y & 3 of the brick
// dwords of up to five bricks along x (a dword holds 8 x by 4 y voxels of one z slice).  Runs of other lanes
// -- the next word of the row, other rows of the same four, other components -- share those dwords, so every
// byte goes in by a vector atomic or; or commutes, so no schedule changes a bit.  The rows were cleared by the
// launch before this one.
__global__ void __launch_bounds__(256) k_fall_stamp(uint32_t* brick, World w, DetachBox b, uint32_t nwords,
                                                    const uint32_t* __restrict__ D, const uint32_t* __restrict__ L,
                                                    const uint32_t* __restrict__ slot, const uint32_t* __restrict__ clearance,
                                                    int32_t max_fall) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= nwords) return;
    uint32_t m = D[g], s, len;
    if (!m) return;
    const DetachWord d = detach_word(b, g);
    const int xs = b.x0 + 32 * d.wx, z = b.z0 + d.zl;
    while (detach_next_run(m, s, len)) {
        const uint32_t r = L[d.base + s];
        const int y = b.y0 + d.yl - (int)fall_rows(clearance[slot[r - 1u]], max_fall);
        if (y < 0 || y >= w.Y) continue;   // never: clearance stops at the floor
        const uint64_t bits = (uint64_t)(detach_low_bits(len) << s) << (xs & 7);
        const uint32_t sh = 8u * ((uint32_t)y & 3u);
        for (int k = 0; k < 5; k++) {
            const uint32_t byte = (uint32_t)(bits >> (8 * k)) & 0xFFu;
            const int bx = (xs >> 3) + k;
            if (!byte || bx * 8 >= w.X) continue;
            atomicOr(brick + brick_word_index(w, bx, y >> 2, z), byte << sh);
        }
    }
}

// ================================================================ launchers
void launch_fall_clearance(hipStream_t s, const World& w, const DetachBox& b, const uint32_t* scratch, uint32_t nc,
                           int32_t max_fall, uint32_t* clearance) {
    const DetachLayout l = detach_layout(b);
    const uint32_t nw = b.words();
    (void)hipMemsetAsync(clearance, 0xFF, (size_t)nc * 4, s);
    hipLaunchKernelGGL(k_fall_clearance, dim3(nblk(nw)), dim3(256), 0, s, w, b, nw, scratch + l.W, scratch + l.D,
                       scratch + l.L, scratch + l.slot, fall_scan_limit(max_fall), clearance);
}

void launch_fall_stamp(hipStream_t s, uint32_t* brick, const World& w, const DetachBox& b, const uint32_t* scratch,
                       int32_t max_fall, const uint32_t* clearance) {
    const DetachLayout l = detach_layout(b);
    const uint32_t nw = b.words();
    hipLaunchKernelGGL(k_fall_stamp, dim3(nblk(nw)), dim3(256), 0, s, brick, w, b, nw, scratch + l.D, scratch + l.L,
                       scratch + l.slot, clearance, max_fall);
}

}  // namespace rv
