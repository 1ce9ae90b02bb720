// rv_detached.h -- the connectivity query of rv_world_detached (include/rvgrt.h holds the definition): the
// RV_HD pieces that the kernels of rv_detached.hip run one lane per word and that rv_world_detached_at runs
// word after word on the CPU -- one function, two views, as rv_bodies.h.
//
// Data.  B = [x0, x0 + nx) x [y0, y0 + ny) x [z0, z0 + nz), V = nx ny nz voxels, voxel (xl, yl, zl) of B has
// index n = xl + nx (yl + ny zl).
//   W   the box-local bits: nwx = ceil(nx / 32) words per row, word g = wx + nwx (yl + ny zl), bit i = voxel
//       xl = 32 wx + i, zero from nx on.  Everything after the gather is independent of the world's layout.
//   L   the union-find parents, V + 1 nodes: node 0 is the virtual anchor, node n + 1 is voxel n.
//       Invariant: L[p] <= p, and p is a root iff L[p] == p.  A voxel starts at the first voxel of its
//       x-run inside its word (the runs of a word are merged for free).
//
// unite(a, b) links the larger of the two roots under the smaller with one atomic min, so the root of a set
// is its least node: 0 for everything attached, else the component's seed + 1.  Nothing depends on the order
// in which lanes arrive: the final partition is that of the edges, and a set's least node is its root.
//
// Why every loop ends, whatever the other lanes do and however stale a read is:
//   * every value ever stored to L[p] is <= p (the initial run start, or the b < a of an atomic min), and a
//     location only decreases.  A load, stale or not, returns a value that was stored there, so
//     find(p) moves to a strictly smaller node at every step or stops: at most p steps.  (The loops also stop
//     on a value > p, which only corrupted memory could hold.)
//   * every value stored to L[p] is a node of p's final set: a link a -> old that an atomic min replaces by
//     a -> b is made good by the lane that replaced it, which goes on to unite(old, b).  So a stale parent is
//     still an ancestor-to-be, find returns a node of the same set, and "a == b" never joins or skips wrongly.
//   * unite trusts only what its atomic returns.  old == a: a was a root and now hangs under b, done.
//     Otherwise a was no root (the lane had believed a stale self-loop, or lost a race) and old < a: the lane
//     continues with (old, b).  Each round replaces the larger of (a, b) by a smaller node, so a + b falls
//     strictly: no lane ever waits for another.
#pragma once
#include "rv_internal.h"

namespace rv {

// the kernels' sums / minima / maxima over the 64 lanes of a wave (every lane active)
__device__ __forceinline__ uint32_t wave_add(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_umin(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = umin(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)v, o); v = v > t ? v : t; }
    return v;
}

// (a component record: DETACH_REC dwords, on the host a DetachRec -- rv_words.h)
struct DetachBox {
    int x0, y0, z0, nx, ny, nz, nwx;
    RV_HD uint32_t voxels() const { return (uint32_t)nx * (uint32_t)ny * (uint32_t)nz; }   // <= 2^21
    RV_HD uint32_t words() const { return (uint32_t)nwx * (uint32_t)ny * (uint32_t)nz; }   // <= voxels()
};
RV_HD DetachBox detach_box(const rv_voxel_box& b) {
    DetachBox d;
    d.x0 = b.x0; d.y0 = b.y0; d.z0 = b.z0;
    d.nx = b.x1 - b.x0; d.ny = b.y1 - b.y0; d.nz = b.z1 - b.z0;
    d.nwx = (d.nx + 31) >> 5;
    return d;
}

// word g of W: its position, the node of its bit 0 and how many of its bits are voxels of B
struct DetachWord { int wx, yl, zl; uint32_t base, count; };
RV_HD DetachWord detach_word(const DetachBox& b, uint32_t g) {
    DetachWord d;
    d.wx = (int)(g % (uint32_t)b.nwx);
    const uint32_t t = g / (uint32_t)b.nwx;
    d.yl = (int)(t % (uint32_t)b.ny);
    d.zl = (int)(t / (uint32_t)b.ny);
    d.base = 1u + 32u * (uint32_t)d.wx + (uint32_t)b.nx * ((uint32_t)d.yl + (uint32_t)b.ny * (uint32_t)d.zl);
    d.count = (uint32_t)imin(32, b.nx - 32 * d.wx);
    return d;
}

RV_HD uint32_t detach_low_bits(uint32_t n) { return n >= 32u ? 0xFFFFFFFFu : (1u << n) - 1u; }

// The lowest run of set bits of m: its first bit and length; the run is taken out of m.
RV_HD bool detach_next_run(uint32_t& m, uint32_t& s, uint32_t& len) {
    if (!m) return false;
    s = (uint32_t)__builtin_ctz(m);
    len = (uint32_t)__builtin_ctzll(~(uint64_t)(m >> s));   // <= 32 - s: the shift brought zeros in
    m &= ~(detach_low_bits(len) << s);
    return true;
}

// The voxel bits of (x .. x + 31, y, z), bit i = voxel x + i; (x, y, z) inside the window, voxels from X on read 0.
// World: a dword holds 8 x by 4 y voxels of one z slice, so the row is byte y & 3 of up to five words.
RV_HD uint32_t detach_row32(const World& w, int x, int y, int z) {
    const uint32_t sh = 8u * ((uint32_t)y & 3u);
    uint64_t acc = 0;
    for (int k = 0; k < 5; k++) {
        const int xb = ((x >> 3) + k) * 8;
        if (xb >= w.X || xb > x + 31) break;
        const uint32_t word = load_dword(w, voxel_word_off(w, (uint32_t)xb, (uint32_t)y, (uint32_t)z));
        acc |= (uint64_t)((word >> sh) & 0xFFu) << (8 * k);
    }
    return (uint32_t)(acc >> (x & 7));
}
// LinearWorld: a dword holds 32 x-consecutive voxels of the row.
RV_HD uint32_t detach_row32(const LinearWorld& w, int x, int y, int z) {
    uint64_t acc = voxel_load(w, voxel_word_off(w, (uint32_t)x, (uint32_t)y, (uint32_t)z));
    const int xn = (x | 31) + 1;
    if ((x & 31) && xn < w.X)
        acc |= (uint64_t)voxel_load(w, voxel_word_off(w, (uint32_t)xn, (uint32_t)y, (uint32_t)z)) << 32;
    return (uint32_t)(acc >> (x & 31));
}

// pass 1: word g of W from the world
template <class WV>
RV_HD uint32_t detach_gather_word(const WV& w, const DetachBox& b, uint32_t g) {
    const DetachWord d = detach_word(b, g);
    return detach_row32(w, b.x0 + 32 * d.wx, b.y0 + d.yl, b.z0 + d.zl) & detach_low_bits(d.count);
}

// The anchored voxels of a word: those of `bits` with a neighbour outside B that is solid by the outside rule
// -- at or above row Y empty, else below row 0 solid, else outside the window along x or z solid, else the
// voxel bit.  A neighbour differs in one coordinate, so across the y faces x and z are inside the window and
// across the x and z faces y is.  Only words on a face of B get here with a load, and only for a face that
// lies inside the window.
template <class WV>
RV_HD uint32_t detach_anchor_word(const WV& w, const DetachBox& b, const DetachWord& d, uint32_t bits) {
    if (!bits) return 0;
    const int xs = b.x0 + 32 * d.wx, y = b.y0 + d.yl, z = b.z0 + d.zl;
    const uint32_t all = detach_low_bits(d.count);
    uint32_t a = 0;
    if (d.yl == 0) a |= y == 0 ? all : detach_row32(w, xs, y - 1, z);
    if (d.yl == b.ny - 1 && y + 1 < w.Y) a |= detach_row32(w, xs, y + 1, z);
    if (d.zl == 0) a |= z == 0 ? all : detach_row32(w, xs, y, z - 1);
    if (d.zl == b.nz - 1) a |= z + 1 >= w.Z ? all : detach_row32(w, xs, y, z + 1);
    if (d.wx == 0) a |= (xs == 0 || (detach_row32(w, xs - 1, y, z) & 1u)) ? 1u : 0u;
    if (d.wx == b.nwx - 1) {
        const int xe = b.x0 + b.nx;
        a |= ((xe >= w.X || (detach_row32(w, xe, y, z) & 1u)) ? 1u : 0u) << (d.count - 1u);
    }
    return a & bits;
}

// L's accesses: relaxed, agent scope on the device (a load served by L2, the min done at the memory side);
// plain on the host, where the words are visited one after the other.
RV_HD uint32_t detach_load(const uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}
RV_HD uint32_t detach_fetch_min(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    const uint32_t old = *p;
    if (v < old) *p = v;
    return old;
#endif
}

RV_HD uint32_t detach_find(const uint32_t* L, uint32_t p) {
    for (;;) {
        const uint32_t q = detach_load(L + p);
        if (q >= p) return p;   // q == p: a root (as far as this load knows)
        p = q;
    }
}

RV_HD void detach_unite(uint32_t* L, uint32_t a, uint32_t b) {
    for (;;) {
        a = detach_find(L, a);
        b = detach_find(L, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = detach_fetch_min(L + a, b);
        if (old >= a) return;   // old == a: a was a root and now hangs under b
        a = old;                // a hung under old already (now under min(old, b)): old and b are still to join
    }
}

// pass 2: every voxel of the word starts at the first voxel of its x-run inside the word
RV_HD void detach_init_word(uint32_t* L, const DetachWord& d, uint32_t bits) {
    uint32_t m = bits, s, len;
    while (detach_next_run(m, s, len))
        for (uint32_t k = 0; k < len; k++) L[d.base + s + k] = d.base + s;
}

// pass 3: the word's edges -- across the word boundary in x, one per run of w & w_prev towards the -y and -z
// rows (within such a run both rows are connected along x), and the anchor for every run that holds an
// anchored voxel
template <class WV>
RV_HD void detach_merge_word(const WV& w, const DetachBox& b, const uint32_t* W, uint32_t* L, uint32_t g) {
    const uint32_t bits = W[g];
    if (!bits) return;
    const DetachWord d = detach_word(b, g);
    uint32_t m, s, len;
    if (d.wx > 0 && (bits & 1u) && (W[g - 1u] >> 31)) detach_unite(L, d.base, d.base - 1u);
    if (d.yl > 0) {
        m = bits & W[g - (uint32_t)b.nwx];
        while (detach_next_run(m, s, len)) detach_unite(L, d.base + s, d.base + s - (uint32_t)b.nx);
    }
    if (d.zl > 0) {
        m = bits & W[g - (uint32_t)b.nwx * (uint32_t)b.ny];
        while (detach_next_run(m, s, len)) detach_unite(L, d.base + s, d.base + s - (uint32_t)b.nx * (uint32_t)b.ny);
    }
    const uint32_t a = detach_anchor_word(w, b, d, bits);
    if (a) {
        m = bits;
        while (detach_next_run(m, s, len))
            if (a & (detach_low_bits(len) << s)) detach_unite(L, d.base + s, 0u);
    }
}

// Dwords of the device scratch of a box, in this order: counters (components, detached voxels), the mask,
// W, D (the detached bits in W's layout), L, the slot of each root, the component records (a box of V voxels
// has at most ceil(V / 2) components, the checkerboard's).
struct DetachLayout {
    size_t cnt, mask, W, D, L, slot, rec, total;
};
inline size_t detach_up64(size_t v) { return (v + 63) & ~(size_t)63; }   // whole 256-B lines
inline DetachLayout detach_layout(const DetachBox& b) {
    const size_t V = b.voxels(), NW = b.words();
    const auto up = detach_up64;
    DetachLayout l;
    l.cnt = 0;
    l.mask = 64;
    l.W = l.mask + up((V + 31) / 32);
    l.D = l.W + up(NW);
    l.L = l.D + up(NW);
    l.slot = l.L + up(V + 1);
    l.rec = l.slot + up(V);
    l.total = l.rec + up(DETACH_REC * ((V + 1) / 2));
    return l;
}

// rv_detached.hip: the five passes of the query over scratch laid out as above (counters and mask zeroed
// here), and the clear of the detached bits D inside the voxel box `box` of B
void launch_detach_query(hipStream_t s, const World& w, const DetachBox& b, uint32_t* scratch);
void launch_detach_clear(hipStream_t s, uint32_t* brick, const World& w, const DetachBox& b, const uint32_t* D,
                         const rv_voxel_box& box);

}  // namespace rv
