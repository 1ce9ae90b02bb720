// rv_stamp.h -- the stamps of rv_world_stamp (include/rvgrt.h holds the definition): which bits an oriented
// pattern lays over the voxels of a brick word, as integer functions that k_stamp (rv_stamp.hip) runs one lane
// per brick word and that rv_world_stamp_at runs on the CPU over RV_WORLD_BITS words -- the validation, the
// oriented dims and the clipped box, the 8 bits of one row of one word with the mask of the ones the stamp
// covers, the fold of a stamp into a word's set and clear masks, and the host evaluation itself.  The header
// needs only <stdint.h>, include/rvgrt.h and rv_words.h: a program can use the host evaluation without the HIP
// runtime (tests/host_stamp).
//
// Two layouts.  A pattern is kept as given, A, and with x and z transposed, T: T has the dims (nz, ny, nx) and
// T(x, y, z) = A(z, y, x), both in the ABI's layout (rows along x padded to 32-bit words) with the padding bits
// zero.  A stamp with RV_ORIENT_SWAP_XZ reads T, one without reads A, and from there on the two are the same
// case: in the layout L it reads, with L's dims (ox, oy, oz), oriented voxel (u, v, w) is L(u', v, w') -- FLIP_Z
// is an index flip, FLIP_X reads the mirrored run of 8 bits and reverses it.  Nothing gathers bit by bit.
#pragma once
#include <stdint.h>

#include "../rvgrt.h"
#include "rv_words.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RV_STAMP_HD __host__ __device__ inline
#else
#define RV_STAMP_HD inline
#endif

namespace rv {

constexpr int32_t STAMP_MAX_AT = 1 << 20;   // |at[a]| <= 2^20

RV_STAMP_HD bool pattern_dims_ok(int32_t nx, int32_t ny, int32_t nz) {
    return nx >= 1 && ny >= 1 && nz >= 1 && nx <= RV_PATTERN_MAX_DIM && ny <= RV_PATTERN_MAX_DIM && nz <= RV_PATTERN_MAX_DIM;
}
RV_STAMP_HD uint32_t pattern_row_words(int32_t nx) { return ((uint32_t)nx + 31u) >> 5; }
RV_STAMP_HD uint32_t pattern_words(int32_t nx, int32_t ny, int32_t nz) {   // <= 8 * 256 * 256
    return pattern_row_words(nx) * (uint32_t)ny * (uint32_t)nz;
}
// the bits of word wx of a row of nx voxels that are voxels
RV_STAMP_HD uint32_t pattern_word_mask(int32_t nx, uint32_t wx) {
    const uint32_t left = (uint32_t)nx - 32u * wx;   // >= 1
    return left >= 32u ? 0xFFFFFFFFu : (1u << left) - 1u;
}

// Everything but the pattern id, which the caller resolves (a context's slots, or the host form's array).
RV_STAMP_HD bool stamp_valid(const rv_stamp& s) {
    if (s.op < RV_STAMP_SET || s.op > RV_STAMP_COPY) return false;
    if (s.orient < 0 || s.orient > 7) return false;
    for (int a = 0; a < 3; a++)
        if (s.at[a] < -STAMP_MAX_AT || s.at[a] > STAMP_MAX_AT) return false;
    return true;
}

// Word g of T, g < pattern_words(nz, ny, nx), from A (dims nx, ny, nz): word (wx, y, z) of T holds
// T(32 wx + j, y, z) = A(z, y, 32 wx + j), j < 32, for the 32 wx + j below nz.
RV_STAMP_HD uint32_t pattern_transpose_word(const uint32_t* A, int32_t nx, int32_t ny, int32_t nz, uint32_t g) {
    const uint32_t nwa = pattern_row_words(nx), nwt = pattern_row_words(nz);
    const uint32_t wx = g % nwt, t = g / nwt, y = t % (uint32_t)ny, z = t / (uint32_t)ny;   // z < nx
    uint32_t out = 0;
    for (uint32_t j = 0; j < 32u && 32u * wx + j < (uint32_t)nz; j++) {
        const uint32_t az = 32u * wx + j;
        out |= ((A[(z >> 5) + nwa * (y + (uint32_t)ny * az)] >> (z & 31u)) & 1u) << j;
    }
    return out;
}

// One stamp made ready: the layout it reads (A or T by SWAP_XZ; padding bits zero) with that layout's dims, and
// its non-empty clipped box.  The list a launch or the host evaluation walks holds only stamps that meet the window.
struct StampRec {
    const uint32_t* bits;
    int32_t ox, oy, oz, nwx;
    int32_t at[3];
    int32_t op, orient;
    rv_voxel_box box;
};

// the oriented dims of a pattern of dims (nx, ny, nz)
RV_STAMP_HD void stamp_dims(int32_t nx, int32_t ny, int32_t nz, int32_t orient, int32_t o[3]) {
    const bool swap = (orient & RV_ORIENT_SWAP_XZ) != 0;
    o[0] = swap ? nz : nx; o[1] = ny; o[2] = swap ? nx : nz;
}

// The clipped box of a valid stamp of oriented dims o in a window of D voxels per axis: per axis
// [max(0, at), min(D, at + o)).  False: empty (b is then all zero).
RV_STAMP_HD bool stamp_clip(const rv_stamp& s, const int32_t o[3], const int32_t D[3], rv_voxel_box& b) {
    int32_t lo[3], hi[3];
    bool any = true;
    for (int a = 0; a < 3; a++) {
        const int32_t h = s.at[a] + o[a];   // |.| <= 2^20 + 2^8
        lo[a] = s.at[a] > 0 ? s.at[a] : 0;
        hi[a] = h < D[a] ? h : D[a];
        any = any && lo[a] < hi[a];
    }
    b = any ? rv_voxel_box{lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]} : rv_voxel_box{0, 0, 0, 0, 0, 0};
    return any;
}

// a, ta: the pattern's two layouts (ta unused without SWAP_XZ; either may be NULL where only boxes are wanted)
RV_STAMP_HD bool stamp_rec(const rv_stamp& s, int32_t nx, int32_t ny, int32_t nz, const uint32_t* a, const uint32_t* ta,
                           const int32_t D[3], StampRec& r) {
    int32_t o[3];
    stamp_dims(nx, ny, nz, s.orient, o);
    r.bits = (s.orient & RV_ORIENT_SWAP_XZ) ? ta : a;
    r.ox = o[0]; r.oy = o[1]; r.oz = o[2]; r.nwx = (int32_t)pattern_row_words(o[0]);
    r.at[0] = s.at[0]; r.at[1] = s.at[1]; r.at[2] = s.at[2];
    r.op = s.op; r.orient = s.orient;
    return stamp_clip(s, o, D, r.box);
}

// the 8 bits p .. p + 7 of a row of nwx words (bit j: p + j), zero where the row has no word: p is any
// integer, so the run may begin before the row, straddle two of its words or end past it -- a 64-bit funnel
RV_STAMP_HD uint32_t stamp_run8(const uint32_t* row, int32_t nwx, int32_t p) {
    const int32_t wi = p >> 5;   // rounds towards -inf
    const uint32_t lo = wi >= 0 && wi < nwx ? row[wi] : 0u;
    const uint32_t hi = wi + 1 >= 0 && wi + 1 < nwx ? row[wi + 1] : 0u;
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (p & 31)) & 0xFFu;
}

RV_STAMP_HD uint32_t stamp_rev8(uint32_t v) {   // bit j <-> bit 7 - j
    v = ((v & 0xF0u) >> 4) | ((v & 0x0Fu) << 4);
    v = ((v & 0xCCu) >> 2) | ((v & 0x33u) << 2);
    return ((v & 0xAAu) >> 1) | ((v & 0x55u) << 1);
}

// The oriented bits of the stamp at the voxels x = X0 .. X0 + 7 of world row (y, z) (bit b: X0 + b), and in
// cover the ones of the 8 that lie inside the stamp along x.  The caller keeps to rows inside the clipped box:
// at.y <= y < at.y + oy and at.z <= z < at.z + oz.  Bits outside cover are zero.
RV_STAMP_HD uint32_t stamp_row_bits(const StampRec& r, int32_t y, int32_t z, int32_t X0, uint32_t& cover) {
    const int32_t v = y - r.at[1], w = z - r.at[2];
    const int32_t ws = (r.orient & RV_ORIENT_FLIP_Z) ? r.oz - 1 - w : w;
    const uint32_t* row = r.bits + (uint32_t)r.nwx * ((uint32_t)v + (uint32_t)r.oy * (uint32_t)ws);
    const int32_t u0 = X0 - r.at[0];   // u of bit 0; |.| < 2^21 + 2^13
    // cover: 0 <= u0 + b < ox
    const int32_t first = u0 < 0 ? -u0 : 0, end = r.ox - u0 < 8 ? r.ox - u0 : 8;   // bits [first, end)
    cover = first < 8 && end > first ? ((1u << end) - 1u) & ~((1u << first) - 1u) : 0u;
    if (!cover) return 0;
    const uint32_t m = (r.orient & RV_ORIENT_FLIP_X) ? stamp_rev8(stamp_run8(row, r.nwx, r.ox - 8 - u0))   // u' of bit 7
                                                     : stamp_run8(row, r.nwx, u0);
    return m & cover;
}

// One stamp's bits m (zero outside cover k) folded into a word's masks; the word becomes (old & ~clr) | set.
RV_STAMP_HD void stamp_fold(int32_t op, uint32_t m, uint32_t k, uint32_t& set, uint32_t& clr) {
    if (op == RV_STAMP_SET) { set |= m; clr &= ~m; }
    else if (op == RV_STAMP_CLEAR) { clr |= m; set &= ~m; }
    else { set = (set & ~k) | m; clr = (clr & ~k) | (~m & k); }
}

// What n made-ready stamps do to the brick word's voxels x = X0 .. X0 + 7, y = Y0 .. Y0 + nrows - 1 of slice z
// (bit 8 r + b: voxel (X0 + b, Y0 + r)): the lane's loop of k_stamp, and with nrows = 1 the host's.
RV_STAMP_HD void stamp_word(const StampRec* recs, int32_t n, int32_t X0, int32_t Y0, int32_t nrows, int32_t z,
                            uint32_t& set, uint32_t& clr) {
    set = 0; clr = 0;
    for (int32_t i = 0; i < n; i++) {
        const rv_voxel_box& e = recs[i].box;
        if (z < e.z0 || z >= e.z1 || X0 + 8 <= e.x0 || X0 >= e.x1 || Y0 + nrows <= e.y0 || Y0 >= e.y1) continue;
        uint32_t m = 0, k = 0;
        for (int32_t r = 0; r < nrows; r++) {
            const int32_t y = Y0 + r;
            if (y < e.y0 || y >= e.y1) continue;
            uint32_t c;
            m |= stamp_row_bits(recs[i], y, z, X0, c) << (8 * r);
            k |= c << (8 * r);
        }
        stamp_fold(recs[i].op, m, k, set, clr);
    }
}

inline uint32_t stamp_popc(uint32_t v) {
    uint32_t n = 0;
    for (; v; v &= v - 1) n++;
    return n;
}

// rv_world_stamp_at's body: n made-ready stamps (all with non-empty boxes, whose union is u) applied in order
// to `bits` in RV_WORLD_BITS' layout (bit x | y << lx | z << (lx + ly) of uint32 words, lx >= 5), in place:
// for every group of 8 x of every row of the union box the fold above, the word written as (old & ~clr) | set,
// the bits that turned on and off counted against the word before the call.
inline void stamps_apply_linear(int lx, int ly, uint32_t* bits, const StampRec* recs, int32_t n, const rv_voxel_box& u,
                                uint64_t* n_set, uint64_t* n_cleared) {
    uint64_t on = 0, off = 0;
    if (n > 0)
        for (int32_t z = u.z0; z < u.z1; z++)
            for (int32_t y = u.y0; y < u.y1; y++)
                for (int32_t X0 = u.x0 & ~7; X0 < u.x1; X0 += 8) {   // X0 + 7 < X: X is a multiple of 8
                    uint32_t set, clr;
                    stamp_word(recs, n, X0, y, 1, z, set, clr);
                    if ((set | clr) == 0) continue;
                    const uint64_t idx = (uint64_t)X0 | (uint64_t)y << lx | (uint64_t)z << (lx + ly);
                    const uint32_t sh = (uint32_t)(idx & 31u);   // 0, 8, 16 or 24
                    uint32_t& w = bits[idx >> 5];
                    const uint32_t old = w, nw = (old & ~(clr << sh)) | (set << sh);
                    on += stamp_popc(nw & ~old);
                    off += stamp_popc(old & ~nw);
                    w = nw;
                }
    if (n_set) *n_set = on;
    if (n_cleared) *n_cleared = off;
}

}  // namespace rv
