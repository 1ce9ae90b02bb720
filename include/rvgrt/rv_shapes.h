// rv_shapes.h -- the shaped edit of rv_world_edit_shapes (include/rvgrt.h holds the definition): which voxels
// an ellipsoid or an axis-aligned elliptic cylinder contains, as integer functions that k_edit_shapes
// (rv_shapes.hip) runs one lane per brick word and that rv_world_edit_shapes_at runs on the CPU over
// RV_WORLD_BITS words -- the validation, the clipped bounding box, the 8-bit mask of one row of one word, and
// the host evaluation itself.  The header needs only <stdint.h>, include/rvgrt.h and rv_words.h: a program can use the
// host evaluation without the HIP runtime (tests/host_shapes).
//
// Everything is in half-voxels: voxel v has its centre at 2 v + 1, d = 2 v + 1 - c2, q = r2 * r2.
//
// The arithmetic and its bound.  Every membership test below first requires d[a]^2 <= q[a] on each axis it
// looks at (a necessary condition of every kind), so whatever the caller passes, a product is only formed
// from |d| <= r2 <= RV_SHAPE_MAX_R2 = 2^9:
//     q <= 2^18;  q q <= 2^36;  q q q <= 2^54;  d^2 q q <= 2^54;
//     the ellipsoid's sum dx^2 qy qz + dy^2 qx qz + dz^2 qx qy <= 3 * 2^54 < 2^56,
// and a row's budget T = qx qy qz - dy^2 qx qz - dz^2 qx qy lies in [-2^55, 2^54]: signed 64-bit integers
// hold all of it with seven bits to spare.  |c2| <= 2^20 and v < 2^13 keep d itself inside int32.
#pragma once
#include <stdint.h>

#include "../rvgrt.h"
#include "rv_words.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RV_SHAPES_HD __host__ __device__ inline
#else
#define RV_SHAPES_HD inline
#endif

namespace rv {

constexpr int32_t SHAPE_MAX_C2 = 1 << 20;   // |c2[a]| <= 2^20

RV_SHAPES_HD bool shape_valid(const rv_edit_shape& s) {
    if (s.kind < RV_SHAPE_ELLIPSOID || s.kind > RV_SHAPE_CYLINDER_Z) return false;
    if (s.solid != 0 && s.solid != 1) return false;
    for (int a = 0; a < 3; a++) {
        if (s.r2[a] < 1 || s.r2[a] > RV_SHAPE_MAX_R2) return false;
        if (s.c2[a] < -SHAPE_MAX_C2 || s.c2[a] > SHAPE_MAX_C2) return false;
    }
    return true;
}

// n shapes as rv_world_edit_shapes takes them
inline bool shapes_ok(const rv_edit_shape* s, int32_t n) {
    if (n < 0 || n > RV_EDIT_MAX_SHAPES || (n > 0 && !s)) return false;
    for (int32_t i = 0; i < n; i++)
        if (!shape_valid(s[i])) return false;
    return true;
}

// The clipped bounding box of a valid shape in a window of D voxels per axis: per axis
// [max(0, floor((c2 - r2) / 2)), min(D, floor((c2 + r2 + 1) / 2))), >> 1 being the division that rounds
// towards -inf.  |2 v + 1 - c2| <= r2 holds exactly for the v of the unclipped interval.  False: empty.
RV_SHAPES_HD bool shape_box(const rv_edit_shape& s, const int32_t D[3], int32_t lo[3], int32_t hi[3]) {
    bool any = true;
    for (int a = 0; a < 3; a++) {
        const int32_t l = (s.c2[a] - s.r2[a]) >> 1, h = (s.c2[a] + s.r2[a] + 1) >> 1;
        lo[a] = l > 0 ? l : 0;
        hi[a] = h < D[a] ? h : D[a];
        any = any && lo[a] < hi[a];
    }
    return any;
}

// What a shape's rows share.  With T the budget of row (y, z), voxel x of the row is inside iff
// dx^2 <= qx and dx^2 * K <= T:
//   ELLIPSOID    K = qy qz, T = qx qy qz - dz^2 qx qy - dy^2 qx qz
//   CYLINDER_Y   K = qz,    T = qx qz - dz^2 qx                       (and dy^2 <= qy)
//   CYLINDER_Z   K = qy,    T = qx qy - dy^2 qx                       (and dz^2 <= qz)
//   CYLINDER_X   K = 1,     T = qx when qy qz - dz^2 qy - dy^2 qz >= 0, else negative
// T = Tz - dy^2 Cy with Tz and Cy functions of z alone; cap >= 0 (CYLINDER_X) replaces a T >= 0 by cap.
struct ShapeTerms { int64_t Tz, Cy, cap; };

RV_SHAPES_HD int64_t shape_k(const rv_edit_shape& s) {
    const int64_t qy = (int64_t)s.r2[1] * s.r2[1], qz = (int64_t)s.r2[2] * s.r2[2];
    return s.kind == RV_SHAPE_ELLIPSOID ? qy * qz : s.kind == RV_SHAPE_CYLINDER_Y ? qz
         : s.kind == RV_SHAPE_CYLINDER_Z ? qy : 1;
}

// The terms of plane z; false when the plane holds nothing (dz^2 > qz).
RV_SHAPES_HD bool shape_z_terms(const rv_edit_shape& s, int32_t z, ShapeTerms& t) {
    const int64_t qx = (int64_t)s.r2[0] * s.r2[0], qy = (int64_t)s.r2[1] * s.r2[1], qz = (int64_t)s.r2[2] * s.r2[2];
    const int64_t dz = (int64_t)2 * z + 1 - s.c2[2], dz2 = dz * dz;
    if (dz2 > qz) return false;   // from here on dz^2 <= 2^18: the bound of the header comment
    t.cap = -1;
    if (s.kind == RV_SHAPE_ELLIPSOID) { t.Tz = (qz - dz2) * (qx * qy); t.Cy = qx * qz; }
    else if (s.kind == RV_SHAPE_CYLINDER_Y) { t.Tz = (qz - dz2) * qx; t.Cy = 0; }
    else if (s.kind == RV_SHAPE_CYLINDER_Z) { t.Tz = qx * qy; t.Cy = qx; }
    else { t.Tz = (qz - dz2) * qy; t.Cy = qz; t.cap = qx; }
    return true;
}

// The budget T of row y of that plane; negative: the row holds nothing.
RV_SHAPES_HD int64_t shape_row_budget(const rv_edit_shape& s, const ShapeTerms& t, int32_t y) {
    const int64_t dy = (int64_t)2 * y + 1 - s.c2[1], dy2 = dy * dy;
    if (dy2 > (int64_t)s.r2[1] * s.r2[1]) return -1;   // dy^2 <= 2^18 below
    const int64_t T = t.Tz - dy2 * t.Cy;               // |.| <= 2^55
    return t.cap < 0 || T < 0 ? T : t.cap;
}

// P[b] = dx^2 * K of voxel X0 + b, b < 8, or INT64_MAX where dx^2 > qx (never inside): shared by the rows of
// a word.  dx^2 <= 2^18 and K <= 2^36 where the product is formed.
RV_SHAPES_HD void shape_x_products(const rv_edit_shape& s, int64_t K, int32_t X0, int64_t P[8]) {
    const int64_t qx = (int64_t)s.r2[0] * s.r2[0];
    for (int b = 0; b < 8; b++) {
        const int64_t dx = (int64_t)2 * (X0 + b) + 1 - s.c2[0], dx2 = dx * dx;
        P[b] = dx2 <= qx ? dx2 * K : INT64_MAX;
    }
}

RV_SHAPES_HD uint32_t shape_bits(const int64_t P[8], int64_t T) {
    uint32_t m = 0;
    for (int b = 0; b < 8; b++) m |= (uint32_t)(P[b] <= T) << b;
    return m;
}

// The 8-bit mask of the voxels x = X0 .. X0 + 7 of row (y, z) that a valid shape contains (bit b: X0 + b).
// The window plays no part: the caller keeps to voxels inside it.
RV_SHAPES_HD uint32_t shape_row_mask(const rv_edit_shape& s, int32_t y, int32_t z, int32_t X0) {
    ShapeTerms t;
    if (!shape_z_terms(s, z, t)) return 0;
    const int64_t T = shape_row_budget(s, t, y);
    if (T < 0) return 0;
    int64_t P[8];
    shape_x_products(s, shape_k(s), X0, P);
    return shape_bits(P, T);
}

// The clipped boxes of n valid shapes and their union, as rv_world_edit_shapes_box returns them: an empty
// box is all zero, and so is the union of none.  each may be NULL.  True when the union is not empty.
inline bool shapes_boxes(int lx, int ly, int lz, const rv_edit_shape* s, int32_t n, rv_voxel_box* each,
                         rv_voxel_box* all) {
    const int32_t D[3] = {1 << lx, 1 << ly, 1 << lz};
    rv_voxel_box u = empty_box();
    for (int32_t i = 0; i < n; i++) {
        int32_t lo[3], hi[3];
        const bool ok = shape_box(s[i], D, lo, hi);
        const rv_voxel_box b = ok ? rv_voxel_box{lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]} : rv_voxel_box{0, 0, 0, 0, 0, 0};
        if (each) each[i] = b;
        if (ok) box_include(u, b);
    }
    const bool any = u.x1 > u.x0;
    *all = any ? u : rv_voxel_box{0, 0, 0, 0, 0, 0};
    return any;
}

inline uint32_t shapes_popc(uint32_t v) {
    uint32_t n = 0;
    for (; v; v &= v - 1) n++;
    return n;
}

// rv_world_edit_shapes_at's body: n valid shapes applied in order to `bits` in RV_WORLD_BITS' layout (bit
// x | y << lx | z << (lx + ly) of uint32 words, lx >= 5: a word holds 32 x-consecutive voxels of one row),
// in place.  Like a lane of the kernel it folds, for every group of 8 x of every row of the union box, all
// shapes into a set mask and a clear mask (a later shape wins bit by bit), writes (old & ~clr) | set and
// counts the bits that turned on and off against the word before the call.
inline void shapes_apply_linear(int lx, int ly, int lz, uint32_t* bits, const rv_edit_shape* s, int32_t n,
                                uint64_t* n_set, uint64_t* n_cleared) {
    uint64_t on = 0, off = 0;
    rv_voxel_box u, each[RV_EDIT_MAX_SHAPES];
    if (n > 0 && shapes_boxes(lx, ly, lz, s, n, each, &u)) {
        for (int32_t z = u.z0; z < u.z1; z++)
            for (int32_t y = u.y0; y < u.y1; y++)
                for (int32_t X0 = u.x0 & ~7; X0 < u.x1; X0 += 8) {   // X0 + 7 < X: X is a multiple of 8
                    uint32_t set = 0, clr = 0;
                    for (int32_t i = 0; i < n; i++) {
                        const rv_voxel_box& e = each[i];   // an empty box is all zero: every test below skips it
                        if (z < e.z0 || z >= e.z1 || y < e.y0 || y >= e.y1 || X0 + 8 <= e.x0 || X0 >= e.x1) continue;
                        const uint32_t m = shape_row_mask(s[i], y, z, X0);
                        if (s[i].solid) { set |= m; clr &= ~m; } else { clr |= m; set &= ~m; }
                    }
                    if ((set | clr) == 0) continue;
                    const uint64_t idx = (uint64_t)X0 | (uint64_t)y << lx | (uint64_t)z << (lx + ly);
                    const uint32_t sh = (uint32_t)(idx & 31u);   // 0, 8, 16 or 24
                    uint32_t& w = bits[idx >> 5];
                    const uint32_t old = w, nw = (old & ~(clr << sh)) | (set << sh);
                    on += shapes_popc(nw & ~old);
                    off += shapes_popc(old & ~nw);
                    w = nw;
                }
    }
    if (n_set) *n_set = on;
    if (n_cleared) *n_cleared = off;
}

}  // namespace rv
