// rv_bodies.h -- the swept-box collision of rv_world_bodies_move (include/rvgrt.h holds the definition):
// one RV_HD function, templated over the world view, that the kernel of rv_bodies.hip calls per lane
// (World, the brick records the frames read) and rv_world_bodies_move_at calls on the CPU (LinearWorld,
// RV_WORLD_BITS layout).
//
// Every solidity test is a box of cells [x0, x1] x [y0, y1] x [z0, z1] (inclusive; a slab is a box one cell
// thick, the start test the whole body).  box_test resolves the parts outside the window from the rule --
// at or above row Y nothing, below row 0 the floor, else outside x or z the walls, or nothing with open edges --
// without a load, clips the box to the window and hands the rest to the view's bodies_box_bits, which tests
// whole bit words under a mask, never voxel by voxel:
//   World        a dword holds 8 x by 4 y voxels of one z slice (voxel_word_off, bit (x & 7) | (y & 3) << 3).
//                Per word the x range is an 8-bit mask replicated over the four rows, and-ed with the mask
//                of the wanted rows.  A slab normal to z is a run of such words over (x / 8, y / 4); one
//                normal to y keeps the x mask in the single row j & 3; one normal to x keeps bit i & 7 of
//                each wanted row.
//   LinearWorld  a dword holds 32 x-consecutive voxels of one row: the x range is a run of bits per word.
#pragma once
#include "../rvgrt.h"
#include "rv_device.h"

namespace rv {

constexpr float BODY_EPS = 0.0078125f;          // 2^-7
constexpr int64_t BODIES_MAX = (int64_t)1 << 24;

// [lo, hi]: the cells an axis occupies, occ(lo, size) = [floor(lo + EPS), ceil((lo + size) - EPS) - 1]
RV_HD void body_occ(float lo, float size, int& c0, int& c1) {
    c0 = (int)floorf(lo + BODY_EPS);
    const float hi = lo + size;
    c1 = (int)ceilf(hi - BODY_EPS) - 1;
}

// Any set bit among the in-window voxels [x0, x1] x [y0, y1] x [z0, z1] (all inside the window, none empty).
RV_HD bool bodies_box_bits(const World& w, int x0, int x1, int y0, int y1, int z0, int z1) {
    const uint32_t sy = (uint32_t)w.lbz + BRICK_SHIFT, sx = (uint32_t)w.lbzy + BRICK_SHIFT;
    uint32_t any = 0;
    for (int q = y0 >> 2; q <= (y1 >> 2); q++) {
        // rows of word q: bytes ra .. rb of the dword
        const uint32_t ra = (uint32_t)imax(y0 - 4 * q, 0), rb = (uint32_t)imin(y1 - 4 * q, 3);
        const uint32_t rows = (0xFFFFFFFFu >> (8u * (3u - rb))) & (0xFFFFFFFFu << (8u * ra));
        const uint32_t oy = (((uint32_t)q & 1u) << 2) | (((uint32_t)q >> 1) << sy);
        for (int b = x0 >> 3; b <= (x1 >> 3); b++) {
            const uint32_t xa = (uint32_t)imax(x0 - 8 * b, 0), xb = (uint32_t)imin(x1 - 8 * b, 7);
            const uint32_t xm = (0xFFu >> (7u - xb)) & (0xFFu << xa) & 0xFFu;
            const uint32_t mask = (xm * 0x01010101u) & rows;
            const uint32_t oxy = oy | ((uint32_t)b << sx);
            for (int z = z0; z <= z1; z++) any |= load_dword(w, oxy | ((uint32_t)z << 3)) & mask;
        }
        if (any) return true;
    }
    return false;
}
RV_HD bool bodies_box_bits(const LinearWorld& w, int x0, int x1, int y0, int y1, int z0, int z1) {
    for (int z = z0; z <= z1; z++)
        for (int y = y0; y <= y1; y++) {
            uint32_t any = 0;
            for (int b = x0 >> 5; b <= (x1 >> 5); b++) {
                const uint32_t xa = (uint32_t)imax(x0 - 32 * b, 0), xb = (uint32_t)imin(x1 - 32 * b, 31);
                const uint32_t mask = (0xFFFFFFFFu >> (31u - xb)) & (0xFFFFFFFFu << xa);
                any |= voxel_load(w, voxel_word_off(w, (uint32_t)(32 * b), (uint32_t)y, (uint32_t)z)) & mask;
            }
            if (any) return true;
        }
    return false;
}

// Whether any cell of the box is solid by the rule; inwin: whether a voxel inside the window is.
template <class WV>
RV_HD bool bodies_box_test(const WV& w, bool open, int x0, int x1, int y0, int y1, int z0, int z1, bool& inwin) {
    bool edge = y0 < 0;                                                       // the floor
    // the walls, below row Y (above it every cell is empty)
    if (!open && y0 < w.Y) edge = edge || x0 < 0 || z0 < 0 || x1 >= w.X || z1 >= w.Z;
    x0 = imax(x0, 0); y0 = imax(y0, 0); z0 = imax(z0, 0);
    x1 = imin(x1, w.X - 1); y1 = imin(y1, w.Y - 1); z1 = imin(z1, w.Z - 1);
    inwin = x0 <= x1 && y0 <= y1 && z0 <= z1 && bodies_box_bits(w, x0, x1, y0, y1, z0, z1);
    return edge || inwin;
}

// One axis of the sweep (A = 0 x, 1 y, 2 z): lo[A] moves by d through the slabs it newly occupies, in order
// of travel, and stops in front of the first that holds a solid cell.  c0 / c1: the occupied cells of the
// three axes at their current values, kept up to date.
template <int A, class WV>
RV_HD void bodies_sweep_axis(const WV& w, bool open, float (&lo)[3], const float (&size)[3], float d, int (&c0)[3],
                             int (&c1)[3], uint32_t& flags) {
    if (d == 0.0f) return;
    const float t = lo[A] + d;
    int n0, n1;
    body_occ(t, size[A], n0, n1);
    int r0[3] = {c0[0], c0[1], c0[2]}, r1[3] = {c1[0], c1[1], c1[2]};
    const bool up = d > 0.0f;
    const int first = up ? c1[A] + 1 : c0[A] - 1, last = up ? n1 : n0, s = up ? 1 : -1;
    bool blocked = false;
    for (int i = first; up ? i <= last : i >= last; i += s) {
        r0[A] = r1[A] = i;
        bool inwin;
        if (bodies_box_test(w, open, r0[0], r1[0], r0[1], r1[1], r0[2], r1[2], inwin)) {
            // max / min that keep lo where the two compare equal (a -0 stays a -0 on every target)
            const float v = up ? (float)i - size[A] : (float)(i + 1);
            if (up ? v > lo[A] : v < lo[A]) lo[A] = v;
            flags |= (up ? 2u : 1u) << (2 * A);
            if (!inwin) flags |= RV_BODY_EDGE;
            blocked = true;
            break;
        }
    }
    if (!blocked) lo[A] = t;
    body_occ(lo[A], size[A], c0[A], c1[A]);
}

RV_HD bool body_valid(const float (&lo)[3], const float (&size)[3], const float (&delta)[3]) {
    bool ok = true;
    for (int a = 0; a < 3; a++)   // a NaN fails every comparison
        ok = ok && fabsf(lo[a]) <= 16384.0f && size[a] >= 0.03125f && size[a] <= 16.0f && fabsf(delta[a]) <= 64.0f;
    return ok;
}

// rv_world_bodies_move for one body.  The body comes as its nine dwords so that an invalid body's lo goes
// out bit for bit (a NaN's payload included).
template <class WV>
RV_HD void bodies_move_one(const WV& w, bool open, const uint32_t (&in)[9], uint32_t (&out)[4]) {
    float lo[3], size[3], delta[3];
    for (int a = 0; a < 3; a++) {
        lo[a] = __builtin_bit_cast(float, in[a]);
        size[a] = __builtin_bit_cast(float, in[3 + a]);
        delta[a] = __builtin_bit_cast(float, in[6 + a]);
    }
    if (!body_valid(lo, size, delta)) {
        out[0] = in[0]; out[1] = in[1]; out[2] = in[2];
        out[3] = RV_BODY_INVALID;
        return;
    }
    int c0[3], c1[3];
    for (int a = 0; a < 3; a++) body_occ(lo[a], size[a], c0[a], c1[a]);
    bool inwin;
    uint32_t flags = bodies_box_test(w, open, c0[0], c1[0], c0[1], c1[1], c0[2], c1[2], inwin) ? RV_BODY_START_SOLID : 0u;
    bodies_sweep_axis<1>(w, open, lo, size, delta[1], c0, c1, flags);   // landing before walking
    bodies_sweep_axis<0>(w, open, lo, size, delta[0], c0, c1, flags);
    bodies_sweep_axis<2>(w, open, lo, size, delta[2], c0, c1, flags);
    for (int a = 0; a < 3; a++) out[a] = __builtin_bit_cast(uint32_t, lo[a]);
    out[3] = flags;
}

// rv_bodies.hip: n bodies (36 B each) -> n results (16 B each), one lane per body
void launch_bodies_move(hipStream_t s, const World& w, const void* in, int64_t n, bool open, void* out);

}  // namespace rv
