// rv_edit.hip -- gfx950 kernels of rv_world_edit (include/rvgrt.h): voxel boxes written into the brick
// bit words in place, and the three CSDF passes of rv_kernels.hip (k_coarse_solid, k_csdf_x, k_csdf_yz;
// src/CoarseArray.cu:11-152) run over the boxes of coarse cells the edit can reach, with scratch indexed
// densely inside those boxes.  The arithmetic of every pass is that of the whole-grid kernels, operation
// for operation, so the bytes equal a whole-grid build's.
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

// ================================================================ local CSDF
__device__ __forceinline__ void box_cell(const CellBox& r, uint64_t idx, int& x, int& y, int& z) {
    x = r.x0 + (int)(idx % (uint64_t)r.nx);
    const uint64_t t = idx / (uint64_t)r.nx;
    y = r.y0 + (int)(t % (uint64_t)r.ny);
    z = r.z0 + (int)(t / (uint64_t)r.ny);
}

// k_coarse_solid over the cells of rs
__global__ void __launch_bounds__(256) k_edit_solid(uint8_t* __restrict__ solid, World w, CellBox rs, uint64_t n) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    int cx, cy, cz;
    box_cell(rs, idx, cx, cy, cz);
    uint32_t s = 0;
#pragma unroll
    for (int q = 0; q < 8; q++)
        s |= is_solid(w, cx * 2 + (q & 1), cy * 2 + ((q >> 1) & 1), cz * 2 + (q >> 2));
    solid[idx] = (uint8_t)s;
}

// k_csdf_x over the cells of rx; solidity in rs, which holds every in-world cell within 64 along x
__global__ void __launch_bounds__(256) k_edit_x(const uint8_t* __restrict__ solid, uint8_t* __restrict__ dx,
                                                CellBox rs, CellBox rx, int SX, uint64_t n) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    int cx, cy, cz;
    box_cell(rx, idx, cx, cy, cz);
    const uint64_t si = rs.at(cx, cy, cz);
    if (solid[si]) { dx[idx] = 0; return; }
    int min_d = 64;
    for (int i = 1; i <= 64; i++)
        if (i <= cx && solid[si - i]) { min_d = i; break; }
    for (int i = 1; i < min_d; i++)
        if (cx + i < SX && solid[si + i]) { min_d = i; break; }
    dx[idx] = (uint8_t)min_d;
}

// k_csdf_yz over the cells of rd: AXIS 1 reads src (indexed in rsrc) along y, AXIS 2 along z; rsrc holds
// every in-world cell within 64 along that axis.  TO_BRICK: the result goes to the brick records.
template <int AXIS, bool TO_BRICK>
__global__ void __launch_bounds__(256) k_edit_yz(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                 uint32_t* __restrict__ brick, World w, CellBox rsrc, CellBox rd,
                                                 int axis_len, uint64_t n) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    int cx, cy, cz;
    box_cell(rd, idx, cx, cy, cz);
    const uint64_t si = rsrc.at(cx, cy, cz);
    const uint64_t stride = AXIS == 1 ? (uint64_t)rsrc.nx : (uint64_t)rsrc.nx * (uint64_t)rsrc.ny;
    const uint8_t cur = src[si];
    uint8_t out;
    if (cur == 0) {
        out = 0;
    } else {
        const int c = AXIS == 1 ? cy : cz;
        float m = (float)cur * (float)cur;
        for (int off = 1; off <= 64; off++) {
            if ((float)(off * off) >= m) break;
            if (c - off >= 0) {
                const uint8_t nb = src[si - (uint64_t)off * stride];
                m = fminf(m, (float)nb * (float)nb + (float)off * (float)off);
            }
            if (c + off < axis_len) {
                const uint8_t nb = src[si + (uint64_t)off * stride];
                m = fminf(m, (float)nb * (float)nb + (float)off * (float)off);
            }
        }
        out = (uint8_t)fminf(64.0f, sqrtf(m));
    }
    if (!TO_BRICK) {
        dst[idx] = out;
    } else {
        const uint64_t b = brick_of(w, cx >> 2, cy >> 2, cz >> 2);
        const uint32_t local = (uint32_t)(cx & 3) | ((uint32_t)(cy & 3) << 2) | ((uint32_t)(cz & 3) << 4);
        reinterpret_cast<uint8_t*>(brick)[csdf_byte_index(w.coff, b, local)] = out;
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

void launch_edit_csdf(hipStream_t s, uint32_t* brick, const World& w, const CellBox& rs, const CellBox& rx,
                      const CellBox& ry, const CellBox& rf, uint8_t* t0, uint8_t* t1) {
    hipLaunchKernelGGL(k_edit_solid, dim3(nblk(rs.cells())), dim3(256), 0, s, t0, w, rs, rs.cells());
    hipLaunchKernelGGL(k_edit_x, dim3(nblk(rx.cells())), dim3(256), 0, s, t0, t1, rs, rx, w.SX, rx.cells());
    hipLaunchKernelGGL((k_edit_yz<1, false>), dim3(nblk(ry.cells())), dim3(256), 0, s, t1, t0, brick, w, rx, ry, w.SY,
                       ry.cells());
    hipLaunchKernelGGL((k_edit_yz<2, true>), dim3(nblk(rf.cells())), dim3(256), 0, s, t0, t1, brick, w, ry, rf, w.SZ,
                       rf.cells());
}

}  // namespace rv
