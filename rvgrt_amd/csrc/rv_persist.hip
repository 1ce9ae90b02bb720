// rv_persist.hip -- gfx950 kernels of rv_world_persist (include/rvgrt.h): brick columns copied between the
// brick records and "column bits", the linear layout the host store keeps (rv_internal.h column_word_dword):
//   k_columns_gather   bit records -> column bits, for a device list of columns (a scroll's leaving dirty
//                      columns, rv_world_persist_flush, rv_world_columns_read),
//   k_columns_scatter  column bits -> bit records (the stored columns among those a build or a scroll step
//                      has just generated).
// A column is Y / 8 bricks of one 64-B bit record each, 64 << lbz bytes apart; in the column bits a brick's
// 16 dwords are eight 8-byte pieces, one per z slice, Y bytes apart.  One workgroup moves one column, COL_CHUNK
// bricks at a time through LDS, so that both sides move 16 B per lane: four lanes one whole record on the
// brick side, runs of 8 * (bricks of the chunk) contiguous bytes on the linear side.  Pure dword
// permutations; the CSDF records are never touched.
#include "../../include/rvgrt/rv_internal.h"

namespace rv {

constexpr uint32_t COL_CHUNK = 64;              // bricks per pass: 256 units of 16 B, one per lane
// LDS image of a chunk of nb bricks: the chunk's part of the column bits, one row of 2 nb dwords per z slice,
// rows COL_PAD dwords apart (16-B aligned rows; the four quarters of a record land 8 banks apart, so a half
// wave's 8-byte writes spread evenly over the 32 banks)
constexpr uint32_t COL_PAD = 4;
constexpr uint32_t COL_LDS = 8 * (2 * COL_CHUNK + COL_PAD);

struct ColumnChunk {
    uint32_t nb, lnb;      // bricks per chunk (a power of two, 2 .. COL_CHUNK), its log2
    uint32_t stride;       // dwords between two z rows of the LDS image
};
__device__ __forceinline__ ColumnChunk column_chunk(const ColumnGeom& g) {
    ColumnChunk c;
    c.lnb = umin((uint32_t)g.ly - 3u, 6u);
    c.nb = 1u << c.lnb;
    c.stride = 2u * c.nb + COL_PAD;
    return c;
}
// Brick-side unit u of the chunk at brick row by0: quarter q = u & 3 of brick by0 + (u >> 2), dwords 4 q ..
// 4 q + 3 of its record = words (2 by, 2 by + 1) of z slice 2 q, then of z slice 2 q + 1.  word: the first
// of them as a column word; lds: where the first pair sits in the LDS image (the second one row further).
__device__ __forceinline__ void column_unit(const ColumnGeom& g, const ColumnChunk& c, uint32_t by0, uint32_t u,
                                            uint32_t& word, uint32_t& lds) {
    const uint32_t j = u >> 2, q = u & 3u;
    word = (2u * (by0 + j)) | ((2u * q) << (g.ly - 2));
    lds = 2u * q * c.stride + 2u * j;
}
// Linear-side unit v of the chunk: 16 B of z row (4 v) >> (lnb + 1).  word: its first column word.
__device__ __forceinline__ void column_run(const ColumnGeom& g, const ColumnChunk& c, uint32_t by0, uint32_t v,
                                           uint32_t& word, uint32_t& lds) {
    const uint32_t z = (4u * v) >> (c.lnb + 1u), r = (4u * v) & (2u * c.nb - 1u);
    word = (z << (g.ly - 2)) + 2u * by0 + r;
    lds = z * c.stride + r;
}

__global__ void __launch_bounds__(256) k_columns_gather(const uint32_t* __restrict__ brick, ColumnGeom g,
                                                        const int2* __restrict__ cols, uint32_t* __restrict__ lin) {
    __shared__ uint4 image[COL_LDS / 4];
    uint32_t* const lds = reinterpret_cast<uint32_t*>(image);
    const int2 col = cols[blockIdx.x];
    const ColumnChunk c = column_chunk(g);
    uint32_t* const out = lin + ((uint64_t)blockIdx.x << (g.ly + 1));
    const uint32_t nby = 1u << (g.ly - 3), t = threadIdx.x;
    const bool on = t < 4u * c.nb;
    for (uint32_t by0 = 0; by0 < nby; by0 += c.nb) {
        if (on) {
            uint32_t word, at;
            column_unit(g, c, by0, t, word, at);
            const uint4 v = *reinterpret_cast<const uint4*>(brick + column_word_dword(g, (uint32_t)col.x, (uint32_t)col.y, word));
            *reinterpret_cast<uint2*>(lds + at) = make_uint2(v.x, v.y);
            *reinterpret_cast<uint2*>(lds + at + c.stride) = make_uint2(v.z, v.w);
        }
        __syncthreads();
        if (on) {
            uint32_t word, at;
            column_run(g, c, by0, t, word, at);
            *reinterpret_cast<uint4*>(out + word) = *reinterpret_cast<const uint4*>(lds + at);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_columns_scatter(uint32_t* __restrict__ brick, ColumnGeom g,
                                                         const int2* __restrict__ cols, const uint32_t* __restrict__ lin) {
    __shared__ uint4 image[COL_LDS / 4];
    uint32_t* const lds = reinterpret_cast<uint32_t*>(image);
    const int2 col = cols[blockIdx.x];
    const ColumnChunk c = column_chunk(g);
    const uint32_t* const in = lin + ((uint64_t)blockIdx.x << (g.ly + 1));
    const uint32_t nby = 1u << (g.ly - 3), t = threadIdx.x;
    const bool on = t < 4u * c.nb;
    for (uint32_t by0 = 0; by0 < nby; by0 += c.nb) {
        if (on) {
            uint32_t word, at;
            column_run(g, c, by0, t, word, at);
            *reinterpret_cast<uint4*>(lds + at) = *reinterpret_cast<const uint4*>(in + word);
        }
        __syncthreads();
        if (on) {
            uint32_t word, at;
            column_unit(g, c, by0, t, word, at);
            const uint2 a = *reinterpret_cast<const uint2*>(lds + at), b = *reinterpret_cast<const uint2*>(lds + at + c.stride);
            *reinterpret_cast<uint4*>(brick + column_word_dword(g, (uint32_t)col.x, (uint32_t)col.y, word)) =
                make_uint4(a.x, a.y, b.x, b.y);
        }
        __syncthreads();
    }
}

// ================================================================ launchers
void launch_columns_gather(hipStream_t s, const uint32_t* brick, const World& w, int ly, const int2* cols, uint32_t n,
                           uint32_t* lin) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_columns_gather, dim3(n), dim3(256), 0, s, brick, column_geom(w, ly), cols, lin);
}

void launch_columns_scatter(hipStream_t s, uint32_t* brick, const World& w, int ly, const int2* cols, uint32_t n,
                            const uint32_t* lin) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_columns_scatter, dim3(n), dim3(256), 0, s, brick, column_geom(w, ly), cols, lin);
}

}  // namespace rv
