// rv_words.h -- what the in-place voxel writes share about a voxel box (rv_voxel_box, include/rvgrt.h): the
// grid of brick words under it that k_edit_bits, k_edit_shapes and k_detach_clear run one lane per word of, the
// brick columns under it, and the component record of the detached query.  The header needs only <stdint.h>
// and include/rvgrt.h, as rv_shapes.h: tests/host_shapes checks it in a program without the HIP runtime.
#pragma once
#include <stdint.h>

#include "../rvgrt.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RV_WORDS_HD __host__ __device__ inline
#else
#define RV_WORDS_HD inline
#endif

namespace rv {

// The union of voxel boxes: box_include grows acc to hold b; empty_box() is its identity.
RV_WORDS_HD rv_voxel_box empty_box() { return rv_voxel_box{INT32_MAX, INT32_MAX, INT32_MAX, 0, 0, 0}; }
RV_WORDS_HD void box_include(rv_voxel_box& acc, const rv_voxel_box& b) {
    acc.x0 = b.x0 < acc.x0 ? b.x0 : acc.x0; acc.y0 = b.y0 < acc.y0 ? b.y0 : acc.y0; acc.z0 = b.z0 < acc.z0 ? b.z0 : acc.z0;
    acc.x1 = b.x1 > acc.x1 ? b.x1 : acc.x1; acc.y1 = b.y1 > acc.y1 ? b.y1 : acc.y1; acc.z1 = b.z1 > acc.z1 ? b.z1 : acc.z1;
}

// The brick words under a voxel box.  A word holds 8 x by 4 y voxels of one z slice: word (wx, wy, z) is the
// voxels x = 8 wx .. 8 wx + 7 (bit & 7), y = 4 wy .. 4 wy + 3 (bit >> 3) of slice z, and lies inside the window
// because X is a multiple of 8 and Y of 4.  The grid is the words that hold a voxel of the box, indexed densely
// with z fastest.
// WordGrid's index is 32-bit: rv_create bounds a world at 2^34 voxels (dims_ok), so a grid has at most
// WORD_GRID_MAX = 2^29 words; word_grid<uint64_t>(b).nwords is the count without that assumption, for a host
// that wants to check it.  Index is a parameter because k_edit_shapes keeps its 64-bit index: the 32-bit form
// needs five more VGPRs (60 against 55).  The fields stand in the order a lane reads them (fewest SGPRs).
template <class Index>
struct WordGridT {
    Index nwords;
    uint32_t nwz, nwy;
    int32_t wx0, wy0, wz0;
    // word g < nwords of the grid
    RV_WORDS_HD void word(Index g, int& wx, int& wy, int& z) const {
        z = wz0 + (int)(g % (Index)nwz);
        const Index t = g / (Index)nwz;
        wy = wy0 + (int)(t % (Index)nwy);
        wx = wx0 + (int)(t / (Index)nwy);
    }
};
using WordGrid = WordGridT<uint32_t>;
constexpr uint64_t WORD_GRID_MAX = (uint64_t)1 << 29;

// b non-empty and inside the window
template <class Index = uint32_t>
RV_WORDS_HD WordGridT<Index> word_grid(const rv_voxel_box& b) {
    WordGridT<Index> g;
    g.wx0 = b.x0 >> 3; g.wy0 = b.y0 >> 2; g.wz0 = b.z0;
    const uint32_t nwx = (uint32_t)(((b.x1 - 1) >> 3) - g.wx0 + 1);
    g.nwy = (uint32_t)(((b.y1 - 1) >> 2) - g.wy0 + 1);
    g.nwz = (uint32_t)(b.z1 - b.z0);
    g.nwords = (Index)nwx * g.nwy * g.nwz;
    return g;
}

// Brick columns [bx0, bx1) x [bz0, bz1) of the window (8 x Y x 8 voxels each); the ones under a non-empty box
struct ColumnRange { int bx0, bx1, bz0, bz1; };
RV_WORDS_HD ColumnRange columns_under(const rv_voxel_box& b) {
    return ColumnRange{b.x0 >> 3, ((b.x1 - 1) >> 3) + 1, b.z0 >> 3, ((b.z1 - 1) >> 3) + 1};
}

// A component record of the detached query (rv_detached.h), DETACH_REC dwords in this order: the voxels, the
// least and the greatest x, y, z (box-local, both inclusive) and the seed, the index n of the component's least
// voxel.  The kernels write the dwords by index (k_detach_flatten, k_detach_stats); the host reads them here.
constexpr uint32_t DETACH_REC = 8;
struct DetachRec { uint32_t voxels, lo[3], hi[3], seed; };
static_assert(sizeof(DetachRec) == 4 * DETACH_REC, "DetachRec is the record's dwords");

// The record's box in window coordinates, half-open.  Box: the query's box, anything with the origin x0, y0,
// z0 (DetachBox, or the rv_voxel_box it was made from).
template <class Box>
RV_WORDS_HD rv_voxel_box detach_rec_box(const Box& b, const DetachRec& r) {
    return rv_voxel_box{b.x0 + (int32_t)r.lo[0], b.y0 + (int32_t)r.lo[1], b.z0 + (int32_t)r.lo[2],
                        b.x0 + (int32_t)r.hi[0] + 1, b.y0 + (int32_t)r.hi[1] + 1, b.z0 + (int32_t)r.hi[2] + 1};
}

}  // namespace rv
