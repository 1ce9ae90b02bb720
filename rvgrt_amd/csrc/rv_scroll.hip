// rv_scroll.hip -- gfx950 kernels of rv_world_scroll (include/rvgrt.h): the world window moved over the
// terrain in place.  One step moves the window along one axis (x or z) by whole bricks:
//   k_scroll_bricks  the bit record and the CSDF record of every retained brick to its new brick index,
//   k_fill_box       the entering slab's voxels (k_fill_bricks' word body, fill_word),
//   k_scroll_gi      the RGBA8 cell of every retained GI cell to its new index,
//   k_scroll_gi_init the entering GI cells (k_gi_init's cell, gi_init_cell),
// and, when the texture origin follows the window (rv_texture_follow_scroll),
//   k_scroll_tex     the retained entries of sampleTexture's tile table to their new index, in place,
//   k_tex_box        the entering entries (k_tex_table's entry, tex_table_entry_at).
// The brick and GI moves go through a dense scratch copy of what is retained (source and destination overlap, and no
// order of concurrently running lanes makes an in-place move safe): one launch gathers the retained
// records into the scratch, a second one writes them to their new places.  The CSDF of the slabs a step can
// change is rebuilt by launch_csdf_box (rv_kernels.hip), the passes of rv_csdf_build.
#include "../../include/rvgrt/rv_shade.h"

namespace rv {

// The retained records of a one-axis shift, as runs of contiguous bricks (bricks are ordered z fastest,
// then y, then x: brick_of).  Retained brick r of the dense order sits at
//   dst = (r / run) * row + r % run + dst0      after the shift, and came from      src = dst + delta.
// x axis: one run (the retained x planes are contiguous), z axis: one run per (bx, by) row of NBZ bricks.
struct BrickShift {
    uint64_t nret;    // retained bricks
    uint64_t run;     // contiguous retained bricks per row
    uint64_t row;     // bricks between the starts of two rows
    uint64_t dst0;    // first retained brick's new index
    int64_t delta;    // old index - new index
};

// 16 B per lane: four lanes move one 64-B record, a wave 1 KiB of contiguous records.  Unit g: quarter g & 3
// of dense record g >> 2; records [0, nret) are the bit records, [nret, 2 nret) the CSDF records (their own
// region, coff bytes further on).  TO_SCRATCH: brick array (old index) -> scratch (dense); else scratch ->
// brick array (new index).
template <bool TO_SCRATCH>
__global__ void __launch_bounds__(256) k_scroll_bricks(uint32_t* __restrict__ brick, uint4* __restrict__ scratch,
                                                       BrickShift s, uint32_t coff) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (g >= s.nret * 8u) return;
    const uint64_t rec = g >> 2;
    const uint32_t q = (uint32_t)g & 3u;
    const bool csdf = rec >= s.nret;
    const uint64_t r = csdf ? rec - s.nret : rec;
    const uint64_t dst = (r / s.run) * s.row + r % s.run + s.dst0;
    const uint64_t b = TO_SCRATCH ? (uint64_t)((int64_t)dst + s.delta) : dst;
    uint4* p = reinterpret_cast<uint4*>(reinterpret_cast<char*>(brick) + (csdf ? (size_t)coff : 0) +
                                        (b << BRICK_SHIFT)) + q;
    if (TO_SCRATCH) scratch[g] = *p;
    else *p = scratch[g];
}

// k_fill_bricks over the bricks of a box: one lane per bit word, word fastest, then the box's bricks z fastest.
__global__ void __launch_bounds__(256) k_fill_box(uint32_t* __restrict__ brick, World w, CellBox b, int seed_x,
                                                  int seed_z, uint64_t nwords) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (g >= nwords) return;
    const uint32_t wd = (uint32_t)(g & 15u);
    uint64_t t = g >> 4;
    const uint32_t bz = (uint32_t)b.z0 + (uint32_t)(t % (uint64_t)b.nz);
    t /= (uint64_t)b.nz;
    const uint32_t by = (uint32_t)b.y0 + (uint32_t)(t % (uint64_t)b.ny), bx = (uint32_t)b.x0 + (uint32_t)(t / (uint64_t)b.ny);
    brick[bits_word_index(brick_of(w, (int)bx, (int)by, (int)bz), wd)] = fill_word(bx, by, bz, wd, seed_x, seed_z);
}

// The GI cells of the box b (the retained cells at their new places), x fastest: cell d of the dense order
// is (x, y, z), and held cell (x + sx, y, z + sz) before the shift.
template <bool TO_SCRATCH>
__global__ void __launch_bounds__(256) k_scroll_gi(uint32_t* __restrict__ gi, uint32_t* __restrict__ scratch, World w,
                                                   CellBox b, int sx, int sz) {
    const uint64_t d = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (d >= b.cells()) return;
    int x, y, z;
    b.cell(d, x, y, z);
    if (TO_SCRATCH) scratch[d] = gi[gi_cell_index(w, x + sx, y, z + sz)];
    else gi[gi_cell_index(w, x, y, z)] = scratch[d];
}

// k_gi_init's cell over the entering cells, straight into the grid (the trace reads the voxels only).
__global__ void __launch_bounds__(256) k_scroll_gi_init(uint32_t* __restrict__ gi, World w, f3 sun, CellBox b,
                                                        uint32_t lit, unsigned long long* counters) {
    const uint64_t d = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool on = d < b.cells();
    if (on) {
        int x, y, z;
        b.cell(d, x, y, z);
        const uint32_t cell = gi_cell_index(w, x, y, z);
        gi[cell] = gi_init_cell(w, sun, cell, lit);
    }
    const unsigned long long traced = __ballot(on);
    if ((threadIdx.x & 63u) == 0 && traced) atomicAdd(&counters[CNT_GI_TRACES], (unsigned long long)__popcll(traced));
}

// The tile table (World::tex: 2-KiB bricks of 512 entries, ordered bz | bx << lbz | by << (lbz + lbx)) has
// no room for a dense scratch copy (4 B per voxel), so it moves slab by slab: one launch copies a slab of at
// most |nb| bricks along the axis to the index |nb| bricks away, so its source and destination are disjoint,
// and the launches walk away from the face the entries leave through, in stream order, so a destination is
// only ever a slab that an earlier launch has read (launch_scroll_tex).  One launch's slab as runs of
// contiguous bricks: brick r of the dense order sits at dst = (r / run) * row + r % run + dst0 and is read
// from dst + delta.  x axis: one run of width * NBZ bricks per by plane; z axis: one run of width bricks
// per (bx, by) row.  16 B per lane, 128 lanes per brick; the table has < 2^25 bricks.
struct TexSlab {
    uint32_t nbricks, run, row, dst0;
    int32_t delta;
};
__global__ void __launch_bounds__(256) k_scroll_tex(uint4* __restrict__ tex, TexSlab s) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t r = (uint32_t)(g >> 7);
    if (r >= s.nbricks) return;
    const uint32_t dst = (r / s.run) * s.row + r % s.run + s.dst0;
    const uint64_t q = g & 127u;
    tex[((uint64_t)dst << 7) + q] = tex[((uint64_t)(uint32_t)((int32_t)dst + s.delta) << 7) + q];
}

// tex_table_entry_at over the table bricks of the box b (bricks; y below tex_ny / 8): one lane per entry, the
// table's own order inside a brick, then the box's bricks z fastest, then x, then y.
__global__ void __launch_bounds__(256) k_tex_box(uint32_t* __restrict__ tex, World w, CellBox b, uint64_t n) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (g >= n) return;
    const uint32_t l = (uint32_t)g & 511u;
    uint64_t t = g >> 9;
    const uint32_t bz = (uint32_t)b.z0 + (uint32_t)(t % (uint64_t)b.nz);
    t /= (uint64_t)b.nz;
    const uint32_t bx = (uint32_t)b.x0 + (uint32_t)(t % (uint64_t)b.nx), by = (uint32_t)b.y0 + (uint32_t)(t / (uint64_t)b.nx);
    const uint32_t x = bx * 8u + ((l >> 3) & 7u), y = by * 8u + (l >> 6), z = bz * 8u + (l & 7u);
    tex[tex_index(w, x, y, z)] = tex_table_entry_at(w, x, y, z);
}

// ================================================================ launchers
void launch_scroll_bricks(hipStream_t s, uint32_t* brick, const World& w, int axis, int nb, void* scratch) {
    const uint64_t NBX = (uint64_t)w.X >> 3, NBY = (uint64_t)w.Y >> 3, NBZ = (uint64_t)w.Z >> 3;
    const uint64_t a = (uint64_t)(nb < 0 ? -nb : nb);   // bricks the window moves by; a < the axis' bricks
    BrickShift sh;
    if (axis == 0) {
        const uint64_t plane = NBY * NBZ;   // = 1 << lbzy
        sh.nret = (NBX - a) * plane;
        sh.run = sh.nret;
        sh.row = 0;
        sh.dst0 = nb > 0 ? 0 : a * plane;
        sh.delta = (int64_t)nb * (int64_t)plane;
    } else {
        sh.run = NBZ - a;
        sh.row = NBZ;
        sh.nret = NBX * NBY * sh.run;
        sh.dst0 = nb > 0 ? 0 : a;
        sh.delta = nb;
    }
    if (sh.nret == 0) return;
    const dim3 grid(nblk(sh.nret * 8u)), wg(256);
    hipLaunchKernelGGL(k_scroll_bricks<true>, grid, wg, 0, s, brick, static_cast<uint4*>(scratch), sh, w.coff);
    hipLaunchKernelGGL(k_scroll_bricks<false>, grid, wg, 0, s, brick, static_cast<uint4*>(scratch), sh, w.coff);
}

void launch_fill_box(hipStream_t s, uint32_t* brick, const World& w, const CellBox& bricks, int sx, int sz) {
    const uint64_t nwords = bricks.cells() * 16u;
    if (nwords == 0) return;
    hipLaunchKernelGGL(k_fill_box, dim3(nblk(nwords)), dim3(256), 0, s, brick, w, bricks, sx, sz, nwords);
}

void launch_scroll_gi(hipStream_t s, uint32_t* gi, const World& w, const CellBox& kept, int sx, int sz,
                      void* scratch) {
    if (kept.cells() == 0) return;
    const dim3 grid(nblk(kept.cells())), wg(256);
    hipLaunchKernelGGL(k_scroll_gi<true>, grid, wg, 0, s, gi, static_cast<uint32_t*>(scratch), w, kept, sx, sz);
    hipLaunchKernelGGL(k_scroll_gi<false>, grid, wg, 0, s, gi, static_cast<uint32_t*>(scratch), w, kept, sx, sz);
}

void launch_scroll_gi_init(hipStream_t s, uint32_t* gi, const World& w, f3 sun, const CellBox& entering, uint32_t lit,
                           unsigned long long* counters) {
    if (entering.cells() == 0) return;
    hipLaunchKernelGGL(k_scroll_gi_init, dim3(nblk(entering.cells())), dim3(256), 0, s, gi, w, sun, entering, lit,
                       counters);
}

void launch_scroll_tex(hipStream_t s, uint32_t* tex, const World& w, int axis, int nb) {
    const int NBX = w.X >> 3, NBY = (int)(w.tex_ny >> 3), NBZ = w.Z >> 3, NB = axis == 0 ? NBX : NBZ;
    const int a = nb < 0 ? -nb : nb;   // bricks the window moves by; 0 < a < NB
    // destination slabs [lo, hi) along the axis, read from [lo + nb, hi + nb): from the face the entries leave
    // through (index 0 for nb > 0, NB for nb < 0) to the other end of the retained range
    for (int j = 0; j * a < NB - a; j++) {
        const int lo = nb > 0 ? j * a : std::max(NB - (j + 1) * a, a);
        const int hi = nb > 0 ? std::min(lo + a, NB - a) : NB - j * a;
        TexSlab sl;
        if (axis == 0) {
            sl.run = (uint32_t)(hi - lo) * (uint32_t)NBZ;
            sl.row = (uint32_t)NBX * (uint32_t)NBZ;
            sl.nbricks = sl.run * (uint32_t)NBY;
            sl.dst0 = (uint32_t)lo * (uint32_t)NBZ;
            sl.delta = nb * NBZ;
        } else {
            sl.run = (uint32_t)(hi - lo);
            sl.row = (uint32_t)NBZ;
            sl.nbricks = sl.run * (uint32_t)NBX * (uint32_t)NBY;
            sl.dst0 = (uint32_t)lo;
            sl.delta = nb;
        }
        if (sl.nbricks == 0) continue;
        hipLaunchKernelGGL(k_scroll_tex, dim3(nblk((uint64_t)sl.nbricks * 128u)), dim3(256), 0, s,
                           reinterpret_cast<uint4*>(tex), sl);
    }
}

void launch_tex_box(hipStream_t s, uint32_t* tex, const World& w, const CellBox& bricks) {
    const uint64_t n = bricks.cells() * 512u;
    if (n == 0) return;
    hipLaunchKernelGGL(k_tex_box, dim3(nblk(n)), dim3(256), 0, s, tex, w, bricks, n);
}

}  // namespace rv
