// rv_fall.h -- the clearance of rv_world_fall (include/rvgrt.h holds the definition): how far the detached
// voxels of one word of D can drop, as RV_HD functions that k_fall_clearance (rv_fall.hip) runs one lane per
// word and rv_world_fall_at runs word after word on the CPU -- one function, two views, as rv_detached.h.
//
// Data: what launch_detach_query left (rv_detached.h) -- W the box-local bits, D the detached bits in W's
// layout, L flattened (L[n + 1] is the root of voxel n: 0 when attached, else its component's seed + 1), the
// slot of each root -- and one dword per slot, the component's clearance so far, which starts at all ones
// and only falls.
//
// A run of D inside a word is x-adjacent, so it is part of one component c with root r.  The run looks down
// row after row, e = 1, 2, ..., at the cells under its columns, having counted e - 1 empty rows:
//   * below row 0 is the floor: the run's constraint is e - 1;
//   * inside B the row is W's word one row down (same wx: the same bit alignment).  A hit bit whose root is r
//     is an own voxel: its columns drop out of the scan without a constraint, because that lower voxel scans
//     for itself and its constraint is the tighter one (what lies e' rows under it lies e' + its distance
//     under this voxel).  A hit bit of another root, 0 included, is solid matter that does not move with c:
//     the constraint is e - 1.  The runs of the hits are x-adjacent solid voxels, so one root each;
//   * below y0 the row comes from the world itself (detach_row32); no voxel of c lies there, so any hit is a
//     constraint;
//   * with no column left the run has no constraint.
// clearance(c) is the least constraint of its runs: every voxel of c is in some run, and a column that
// dropped out is covered by the own voxel it met.  Every component has a lowest voxel over the floor, so at
// least one run of it reports.
//
// Two cuts that change no result.  With a limit (max_fall > 0) only min(clearance, max_fall + 1) matters --
// fall = min(clearance, max_fall), and the component was stopped iff clearance <= max_fall -- so a run
// that has counted max_fall + 1 empty rows reports that.  And a run that has counted as many rows as its
// component's dword already holds cannot lower it and reports nothing; the dword only falls, so a stale
// read only costs rows.
#pragma once
#include "rv_detached.h"

namespace rv {

constexpr uint32_t FALL_NONE = 0xFFFFFFFFu;   // a run without a constraint; a slot no run has reported to yet

// the most rows a scan counts: max_fall + 1 with a limit, else no bound
RV_HD uint32_t fall_scan_limit(int32_t max_fall) { return max_fall > 0 ? (uint32_t)max_fall + 1u : FALL_NONE; }
// fall(c) from the slot's dword = min(clearance, limit)
RV_HD uint32_t fall_rows(uint32_t clearance, int32_t max_fall) {
    return max_fall > 0 ? umin(clearance, (uint32_t)max_fall) : clearance;
}
RV_HD bool fall_stopped(uint32_t clearance, int32_t max_fall) { return max_fall <= 0 || clearance <= (uint32_t)max_fall; }

// The constraint of the run [s, s + len) of word g of D (root r, d = detach_word(b, g)), or FALL_NONE.
// best: the dword of r's slot.
template <class WV>
RV_HD uint32_t fall_run_clearance(const WV& w, const DetachBox& b, const uint32_t* W, const uint32_t* L,
                                  const DetachWord& d, uint32_t g, uint32_t s, uint32_t len, uint32_t r, uint32_t limit,
                                  const uint32_t* best) {
    uint32_t cols = detach_low_bits(len) << s;
    const int xs = b.x0 + 32 * d.wx, z = b.z0 + d.zl;
    for (uint32_t e = 1;; e++) {
        const uint32_t count = e - 1u;
        if (count >= limit) return limit;
        if (count >= detach_load(best)) return FALL_NONE;
        const int yl = d.yl - (int)e, y = b.y0 + yl;
        if (y < 0) return count;   // the floor
        if (yl >= 0) {
            uint32_t hit = W[g - e * (uint32_t)b.nwx] & cols, hs, hlen;
            const uint32_t base = d.base - e * (uint32_t)b.nx;
            while (detach_next_run(hit, hs, hlen)) {
                if (L[base + hs] != r) return count;
                cols &= ~(detach_low_bits(hlen) << hs);
            }
            if (!cols) return FALL_NONE;
        } else if (detach_row32(w, xs, y, z) & cols) {
            return count;
        }
    }
}

// rv_fall.hip: the clearances of the nc components of a finished query into clearance[slot] (set to all ones
// here), and the detached bits D stamped `fall` rows lower into the brick records; scratch as
// launch_detach_query laid it out.  The stamp follows launch_detach_clear on the same stream.
void launch_fall_clearance(hipStream_t s, const World& w, const DetachBox& b, const uint32_t* scratch, uint32_t nc,
                           int32_t max_fall, uint32_t* clearance);
void launch_fall_stamp(hipStream_t s, uint32_t* brick, const World& w, const DetachBox& b, const uint32_t* scratch,
                       int32_t max_fall, const uint32_t* clearance);

}  // namespace rv
