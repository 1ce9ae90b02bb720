// The host evaluation of rv_world_stamp (stamps_apply_linear, include/rvgrt/rv_stamp.h) under AddressSanitizer and
// UndefinedBehaviorSanitizer: every orientation and op, pattern rows of 1 .. 256 voxels at every x offset mod 32,
// stamps through and beyond every face, the far corners of the bit array and of the patterns, the extreme
// offsets, and a few hundred random lists, each checked voxel by voxel against the definition written out
// naively.  The world and both layouts of every pattern are heap blocks of exactly their size, so a word read
// or written past either end is a report.  Exit status 0: all agreed.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../include/rvgrt/rv_stamp.h"

using namespace rv;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static int failures = 0;

// A pattern as the caller gives it (junk in the padding bits) and as the library keeps it: A cleaned, T made by
// pattern_transpose_word, each a heap block of exactly its size.
struct Pat {
    int nx, ny, nz;
    std::unique_ptr<uint32_t[]> given, a, t;
    bool bit(int x, int y, int z) const {   // the definition: bit x & 31 of word (x >> 5) + nwx * (y + ny * z)
        const uint32_t nwx = ((uint32_t)nx + 31u) / 32u;
        return (given[(uint32_t)(x >> 5) + nwx * ((uint32_t)y + (uint32_t)ny * (uint32_t)z)] >> (x & 31)) & 1u;
    }
};

static Pat make_pattern(int nx, int ny, int nz, uint32_t fill) {
    Pat p{nx, ny, nz, nullptr, nullptr, nullptr};
    const uint32_t nwx = pattern_row_words(nx), nw = pattern_words(nx, ny, nz), nt = pattern_words(nz, ny, nx);
    p.given.reset(new uint32_t[nw]);
    p.a.reset(new uint32_t[nw]);
    p.t.reset(new uint32_t[nt]);
    for (uint32_t g = 0; g < nw; g++) {
        uint32_t w = 0;
        for (int b = 0; b < 32; b++) w |= (uint32_t)((rnd() & 255u) < fill) << b;
        p.given[g] = w;   // junk at x >= nx stays in
        p.a[g] = w & pattern_word_mask(nx, g % nwx);
    }
    for (uint32_t g = 0; g < nt; g++) p.t[g] = pattern_transpose_word(p.a.get(), nx, ny, nz, g);
    // T against its definition, padding bits included
    const uint32_t nwt = pattern_row_words(nz);
    for (int z = 0; z < nx; z++)
        for (int y = 0; y < ny; y++)
            for (uint32_t x = 0; x < 32u * nwt; x++) {
                const bool got = (p.t[(x >> 5) + nwt * ((uint32_t)y + (uint32_t)ny * (uint32_t)z)] >> (x & 31u)) & 1u;
                const bool want = x < (uint32_t)nz && p.bit(z, y, (int)x);
                if (got != want) { std::printf("transpose %d %d %d\n", nx, ny, nz); failures++; return p; }
            }
    return p;
}

// the oriented pattern's bit by the header comment's formulas
static bool oriented_bit(const Pat& p, int orient, int u, int v, int w) {
    const bool swap = orient & RV_ORIENT_SWAP_XZ;
    const int ox = swap ? p.nz : p.nx, oz = swap ? p.nx : p.nz;
    const int us = (orient & RV_ORIENT_FLIP_X) ? ox - 1 - u : u, ws = (orient & RV_ORIENT_FLIP_Z) ? oz - 1 - w : w;
    return swap ? p.bit(ws, v, us) : p.bit(us, v, ws);
}

// one list on one world of log2 dims (lx, ly, lz) whose voxels are solid with probability fill / 256
static void run(int lx, int ly, int lz, const std::vector<Pat>& pats, const std::vector<rv_stamp>& list, uint32_t fill,
                const char* what) {
    const int X = 1 << lx, Y = 1 << ly, Z = 1 << lz;
    const size_t words = ((size_t)X * Y * Z) >> 5;
    std::unique_ptr<uint32_t[]> bits(new uint32_t[words]);
    std::vector<uint32_t> before(words);
    for (size_t i = 0; i < words; i++) {
        uint32_t w = 0;
        for (int b = 0; b < 32; b++) w |= (uint32_t)((rnd() & 255u) < fill) << b;
        bits[i] = before[i] = w;
    }
    const int32_t D[3] = {X, Y, Z};
    std::vector<StampRec> recs;
    std::vector<rv_voxel_box> each;
    rv_voxel_box u = empty_box();
    for (const rv_stamp& s : list) {
        if (!stamp_valid(s) || s.pattern < 0 || s.pattern >= (int)pats.size()) { std::printf("%s: stamp rejected\n", what); failures++; return; }
        const Pat& p = pats[(size_t)s.pattern];
        StampRec r;
        const bool ok = stamp_rec(s, p.nx, p.ny, p.nz, p.a.get(), p.t.get(), D, r);
        each.push_back(r.box);
        if (!ok) continue;
        box_include(u, r.box);
        recs.push_back(r);
    }
    if (recs.empty()) u = rv_voxel_box{0, 0, 0, 0, 0, 0};
    uint64_t on = 0, off = 0;
    stamps_apply_linear(lx, ly, bits.get(), recs.data(), (int32_t)recs.size(), u, &on, &off);
    uint64_t won = 0, woff = 0, bad = 0;
    for (int z = 0; z < Z; z++)
        for (int y = 0; y < Y; y++)
            for (int x = 0; x < X; x++) {
                const uint64_t i = (uint64_t)x | (uint64_t)y << lx | (uint64_t)z << (lx + ly);
                const bool was = (before[i >> 5] >> (i & 31)) & 1u, is = (bits[i >> 5] >> (i & 31)) & 1u;
                bool want = was;
                for (size_t k = 0; k < list.size(); k++) {
                    const rv_stamp& s = list[k];
                    const Pat& p = pats[(size_t)s.pattern];
                    int32_t o[3];
                    stamp_dims(p.nx, p.ny, p.nz, s.orient, o);
                    const int64_t uu = (int64_t)x - s.at[0], vv = (int64_t)y - s.at[1], ww = (int64_t)z - s.at[2];
                    if (uu < 0 || vv < 0 || ww < 0 || uu >= o[0] || vv >= o[1] || ww >= o[2]) continue;
                    const rv_voxel_box& e = each[k];
                    if (x < e.x0 || x >= e.x1 || y < e.y0 || y >= e.y1 || z < e.z0 || z >= e.z1) bad++;
                    const bool b = oriented_bit(p, s.orient, (int)uu, (int)vv, (int)ww);
                    if (s.op == RV_STAMP_COPY) want = b;
                    else if (b) want = s.op == RV_STAMP_SET;
                }
                if (want != is) bad++;
                won += !was && want;
                woff += was && !want;
            }
    if (bad || won != on || woff != off) {
        std::printf("%s: %llu voxels differ, counts %llu/%llu want %llu/%llu\n", what, (unsigned long long)bad,
                    (unsigned long long)on, (unsigned long long)off, (unsigned long long)won, (unsigned long long)woff);
        failures++;
    }
}

static rv_stamp stamp(int pattern, int op, int orient, int x, int y, int z) { return rv_stamp{pattern, op, orient, {x, y, z}}; }

int main() {
    const int A = STAMP_MAX_AT, M = RV_PATTERN_MAX_DIM;
    // rows of every interesting width, at every x offset mod 32 on both sides of the window's wall, every
    // orientation and op
    std::vector<Pat> pats;
    const int widths[] = {1, 7, 8, 9, 31, 32, 33, 37, 63, 64, 65, M};
    for (int nx : widths) pats.push_back(make_pattern(nx, 3, 5, 128));
    for (int i = 0; i < (int)pats.size(); i++)
        for (int orient = 0; orient < 8; orient++) {
            std::vector<rv_stamp> list;
            for (int k = 0; k < 32; k++) list.push_back(stamp(i, (k + orient) % 3, orient, k - 16, (k * 5) % 61 - 1, (k * 7) % 29 - 2));
            run(6, 6, 5, pats, list, 128, "widths");
        }
    // the largest patterns: all of one covering the whole window from every side, in thin and thick forms
    std::vector<Pat> big;
    big.push_back(make_pattern(M, 1, M, 128));
    big.push_back(make_pattern(M, M, 1, 128));
    big.push_back(make_pattern(1, M, M, 128));
    big.push_back(make_pattern(M, 2, 33, 200));
    for (int orient = 0; orient < 8; orient++)
        for (int i = 0; i < (int)big.size(); i++) {
            run(5, 5, 5, big, {stamp(i, RV_STAMP_COPY, orient, -100, -100, -100)}, 128, "covering");
            // the far corner of the bit array from the pattern's first voxel, the first word from its last
            run(5, 5, 6, big, {stamp(i, RV_STAMP_COPY, orient, 31, 31, 63), stamp(i, RV_STAMP_SET, orient, 1 - M, 1 - M, 1 - M),
                               stamp(i, RV_STAMP_CLEAR, orient, 1 - M, 31, 1 - M)}, 128, "corners");
            // the extreme offsets: far outside, nothing may be touched or read
            for (int sgn = -1; sgn <= 1; sgn += 2)
                run(5, 5, 5, big, {stamp(i, RV_STAMP_COPY, orient, sgn * A, sgn * A, sgn * A), stamp(i, RV_STAMP_COPY, orient, sgn * A, 3, 3),
                                   stamp(i, RV_STAMP_COPY, orient, 3, sgn * A, 3), stamp(i, RV_STAMP_COPY, orient, 3, 3, sgn * A)},
                    128, "max |at|");
        }
    // invalid stamps are rejected
    const rv_stamp bad[] = {stamp(0, 3, 0, 1, 1, 1), stamp(0, -1, 0, 1, 1, 1), stamp(0, 0, 8, 1, 1, 1), stamp(0, 0, -1, 1, 1, 1),
                            stamp(0, 0, 0, A + 1, 1, 1), stamp(0, 0, 0, 1, -A - 1, 1), stamp(0, 0, 0, 1, 1, A + 1)};
    for (const rv_stamp& b : bad)
        if (stamp_valid(b)) { std::printf("an invalid stamp was accepted\n"); failures++; }
    if (pattern_dims_ok(0, 1, 1) || pattern_dims_ok(1, M + 1, 1) || pattern_dims_ok(1, 1, -1) || !pattern_dims_ok(M, M, M) ||
        !pattern_dims_ok(1, 1, 1)) { std::printf("pattern dims\n"); failures++; }
    // random lists of 1 .. 12 stamps (and a few of RV_STAMP_MAX) over random patterns on worlds of three forms,
    // offsets up to 40 voxels beyond the faces
    const int forms[3][3] = {{5, 5, 5}, {6, 5, 7}, {7, 4, 5}};
    for (int t = 0; t < 240; t++) {
        const int* f = forms[t % 3];
        std::vector<Pat> ps;
        for (int i = 0; i < 3; i++) ps.push_back(make_pattern(rnd_in(1, t % 5 == 0 ? M : 70), rnd_in(1, 20), rnd_in(1, t % 7 == 0 ? M : 40), (uint32_t)rnd_in(0, 256)));
        std::vector<rv_stamp> list((size_t)(t % 80 == 79 ? RV_STAMP_MAX : rnd_in(1, 12)));
        for (rv_stamp& s : list)
            s = stamp(rnd_in(0, 2), rnd_in(0, 2), rnd_in(0, 7), rnd_in(-40, (1 << f[0]) + 40) - (t % 4 == 0 ? 60 : 0), rnd_in(-20, (1 << f[1]) + 5),
                      rnd_in(-40, (1 << f[2]) + 40));
        run(f[0], f[1], f[2], ps, list, (uint32_t)rnd_in(0, 256), "random");
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("host_stamp ok\n");
    return 0;
}
