// The host evaluation of rv_world_edit_shapes (shapes_apply_linear, include/rvgrt/rv_shapes.h) under
// AddressSanitizer and UndefinedBehaviorSanitizer: the extremes of the arithmetic (the largest radii and centre
// coordinates), rows and words at the far corner of the bit array, and a few hundred random lists, each checked
// voxel by voxel against the definition written out with 128-bit integers.  The bit array is a heap block of
// exactly the world's size, so a word written past either end is a report.  Exit status 0: all agreed.
//
// And what the in-place voxel writes share (include/rvgrt/rv_words.h): the word grid of a voxel box against a
// brute-force scan of the box's voxels, the brick columns under a box, and a component record's box.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/rvgrt/rv_shapes.h"
#include "../../include/rvgrt/rv_words.h"

using namespace rv;

typedef __int128 i128;

static bool inside(const rv_edit_shape& s, int x, int y, int z) {
    const i128 d[3] = {(i128)2 * x + 1 - s.c2[0], (i128)2 * y + 1 - s.c2[1], (i128)2 * z + 1 - s.c2[2]};
    const i128 q[3] = {(i128)s.r2[0] * s.r2[0], (i128)s.r2[1] * s.r2[1], (i128)s.r2[2] * s.r2[2]};
    const i128 e[3] = {d[0] * d[0], d[1] * d[1], d[2] * d[2]};
    if (s.kind == RV_SHAPE_ELLIPSOID) return e[0] * q[1] * q[2] + e[1] * q[0] * q[2] + e[2] * q[0] * q[1] <= q[0] * q[1] * q[2];
    const int a = s.kind == RV_SHAPE_CYLINDER_X ? 0 : s.kind == RV_SHAPE_CYLINDER_Y ? 1 : 2;
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    return e[a] <= q[a] && e[b] * q[c] + e[c] * q[b] <= q[b] * q[c];
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static int failures = 0;

// one list on one world of log2 dims (lx, ly, lz) whose voxels are solid with probability fill / 256
static void run(int lx, int ly, int lz, const std::vector<rv_edit_shape>& list, uint32_t fill, const char* what) {
    const int X = 1 << lx, Y = 1 << ly, Z = 1 << lz;
    const size_t words = ((size_t)X * Y * Z) >> 5;
    std::vector<uint32_t> bits(words), before;
    for (uint32_t& w : bits) {
        w = 0;
        for (int b = 0; b < 32; b++) w |= (uint32_t)((rnd() & 255u) < fill) << b;
    }
    before = bits;
    const int n = (int)list.size();
    if (!shapes_ok(list.data(), n)) { std::printf("%s: list rejected\n", what); failures++; return; }
    uint64_t on = 0, off = 0;
    shapes_apply_linear(lx, ly, lz, bits.data(), list.data(), n, &on, &off);
    std::vector<rv_voxel_box> each((size_t)(n > 0 ? n : 1));
    rv_voxel_box all;
    shapes_boxes(lx, ly, lz, list.data(), n, each.data(), &all);
    uint64_t won = 0, woff = 0, bad = 0;
    for (int z = 0; z < Z; z++)
        for (int y = 0; y < Y; y++)
            for (int x = 0; x < X; x++) {
                const uint64_t i = (uint64_t)x | (uint64_t)y << lx | (uint64_t)z << (lx + ly);
                const bool was = (before[i >> 5] >> (i & 31)) & 1u, is = (bits[i >> 5] >> (i & 31)) & 1u;
                bool want = was;
                for (int k = 0; k < n; k++)
                    if (inside(list[(size_t)k], x, y, z)) {
                        want = list[(size_t)k].solid != 0;
                        const rv_voxel_box& e = each[(size_t)k];
                        if (x < e.x0 || x >= e.x1 || y < e.y0 || y >= e.y1 || z < e.z0 || z >= e.z1) bad++;
                        if (shape_row_mask(list[(size_t)k], y, z, x & ~7) >> (x & 7) & 1u) continue;
                        bad++;
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

static rv_edit_shape shape(int kind, int solid, int cx, int cy, int cz, int rx, int ry, int rz) {
    return rv_edit_shape{kind, solid, {cx, cy, cz}, {rx, ry, rz}};
}

// The word grid and the columns of one box in a window of X Y Z voxels: the words enumerated by g in
// [0, nwords) are pairwise distinct, lie inside the window, and are exactly the words that hold a voxel of the
// box (the words of its word-aligned hull); both index widths enumerate the same words; the columns are the
// ones the box's voxels stand on.
static void check_box(int X, int Y, int Z, const rv_voxel_box& b) {
    const WordGrid g = word_grid(b);
    const WordGridT<uint64_t> g64 = word_grid<uint64_t>(b);
    const int NWX = X / 8, NWY = Y / 4, NBX = X / 8, NBZ = Z / 8;
    std::vector<uint8_t> want((size_t)NWX * NWY * Z, 0), got(want.size(), 0), cols((size_t)NBX * NBZ, 0), rc(cols.size(), 0);
    size_t nwant = 0;
    for (int z = b.z0; z < b.z1; z++)
        for (int y = b.y0; y < b.y1; y++)
            for (int x = b.x0; x < b.x1; x++) {
                uint8_t& m = want[(size_t)(x >> 3) + (size_t)NWX * ((size_t)(y >> 2) + (size_t)NWY * (size_t)z)];
                nwant += !m;
                m = 1;
                cols[(size_t)(x >> 3) + (size_t)NBX * (size_t)(z >> 3)] = 1;
            }
    bool ok = g64.nwords == g.nwords && g64.nwords <= WORD_GRID_MAX && g.nwords == nwant;
    for (uint32_t i = 0; ok && i < g.nwords; i++) {
        int wx, wy, z, wx2, wy2, z2;
        g.word(i, wx, wy, z);
        g64.word(i, wx2, wy2, z2);
        ok = wx == wx2 && wy == wy2 && z == z2 && wx >= 0 && wy >= 0 && z >= 0 && wx < NWX && wy < NWY && z < Z;
        if (!ok) break;
        uint8_t& m = got[(size_t)wx + (size_t)NWX * ((size_t)wy + (size_t)NWY * (size_t)z)];
        ok = !m;   // pairwise distinct
        m = 1;
    }
    ok = ok && got == want;
    const ColumnRange r = columns_under(b);
    for (int bz = r.bz0; bz < r.bz1; bz++)
        for (int bx = r.bx0; bx < r.bx1; bx++) {
            if (bx < 0 || bx >= NBX || bz < 0 || bz >= NBZ) { ok = false; continue; }
            rc[(size_t)bx + (size_t)NBX * (size_t)bz] = 1;
        }
    ok = ok && rc == cols;
    if (!ok) {
        std::printf("word grid / columns of box %d %d %d .. %d %d %d in %d %d %d\n", b.x0, b.y0, b.z0, b.x1, b.y1, b.z1, X, Y, Z);
        failures++;
    }
}

// Boxes whose x0 and x1 - 1 take the residues {0, 1, 7} mod 8 and whose y0 and y1 - 1 the residues {0, 3} mod 4,
// in the first and the last brick of the axis (both window faces), over a few z ranges; 200 random boxes; and
// component records against the boxes they were built from.
static void check_words(int X, int Y, int Z) {
    std::vector<int> xs, ys;
    for (int base : {0, X - 8})
        for (int r : {0, 1, 7}) xs.push_back(base + r);
    for (int base : {0, Y - 4})
        for (int r : {0, 3}) ys.push_back(base + r);
    const int zs[4][2] = {{0, 1}, {Z - 1, Z}, {7, 9}, {0, Z}};
    for (int x0 : xs) for (int xl : xs) for (int y0 : ys) for (int yl : ys) for (const int* z : zs)
        if (xl >= x0 && yl >= y0) check_box(X, Y, Z, rv_voxel_box{x0, y0, z[0], xl + 1, yl + 1, z[1]});
    for (int t = 0; t < 200; t++) {
        const int x0 = rnd_in(0, X - 1), y0 = rnd_in(0, Y - 1), z0 = rnd_in(0, Z - 1);
        const rv_voxel_box b{x0, y0, z0, rnd_in(x0 + 1, X), rnd_in(y0 + 1, Y), rnd_in(z0 + 1, Z)};
        check_box(X, Y, Z, b);
        // a record of the query box b: inclusive box-local bounds lo <= hi
        DetachRec rec{};
        const int n[3] = {b.x1 - b.x0, b.y1 - b.y0, b.z1 - b.z0};
        for (int a = 0; a < 3; a++) { rec.lo[a] = (uint32_t)rnd_in(0, n[a] - 1); rec.hi[a] = (uint32_t)rnd_in((int)rec.lo[a], n[a] - 1); }
        const rv_voxel_box v = detach_rec_box(b, rec);
        const int o[3] = {b.x0, b.y0, b.z0}, vlo[3] = {v.x0, v.y0, v.z0}, vhi[3] = {v.x1, v.y1, v.z1};
        for (int a = 0; a < 3; a++)
            if (vlo[a] != o[a] + (int)rec.lo[a] || vhi[a] != o[a] + (int)rec.hi[a] + 1) { std::printf("detach_rec_box\n"); failures++; break; }
    }
    // the record is the eight dwords the kernels write by index: voxels, min x y z, max x y z, seed
    const uint32_t raw[DETACH_REC] = {10, 1, 2, 3, 4, 5, 6, 7};
    DetachRec rec;
    std::memcpy(&rec, raw, sizeof(rec));
    if (rec.voxels != 10 || rec.lo[0] != 1 || rec.lo[2] != 3 || rec.hi[0] != 4 || rec.hi[2] != 6 || rec.seed != 7) {
        std::printf("DetachRec field order\n");
        failures++;
    }
}

int main() {
    check_words(32, 16, 16);
    check_words(64, 32, 16);
    const int R = RV_SHAPE_MAX_R2, CMAX = SHAPE_MAX_C2;
    // extremes: the largest radii around the centre, thin slabs at an odd and an even centre, every kind
    for (int kind = 0; kind < 4; kind++) {
        run(6, 6, 6, {shape(kind, 1, 64, 64, 64, R, R, R)}, 0, "max radii");
        run(6, 6, 6, {shape(kind, 0, 65, 65, 65, R, R, R)}, 256, "max radii, clearing");
        run(6, 6, 6, {shape(kind, 1, 64, 65, 64, R, 1, R), shape(kind, 1, 64, 64, 64, R, 1, R)}, 0, "thin y");
        run(6, 6, 6, {shape(kind, 1, 65, 64, 64, 1, R, R), shape(kind, 1, 64, 64, 65, R, R, 1)}, 64, "thin x, z");
        // the far corner of the bit array: the last word's last bits, reached from inside and from outside
        run(6, 5, 5, {shape(kind, 1, 127, 63, 63, 1, 1, 1), shape(kind, 0, 128 + R - 1, 63, 63, R, R, R)}, 128, "far corner");
        run(5, 5, 6, {shape(kind, 1, 64 + 9, 64 + 9, 128 + 9, 20, 20, 20), shape(kind, 0, -9, -9, -9, 20, 20, 20)}, 128, "both corners");
        // the largest centre coordinates: far outside, nothing may be touched
        for (int sgn = -1; sgn <= 1; sgn += 2) {
            run(5, 5, 5, {shape(kind, 0, sgn * CMAX, sgn * CMAX, sgn * CMAX, R, R, R)}, 256, "max |c2|");
            run(5, 5, 5, {shape(kind, 1, sgn * CMAX, 33, 33, R, R, R), shape(kind, 1, 33, sgn * CMAX, 33, R, R, R),
                          shape(kind, 1, 33, 33, sgn * CMAX, R, R, R)}, 0, "max |c2| per axis");
        }
    }
    // invalid lists are rejected before anything is evaluated
    const rv_edit_shape bad[] = {shape(4, 0, 1, 1, 1, 1, 1, 1), shape(0, 2, 1, 1, 1, 1, 1, 1), shape(0, 0, 1, 1, 1, 0, 1, 1),
                                 shape(0, 0, 1, 1, 1, 1, R + 1, 1), shape(0, 0, CMAX + 1, 1, 1, 1, 1, 1),
                                 shape(0, 0, 1, -CMAX - 1, 1, 1, 1, 1), shape(-1, 0, 1, 1, 1, 1, 1, 1)};
    for (const rv_edit_shape& b : bad)
        if (shapes_ok(&b, 1)) { std::printf("an invalid shape was accepted\n"); failures++; }
    if (shapes_ok(nullptr, 1) || shapes_ok(bad, -1) || shapes_ok(bad, RV_EDIT_MAX_SHAPES + 1) || !shapes_ok(nullptr, 0)) {
        std::printf("list bounds\n");
        failures++;
    }
    // random lists of 1 .. 8 shapes (and a few long ones) on worlds of three forms, centres up to 40 half-voxels
    // beyond the faces
    const int forms[3][3] = {{5, 5, 5}, {6, 5, 7}, {7, 4, 5}};
    for (int t = 0; t < 300; t++) {
        const int* f = forms[t % 3];
        std::vector<rv_edit_shape> list((size_t)(t % 100 == 99 ? RV_EDIT_MAX_SHAPES : rnd_in(1, 8)));
        const int rmax = list.size() > 8 ? 12 : (t % 7 == 0 ? R : 40);
        for (rv_edit_shape& s : list)
            s = shape(rnd_in(0, 3), rnd_in(0, 1), rnd_in(-40, (2 << f[0]) + 40), rnd_in(-40, (2 << f[1]) + 40),
                      rnd_in(-40, (2 << f[2]) + 40), rnd_in(1, rmax), rnd_in(1, rmax), rnd_in(1, rmax));
        run(f[0], f[1], f[2], list, (uint32_t)rnd_in(0, 256), "random");
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("host_shapes ok\n");
    return 0;
}
