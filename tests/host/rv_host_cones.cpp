// rv_host_cones.cpp -- TEST INFRASTRUCTURE: the product's cone code (include/rvgrt/rv_device.h:
// trace_cones6 with the first-sample offset table, its interior fast path and its one cold loop)
// compiled for the CPU next to the reference form, six trace_cone calls summed in order, so
// tests/test_host_cones.py can compare the two bit for bit on hosts without a GPU.  On the host a
// "wave" is one lane: every hit chooses its path by itself.  Not linked into librvgrt_hip.so.
// With -DRVC_MAIN the file is a stand-alone program (its own random inputs) for sanitizer builds.
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../include/rvgrt/rv_device.h"

using namespace rv;

namespace {
struct HostWorld {
    std::vector<uint32_t> brick;
    World w{};
};

// An all-air brick world of these log2 dims with the CSDF bytes `csdf` (x fastest) and the GI grid gi.
void build(HostWorld& h, int lx, int ly, int lz, const uint8_t* csdf, const uint32_t* gi) {
    World& w = h.w;
    w.X = 1 << lx; w.Y = 1 << ly; w.Z = 1 << lz;
    w.lbx = lx - 3; w.lbxy = (lx - 3) + (ly - 3);
    w.lbz = lz - 3; w.lbzy = (lz - 3) + (ly - 3);
    w.SX = w.X / 2; w.SY = w.Y / 2; w.SZ = w.Z / 2;
    w.GX = w.X / 4; w.GY = w.Y / 4; w.GZ = w.Z / 4;
    w.fX = (float)w.X; w.fY = (float)w.Y; w.fZ = (float)w.Z;
    const uint64_t nbricks = ((uint64_t)w.X * w.Y * w.Z) / 512;
    world_set_regions(w, nbricks);
    h.brick.assign((size_t)(nbricks * 32), 0u);
    uint8_t* bytes = reinterpret_cast<uint8_t*>(h.brick.data());
    for (uint64_t cz = 0; cz < (uint64_t)w.SZ; cz++)
        for (uint64_t cy = 0; cy < (uint64_t)w.SY; cy++)
            for (uint64_t cx = 0; cx < (uint64_t)w.SX; cx++) {
                const uint64_t b = brick_of(w, (int)(cx >> 2), (int)(cy >> 2), (int)(cz >> 2));
                const uint32_t local = (uint32_t)((cx & 3) | ((cy & 3) << 2) | ((cz & 3) << 4));
                bytes[csdf_byte_index(w.coff, b, local)] = csdf[(cz * w.SY + cy) * w.SX + cx];
            }
    world_set_brick(w, h.brick.data());
    w.gi = gi;
}

// computeColor's basis as the reference writes it (src/StateRender.cu:110-112), no constant scales
void basis_ref(f3 up, f3& right, f3& fwd) {
    right = normalize(cross(up, V(0.577f, 0.577f, 0.577f)));
    fwd = normalize(cross(up, right));
}
}  // namespace

extern "C" {

// the product's table, [normal code][cone][xyz] without the row padding
void rvc_table(float* out) {
    float tab[CONE_TAB_FLOATS];
    cone_offset_table(tab);
    for (int c = 0; c < 6; c++)
        for (int i = 0; i < 18; i++) out[c * 18 + i] = tab[c * CONE_ROW + i];
}
// the generic offsets scale(cone_dir(k, ...), 3.0f) of the six axis normals, in the same order
void rvc_table_generic(float* out) {
    for (uint32_t c = 0; c < 6; c++) {
        const f3 up = cone_code_normal(c);
        f3 right, fwd;
        basis_ref(up, right, fwd);
        for (int k = 0; k < 6; k++) {
            const f3 o = scale(cone_dir(k, up, right, fwd), 3.0f);
            out[c * 18 + 3 * k] = o.x; out[c * 18 + 3 * k + 1] = o.y; out[c * 18 + 3 * k + 2] = o.z;
        }
    }
}
// cone_normal_code of the normal cone_code_normal(c) is c, and its components
int rvc_normal_code(float x, float y, float z) { return (int)cone_normal_code(V(x, y, z)); }

// trace_cones6 of n hits (pos, nrm: xyz floats); use_tab = 0: without the table (the generic step 0)
int rvc_cones(int lx, int ly, int lz, const uint8_t* csdf, const uint32_t* gi, const float* pos, const float* nrm,
              int64_t n, int use_tab, float* sum, uint32_t* steps) {
    HostWorld h;
    build(h, lx, ly, lz, csdf, gi);
    float tab[CONE_TAB_FLOATS];
    cone_offset_table(tab);
    float k1, k2;
    cone_basis_scales(k1, k2);
    for (int64_t i = 0; i < n; i++) {
        uint32_t st = 0;
        const f3 s = trace_cones6<true>(h.w, V(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]),
                                        V(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]), k1, k2,
                                        use_tab ? tab : nullptr, st);
        sum[3 * i] = s.x; sum[3 * i + 1] = s.y; sum[3 * i + 2] = s.z;
        steps[i] = st;
    }
    return 0;
}

// the reference form: six trace_cone calls summed in order; more[i] = cones of hit i with more than one step
int rvc_cones_ref(int lx, int ly, int lz, const uint8_t* csdf, const uint32_t* gi, const float* pos, const float* nrm,
                  int64_t n, float* sum, uint32_t* steps, uint32_t* more) {
    HostWorld h;
    build(h, lx, ly, lz, csdf, gi);
    for (int64_t i = 0; i < n; i++) {
        const f3 p = V(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]), up = V(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
        f3 right, fwd;
        basis_ref(up, right, fwd);
        uint32_t st = 0, m = 0;
        f3 ind = V(0.0f, 0.0f, 0.0f);
        for (int k = 0; k < 6; k++) {
            uint32_t s1 = 0;
            const f3 acc = trace_cone<true>(h.w, p, cone_dir(k, up, right, fwd), s1);
            ind = k == 0 ? acc : add(ind, acc);
            st += s1;
            m += s1 > 1u;
        }
        sum[3 * i] = ind.x; sum[3 * i + 1] = ind.y; sum[3 * i + 2] = ind.z;
        steps[i] = st;
        more[i] = m;
    }
    return 0;
}

}  // extern "C"

#ifdef RVC_MAIN
#include <stdio.h>
// Random CSDF bytes (mostly open), GI texels with the alphas {0, 1, 128, 254, 255} (then all 255) and hits on
// voxel faces of every normal and with a zero normal, anywhere in a 32^3 world: both forms, compared.
int main() {
    const int lg = 5, N = 1 << lg, n = 6000;
    uint32_t s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    std::vector<uint8_t> csdf((size_t)(N / 2) * (N / 2) * (N / 2));
    for (auto& c : csdf) c = (uint8_t)(rnd() % 8u == 0 ? 0u : 1u + rnd() % 6u);
    static const uint32_t alphas[5] = {0u, 1u, 128u, 254u, 255u};
    std::vector<float> pos(3 * n), nrm(3 * n), a(3 * n), b(3 * n);
    std::vector<uint32_t> sa(n), sb(n), more(n);
    int bad = 0;
    for (int pass = 0; pass < 2; pass++) {
        std::vector<uint32_t> gi((size_t)(N / 4) * (N / 4) * (N / 4));
        for (auto& g : gi) g = (rnd() & 0xFFFFFFu) | ((pass ? 255u : alphas[rnd() % 5u]) << 24);
        for (int i = 0; i < n; i++) {
            const uint32_t code = rnd() % 7u;
            const f3 nn = code < 6u ? cone_code_normal(code) : V(0.0f, 0.0f, 0.0f);
            float p[3];
            for (int j = 0; j < 3; j++) p[j] = (float)(rnd() % (uint32_t)(N * 256)) / 256.0f;
            if (code < 6u) p[code >> 1] = (float)(rnd() % (uint32_t)(N + 1));   // on a face plane
            memcpy(&pos[3 * i], p, 12);
            nrm[3 * i] = nn.x; nrm[3 * i + 1] = nn.y; nrm[3 * i + 2] = nn.z;
        }
        rvc_cones_ref(lg, lg, lg, csdf.data(), gi.data(), pos.data(), nrm.data(), n, b.data(), sb.data(), more.data());
        for (int tabbed = 0; tabbed < 2; tabbed++) {
            rvc_cones(lg, lg, lg, csdf.data(), gi.data(), pos.data(), nrm.data(), n, tabbed, a.data(), sa.data());
            bad += memcmp(a.data(), b.data(), a.size() * 4) != 0;
            bad += memcmp(sa.data(), sb.data(), sa.size() * 4) != 0;
        }
    }
    float t0[108], t1[108];
    rvc_table(t0);
    rvc_table_generic(t1);
    bad += memcmp(t0, t1, sizeof(t0)) != 0;
    printf(bad ? "MISMATCH %d\n" : "cones ok\n", bad);
    return bad != 0;
}
#endif
