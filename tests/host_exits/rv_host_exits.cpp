// rv_host_exits.cpp -- TEST INFRASTRUCTURE for tests/test_exits_ref.py: the exit tables as the host harness
// builds them.  It compiles tests/host/rv_host_trace.cpp into this library unchanged (one translation unit,
// so its world_ytop, world_horizon and world_dtop -- the functions the table kernels call, driven by host
// loops -- are the ones used here) and adds the one entry point that harness lacks: the tables themselves.
#include "../host/rv_host_trace.cpp"

extern "C" {

// ytop, the (Z/2)*(X/2) column tops and sun horizon, the (Z/8)*(X/8) neighbourhood tops, all x fastest,
// from the canonical bits for the sun direction `sun`.
int rvh_exit_tables(int lx, int ly, int lz, const uint32_t* bits, const float* sun, uint32_t* ytop, uint32_t* coltop_out,
                    uint32_t* hz_out, int32_t* dtop_out) {
    HostWorld h;
    const std::vector<uint8_t> csdf((size_t)1 << (lx + ly + lz - 3), 0);   // the tables read the bits only
    build(h, lx, ly, lz, bits, csdf.data());
    h.w.ytop = world_ytop(h);
    *ytop = h.w.ytop;
    std::vector<uint32_t> coltop, hz;
    world_horizon(h, sun, coltop, hz);
    world_dtop(h);
    memcpy(coltop_out, coltop.data(), coltop.size() * 4);
    memcpy(hz_out, hz.data(), hz.size() * 4);
    memcpy(dtop_out, reinterpret_cast<const char*>(h.brick.data()) + dtop_byte(h.w.coff, h.w.X, h.w.Z),
           dtop_bytes(h.w.X, h.w.Z));
    return 0;
}

}  // extern "C"
