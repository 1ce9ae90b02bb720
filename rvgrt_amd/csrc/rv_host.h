// rv_host.h -- internal to librvgrt_hip.so (not installed): the context (rv_ctx), the communicator and
// the host helpers shared by the parts of the C ABI declared in include/rvgrt.h --
//   rv_abi.cpp    contexts, world build / import / export, the GI update, single frames (flow frames,
//                 drawCUDA), readback, stats;
//   rv_loops.cpp  the native frame loops (batched, pipelined, grouped), tile shards;
//   rv_comm.cpp   the transport: RCCL resolved at run time, or the in-process loopback group;
//   rv_edit.cpp   voxel edits in place (rv_world_edit);
//   rv_relight.cpp  the GI refresh of a cell box (rv_gi_relight);
//   rv_scroll.cpp   the world window moved over the terrain (rv_world_scroll);
//   rv_persist.cpp  edited columns kept across scrolls (rv_world_persist);
//   rv_bodies.cpp   swept box collision against the voxel window (rv_world_bodies_move);
//   rv_detached.cpp voxels an edit left floating, found and cleared (rv_world_detached);
//   rv_fall.cpp     detached components dropped in place (rv_world_fall);
//   rv_shapes.cpp   ellipsoid and cylinder edits in one launch (rv_world_edit_shapes);
//   rv_stamp.cpp    patterns kept on the device and pasted, oriented, many per launch (rv_world_stamp).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types only: RCCL is resolved at run time (rccl_load)

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <thread>
#include <tuple>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rvgrt/rv_frame.h"
#include "../../include/rvgrt/rv_stamp.h"
#ifndef RV_PIPE_DIAG
#define RV_PIPE_DIAG 0   // per-wave diagnostics of the pipelined and flow launches (tools/pipe_waves.py, tools/flow_waves.py)
#endif

using namespace rv;

inline rv_status fail(rv_ctx* c, rv_status s, const std::string& msg);

#define HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail((ctx), e_ == hipErrorOutOfMemory ? RV_ERR_OOM : RV_ERR_HIP,          \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                  \
    } while (0)

#define LAUNCH_CHECK(ctx) HIP_TRY(ctx, hipGetLastError())

// ---------------------------------------------------------------- owners
// Every device buffer, pinned host buffer, event and stream the library creates is a member (or a local) of
// one of these four move-only types, which are the only places that acquire and release them: what a struct
// below holds goes with the struct, and rv_destroy is `delete`.  A raw pointer or handle owns nothing.

// A device allocation and its capacity in bytes; converts to the typed pointer.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DevBuf() { reset(); }
    operator T*() const { return p; }
    void reset() { if (p) hipFree(p); p = nullptr; cap = 0; }
    void trim(size_t limit) { if (cap > limit) reset(); }
    // grows to `bytes` (never shrinks; the contents are not kept); empty after a failure
    rv_status reserve(rv_ctx* c, size_t bytes) {
        if (bytes <= cap) return RV_OK;
        reset();
        HIP_TRY(c, hipMalloc((void**)&p, bytes));
        cap = bytes;
        return RV_OK;
    }
};

// The same for pinned host memory.
template <class T>
struct HostBuf {
    T* p = nullptr;
    size_t cap = 0;
    HostBuf() = default;
    HostBuf(HostBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    HostBuf& operator=(HostBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~HostBuf() { reset(); }
    operator T*() const { return p; }
    void reset() { if (p) hipHostFree(p); p = nullptr; cap = 0; }
    void trim(size_t limit) { if (cap > limit) reset(); }
    rv_status reserve(rv_ctx* c, size_t bytes) {
        if (bytes <= cap) return RV_OK;
        reset();
        HIP_TRY(c, hipHostMalloc((void**)&p, bytes, hipHostMallocDefault));
        cap = bytes;
        return RV_OK;
    }
};

// An event, created on first use: without timing unless asked (rv_ctx::ev).
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
    rv_status ensure(rv_ctx* c, unsigned flags = hipEventDisableTiming) {
        if (!e) HIP_TRY(c, hipEventCreateWithFlags(&e, flags));
        return RV_OK;
    }
};

// A non-blocking stream, created on first use: at the default priority or at a given one.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    Stream& operator=(Stream&& o) noexcept { std::swap(s, o.s); return *this; }
    ~Stream() { if (s) hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
    rv_status ensure(rv_ctx* c) {
        if (!s) HIP_TRY(c, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return RV_OK;
    }
    rv_status ensure(rv_ctx* c, int prio) {
        if (!s) HIP_TRY(c, hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio));
        return RV_OK;
    }
};

// Device copy of a host id list, uploaded only when the list changes.
struct DevIds {
    DevBuf<int> d;
    std::vector<int32_t> h;
};

// Per-frame resources of one frame in flight (rv_set_frames_in_flight): the
// library-owned output images, the half-res pre-pass images and the
// SCHED_COST order/cost arrays.  There is one copy of this state: everything
// reads the active slot through cur(c) = slots[cur_slot], and slot_load only
// selects the slot and re-points the output views that are not bound.
struct FrameSlot {
    DevBuf<uint32_t> own_color, own_mv; DevBuf<uint16_t> own_depth;
    DevBuf<float> hdist, hshadow;
    DevBuf<int> chunk_order[2]; DevBuf<uint32_t> chunk_cost[2];   // SCHED_COST feedback per grid (CG_*)
    DevBuf<int> tile_order; DevBuf<uint32_t> tile_cost;           // SCHED_COST per tile slot (equal capacities)
    int tiles_px = 0;             // tile size of the list the order arrays are for
    uint32_t frames_since_order = 0;
    uint64_t tiles_seen = ~0ull;  // list version (rv_ctx::tiles_ver) the order arrays are for
    Event done;                   // recorded after the slot's last frame work
    bool pending = false;         // `done` has been recorded at least once
    hipStream_t last_stream = nullptr;   // stream of the slot's last frame
    uint64_t submitted = 0;       // frame_seq of the slot's last frame
    uint64_t world_seen = 0;      // world version the slot's last frame waited for
    // rv_render_frames with a tile shard: packed tiles, rank-0 gather buffer (sized exactly)
    DevBuf<uint32_t> tbuf, gbuf;
    Event gathered;               // recorded on the comm stream after the slot's gather
};

// rv_render_frames batches: B frames per launch, two sets in ping-pong (set
// j & 1 also uses frame slot j & 1's scheduling state).
struct BatchSet {
    DevBuf<uint32_t> color, mv; DevBuf<uint16_t> depth;
    DevBuf<float> hdist, hshadow;
    DevBuf<uint32_t> tbuf, gbuf;
    int nb = 0; size_t slice = 0, gbytes = 0;   // allocated for
    Event rendered, gathered;
    bool pending = false;
};

// Owned: every DevBuf, HostBuf, Event and Stream member.  Not owned: every raw pointer and handle -- `stream`
// (the caller's, rv_set_stream), color / mv / depth (views of a bound output or of the active slot's image),
// ext_tilebuf, comm_attached, world_stream, spec_stream and the slots' last_stream.
struct rv_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    rv_config cfg{};
    int lx = 0, ly = 0, lz = 0;
    World w{};
    DevBuf<uint32_t> d_top;        // world_top scratch (one dword)
    DevBuf<uint32_t> coltop;       // sun horizon: highest solid row + 1 per brick column
    DevBuf<uint32_t> brick;
    size_t brick_bytes = 0;
    DevBuf<uint32_t> gi;          // current grid
    DevBuf<uint32_t> gi_tmp;      // update target (double buffer)
    size_t gi_bytes = 0;
    DevBuf<uint32_t> atlas;
    DevBuf<float> cone_tab;       // cone_offset_table(): the cones' first-sample offsets per axis normal
    DevBuf<uint32_t> tex;        // sampleTexture's tile table (World::tex), or empty
    bool tex_tried = false;       // tex_table() ran (the table is built once per context)
    // frame images: the active slot's own ones unless bound
    uint32_t* color = nullptr; size_t color_pitch = 0; bool color_ext = false;
    uint32_t* mv = nullptr; size_t mv_pitch = 0; bool mv_ext = false;
    uint16_t* depth = nullptr; size_t depth_pitch = 0; bool depth_ext = false;
    size_t own_color_pitch = 0, own_mv_pitch = 0, own_depth_pitch = 0;
    DevBuf<unsigned long long> counters;
    DevIds tiles;                 // rv_frame_tiles list (device copy, re-uploaded on change)
    DevIds untile_ids;            // rv_untile list
    uint64_t tiles_ver = 0;       // bumped when the device tile list changes
    std::vector<int> tile_ident;
    DevBuf<uint32_t> tilebuf;
    uint32_t* ext_tilebuf = nullptr; size_t ext_tilebuf_bytes = 0;
    // stage timing (rv_timing_enable): EV_PER_FRAME events per frame (created with timing)
    int timing_cap = 0, timing_n = 0;
    std::vector<Event> ev;
    std::vector<char> gi_timed;
    std::vector<signed char> ev_stage;   // stage of each frame event slot (-1: end of frame)
    std::vector<int> ev_used;            // frame event slots used per frame
    bool megakernel = true;       // RV_PATH_FUSED (k_prepass/k_render); false: wavefront stages
    // asynchronous GI update (rv_set_gi_async): kernel on gi_stream, copy-back on stream
    bool gi_async = true;
    Stream gi_stream;
    int prio_lo = 0, prio_hi = 0;  // stream priority range (numerically: lo = least urgent)
    int gi_low_prio = 1;           // 1 = GI stream at the lowest priority (fills the frame's gaps)
    Event ev_world;               // recorded on `stream` after the last world/GI write
    Event ev_gi_done;             // recorded on gi_stream after a GI kernel
    int enq = 1;                  // wavefront path: queue append granularity (FrameParams::enq)
    // wavefront buffers
    DevBuf<float4> hpos, hsec, pphit; DevBuf<uint32_t> hinfo;
    DevBuf<int> wq[NQUEUE];       // per queue, all sub-queues
    DevBuf<unsigned> qcount;
    DevBuf<uint32_t> wtrace;      // RV_WAVE_TRACE builds: per-wave records of the last k_render
    uint32_t gi_frame = 0;
    uint64_t gi_offset = 0;
    bool world_ready = false;
    int sched = SCHED_COST;
    int order_every = 4;          // frames between chunk re-orderings
    int pipe = 1;                 // rv_set_pipeline: pipelined reference frames
    uint32_t pipe_order = 0x102;  // RV_OPT_PIPE_ORDER: dispatch order, hex digits PIPE_* (first = high): pre-pass, GI, render
    // RV_OPT_PIPE_MIX: k_ref_pipe's whole-frame dispatch pattern, head rows << 24 | pre-pass << 16 | GI << 8 |
    // render rows per period (0: the three contiguous ranges); pipe_mix_last: what the last launch used.
    // The default is for the throughput variant's launches (C4 -2.5 %, profiles/r07/pipe_mix_ab.txt); the
    // latency variant's keep the contiguous order until the option is set (pipe_mix_set)
    uint64_t pipe_mix = PIPE_MIX_DEFAULT, pipe_mix_last = 0;
    bool pipe_mix_set = false;
    DevBuf<float> pipe_half[2][2];   // [k & 1] {dist, shadow}
    bool gi_stats = false;        // rv_set_gi_stats
    // pipelined tile loop: packed tiles / rank-0 gather buffers per frame parity, GI shard staging
    DevBuf<uint32_t> pipe_tbuf[2], pipe_gbuf[2];
    size_t pipe_slice = 0, pipe_gbytes = 0;
    DevBuf<uint32_t> pipe_gi_stage, pipe_gi_all;
    uint64_t pipe_chunk = 0; int pipe_chunk_n = 0;
    Event pipe_ev[4];             // rendered, all-gathered, gathered[2]
    DevBuf<uint32_t> pipe_wstat;  // env RV_PIPE_WAVE_STATS: per-wave records of the first launches
    // env RV_FLOW_WAVE_TRACE=<file> (RV_PIPE_DIAG builds): the last flow launch's per-wave records, dumped at
    // rv_destroy (tools/flow_waves.py)
    DevBuf<uint32_t> flow_wtrace; uint32_t flow_wtrace_n = 0, flow_wlen[3] = {0, 0, 0};
    uint32_t pipe_launches = 0;
    uint32_t pipe_wnb[64] = {};       // workgroups of each recorded launch
    int gather_bpp = 3;           // rv_set_gather_bpp: packed pixel bytes of rv_render_frames' tile gather (3 or 4)
    std::vector<FrameSlot> slots;  // frames in flight; the active one is slots[cur_slot]
    std::vector<Stream> fstreams;  // rv_render_frames: streams of slots 1..n-1 (slot 0: `stream`)
    int fstream_prio = 0;
    Stream comm_stream;           // rv_render_frames: RCCL gathers, in frame order
    Event ev_loop;                // scratch event of rv_render_frames
    BatchSet bsets[2];
    int batch_streams = 1;               // RV_OPT_BATCH_STREAMS: streams rv_render_frames' groups alternate over
    // rv_set_tile_shard: this rank's tiles and the gathered layout (rank 0)
    int shard_px = 0, shard_rank = 0, shard_n = 0, shard_max = 0;
    std::vector<int32_t> shard_ids, shard_all;
    uint64_t world_ver = 1;        // bumped by every world/GI write (mark_world)
    uint64_t geom_ver = 1;         // bumped by every voxel-bits / CSDF write (what the pre-pass reads)
    // Pipelined loop: the next frame's GI update and pre-pass computed by the last launch of a call and
    // kept for the next call (rv_render_frame_seq).  gi: update `carry_fr` of [carry_first, +count) in
    // gi_tmp (or this rank's shard in pipe_gi_stage), not yet copied back; pp: pre-pass of the camera
    // `carry_key` in pipe_half[carry_half].
    bool carry_gi = false, carry_pp = false;
    uint32_t carry_fr = 0; uint64_t carry_first = 0, carry_count = 0, carry_world = 0, carry_geom = 0;
    uint64_t carry_chunk = 0; int carry_n = 0, carry_r = 0, carry_half = 0;
    float carry_key[24] = {};
    int pipe_carry = 1;            // the next frame's GI update and pre-pass are kept between calls
    // Flow frames (rv_set_flow; rv_frame / rv_draw_cuda of a frame with the pre-pass): one k_ref_flow
    // launch per frame.  Tile-major half-res hand-off buffer, per-tile flags, the launch epoch and the
    // count of render waves that fell back to evaluating their window.
    int flow = 1;
    DevBuf<unsigned long long> flow_half; size_t flow_tiles = 0;
    uint32_t flow_epoch = 0;
    DevBuf<unsigned long long> flow_fb;
    Event ev_flow;                  // recorded after every flow launch, on the stream it ran on
    uint64_t flow_launches = 0;
    // RV_OPT_GI_PAIRS: latency-variant launches trace a GI cell's two rays on a lane pair (1 all, 0 none);
    // default -1: a rank's tile share only -- its GI part is 1/N of the cells and its longest GI waves
    // were the launch's floor (8-rank C4 share 137.4 -> 132.8 us/frame, GI longest wave 127.5 -> 98.9 us),
    // while a whole C3 frame's GI waves double for no gain (0.204 -> 0.240 ms; profiles/r04/gi_pairs_ab.txt)
    int gi_pairs = -1;
    uint32_t flow_spin = 16384;      // RV_OPT_FLOW_SPIN: polls before a render wave evaluates its window
    bool flow_force_fallback = false;   // RV_OPT_FLOW_FORCE_FALLBACK (tests): no wave waits, all evaluate
    bool gi_shard_probe = false;     // RV_OPT_GI_SHARD_PROBE: a sharded loop without a communicator runs its 1/N GI share
    // The next UpdateGIData computed ahead by a flow launch (camera-independent): update `spec_fr` of
    // [spec_first, + spec_count) in gi_tmp, valid while the world/GI version is spec_world; recorded
    // on the launch's stream (ev_spec).  upd_since_frame: an UpdateGIData came since the last frame
    // (the caller runs renderLoop's per-frame update, so the next one is worth computing ahead).
    bool spec_gi = false;
    uint32_t spec_fr = 0; uint64_t spec_first = 0, spec_count = 0, spec_world = 0;
    Event ev_spec; hipStream_t spec_stream = nullptr; bool spec_rec = false;
    bool upd_since_frame = false;
    // grouped reference frames (rv_set_frame_group): frame sets per group parity, phase-A records
    // (this rank's stage slots and the all-gathered ones, 3 groups each), the update ring, the
    // phase-B stream and the loop's events
    int group = 0;
    BatchSet gsets[2];
    DevBuf<uint2> grec_stage, grec_all;
    DevBuf<uint32_t> gring;
    Stream grp_stream;
    Event gev[8];
    rv_comm* comm_attached = nullptr;   // the communicator of the last rv_render_frame_seq (bounded rv_sync)
    float shard_w0 = 1.0f;              // rank 0's tile weight of the shard (rv_set_tile_shard_weighted)
    // per-frame camera table of batched launches (rv_render_frame_seq): device copy, pinned staging
    DevBuf<FrameCam> cam_dev; HostBuf<FrameCam> cam_host;   // equal capacities
    Event cam_ev; bool cam_pending = false;
    uint64_t gi_swapped_at = 0;    // frame_seq at the last GI buffer flip: older frames read gi_tmp
    hipStream_t world_stream = nullptr;   // stream ev_world was recorded on
    // rv_world_edit: the boxes' device copy (and the stable host copy it is uploaded from), the
    // "a word changed" flag, the local CSDF passes' scratch (kept while small) and rv_world_edit_info's record
    std::vector<rv_edit_box> edit_h;
    DevBuf<rv_edit_box> edit_boxes;
    DevBuf<uint32_t> edit_flag;
    DevBuf<uint8_t> edit_t0, edit_t1;
    uint64_t edit_count = 0, edit_cells = 0; int edit_full = 0;
    // rv_gi_relight: the steps' records and the box's two dense value arrays (kept between calls),
    // rv_gi_relight_info's sums
    DevBuf<uint2> relight_rec;
    DevBuf<uint32_t> relight_dense[2];
    uint64_t relight_calls = 0, relight_cells = 0, relight_records = 0;
    // rv_world_scroll: the scratch copy of the retained records (freed after a call when above the edit
    // scratch's keep limit) and rv_world_scroll_info's record; the window's origin is cfg.seed_x / seed_z
    DevBuf<void> scroll_tmp;
    uint64_t scroll_count = 0, scroll_cells = 0; int scroll_full = 0;
    bool tex_follow = false;       // rv_texture_follow_scroll: a scroll adds its step to w.tex_ox / tex_oz
    // rv_world_persist (rv_persist.cpp).  A column's key is (wz, wx), the terrain coordinate of its low corner,
    // so both containers iterate in rv_world_store_list's order.  dirty: columns of the window whose bits may
    // differ from the generator's; store: saved column bits (2 Y words), used the next time the library
    // generates the column.  The device list of columns and the staging buffer of their bits, the host copies
    // they are filled from or read into (both staging buffers freed after a call when above the edit scratch's
    // keep limit), and rv_world_persist_info's totals.
    bool persist = false;
    std::set<std::pair<int32_t, int32_t>> persist_dirty;
    std::map<std::pair<int32_t, int32_t>, std::vector<uint32_t>> persist_store;
    DevBuf<int2> persist_cols;
    DevBuf<uint32_t> persist_stage;
    std::vector<int2> persist_cols_h;
    HostBuf<uint32_t> persist_stage_h;   // pinned: the two 1-MiB copies of a C4 step
    uint64_t persist_captured = 0, persist_restored = 0;
    // rv_world_bodies_move (rv_bodies.cpp): the host form's device copies of its arrays (kept between calls)
    // and rv_world_bodies_info's sums
    DevBuf<void> bodies_in, bodies_out;
    uint64_t bodies_calls = 0, bodies_moved = 0;
    // rv_world_detached (rv_detached.cpp): the query's device scratch (one allocation laid out by
    // detach_layout, freed after a call when above the edit scratch's keep limit), the host copy of the
    // component records and rv_world_detached_info's sums
    DevBuf<uint32_t> detach_scratch;
    std::vector<DetachRec> detach_h;
    uint64_t detach_calls = 0, detach_scanned = 0, detach_cleared = 0;
    // rv_world_fall (rv_fall.cpp): it works in detach_scratch, its clearances behind the query's layout; the
    // host copy of the clearances and rv_world_fall_info's sums
    std::vector<uint32_t> fall_h;
    uint64_t fall_calls = 0, fall_comps = 0, fall_voxels = 0;
    // rv_world_edit_shapes (rv_shapes.cpp): the shapes' device copy, the stable host copy it is uploaded from
    // with the shapes' clipped boxes, and the two 64-bit sums (voxels turned on, turned off) the kernel adds to
    std::vector<rv_edit_shape> shape_h;
    std::vector<rv_voxel_box> shape_box_h;
    DevBuf<rv_edit_shape> shape_list;
    DevBuf<unsigned long long> shape_counts;
    // Patterns and rv_world_stamp (rv_stamp.cpp).  Both layouts of a live slot (A as given, T with x and z
    // transposed: rv_stamp.h) have their padding bits zero.  A destroyed slot keeps its two allocations while they
    // are small (PATTERN_KEEP each), for the next pattern that takes the slot: releasing device memory waits for
    // the whole device, and a capture / stamp / destroy cycle (world_move) runs inside frame loops.  The made-ready
    // stamps' stable host copy with the boxes of all stamps, its device copy, the two sums the kernel adds to,
    // and rv_world_stamp_info's sums.
    struct Pattern {
        int32_t nx = 0, ny = 0, nz = 0;
        DevBuf<uint32_t> a, t;
        bool on = false;
        bool live() const { return on; }
    };
    static constexpr size_t PATTERN_KEEP = (size_t)64 << 10;   // 256 slots x 2 layouts: 32 MiB at the most
    Pattern patterns[RV_PATTERN_MAX];
    std::vector<StampRec> stamp_h;
    std::vector<rv_voxel_box> stamp_box_h;
    DevBuf<StampRec> stamp_list;
    DevBuf<unsigned long long> stamp_counts;
    uint64_t stamp_calls = 0, stamp_applied = 0;
    int cur_slot = 0;
    uint64_t frame_seq = 0;
    std::string err;
};

// ---------------------------------------------------------------- transport
// Everything the loops exchange goes through four operations on a
// communicator: an all-gather (the GI update's cells) and grouped
// send/recv (packed tiles to rank 0).  Two backends:
//   RCCL     -- one process per GPU over xGMI (ncclAllGather / ncclSend /
//               ncclRecv inside ncclGroupStart/End);
//   loopback -- N contexts of one process (one GPU): each rank's host thread
//               posts its side of an operation, the group meets at a host
//               barrier, and every rank enqueues on its own stream the
//               device-to-device copies that fetch what it receives, after
//               the senders' ready events; a second barrier lets every rank
//               wait for the copies that read its buffers.  It runs the real
//               multi-rank code paths (shard slices, padded deals, RGB24
//               packing, GI all-gather) without N GPUs.
// Waits are bounded (rv_comm_wait): a dead or diverged peer is an error
// after a timeout, the communicator is aborted.
struct LoopGroup {
    struct Post {
        int kind = 0;                   // 1 all-gather, 2 grouped send/recv
        const void* send = nullptr; void* recv = nullptr; size_t bytes = 0;
        std::vector<std::tuple<int, int, const void*, void*, size_t>> p2p;   // (is_send, peer, sbuf, rbuf, bytes)
        hipEvent_t ready = nullptr, done = nullptr;
    };
    int n = 0;
    std::mutex m;
    std::condition_variable cv;
    uint64_t gen = 0;                   // barrier generation
    int arrived = 0;
    bool aborted = false;
    std::vector<Post> post;
    double timeout_s = 60.0;
    // the barrier all ranks of a round pass twice; false on timeout or abort
    bool barrier() {
        std::unique_lock<std::mutex> lk(m);
        if (aborted) return false;
        const uint64_t g = gen;
        if (++arrived == n) {
            arrived = 0;
            gen++;
            cv.notify_all();
            return true;
        }
        const bool ok = cv.wait_for(lk, std::chrono::duration<double>(timeout_s),
                                    [&] { return gen != g || aborted; });
        if (!ok || aborted) { aborted = true; cv.notify_all(); return false; }
        return true;
    }
    void abort() {
        std::lock_guard<std::mutex> lk(m);
        aborted = true;
        cv.notify_all();
    }
};

struct rv_comm {
    ncclComm_t comm = nullptr;   // RCCL backend
    LoopGroup* loop = nullptr;   // loopback backend (not owned)
    int rank = 0, nranks = 1, device = 0;
    rv_ctx* ctx = nullptr;       // the context it was created with (bounded waits, rv_comm_destroy)
    bool in_group = false;
    LoopGroup::Post pending;     // loopback: the ops of the open group
    Event ready, done;           // loopback: this rank's events of a round
    uint64_t verified = 0;       // config record the ranks last agreed on (shard / bpp)
    bool aborted = false;
    // verify_ranks' exchange buffers, allocated on first use and kept: (nranks + 1) x 8 B on the device
    // (the all-gather's output, then this rank's hash), nranks x 8 B pinned on the host
    DevBuf<uint64_t> vdev;
    HostBuf<uint64_t> vhost;
};


// ---------------------------------------------------------------- helpers

inline int gi_prio(const rv_ctx* c) { return c->gi_low_prio ? c->prio_lo : c->prio_hi; }

inline rv_status fail(rv_ctx* c, rv_status s, const std::string& msg) {
    if (c) c->err = msg;
    return s;
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

inline FrameSlot& cur(rv_ctx* c) { return c->slots[c->cur_slot]; }   // the active slot

// Selects the active slot: the output views that are not bound follow it.
inline void slot_load(rv_ctx* c, int s) {
    c->cur_slot = s;
    const FrameSlot& sl = c->slots[s];
    if (!c->color_ext) c->color = sl.own_color;
    if (!c->mv_ext) c->mv = sl.own_mv;
    if (!c->depth_ext) c->depth = sl.own_depth;
}

// Images (rows padded to 256 B like a D3D12 placed footprint), half-res
// pre-pass images, identity chunk orders and zero costs of one slot.
inline bool slot_alloc(rv_ctx* c, FrameSlot& sl) {
    const int W = c->cfg.width, H = c->cfg.height;
    const size_t hbytes = (size_t)(W / 2) * (H / 2) * 4;
    if (sl.own_color.reserve(c, c->own_color_pitch * H) || sl.own_mv.reserve(c, c->own_mv_pitch * H) ||
        sl.own_depth.reserve(c, c->own_depth_pitch * H) || sl.hdist.reserve(c, hbytes) || sl.hshadow.reserve(c, hbytes))
        return false;
    hipMemset(sl.own_color, 0, c->own_color_pitch * H);
    hipMemset(sl.own_mv, 0, c->own_mv_pitch * H);
    hipMemset(sl.own_depth, 0, c->own_depth_pitch * H);
    hipMemset(sl.hdist, 0, hbytes);
    hipMemset(sl.hshadow, 0, hbytes);
    const uint32_t nb[2][2] = {{(uint32_t)(W / 2), (uint32_t)(H / 2)}, {(uint32_t)W, (uint32_t)H}};
    for (int g = 0; g < 2; g++) {
        uint32_t npad = n_chunks_pad(nb[g][0], nb[g][1]);
        std::vector<int> id(npad);
        for (uint32_t i = 0; i < npad; i++) id[i] = (int)i;
        if (sl.chunk_order[g].reserve(c, npad * 4) || sl.chunk_cost[g].reserve(c, npad * 4)) return false;
        hipMemcpy(sl.chunk_order[g], id.data(), npad * 4, hipMemcpyHostToDevice);
        hipMemset(sl.chunk_cost[g], 0, npad * 4);
    }
    return sl.done.ensure(c) == RV_OK && sl.gathered.ensure(c) == RV_OK;
}

// per frame: [0, NSTAGE-1) start of each frame stage, [NSTAGE-1] end of the
// frame, [NSTAGE] / [NSTAGE+1] start / end of the GI update before it
constexpr int EV_PER_FRAME = NSTAGE + 2;

inline uint64_t n_gi(const rv_ctx* c) { return (uint64_t)c->w.GX * c->w.GY * c->w.GZ; }
inline uint64_t n_csdf(const rv_ctx* c) { return (uint64_t)c->w.SX * c->w.SY * c->w.SZ; }
inline uint64_t n_bits_words(const rv_ctx* c) { return ((uint64_t)c->w.X * c->w.Y * c->w.Z) >> 5; }

inline f3 host_v(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }

// glm::normalize(vec3(10,5,-4)) (src/StateRender.cu:299, src/CoarseArray.cu:359)
inline f3 sun_dir() {
    float d = 10.0f * 10.0f + 5.0f * 5.0f + (-4.0f) * (-4.0f);
    float inv = 1.0f / sqrtf(d);
    return host_v(10.0f * inv, 5.0f * inv, -4.0f * inv);
}

inline World current_world(const rv_ctx* c) {
    World w = c->w;
    world_set_brick(w, c->brick);
    w.gi = c->gi;
    w.atlas = c->atlas;
    return w;
}



// A frame sequence: desc k = d[k * stride] (stride 0: one camera for every
// frame); after() = the frame that follows the sequence.
struct Seq {
    const rv_frame_desc* d = nullptr;
    int stride = 0, n = 0;
    const rv_frame_desc* next = nullptr;
    const rv_frame_desc& at(int k) const { return d[(size_t)k * stride]; }
    const rv_frame_desc& after() const { return next ? *next : at(n - 1); }
    bool uniform(int k0, int k1) const {   // frames [k0, k1) share one camera
        if (stride == 0) return true;
        for (int k = k0 + 1; k < k1; k++)
            if (std::memcmp(&at(k), &at(k0), sizeof(rv_frame_desc)) != 0) return false;
        return true;
    }
};


// ---------------------------------------------------------------- shared between the parts
// Not exported from the library (hidden visibility).
#define RV_HIDDEN __attribute__((visibility("hidden")))

// rv_abi.cpp (C linkage: defined inside its extern "C" block)
extern "C" {
RV_HIDDEN rv_status end_frame(rv_ctx* c);
RV_HIDDEN rv_status wait_all_frames(rv_ctx* c);   // every frame in flight and the last world/GI write
RV_HIDDEN rv_status mark_world(rv_ctx* c);        // a world/GI write: versions bumped, ev_world recorded
RV_HIDDEN rv_status world_top(rv_ctx* c);         // the exact early exits from the bits, after every write of them
RV_HIDDEN rv_status upload_ids(rv_ctx* c, DevIds& ids, const int32_t* src, int n, bool* changed);
RV_HIDDEN FrameParams make_params_d(rv_ctx* c, const rv_frame_desc& d, int32_t flags);
RV_HIDDEN rv_status upload_cams(rv_ctx* c, const Seq& q, hipStream_t st, const FrameCam** out,
                                const std::function<void(int, FrameCam&)>& fill = nullptr);
RV_HIDDEN rv_status run_stages(rv_ctx* c, FrameParams f, bool tiles, int which = 3);
RV_HIDDEN rv_status tile_list(rv_ctx* c, const int32_t* tile_ids, int32_t ntiles, int32_t tile_px);
}

// rv_edit.cpp: rv_create's limits on the world dims; a box list's validity in such a world
RV_HIDDEN bool dims_ok(int lx, int ly, int lz);
RV_HIDDEN bool boxes_ok(int lx, int ly, int lz, const rv_edit_box* b, int n);
// the dims of the host-only forms that take RV_WORLD_BITS words: a word is 32 x-consecutive voxels of one row
inline bool linear_dims_ok(int lx, int ly, int lz) { return dims_ok(lx, ly, lz) && lx >= 5; }
// rv_voxel_box is the host's voxel box [lo, hi) (its union, WordGrid and ColumnRange: include/rvgrt/rv_words.h).
// voxel_box_ok: inside a window of X Y Z voxels and non-empty
inline bool voxel_box_ok(int X, int Y, int Z, const rv_voxel_box& b) {
    return b.x0 >= 0 && b.y0 >= 0 && b.z0 >= 0 && b.x1 <= X && b.y1 <= Y && b.z1 <= Z && b.x1 > b.x0 && b.y1 > b.y0 &&
           b.z1 > b.z0;
}
// The nested boxes of a local CSDF rebuild (launch_csdf_box) around the coarse cells E = [e0, e1) whose
// solidity may have changed, in a grid of S cells: rf = E grown by 64 per axis, and the inputs it needs
// read backwards through the passes (rv_edit.cpp), each clipped to the grid; passes() = the cells the four
// passes visit.  An empty E on an axis (e0 == e1, at a face) stands for cells that left the grid there.
struct CsdfBoxes {
    CellBox rs, rx, ry, rf;
    uint64_t passes() const { return rs.cells() + rx.cells() + ry.cells() + rf.cells(); }
};
RV_HIDDEN CsdfBoxes csdf_boxes(const int e0[3], const int e1[3], const int S[3]);
// Scratch of the local passes is kept between calls while it is small (a single block's is 26 MB).
constexpr size_t EDIT_SCRATCH_KEEP = (size_t)64 << 20;
// the passes over `n` sets of boxes, one after the other, through edit_t0 / edit_t1; waits for them, then
// frees the scratch when it is above EDIT_SCRATCH_KEEP
RV_HIDDEN rv_status csdf_rebuild_boxes(rv_ctx* c, const CsdfBoxes* b, int n);
// The end of an edit whose changed voxels lie in the voxel box `changed`, after the caller has waited for the
// frames, written the bits and marked the columns: geom_ver, the exits (world_top), the local CSDF rebuild
// and mark_world or the whole-grid build, whichever visits fewer cells, and rv_world_edit_info's record
RV_HIDDEN rv_status edit_finish(rv_ctx* c, const rv_voxel_box& changed);

// rv_detached.cpp: what rv_world_fall shares with rv_world_detached -- the check of the box, flags, cap and
// arrays; the slots of nc component records in ascending order of their seeds and one record as rv_component
// in window coordinates; the host form of the query: the kernels' passes word after word, which leave what
// launch_detach_query leaves on the device (include/rvgrt/rv_detached.h); and the device form's opening.
namespace rv { struct DetachBox; }
struct DetachHost {
    std::vector<uint32_t> W, D, L, slot;
    std::vector<DetachRec> rec;
    uint64_t voxels = 0;   // detached
};
RV_HIDDEN bool detach_args_ok(int X, int Y, int Z, const rv_voxel_box* b, int32_t flags, const void* comps, int64_t cap,
                              const uint32_t* mask, size_t mask_bytes);
RV_HIDDEN std::vector<uint32_t> detach_seed_order(const DetachRec* rec, uint32_t nc);
RV_HIDDEN rv_component detach_component(const rv::DetachBox& b, const DetachRec& r);
RV_HIDDEN void detach_host_query(const LinearWorld& w, const rv::DetachBox& b, uint32_t* mask, DetachHost& q);
// detach_run_query: detach_scratch reserved (the query's layout + extra_dwords), the wait for a world write on
// another stream, the query's launches, cnt = {components, detached voxels} read back (waits for the stream).
// detach_copy_records: the copy of nc records into detach_h enqueued; the caller adds its own and waits once.
RV_HIDDEN rv_status detach_run_query(rv_ctx* c, const rv::DetachBox& b, size_t extra_dwords, uint32_t cnt[2]);
RV_HIDDEN rv_status detach_copy_records(rv_ctx* c, const rv::DetachBox& b, uint32_t nc);

// rv_persist.cpp: the marking, capturing and restoring that rv_world_edit, rv_world_import, rv_world_build
// and rv_world_scroll do while persistence is on (every one returns at once while it is off).  A range is
// the brick columns [bx0, bx1) x [bz0, bz1) of the window (ColumnRange, rv_words.h); keys are taken at the origin
// (ox, oz).
RV_HIDDEN void persist_mark(rv_ctx* c, const ColumnRange& r);
// how many columns of r are dirty / have an entry in the store when the window's origin is (ox, oz)
RV_HIDDEN size_t persist_dirty_in(const rv_ctx* c, const ColumnRange& r, int32_t ox, int32_t oz);
RV_HIDDEN size_t persist_stored_in(const rv_ctx* c, const ColumnRange& r, int32_t ox, int32_t oz);
// the device list and staging buffer for n columns; before anything is written, like scroll_tmp
RV_HIDDEN rv_status persist_reserve(rv_ctx* c, size_t ncols);
// the dirty columns of r: gathered, copied to the host (waits for the stream), put into the store (a newer
// copy replaces an entry) and, unless keep_dirty, taken out of the dirty set.  Nothing dirty: no launch, copy or wait
RV_HIDDEN rv_status persist_capture(rv_ctx* c, const ColumnRange& r, bool keep_dirty);
// the stored columns of r, at the context's current origin: scattered over the freshly generated bits (waits
// for the stream), taken out of the store and marked dirty.  Nothing stored: no launch, copy or wait
RV_HIDDEN rv_status persist_restore(rv_ctx* c, const ColumnRange& r);
RV_HIDDEN void persist_trim(rv_ctx* c);   // frees the device buffers when above EDIT_SCRATCH_KEEP

// rv_comm.cpp: the four exchange operations of the loops and the bounded wait
RV_HIDDEN double comm_timeout_s();
RV_HIDDEN void comm_detach(rv_comm* m);
RV_HIDDEN rv_status comm_wait_bounded(rv_ctx* c, rv_comm* m, double timeout_s);
RV_HIDDEN rv_status comm_all_gather(rv_ctx* c, rv_comm* m, const void* send, void* recv, size_t bytes, hipStream_t s);
RV_HIDDEN rv_status comm_group_start(rv_ctx* c, rv_comm* m);
RV_HIDDEN rv_status comm_send(rv_ctx* c, rv_comm* m, const void* buf, size_t bytes, int peer, hipStream_t s);
RV_HIDDEN rv_status comm_recv(rv_ctx* c, rv_comm* m, void* buf, size_t bytes, int peer, hipStream_t s);
RV_HIDDEN rv_status comm_group_end(rv_ctx* c, rv_comm* m, hipStream_t s);
