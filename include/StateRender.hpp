// StateRender.hpp -- header-only C++ facade over the C ABI (rvgrt.h) with
// the reference's host interface, so the reference's host code keeps its
// call sites:
//   class StateRender           <- include/StateRender.cuh:11-47
//   StateRender::drawCUDA(...)  <- src/StateRender.cu:289-346 (same signature)
//   CoarseArray::UpdateGIData   <- src/CoarseArray.cu:376-395 (updateGIData)
//   State::Create init sequence <- src/State.cpp:24-56 (create)
//   Camera                      <- include/Camera.hpp:5-17
// The vector/matrix types are layout-compatible with glm::vec3 / glm::mat4
// (3 floats; 16 floats, column-major).  With glm on the include path define
// RVGRT_USE_GLM to take glm's own types.  Errors throw std::runtime_error
// (as the reference's CUDA_CHECK does, include/cumath.cuh:10-14).
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "rvgrt.h"

#ifdef RVGRT_USE_GLM
#include <glm/glm.hpp>
#endif

namespace rvgrt {

#ifdef RVGRT_USE_GLM
using vec3 = glm::vec3;
using mat4 = glm::mat4;
inline const float* data(const vec3& v) { return &v.x; }
inline const float* data(const mat4* m) { return m ? &(*m)[0][0] : nullptr; }
#else
struct vec3 { float x = 0, y = 0, z = 0; };
struct mat4 { float m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}; };
inline const float* data(const vec3& v) { return &v.x; }
inline const float* data(const mat4* m) { return m ? m->m : nullptr; }
#endif

// include/Camera.hpp:5-17
struct Camera {
    vec3 pos, forward, right, up;
    float cameraMultiplyFactor[2] = {0, 0};
    float cameraAddFactor[2] = {0, 0};
};

inline void check(rv_status s, rv_ctx* c, const char* what) {
    if (s != RV_OK)
        throw std::runtime_error(std::string(what) + " failed (" + std::to_string((int)s) +
                                 "): " + (c ? rv_last_error(c) : ""));
}

struct Settings {
    int log2_x = 12, log2_y = 9, log2_z = 12;   // reference world 4096 x 512 x 4096
    int width = 1280, height = 800;             // reference dispWIDTH x dispHEIGHT
    int flags = RV_FLAGS_REFERENCE;             // INCLUDEGI build
    bool ref_compat = true;                     // c_cam off-by-one
    int device = 0;
};

class StateRender {
public:
    explicit StateRender(const Settings& s = Settings(), const uint8_t* atlas_rgba8 = nullptr, int atlas_w = 256,
                         int atlas_h = 256) : settings_(s) {
        rv_config cfg{};
        cfg.log2_x = s.log2_x; cfg.log2_y = s.log2_y; cfg.log2_z = s.log2_z;
        cfg.width = s.width; cfg.height = s.height; cfg.flags = s.flags;
        cfg.ref_compat = s.ref_compat ? 1 : 0;
        cfg.atlas_rgba8 = atlas_rgba8; cfg.atlas_w = atlas_w; cfg.atlas_h = atlas_h;
        check(rv_create(&cfg, s.device, &ctx_), nullptr, "rv_create");
    }
    ~StateRender() { rv_destroy(ctx_); }
    StateRender(const StateRender&) = delete;
    StateRender& operator=(const StateRender&) = delete;

    // State::Create: CArray::fill -> CoarseArray::GenerateSDF -> InitializeGIData
    void create() { check(rv_world_build(ctx_), ctx_, "rv_world_build"); }

    // CoarseArray::UpdateGIData: RAYPS cells per call, rolling offset
    void updateGIData() { check(rv_update_gi_data(ctx_), ctx_, "rv_update_gi_data"); }

    // Place / break blocks (no reference counterpart: its world is fixed after CArray::fill): voxel
    // boxes set or cleared in place, the CSDF and the early exits rebuilt around them (rv_world_edit)
    void editWorld(const rv_edit_box* boxes, int n) { check(rv_world_edit(ctx_, boxes, n), ctx_, "rv_world_edit"); }
    // Craters, shafts, domes, boulders: ellipsoids and axis-aligned elliptic cylinders (half-voxel centre and
    // radii) set or cleared in order by one launch, clipped to the window; the voxels that turned solid / empty
    // into *set / *cleared (rv_world_edit_shapes)
    void editShapes(const rv_edit_shape* shapes, int n, uint64_t* set = nullptr, uint64_t* cleared = nullptr) {
        check(rv_world_edit_shapes(ctx_, shapes, n, set, cleared), ctx_, "rv_world_edit_shapes");
    }
    // Prefabs kept on the device: an nx x ny x nz block of bits (rows along x padded to 32-bit words) becomes a
    // pattern, as does a voxel box of the world without leaving the device; the id is the lowest free slot
    // (rv_pattern_create, rv_pattern_capture, rv_pattern_read, rv_pattern_destroy)
    int patternCreate(int nx, int ny, int nz, const uint32_t* bits, size_t bytes) {
        int32_t id = -1;
        check(rv_pattern_create(ctx_, nx, ny, nz, bits, bytes, &id), ctx_, "rv_pattern_create");
        return id;
    }
    int patternCapture(const rv_voxel_box& box) {
        int32_t id = -1;
        check(rv_pattern_capture(ctx_, &box, &id), ctx_, "rv_pattern_capture");
        return id;
    }
    void patternRead(int id, int32_t dims[3], uint32_t* bits = nullptr, size_t bytes = 0) {
        check(rv_pattern_read(ctx_, id, dims, bits, bytes), ctx_, "rv_pattern_read");
    }
    void patternDestroy(int id) { check(rv_pattern_destroy(ctx_, id), ctx_, "rv_pattern_destroy"); }
    // Patterns pasted into the world by one launch, in order, each at an offset, in one of the 8 orientations that
    // keep y up, setting, clearing or copying, clipped to the window; the voxels that turned solid / empty into
    // *set / *cleared, the union of the clipped boxes into *changed (rv_world_stamp)
    void stampWorld(const rv_stamp* stamps, int n, uint64_t* set = nullptr, uint64_t* cleared = nullptr,
                    rv_voxel_box* changed = nullptr) {
        check(rv_world_stamp(ctx_, stamps, n, set, cleared, changed), ctx_, "rv_world_stamp");
    }
    // Matter moved by (dx, dy, dz), composed of the calls above: the box captured, cleared where it was and copied
    // to where it goes in one stampWorld; the horizontal counterpart of fallDetached
    void moveWorld(const rv_voxel_box& box, int dx, int dy, int dz, uint64_t* set = nullptr, uint64_t* cleared = nullptr,
                   rv_voxel_box* changed = nullptr) {
        const int id = patternCapture(box);
        const rv_stamp s[2] = {{id, RV_STAMP_CLEAR, 0, {box.x0, box.y0, box.z0}},
                               {id, RV_STAMP_COPY, 0, {box.x0 + dx, box.y0 + dy, box.z0 + dz}}};
        const rv_status st = rv_world_stamp(ctx_, s, 2, set, cleared, changed);
        rv_pattern_destroy(ctx_, id);
        check(st, ctx_, "rv_world_stamp");
    }
    // What an edit left floating in a voxel box: up to cap components into comps, their total returned; with
    // RV_DETACHED_CLEAR they are cleared like an editWorld of those voxels (rv_world_detached)
    int64_t findDetached(const rv_voxel_box& box, int flags, rv_component* comps, int64_t cap, uint64_t* voxels = nullptr) {
        int64_t n = 0;
        check(rv_world_detached(ctx_, &box, flags, comps, cap, &n, voxels, nullptr, 0), ctx_, "rv_world_detached");
        return n;
    }
    // One round of falling: every detached component of the box drops until something stops it, or maxFall rows
    // (0: no limit); up to cap records into comps, their total returned, the changed voxel box into *changed.
    // Repeat over *changed until it returns 0 (rv_world_fall)
    int64_t fallDetached(const rv_voxel_box& box, int maxFall, rv_fallen* comps, int64_t cap, rv_voxel_box* changed = nullptr) {
        int64_t n = 0;
        check(rv_world_fall(ctx_, &box, maxFall, comps, cap, &n, nullptr, changed), ctx_, "rv_world_fall");
        return n;
    }
    // The world window moved by (dx, 0, dz) voxels over the generated terrain, in place (rv_world_scroll)
    void scroll(int dx, int dz) { check(rv_world_scroll(ctx_, dx, dz), ctx_, "rv_world_scroll"); }
    // The texture origin (rv_texture_origin_set) and whether scroll() moves it with the window
    // (rv_texture_follow_scroll): setTextureOrigin(seed_x, seed_z) once, then textureFollowScroll(true), anchors the
    // block textures to the terrain
    void setTextureOrigin(int ox, int oz) { check(rv_texture_origin_set(ctx_, ox, oz), ctx_, "rv_texture_origin_set"); }
    void textureFollowScroll(bool on) { check(rv_texture_follow_scroll(ctx_, on ? 1 : 0), ctx_, "rv_texture_follow_scroll"); }
    void textureOrigin(int& ox, int& oz, bool& follow) const {
        int32_t x = 0, z = 0, f = 0;
        check(rv_texture_origin_get(ctx_, &x, &z, &f), ctx_, "rv_texture_origin_get");
        ox = x; oz = z; follow = f != 0;
    }
    // The GI cells of a box refreshed at once after an edit: `iterations` update steps with RNG frames
    // frame0, frame0 + 1, ... (rv_gi_relight; rv_gi_relight_box picks the box around the edit)
    void relightGI(const rv_gi_box& box, uint32_t frame0, int iterations, bool init = false) {
        check(rv_gi_relight(ctx_, &box, frame0, iterations, init ? RV_RELIGHT_INIT : 0), ctx_, "rv_gi_relight");
    }

    // StateRender::drawCUDA, identical parameter list and order
    void drawCUDA(const vec3& pos, const vec3& fo, const vec3& up, const vec3& ri,
                  mat4* unjitteredViewProjectionMatrix, mat4* prevUnjitteredViewProjectionMatrix,
                  float jitterX, float jitterY) {
        check(rv_draw_cuda(ctx_, data(pos), data(fo), data(up), data(ri), data(unjitteredViewProjectionMatrix),
                           data(prevUnjitteredViewProjectionMatrix), jitterX, jitterY),
              ctx_, "rv_draw_cuda");
    }

    // Offscreen replacement of the D3D12 present: RGBA8, tightly packed rows
    std::vector<uint8_t> readbackColor() {
        std::vector<uint8_t> px((size_t)settings_.width * settings_.height * 4);
        check(rv_readback(ctx_, RV_IMAGE_COLOR, px.data(), 0), ctx_, "rv_readback");
        return px;
    }

    // Bind caller-owned device buffers like the reference's interop heaps
    void bindOutput(rv_image_kind kind, void* devPtr, size_t pitch) {
        check(rv_bind_output(ctx_, kind, devPtr, pitch), ctx_, "rv_bind_output");
    }

    static Camera cameraFromPose(float px, float py, float pz, float yaw, float pitch, int w, int h, mat4* vp) {
        rv_camera c{};
        check(rv_camera_from_pose(px, py, pz, yaw, pitch, w, h, &c, vp ? const_cast<float*>(data(vp)) : nullptr),
              nullptr, "rv_camera_from_pose");
        Camera out;
        out.pos = {c.pos[0], c.pos[1], c.pos[2]};
        out.forward = {c.forward[0], c.forward[1], c.forward[2]};
        out.right = {c.right[0], c.right[1], c.right[2]};
        out.up = {c.up[0], c.up[1], c.up[2]};
        for (int i = 0; i < 2; i++) { out.cameraMultiplyFactor[i] = c.mul[i]; out.cameraAddFactor[i] = c.add[i]; }
        return out;
    }

    void sync() { check(rv_sync(ctx_), ctx_, "rv_sync"); }
    rv_ctx* handle() { return ctx_; }
    const Settings& settings() const { return settings_; }

private:
    Settings settings_;
    rv_ctx* ctx_ = nullptr;
};

}  // namespace rvgrt
