"""ctypes binding of the C ABI in include/rvgrt.h (librvgrt_hip.so).

The shared library is built in-tree by __graft_entry__.build() /
`make -C rvgrt_amd/csrc`.  There is no fallback: if the library (or a
gfx950 device) is missing, loading fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RVGRT_LIB: an alternative build of the same library (A/B experiments)
LIB_PATH = os.environ.get("RVGRT_LIB") or os.path.join(_HERE, "librvgrt_hip.so")

RV_OK, RV_ERR_INVALID, RV_ERR_HIP, RV_ERR_OOM, RV_ERR_STATE, RV_ERR_NO_DEVICE = range(6)
RV_F_PREPASS, RV_F_WATER, RV_F_GI, RV_F_SHADOW, RV_F_STATS, RV_F_REF_FETCH = 1, 2, 4, 8, 16, 32
RV_FLAGS_REFERENCE = RV_F_PREPASS | RV_F_WATER | RV_F_GI
RV_IMAGE_COLOR, RV_IMAGE_MOTION, RV_IMAGE_DEPTH, RV_IMAGE_HALF_DIST, RV_IMAGE_HALF_SHADOW = range(5)
RV_WORLD_BITS, RV_WORLD_CSDF, RV_WORLD_GI = range(3)
# test hooks (rv_world_export only): the exit tables as built on the device
RV_WORLD_COLTOP, RV_WORLD_HORIZON, RV_WORLD_DTOP = 3, 4, 5
# rv_trace_rays_variant: look-ahead group (1, 4, 8) | these bits
RV_TRACE_SKY, RV_TRACE_SUN, RV_TRACE_COL = 0x100, 0x200, 0x400
RV_PATH_FUSED, RV_PATH_WAVEFRONT = 0, 1
# rv_set_option (include/rvgrt.h rv_option)
RV_OPT_PIPE_ORDER, RV_OPT_BATCH_STREAMS, RV_OPT_FLOW_SPIN, RV_OPT_FLOW_FORCE_FALLBACK, RV_OPT_GI_PAIRS, \
    RV_OPT_GI_SHARD_PROBE, RV_OPT_PIPE_MIX, RV_OPT_PIPE_MIX_LAST = range(1, 9)
# rv_config.exits_off bits
RV_EXIT_SKY, RV_EXIT_COLUMN, RV_EXIT_SUN = 1, 2, 4

STAGES = ["pp_primary", "pp_shadow", "primary", "shadow", "water", "cones", "shade", "gi"]
STATUS_NAMES = {0: "RV_OK", 1: "RV_ERR_INVALID", 2: "RV_ERR_HIP", 3: "RV_ERR_OOM",
                4: "RV_ERR_STATE", 5: "RV_ERR_NO_DEVICE"}


class rv_config(C.Structure):
    _fields_ = [("log2_x", C.c_int32), ("log2_y", C.c_int32), ("log2_z", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32), ("flags", C.c_int32),
                ("seed_x", C.c_int32), ("seed_z", C.c_int32),
                ("ref_compat", C.c_int32), ("ref_oob_jy", C.c_float),
                ("atlas_rgba8", C.c_void_p), ("atlas_w", C.c_int32), ("atlas_h", C.c_int32),
                ("gi_rays_per_frame", C.c_uint32), ("gi_init_saturate", C.c_int32),
                ("tex_table", C.c_int32), ("exits_off", C.c_int32)]


class rv_camera(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("forward", C.c_float * 3), ("right", C.c_float * 3),
                ("up", C.c_float * 3), ("mul", C.c_float * 2), ("add", C.c_float * 2)]


class rv_frame_desc(C.Structure):
    _fields_ = [("cam", rv_camera), ("vp", C.c_float * 16), ("prev_vp", C.c_float * 16),
                ("time", C.c_float), ("jitter_x", C.c_float), ("jitter_y", C.c_float)]


class rv_hit(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("normal", C.c_float * 3), ("u", C.c_float),
                ("v", C.c_float), ("hit", C.c_int32), ("undef", C.c_int32),
                ("sphere_steps", C.c_int32), ("dda_steps", C.c_int32),
                ("csdf_checks", C.c_int32), ("pad", C.c_int32)]


class rv_edit_box(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("z0", C.c_int32),
                ("x1", C.c_int32), ("y1", C.c_int32), ("z1", C.c_int32), ("solid", C.c_int32)]


RV_EDIT_MAX_BOXES = 1024


class rv_edit_shape(C.Structure):
    _fields_ = [("kind", C.c_int32), ("solid", C.c_int32), ("c2", C.c_int32 * 3), ("r2", C.c_int32 * 3)]


# rv_edit_shape.kind; the caps on a list and on a radius (half-voxels)
RV_SHAPE_ELLIPSOID, RV_SHAPE_CYLINDER_X, RV_SHAPE_CYLINDER_Y, RV_SHAPE_CYLINDER_Z = range(4)
RV_EDIT_MAX_SHAPES = 256
RV_SHAPE_MAX_R2 = 512


class rv_gi_box(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("z0", C.c_int32),
                ("x1", C.c_int32), ("y1", C.c_int32), ("z1", C.c_int32)]


RV_RELIGHT_INIT = 1
RV_RELIGHT_MAX_RECORDS = 1 << 23


class rv_body(C.Structure):
    _fields_ = [("lo", C.c_float * 3), ("size", C.c_float * 3), ("delta", C.c_float * 3)]


class rv_body_out(C.Structure):
    _fields_ = [("lo", C.c_float * 3), ("flags", C.c_uint32)]


# rv_body_out.flags, rv_world_bodies_move's flags
RV_BODY_XN, RV_BODY_XP, RV_BODY_YN, RV_BODY_YP, RV_BODY_ZN, RV_BODY_ZP = 1, 2, 4, 8, 16, 32
RV_BODY_START_SOLID, RV_BODY_EDGE, RV_BODY_INVALID = 64, 128, 256
RV_BODIES_OPEN_EDGES = 1
RV_BODIES_MAX = 1 << 24


class rv_voxel_box(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("z0", C.c_int32),
                ("x1", C.c_int32), ("y1", C.c_int32), ("z1", C.c_int32)]


class rv_component(C.Structure):
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("seed", C.c_int32 * 3), ("voxels", C.c_uint32)]


# rv_world_detached's flags and the cap on a box's volume
RV_DETACHED_CLEAR = 1
RV_DETACHED_MAX_VOXELS = 1 << 21


class rv_fallen(C.Structure):
    _fields_ = [("comp", rv_component), ("fall", C.c_int32), ("flags", C.c_uint32)]


# rv_fallen.flags
RV_FALL_STOPPED = 1


class rv_stamp(C.Structure):
    _fields_ = [("pattern", C.c_int32), ("op", C.c_int32), ("orient", C.c_int32), ("at", C.c_int32 * 3)]


class rv_pattern_host(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("bits", C.c_void_p)]


# rv_stamp.op, rv_stamp.orient (any OR); the caps on a pattern's dims, a context's patterns and a stamp list
RV_STAMP_SET, RV_STAMP_CLEAR, RV_STAMP_COPY = range(3)
RV_ORIENT_SWAP_XZ, RV_ORIENT_FLIP_X, RV_ORIENT_FLIP_Z = 1, 2, 4
RV_PATTERN_MAX_DIM = 256
RV_PATTERN_MAX = 256
RV_STAMP_MAX = 1024

STAT_FIELDS = ["traces", "primary", "shadow", "refl", "refl_shadow", "prepass_primary",
               "prepass_shadow", "cones", "cone_steps", "sphere_steps", "dda_steps",
               "csdf_checks", "tex_samples", "undef_hits", "gi_traces", "frames"]


class rv_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in STAT_FIELDS]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in STAT_FIELDS}


# (name, restype, argtypes) for every entry point declared in include/rvgrt.h
P, I32, U32, U64, I64, F, SZ = (C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_int64,
                                C.c_float, C.c_size_t)
FP = C.POINTER(C.c_float)
SIGNATURES = [
    ("rv_abi_version", I32, []),
    ("rv_create", I32, [C.POINTER(rv_config), I32, C.POINTER(P)]),
    ("rv_destroy", None, [P]),
    ("rv_last_error", C.c_char_p, [P]),
    ("rv_set_stream", I32, [P, P]),
    ("rv_set_option", I32, [P, I32, C.c_int64]),
    ("rv_get_option", I32, [P, I32, C.POINTER(C.c_int64)]),
    ("rv_pipe_layout_map", I32, [C.c_int64, C.c_int64, C.POINTER(U32), U32, U32, P, P]),
    ("rv_set_frame_path", I32, [P, I32]),
    ("rv_tile_shard_assign", I32, [I32, I32, I32, I32, C.c_float, P]),
    ("rv_set_gi_async", I32, [P, I32]),
    ("rv_set_pipeline", I32, [P, I32]),
    ("rv_set_frame_group", I32, [P, I32]),
    ("rv_get_frame_group", I32, [P, C.POINTER(C.c_int32)]),
    ("rv_set_flow", I32, [P, I32]),
    ("rv_tex_table_info", I32, [P, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    ("rv_flow_info", I32, [P, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("rv_set_gi_stats", I32, [P, I32]),
    ("rv_set_frames_in_flight", I32, [P, I32]),
    ("rv_world_build", I32, [P]),
    ("rv_world_import", I32, [P, I32, P, SZ]),
    ("rv_world_export", I32, [P, I32, P, SZ]),
    ("rv_csdf_build", I32, [P]),
    ("rv_gi_init", I32, [P]),
    ("rv_world_edit", I32, [P, C.POINTER(rv_edit_box), I32]),
    ("rv_world_edit_info", I32, [P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    ("rv_world_edit_region", I32, [I32, I32, I32, C.POINTER(rv_edit_box), I32, C.POINTER(C.c_int32),
                                   C.POINTER(C.c_uint64)]),
    ("rv_world_edit_shapes", I32, [P, P, I32, C.POINTER(U64), C.POINTER(U64)]),
    ("rv_world_edit_shapes_at", I32, [I32, I32, I32, P, P, I32, C.POINTER(U64), C.POINTER(U64)]),
    ("rv_world_edit_shapes_box", I32, [I32, I32, I32, P, I32, P, P]),
    ("rv_gi_relight", I32, [P, C.POINTER(rv_gi_box), U32, I32, I32]),
    ("rv_gi_relight_info", I32, [P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("rv_gi_relight_box", I32, [I32, I32, I32, C.POINTER(rv_edit_box), I32, I32, C.POINTER(rv_gi_box)]),
    ("rv_world_scroll", I32, [P, I32, I32]),
    ("rv_world_scroll_info", I32, [P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("rv_world_scroll_region", I32, [I32, I32, I32, I32, I32, C.POINTER(C.c_int32), C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_int32)]),
    ("rv_scroll_view", I32, [I32, I32, C.POINTER(rv_camera), P, P]),
    ("rv_world_persist", I32, [P, I32]),
    ("rv_world_persist_info", I32, [P, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("rv_world_persist_flush", I32, [P]),
    ("rv_world_store_list", I32, [P, P, I64, C.POINTER(C.c_int64)]),
    ("rv_world_store_get", I32, [P, I32, I32, P, SZ]),
    ("rv_world_store_put", I32, [P, I32, I32, P, SZ]),
    ("rv_world_store_clear", I32, [P]),
    ("rv_world_columns_read", I32, [P, P, I32, P, SZ]),
    ("rv_persist_column_map", I32, [I32, I32, I32, I32, I32, P]),
    ("rv_world_bodies_move", I32, [P, P, I64, I32, P]),
    ("rv_world_bodies_move_device", I32, [P, P, I64, I32, P]),
    ("rv_world_bodies_move_at", I32, [I32, I32, I32, P, P, I64, I32, P]),
    ("rv_world_bodies_info", I32, [P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("rv_world_detached", I32, [P, C.POINTER(rv_voxel_box), I32, P, I64, C.POINTER(I64), C.POINTER(U64), P, SZ]),
    ("rv_world_detached_at", I32, [I32, I32, I32, P, C.POINTER(rv_voxel_box), P, I64, C.POINTER(I64),
                                   C.POINTER(U64), P, SZ]),
    ("rv_world_detached_info", I32, [P, C.POINTER(U64), C.POINTER(U64), C.POINTER(U64)]),
    ("rv_world_fall", I32, [P, C.POINTER(rv_voxel_box), I32, P, I64, C.POINTER(I64), C.POINTER(U64),
                            C.POINTER(rv_voxel_box)]),
    ("rv_world_fall_at", I32, [I32, I32, I32, P, C.POINTER(rv_voxel_box), I32, P, I64, C.POINTER(I64),
                               C.POINTER(U64), C.POINTER(rv_voxel_box), P, SZ]),
    ("rv_world_fall_info", I32, [P, C.POINTER(U64), C.POINTER(U64), C.POINTER(U64)]),
    ("rv_pattern_create", I32, [P, I32, I32, I32, P, SZ, C.POINTER(I32)]),
    ("rv_pattern_capture", I32, [P, C.POINTER(rv_voxel_box), C.POINTER(I32)]),
    ("rv_pattern_read", I32, [P, I32, C.POINTER(I32), P, SZ]),
    ("rv_pattern_destroy", I32, [P, I32]),
    ("rv_world_stamp", I32, [P, P, I32, C.POINTER(U64), C.POINTER(U64), C.POINTER(rv_voxel_box)]),
    ("rv_world_stamp_at", I32, [I32, I32, I32, P, P, I32, P, I32, C.POINTER(U64), C.POINTER(U64)]),
    ("rv_world_stamp_box", I32, [I32, I32, I32, P, I32, P, I32, P, P]),
    ("rv_world_stamp_info", I32, [P, C.POINTER(U64), C.POINTER(U64), C.POINTER(I32), C.POINTER(U64)]),
    ("rv_texture_origin_set", I32, [P, I32, I32]),
    ("rv_texture_follow_scroll", I32, [P, I32]),
    ("rv_texture_origin_get", I32, [P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("rv_texture_tiles", I32, [P, P, I64, P]),
    ("rv_texture_tile_at", I32, [I32, I32, P, I64, P]),
    ("rv_gi_update", I32, [P, U32, U64, U64]),
    ("rv_update_gi_data", I32, [P]),
    ("rv_draw_cuda", I32, [P, P, P, P, P, P, P, F, F]),
    ("rv_frame", I32, [P, C.POINTER(rv_camera), P, P, F, F, F, I32]),
    ("rv_frame_tiles", I32, [P, C.POINTER(rv_camera), P, P, F, F, F, I32, P, I32, I32]),
    ("rv_tile_buffer", I32, [P, C.POINTER(P), C.POINTER(SZ)]),
    ("rv_bind_tile_buffer", I32, [P, P, SZ]),
    ("rv_untile", I32, [P, P, P, I32, I32]),
    ("rv_bind_output", I32, [P, I32, P, SZ]),
    ("rv_image_ptr", I32, [P, I32, C.POINTER(P), C.POINTER(SZ)]),
    ("rv_readback", I32, [P, I32, P, SZ]),
    ("rv_trace_rays", I32, [P, P, P, P, I64, P]),
    ("rv_trace_rays_variant", I32, [P, I32, P, P, P, I64, P]),
    ("rv_world_top_info", I32, [P, C.POINTER(U32)]),
    ("rv_camera_from_pose", I32, [F, F, F, F, F, I32, I32, C.POINTER(rv_camera), P]),
    ("rv_stats_get", I32, [P, C.POINTER(rv_stats)]),
    ("rv_stats_stage", I32, [P, I32, C.POINTER(rv_stats)]),
    ("rv_stats_reset", I32, [P]),
    ("rv_timing_enable", I32, [P, I32]),
    ("rv_timing_get", I32, [P, C.POINTER(C.c_double), C.POINTER(I32)]),
    ("rv_timing_stages", I32, [P, C.POINTER(C.c_double), I32, C.POINTER(I32)]),
    ("rv_timing_launches", I32, [P, C.POINTER(I32), I32]),
    ("rv_sync", I32, [P]),
    ("rv_comm_unique_id", I32, [C.c_char_p, P, SZ]),
    ("rv_comm_create", I32, [P, C.c_char_p, P, SZ, I32, I32, C.POINTER(P)]),
    ("rv_comm_destroy", None, [P]),
    ("rv_comm_wait", I32, [P, I32]),
    ("rv_loopback_group_create", I32, [I32, I32, C.POINTER(P)]),
    ("rv_loopback_group_destroy", None, [P]),
    ("rv_comm_create_loopback", I32, [P, P, I32, I32, C.POINTER(P)]),
    ("rv_set_tile_shard_weighted", I32, [P, I32, I32, I32, F]),
    ("rv_set_gather_bpp", I32, [P, I32]),
    ("rv_set_tile_shard", I32, [P, I32, I32, I32]),
    ("rv_render_frames", I32, [P, I32, C.POINTER(rv_camera), P, P, F, F, F, I32, I32, P]),
    ("rv_render_frame_seq", I32, [P, I32, C.POINTER(rv_frame_desc), C.POINTER(rv_frame_desc), I32, I32, P]),
]

_lib = None


def load() -> C.CDLL:
    """Load librvgrt_hip.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run __graft_entry__.build() "
                               "(make -C rvgrt_amd/csrc); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, res, args in SIGNATURES:
            if os.environ.get("RVGRT_LIB") and not hasattr(L, name):
                continue   # an older experiment build: entry points it predates stay unbound
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class RvError(RuntimeError):
    pass
