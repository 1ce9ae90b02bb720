"""rvgrt_amd -- MI355X-native voxel ray-tracing render path.

A drop-in for RubenVlieger/RVGRT's CUDA render path (StateRender::drawCUDA
and the raytracing_functions it calls), rebuilt as hand-written HIP kernels
for gfx950 behind the C ABI in include/rvgrt.h (librvgrt_hip.so).
"""
from . import _lib
from ._lib import (RV_F_GI, RV_F_PREPASS, RV_F_REF_FETCH, RV_F_SHADOW, RV_F_STATS, RV_F_WATER,
                   RV_FLAGS_REFERENCE, RV_IMAGE_COLOR, RV_IMAGE_DEPTH, RV_IMAGE_HALF_DIST,
                   RV_IMAGE_HALF_SHADOW, RV_IMAGE_MOTION, RV_WORLD_BITS, RV_WORLD_CSDF,
                   RV_WORLD_GI, RvError, RV_OPT_PIPE_ORDER, RV_OPT_BATCH_STREAMS, RV_OPT_FLOW_SPIN,
                   RV_OPT_FLOW_FORCE_FALLBACK, RV_OPT_GI_PAIRS, RV_OPT_GI_SHARD_PROBE, RV_OPT_PIPE_MIX,
                   RV_OPT_PIPE_MIX_LAST, RV_EXIT_SKY,
                   RV_EXIT_COLUMN, RV_EXIT_SUN, RV_WORLD_COLTOP, RV_WORLD_HORIZON, RV_WORLD_DTOP,
                   RV_TRACE_SKY, RV_TRACE_SUN, RV_TRACE_COL, RV_BODY_XN, RV_BODY_XP, RV_BODY_YN, RV_BODY_YP,
                   RV_BODY_ZN, RV_BODY_ZP, RV_BODY_START_SOLID, RV_BODY_EDGE, RV_BODY_INVALID,
                   RV_BODIES_OPEN_EDGES, RV_DETACHED_CLEAR, RV_DETACHED_MAX_VOXELS, RV_FALL_STOPPED,
                   RV_SHAPE_ELLIPSOID, RV_SHAPE_CYLINDER_X, RV_SHAPE_CYLINDER_Y, RV_SHAPE_CYLINDER_Z,
                   RV_EDIT_MAX_SHAPES, RV_SHAPE_MAX_R2, RV_STAMP_SET, RV_STAMP_CLEAR, RV_STAMP_COPY,
                   RV_ORIENT_SWAP_XZ, RV_ORIENT_FLIP_X, RV_ORIENT_FLIP_Z, RV_PATTERN_MAX_DIM, RV_PATTERN_MAX,
                   RV_STAMP_MAX)
from .configs import CONFIGS, RenderConfig
from .render import Comm, LoopbackGroup, StateRender, camera_dict, camera_from_pose, edit_region, frame_desc, relight_box, scroll_region, scroll_view, texture_tile_at, persist_column_map, bodies_move_at, detached_at, COMPONENT_DTYPE, fall_at, FALLEN_DTYPE, edit_shapes_at, edit_shapes_box, settle_parts, stamp_at, stamp_box

__all__ = ["StateRender", "Comm", "LoopbackGroup", "camera_from_pose", "camera_dict", "frame_desc", "edit_region", "relight_box", "scroll_region", "scroll_view", "texture_tile_at", "persist_column_map", "bodies_move_at", "detached_at", "COMPONENT_DTYPE", "RV_DETACHED_CLEAR", "RV_DETACHED_MAX_VOXELS", "fall_at", "FALLEN_DTYPE", "RV_FALL_STOPPED", "edit_shapes_at", "edit_shapes_box", "settle_parts", "RV_SHAPE_ELLIPSOID", "RV_SHAPE_CYLINDER_X", "RV_SHAPE_CYLINDER_Y", "RV_SHAPE_CYLINDER_Z", "RV_EDIT_MAX_SHAPES", "RV_SHAPE_MAX_R2", "stamp_at", "stamp_box", "RV_STAMP_SET", "RV_STAMP_CLEAR", "RV_STAMP_COPY", "RV_ORIENT_SWAP_XZ", "RV_ORIENT_FLIP_X", "RV_ORIENT_FLIP_Z", "RV_PATTERN_MAX_DIM", "RV_PATTERN_MAX", "RV_STAMP_MAX", "CONFIGS", "RenderConfig", "RvError",
           "RV_F_GI", "RV_F_PREPASS", "RV_F_REF_FETCH", "RV_F_SHADOW", "RV_F_STATS", "RV_F_WATER",
           "RV_FLAGS_REFERENCE", "RV_IMAGE_COLOR", "RV_IMAGE_DEPTH", "RV_IMAGE_HALF_DIST",
           "RV_IMAGE_HALF_SHADOW", "RV_IMAGE_MOTION", "RV_WORLD_BITS", "RV_WORLD_CSDF",
           "RV_WORLD_GI", "_lib"]
