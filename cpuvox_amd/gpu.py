"""ctypes binding of libcpuvox_gpu.so (include/cpuvox_gpu.h): the C-ABI
drop-in for RenderManager.DrawSegments (Assets/Code/RenderManager.cs:258-372)
running as HIP kernels on MI355X.

There is NO CPU fallback: if the library or a HIP device is missing every
call raises.  (The CPU oracle lives under oracle/ and is test infrastructure;
this package never imports it.)
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .host import CameraData, Frame, LOD_LEVELS, SegmentData, WorldSet

_HERE = os.path.dirname(os.path.abspath(__file__))

RAYBUFFER_TOPDOWN = 0
RAYBUFFER_LEFTRIGHT = 1
DRAW_SYNC = 0
DRAW_ASYNC = 1
LATENCY_AUTO, LATENCY_NEVER, LATENCY_ALWAYS = 0, 1, 2  # cvx_set_latency_kernel

# The export lists, one per header under include/ that declares cvx_ entry points, and ABI_HEADERS, the table of them.
# tests/test_abi_mirrors.py checks every list against its header, the libraries, the C# file and the argtypes of _bind.
# include/cpuvox_gpu.h: the list its hosts were built against
EXPORTS = [
    "cvx_create", "cvx_destroy", "cvx_last_error", "cvx_set_stream", "cvx_world_upload", "cvx_set_resolution",
    "cvx_set_buffer_count", "cvx_draw_segments", "cvx_draw_segments_batch", "cvx_set_shard", "cvx_set_latency_kernel", "cvx_set_world_repeat", "cvx_synchronize",
    "cvx_clear_raybuffer", "cvx_read_raybuffer", "cvx_blit_segments", "cvx_blit_segments_batch", "cvx_raybuffer_device_ptr",
    "cvx_screen_device_ptr", "cvx_last_draw_ms", "cvx_enable_counters", "cvx_get_counters",
    "cvx_get_raybuffer_layout", "cvx_version", "cvx_bind_raybuffers", "cvx_draw_time_stats", "cvx_copy_rows", "cvx_draw_segments_placed",
    "cvx_world_downsample", "cvx_world_build_lods", "cvx_free", "cvx_world_set_columns", "cvx_world_edit", "cvx_world_edit_stats",
    "cvx_world_brush", "cvx_world_pick", "cvx_world_pick_device",
    "cvx_world_read_region", "cvx_world_read_level", "cvx_world_compact", "cvx_world_stamp_mesh", "cvx_world_copy", "cvx_world_pieces", "cvx_world_settle",
    "cvx_world_cavities",
    "cvx_world_light", "cvx_world_light_lamps", "cvx_world_move", "cvx_world_move_device",
    "cvx_world_nav_build", "cvx_nav_field_goals", "cvx_nav_query", "cvx_nav_query_device", "cvx_nav_field_destroy",
    "cvx_world_surface", "cvx_world_surface_device", "cvx_surface_triangles",
    "cvx_world_read_voxels", "cvx_world_read_voxels_device", "cvx_world_write_voxels", "cvx_world_write_voxels_device",
    "cvx_world_distance", "cvx_world_distance_device",
    "cvx_shard_plan_create", "cvx_shard_plan_destroy", "cvx_shard_plan_tile_count", "cvx_shard_plan_sections", "cvx_shard_plan_tile_out", "cvx_shard_plan_transfer",
    "cvx_comm_unique_id", "cvx_comm_create", "cvx_comm_create_timeout", "cvx_comm_destroy", "cvx_exchange",
    "cvx_image_plan_create", "cvx_image_plan_destroy", "cvx_image_plan_tile_count", "cvx_image_plan_sizes", "cvx_image_plan_transfer",
    "cvx_image_plan_tile_out", "cvx_image_pack", "cvx_image_exchange", "cvx_image_unpack",
]
# include/cpuvox_gpu_heights.h: terrain as height maps
HEIGHTS_EXPORTS = ["cvx_world_read_heights", "cvx_world_read_heights_device", "cvx_world_write_heights", "cvx_world_write_heights_device"]
# include/cpuvox_gpu_models.h: voxel models at any orientation and scale
MODELS_EXPORTS = ["cvx_world_place_models", "cvx_world_place_models_device", "cvx_world_read_model", "cvx_world_read_model_device",
                  "cvx_model_instance_from_matrix"]
# include/cpuvox_gpu_spread.h: travel-distance fields through air or solid
SPREAD_EXPORTS = ["cvx_world_spread", "cvx_world_spread_device"]
# include/cpuvox_gpu_surface_rects.h: the exposed faces merged into rectangles
SURFACE_RECTS_EXPORTS = ["cvx_world_surface_rects", "cvx_world_surface_rects_device", "cvx_surface_rect_triangles"]
# include/cpuvox_gpu_snapshot.h: snapshots of rectangles that stay on the device
SNAPSHOT_EXPORTS = ["cvx_world_snapshot", "cvx_snapshot_info_get", "cvx_world_snapshot_restore", "cvx_world_snapshot_diff", "cvx_world_snapshot_diff_device",
                    "cvx_snapshot_destroy"]
# include/cpuvox_gpu_lift.h: the floating pieces as models with mass moments
LIFT_EXPORTS = ["cvx_world_lift_pieces", "cvx_world_lift_pieces_device", "cvx_lifted_piece_mass"]
# include/cpuvox_gpu_contacts.h: where placed models touch the world.  A family of its own (prefix cvxc_, as the host library's cvxh_), so not a row
# of ABI_HEADERS: tests/test_abi_contacts.py checks this list against its header, the libraries, the C# file and the argtypes of _bind.
CONTACTS_EXPORTS = ["cvxc_world_contacts", "cvxc_world_contacts_device", "cvxc_contact_response"]
# include/cpuvox_gpu_pair_contacts.h: where placed models touch each other.  Another family of its own (prefix cvxp_), no row of ABI_HEADERS either:
# tests/test_abi_pair_contacts.py checks it.
PAIR_CONTACTS_EXPORTS = ["cvxp_model_contacts", "cvxp_model_contacts_device", "cvxp_box_pairs", "cvxp_pair_response"]
# include/cpuvox_gpu_model_pick.h: first-hit rays against placed models.  A family of its own again (prefix cvxq_), no row of ABI_HEADERS:
# tests/test_abi_model_pick.py checks it.
MODEL_PICK_EXPORTS = ["cvxq_model_pick", "cvxq_model_pick_device"]
# include/cpuvox_gpu_model_draw.h: placed models drawn into the rendered frame.  One more family of its own (prefix cvxv_), no row of ABI_HEADERS:
# tests/test_abi_model_draw.py checks it.
MODEL_DRAW_EXPORTS = ["cvxv_view_from_camera", "cvxv_view_rays", "cvxv_models_draw", "cvxv_models_draw_device"]
# include/cpuvox_gpu_sweep.h: how far placed models can move before they touch the world.  A family of its own too (prefix cvxs_), no row of
# ABI_HEADERS: tests/test_abi_sweep.py checks it.
SWEEP_EXPORTS = ["cvxs_world_sweep", "cvxs_world_sweep_device", "cvxs_sweep_offset", "cvxs_instance_moved"]
# include/cpuvox_gpu_pair_sweep.h: how far placed models can move before they touch each other.  A family of its own as well (prefix cvxm_), no
# row of ABI_HEADERS: tests/test_abi_pair_sweep.py checks it.
PAIR_SWEEP_EXPORTS = ["cvxm_pair_sweep", "cvxm_pair_sweep_device"]
# include/cpuvox_gpu_model_brush.h: world-space brush strokes that carve and paint placed models.  A family of its own too (prefix cvxd_, which
# the diagnostic cvxd_clip_census of include/cpuvox_gpu_diag.h shares), no row of ABI_HEADERS: tests/test_abi_model_brush.py checks it.
MODEL_BRUSH_EXPORTS = ["cvxd_models_brush", "cvxd_models_brush_device", "cvxd_model_mass"]
# include/cpuvox_gpu_diag.h: only the experiment / profiling builds export these (cpuvox_amd.gpu.use_library(".../libcpuvox_gpu_exp.so"))
DIAG_EXPORTS = ["cvx_selftest_math", "cvx_selftest_scan", "cvx_selftest_lone", "cvx_debug_occupancy", "cvx_debug_section_cycles", "cvx_debug_section_histogram",
                "cvx_debug_last_launch", "cvx_debug_settle", "cvx_debug_cavities"]
# (header, its export list, its file under host/csharp/ or None), in the order the headers came; every build exports all but the last list
ABI_HEADERS = [
    ("cpuvox_gpu.h", EXPORTS, "CpuVoxGpu.cs"),
    ("cpuvox_gpu_heights.h", HEIGHTS_EXPORTS, "CpuVoxGpuHeights.cs"),
    ("cpuvox_gpu_models.h", MODELS_EXPORTS, "CpuVoxGpuModels.cs"),
    ("cpuvox_gpu_spread.h", SPREAD_EXPORTS, "CpuVoxGpuSpread.cs"),
    ("cpuvox_gpu_surface_rects.h", SURFACE_RECTS_EXPORTS, "CpuVoxGpuSurfaceRects.cs"),
    ("cpuvox_gpu_snapshot.h", SNAPSHOT_EXPORTS, "CpuVoxGpuSnapshot.cs"),
    ("cpuvox_gpu_lift.h", LIFT_EXPORTS, "CpuVoxGpuLift.cs"),
    ("cpuvox_gpu_diag.h", DIAG_EXPORTS, None),
]
# cvx_debug_last_launch: out[0], the kernel instance a draw went to
INSTANCE_COUNTING, INSTANCE_BATCH, INSTANCE_LONE, INSTANCE_LONE_WIDE = 0, 1, 2, 3
LAUNCH_FIELDS = ("instance", "tiles", "waves", "min_rays", "max_rays", "max_dup_shift", "split", "lds_words")
# cvxd_clip_census (include/cpuvox_gpu_diag.h; the first of the diagnostics with the prefix cvxd_, which like the cvxc_ / cvxp_ / cvxq_ families are no rows of the
# cvx_ export lists above): a lane's class at one end of the frustum clip, and the wave-uniform predicates counted
CLIP_CLASSES = ("straddle", "foot below / top inside", "foot inside / top above", "both inside", "entirely outside", "inverted straddle", "inverted rest")
CLIP_PREDICATES = (("nothing_clipped", "a1 and b2 false in every lane at both ends"), ("no_max_clip", "... and a2 false too"), ("no_min_clip", "... and b1 false too"),
                   ("mirror_nothing_clipped", "b1 and a2 false in every lane at both ends"), ("mirror_no_max_clip", "... and b2 false too"),
                   ("mirror_no_min_clip", "... and a1 false too"), ("inverted_straddle", "a1 and b2 true, a2 false in every lane at both ends"))


class Counters(C.Structure):
    _fields_ = [("S", C.c_int64), ("E", C.c_int64), ("C", C.c_int64), ("P", C.c_int64), ("R", C.c_int64),
                ("lodVisits", C.c_int64 * LOD_LEVELS)]

    def algorithmic_bytes(self) -> int:
        return 12 * self.S + 4 * self.E + 4 * self.C + 4 * self.P + 80 * self.R

    def as_dict(self):
        return {"S": self.S, "E": self.E, "C": self.C, "P": self.P, "R": self.R,
                "lodVisits": list(self.lodVisits), "bytes": self.algorithmic_bytes()}


BRUSH_FILL, BRUSH_CARVE, BRUSH_PAINT = 0, 1, 2  # cvx_brush_stroke.op
SHAPE_BOX, SHAPE_SPHERE = 0, 1                  # cvx_brush_stroke.shape
SHAPE_CAPSULE, SHAPE_ELLIPSOID = 16, 17         # (the codes 2 .. 15 are not shapes)
BRUSH_MAX_STROKES = 4096
COPY_REPLACE = 3                                # cvx_copy_placement.op, besides BRUSH_FILL / CARVE / PAINT
COPY_MAX_PLACEMENTS = 1024
PIECES_REPORT, PIECES_REMOVE = 0, 1              # cvx_world_pieces: op
ANCHOR_GROUND, ANCHOR_OUTSIDE, ANCHOR_LARGEST = 1, 2, 4  # ... anchors (bits)
SETTLE_UNLIMITED = 0                             # cvx_world_settle: maxDrop
CAVITIES_REPORT, CAVITIES_FILL = 0, 1            # cvx_cavity_params.op
CAVITY_OPEN_DEFAULT = 0x3B                       # ... openFaces: every face but -Y
LIGHT_TO_RGB, LIGHT_TO_ALPHA = 0, 1              # cvx_light_params.target
LIGHT_MAX_LAMPS, LAMP_MAX_RADIUS = 4096, 64      # cvx_world_light_lamps
MOVE_UNIT = 256                                  # cvx_move_body: position units per LOD-0 voxel
MOVE_SOLID_BELOW, MOVE_SOLID_SIDES = 1, 2        # cvx_move_body.flags
MOVED_BLOCKED_MASK, MOVED_RESTING, MOVED_STARTS_SOLID, MOVED_STEPPED, MOVED_INVALID = 0x3F, 1 << 6, 1 << 7, 1 << 8, -(1 << 31)  # cvx_move_result.flags
SURFACE_OUTSIDE_DEFAULT = 0x04                   # cvx_world_surface: solidOutside, the ground below y = 0 is solid
SURFACE_IGNORE_COLOUR = 1                        # ... flags
DISTANCE_FAR = 0x7FFFFFFF                        # cvx_world_distance: no such voxel within max_distance
DISTANCE_TO_SOLID, DISTANCE_TO_AIR, DISTANCE_SIGNED = 0, 1, 2  # ... mode
HEIGHTS_WALLED = 1                               # cvx_world_write_heights: flags, a neighbour outside the footprint counts as y0
MODELS_MAX_MODELS, MODELS_MAX_INSTANCES = 256, 4096  # cvx_world_place_models: modelCount, instanceCount
SPREAD_AIR, SPREAD_SOLID = 0, 1                  # cvx_spread_params.medium
SPREAD_UNREACHED, SPREAD_BLOCKED = -1, -2        # cvx_world_spread: passable but not reached within max_steps / not passable
SPREAD_MAX_SEEDS, SPREAD_MAX_STEPS = 4096, 65534
SPREAD_TILE = (8, 64, 8)                         # CVX_SPREAD_TILE_X / _Y / _Z: the (x, y, z) extents of the tile a workgroup relaxes
SNAPSHOT_IGNORE_COLOUR = 1                       # cvx_world_snapshot_diff: flags
LIFT_COPY, LIFT_REMOVE = 0, 1                    # cvx_world_lift_pieces: op
PAIR_CONTACTS_MAX_PAIRS = 65536                  # CVXP_MAX_PAIRS: cvxp_model_contacts, pairCount
MODEL_PICK_MAX_RAYS = 65536                      # CVXQ_PICK_MAX_RAYS: cvxq_model_pick, rayCount
DRAW_WORLD, DRAW_DEPTH_TEST = 1, 2                # CVXV_DRAW_WORLD, CVXV_DRAW_DEPTH_TEST: cvxv_models_draw, flags
DRAW_MAX_SIZE = 8192                             # CVXV_MAX_SIZE: cvxv_view, width and height
SWEEP_MAX_MOTION = 4096                          # CVXS_MAX_MOTION: cvxs_world_sweep, every component of a motion
NAV_MAX_GOALS = 4096                             # cvx_world_nav_build / cvx_nav_field_goals: goalCount
FACE_INSIDE, FACE_MISS = 6, -1                  # cvx_pick_hit.face besides 0..5 = -X, +X, -Y, +Y, -Z, +Z


class ModelMap(C.Structure):
    """cvx_model_map: image_i = (m[i][0] (2 v0 + 1) + m[i][1] (2 v1 + 1) + m[i][2] (2 v2 + 1) + 2 t[i]) >> 17, m and t in units of 2^-16."""
    _fields_ = [("m", (C.c_int32 * 3) * 3), ("pad_", C.c_int32), ("t", C.c_int64 * 3)]


class Model(C.Structure):
    _fields_ = [("size", C.c_int32 * 3), ("pad_", C.c_int32), ("argb", C.c_void_p), ("solid", C.c_void_p)]


class ModelInstance(C.Structure):
    _fields_ = [("toModel", ModelMap), ("boxMin", C.c_int32 * 3), ("boxMax", C.c_int32 * 3), ("model", C.c_int32), ("op", C.c_int32)]


class ContactResult(C.Structure):  # cvxc_contact_result
    _fields_ = [("voxels", C.c_int64), ("overlap", C.c_int64), ("points", C.c_int64), ("firstPoint", C.c_int64), ("sum", C.c_uint64 * 3),
                ("normal", C.c_int64 * 3), ("origin", C.c_int32 * 3), ("min", C.c_int32 * 3), ("max", C.c_int32 * 3), ("pad_", C.c_int32)]


class ContactPoint(C.Structure):  # cvxc_contact_point
    _fields_ = [("voxel", C.c_int32 * 3), ("instance", C.c_int32), ("faces", C.c_int32), ("argb", C.c_uint32)]


class ContactsSummary(C.Structure):  # cvxc_contacts_summary
    _fields_ = [("touching", C.c_int64), ("overlap", C.c_int64), ("points", C.c_int64), ("voxels", C.c_int64)]


class PairResult(C.Structure):  # cvxp_pair_result
    _fields_ = [("overlap", C.c_int64), ("points", C.c_int64), ("firstPoint", C.c_int64), ("sum", C.c_uint64 * 3), ("pushA", C.c_int64 * 3),
                ("pushB", C.c_int64 * 3), ("origin", C.c_int32 * 3), ("min", C.c_int32 * 3), ("max", C.c_int32 * 3), ("a", C.c_int32), ("b", C.c_int32),
                ("pad_", C.c_int32)]


class PairPoint(C.Structure):  # cvxp_pair_point
    _fields_ = [("voxel", C.c_int32 * 3), ("pair", C.c_int32), ("facesA", C.c_int32), ("facesB", C.c_int32), ("argbA", C.c_uint32), ("argbB", C.c_uint32)]


class PairsSummary(C.Structure):  # cvxp_pairs_summary
    _fields_ = [("touching", C.c_int64), ("overlap", C.c_int64), ("points", C.c_int64), ("jobs", C.c_int64)]


class ModelHit(C.Structure):  # cvxq_model_hit
    _fields_ = [("voxel", C.c_int32 * 3), ("face", C.c_int32), ("argb", C.c_uint32), ("t", C.c_float), ("instance", C.c_int32), ("modelVoxel", C.c_int32 * 3),
                ("pad_", C.c_int32 * 2)]


class SweepResult(C.Structure):  # cvxs_sweep_result
    _fields_ = [("steps", C.c_int32), ("hit", C.c_int32), ("axis", C.c_int32), ("sign", C.c_int32), ("free", C.c_int32 * 3), ("at", C.c_int32 * 3),
                ("pad_", C.c_int32 * 2)]


class SweepsSummary(C.Structure):  # cvxs_sweeps_summary
    _fields_ = [("hits", C.c_int64), ("startsSolid", C.c_int64), ("jobs", C.c_int64), ("points", C.c_int64)]


class PairSweepResult(C.Structure):  # cvxm_pair_sweep_result
    _fields_ = [("sweep", SweepResult), ("a", C.c_int32), ("b", C.c_int32)]


class PairSweepsSummary(C.Structure):  # cvxm_pair_sweeps_summary
    _fields_ = [("hits", C.c_int64), ("startsSolid", C.c_int64), ("jobs", C.c_int64), ("pad_", C.c_int64)]


class ModelBrushResult(C.Structure):  # cvxd_model_result
    _fields_ = [("voxels", C.c_int64), ("carved", C.c_int64), ("painted", C.c_int64), ("sum", C.c_uint64 * 3), ("moment", C.c_uint64 * 6), ("min", C.c_int32 * 3),
                ("max", C.c_int32 * 3), ("pad_", C.c_int32 * 2)]


class ModelBrushInstanceResult(C.Structure):  # cvxd_instance_result
    _fields_ = [("carved", C.c_int64), ("painted", C.c_int64)]


class ModelBrushSummary(C.Structure):  # cvxd_brush_summary
    _fields_ = [("carved", C.c_int64), ("painted", C.c_int64), ("models", C.c_int64), ("jobs", C.c_int64)]


class DrawView(C.Structure):  # cvxv_view
    _fields_ = [("origin", C.c_float * 3), ("maxT", C.c_float), ("dir0", C.c_double * 3), ("dirX", C.c_double * 3), ("dirY", C.c_double * 3),
                ("width", C.c_int32), ("height", C.c_int32)]


class DrawSummary(C.Structure):  # cvxv_draw_summary
    _fields_ = [("pixelsDrawn", C.c_int64), ("pixelsOccluded", C.c_int64), ("jobs", C.c_int64), ("pad_", C.c_int64)]


class SpreadParams(C.Structure):  # cvx_spread_params
    _fields_ = [("boxMin", C.c_int32 * 3), ("boxMax", C.c_int32 * 3), ("medium", C.c_int32), ("stepFaces", C.c_int32), ("maxSteps", C.c_int32),
                ("pad_", C.c_int32)]


class SpreadSeed(C.Structure):  # cvx_spread_seed
    _fields_ = [("voxel", C.c_int32 * 3), ("start", C.c_int32)]


class SpreadSummary(C.Structure):  # cvx_spread_summary
    _fields_ = [("passable", C.c_int64), ("reached", C.c_int64), ("largestDistance", C.c_int32), ("seedsUsed", C.c_int32), ("launches", C.c_int32),
                ("pad_", C.c_int32), ("tileVisits", C.c_int64)]


class SnapshotInfo(C.Structure):  # cvx_snapshot_info
    _fields_ = [("x0", C.c_int32), ("z0", C.c_int32), ("sizeX", C.c_int32), ("sizeZ", C.c_int32), ("levelCount", C.c_int32), ("dimX", C.c_int32),
                ("dimY", C.c_int32), ("dimZ", C.c_int32), ("deviceBytes", C.c_int64), ("elements", C.c_int64)]


class SnapshotChange(C.Structure):  # cvx_snapshot_change
    _fields_ = [("x", C.c_int32), ("z", C.c_int32), ("yMin", C.c_int32), ("yMax", C.c_int32)]


class SnapshotDiffSummary(C.Structure):  # cvx_snapshot_diff_summary
    _fields_ = [("changedColumns", C.c_int64), ("changedVoxels", C.c_int64), ("min", C.c_int32 * 3), ("max", C.c_int32 * 3), ("pad_", C.c_int32 * 2)]


class BrushStroke(C.Structure):
    _fields_ = [("op", C.c_int32), ("shape", C.c_int32), ("a", C.c_int32 * 3), ("b", C.c_int32 * 3), ("argb", C.c_uint32), ("pad_", C.c_int32)]


class PickRay(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("direction", C.c_float * 3), ("maxT", C.c_float), ("pad_", C.c_float)]


class PickHit(C.Structure):
    _fields_ = [("voxel", C.c_int32 * 3), ("face", C.c_int32), ("argb", C.c_uint32), ("t", C.c_float)]


class CopyPlacement(C.Structure):
    _fields_ = [("srcMin", C.c_int32 * 3), ("srcMax", C.c_int32 * 3), ("dst", C.c_int32 * 3), ("transform", C.c_int32), ("op", C.c_int32),
                ("move", C.c_int32)]


class Piece(C.Structure):  # cvx_piece
    _fields_ = [("min", C.c_int32 * 3), ("max", C.c_int32 * 3), ("seed", C.c_int32 * 3), ("pad_", C.c_int32), ("voxels", C.c_int64)]


class PiecesSummary(C.Structure):  # cvx_pieces_summary
    _fields_ = [("floatingPieces", C.c_int64), ("floatingVoxels", C.c_int64), ("anchoredPieces", C.c_int64), ("anchoredVoxels", C.c_int64)]


class LiftedPiece(C.Structure):  # cvx_lifted_piece
    _fields_ = [("piece", Piece), ("offset", C.c_int64), ("sum", C.c_uint64 * 3), ("moment", C.c_uint64 * 6)]


class LiftSummary(C.Structure):  # cvx_lift_summary
    _fields_ = [("pieces", PiecesSummary), ("storedPieces", C.c_int64), ("storedVoxels", C.c_int64), ("neededVoxels", C.c_int64), ("pad_", C.c_int64)]


class SettleSummary(C.Structure):  # cvx_settle_summary
    _fields_ = [("floatingPieces", C.c_int64), ("floatingVoxels", C.c_int64), ("fallenPieces", C.c_int64), ("fallenVoxels", C.c_int64),
                ("largestDrop", C.c_int32), ("pad_", C.c_int32)]


class CavityParams(C.Structure):  # cvx_cavity_params
    _fields_ = [("boxMin", C.c_int32 * 3), ("boxMax", C.c_int32 * 3), ("openFaces", C.c_int32), ("op", C.c_int32), ("argb", C.c_uint32), ("pad_", C.c_int32),
                ("maxVoxels", C.c_int64)]


class CavitiesSummary(C.Structure):  # cvx_cavities_summary
    _fields_ = [("enclosedCavities", C.c_int64), ("enclosedVoxels", C.c_int64), ("selectedCavities", C.c_int64), ("selectedVoxels", C.c_int64),
                ("openRegions", C.c_int64), ("openVoxels", C.c_int64)]


class LightParams(C.Structure):  # cvx_light_params
    _fields_ = [("boxMin", C.c_int32 * 3), ("boxMax", C.c_int32 * 3), ("sunDir", C.c_int32 * 3), ("sunLevel", C.c_int32), ("sunRange", C.c_int32),
                ("skyLevel", C.c_int32), ("skyRange", C.c_int32), ("floorLevel", C.c_int32), ("target", C.c_int32), ("pad_", C.c_int32)]


class Lamp(C.Structure):  # cvx_lamp
    _fields_ = [("pos", C.c_int32 * 3), ("radius", C.c_int32), ("level", C.c_int32), ("pad_", C.c_int32 * 3)]


class MoveBody(C.Structure):  # cvx_move_body
    _fields_ = [("pos", C.c_int32 * 3), ("size", C.c_int32 * 3), ("delta", C.c_int32 * 3), ("stepUp", C.c_int32), ("flags", C.c_int32), ("pad_", C.c_int32)]


class MoveResult(C.Structure):  # cvx_move_result
    _fields_ = [("pos", C.c_int32 * 3), ("flags", C.c_int32)]


class NavParams(C.Structure):  # cvx_nav_params
    _fields_ = [("boxMin", C.c_int32 * 3), ("boxMax", C.c_int32 * 3), ("width", C.c_int32), ("height", C.c_int32), ("stepUp", C.c_int32),
                ("maxDrop", C.c_int32), ("maxSteps", C.c_int32), ("pad_", C.c_int32)]


class NavStep(C.Structure):  # cvx_nav_step
    _fields_ = [("cell", C.c_int32 * 3), ("distance", C.c_int32), ("next", C.c_int32 * 3), ("direction", C.c_int32)]


class NavSummary(C.Structure):  # cvx_nav_summary
    _fields_ = [("nodes", C.c_int64), ("reached", C.c_int64), ("goalsResolved", C.c_int32), ("largestDistance", C.c_int32),
                ("columnsWithSeveralNodes", C.c_int64), ("launches", C.c_int32), ("pad_", C.c_int32)]


class SurfaceQuad(C.Structure):  # cvx_surface_quad
    _fields_ = [("voxel", C.c_int32 * 3), ("face", C.c_int32), ("length", C.c_int32), ("argb", C.c_uint32)]


class SurfaceSummary(C.Structure):  # cvx_surface_summary
    _fields_ = [("quads", C.c_int64), ("unitFaces", C.c_int64), ("quadsPerFace", C.c_int64 * 6)]


class SurfaceRect(C.Structure):  # cvx_surface_rect
    _fields_ = [("voxel", C.c_int32 * 3), ("size", C.c_int32 * 3), ("face", C.c_int32), ("argb", C.c_uint32)]


class SurfaceRectsSummary(C.Structure):  # cvx_surface_rects_summary
    _fields_ = [("rects", C.c_int64), ("strips", C.c_int64), ("unitFaces", C.c_int64), ("rectsPerFace", C.c_int64 * 6)]


class _TextureStruct(C.Structure):  # cvx_mesh_texture
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgba", C.c_void_p)]


# numpy views of the same layouts: one declaration each, the structure's
STROKE_DTYPE, PICK_RAY_DTYPE, PICK_HIT_DTYPE = np.dtype(BrushStroke), np.dtype(PickRay), np.dtype(PickHit)
COPY_PLACEMENT_DTYPE = np.dtype(CopyPlacement)
PIECE_DTYPE, PIECES_SUMMARY_DTYPE = np.dtype(Piece), np.dtype(PiecesSummary)
LIFTED_PIECE_DTYPE = np.dtype(LiftedPiece)
SETTLE_SUMMARY_DTYPE = np.dtype(SettleSummary)
CAVITIES_SUMMARY_DTYPE = np.dtype(CavitiesSummary)
MOVE_BODY_DTYPE, MOVE_RESULT_DTYPE = np.dtype(MoveBody), np.dtype(MoveResult)
NAV_STEP_DTYPE, NAV_SUMMARY_DTYPE = np.dtype(NavStep), np.dtype(NavSummary)
SPREAD_SEED_DTYPE, SPREAD_SUMMARY_DTYPE = np.dtype(SpreadSeed), np.dtype(SpreadSummary)
SNAPSHOT_CHANGE_DTYPE = np.dtype(SnapshotChange)
SURFACE_QUAD_DTYPE, SURFACE_SUMMARY_DTYPE = np.dtype(SurfaceQuad), np.dtype(SurfaceSummary)
SURFACE_RECT_DTYPE, SURFACE_RECTS_SUMMARY_DTYPE = np.dtype(SurfaceRect), np.dtype(SurfaceRectsSummary)
CONTACT_RESULT_DTYPE, CONTACT_POINT_DTYPE, CONTACTS_SUMMARY_DTYPE = np.dtype(ContactResult), np.dtype(ContactPoint), np.dtype(ContactsSummary)
PAIR_RESULT_DTYPE, PAIR_POINT_DTYPE, PAIRS_SUMMARY_DTYPE = np.dtype(PairResult), np.dtype(PairPoint), np.dtype(PairsSummary)
MODEL_HIT_DTYPE = np.dtype(ModelHit)
DRAW_VIEW_DTYPE, DRAW_SUMMARY_DTYPE = np.dtype(DrawView), np.dtype(DrawSummary)
SWEEP_RESULT_DTYPE, SWEEPS_SUMMARY_DTYPE = np.dtype(SweepResult), np.dtype(SweepsSummary)
PAIR_SWEEP_RESULT_DTYPE, PAIR_SWEEPS_SUMMARY_DTYPE = np.dtype(PairSweepResult), np.dtype(PairSweepsSummary)
MODEL_BRUSH_RESULT_DTYPE, MODEL_BRUSH_INSTANCE_RESULT_DTYPE = np.dtype(ModelBrushResult), np.dtype(ModelBrushInstanceResult)
MODEL_BRUSH_SUMMARY_DTYPE = np.dtype(ModelBrushSummary)
MESH_VERTEX_DTYPE = np.dtype([("position", "<f4", 3), ("rgba", "u1", 4), ("uv", "<f4", 2), ("material", "<i4")])  # cvx_mesh_vertex (no structure here)
STAMP_MAX_MATERIALS = 128


def surface_triangles(quads):
    """cvx_surface_triangles: a SURFACE_QUAD_DTYPE array -> (4 n vertices as a MESH_VERTEX_DTYPE array, 6 n int32 indices): every quad's rectangle
    on its face plane, wound outward, with the vertex colour cvx_world_stamp_mesh turns back into the quad's colour word.  A pure host call."""
    q = np.ascontiguousarray(quads, dtype=SURFACE_QUAD_DTYPE)
    vertices = np.zeros(4 * q.size, dtype=MESH_VERTEX_DTYPE)
    indices = np.zeros(6 * q.size, dtype=np.int32)
    rc = lib().cvx_surface_triangles(q.ctypes.data if q.size else None, q.size, vertices.ctypes.data if q.size else None, indices.ctypes.data if q.size else None)
    if rc != 0:
        raise CvxError(f"cvx error {rc}: {lib().cvx_last_error(None).decode()}")
    return vertices, indices


def surface_rect_triangles(rects):
    """cvx_surface_rect_triangles: a SURFACE_RECT_DTYPE array -> (4 n vertices as a MESH_VERTEX_DTYPE array, 6 n int32 indices): every rectangle
    on its face plane, wound outward as surface_triangles winds a quad, with the same vertex colour.  A merged mesh has T-junctions.  A pure host
    call."""
    r = np.ascontiguousarray(rects, dtype=SURFACE_RECT_DTYPE)
    vertices = np.zeros(4 * r.size, dtype=MESH_VERTEX_DTYPE)
    indices = np.zeros(6 * r.size, dtype=np.int32)
    rc = lib().cvx_surface_rect_triangles(r.ctypes.data if r.size else None, r.size, vertices.ctypes.data if r.size else None, indices.ctypes.data if r.size else None)
    if rc != 0:
        raise CvxError(f"cvx error {rc}: {lib().cvx_last_error(None).decode()}")
    return vertices, indices


def strokes_array(strokes) -> np.ndarray:
    """A list of dicts {op, shape, a, b, argb} (b of a sphere may be just the radius) or a STROKE_DTYPE array -> a contiguous STROKE_DTYPE array.
    A capsule is {op, shape: SHAPE_CAPSULE, a, b, radius, argb}: the voxels within `radius` (into pad_) of the segment from voxel a to voxel b;
    an ellipsoid {op, shape: SHAPE_ELLIPSOID, a, b: (rx, ry, rz), argb}: centre a, radii b."""
    if isinstance(strokes, np.ndarray):
        return np.ascontiguousarray(strokes.astype(STROKE_DTYPE, copy=False))
    out = np.zeros(len(strokes), dtype=STROKE_DTYPE)
    for i, s in enumerate(strokes):
        b = s["b"] if "b" in s else s["radius"]
        out[i]["op"], out[i]["shape"] = s["op"], s["shape"]
        out[i]["a"] = s["a"]
        out[i]["b"] = [b, 0, 0] if np.isscalar(b) else b
        out[i]["argb"] = s.get("argb", 0) & 0xFFFFFFFF
        if s["shape"] == SHAPE_CAPSULE:
            out[i]["pad_"] = s["radius"]
    return out


def seeds_array(seeds) -> np.ndarray:
    """A list of (x, y, z) or (x, y, z, start) or a SPREAD_SEED_DTYPE array -> a contiguous SPREAD_SEED_DTYPE array."""
    if isinstance(seeds, np.ndarray) and seeds.dtype == SPREAD_SEED_DTYPE:
        return np.ascontiguousarray(seeds)
    out = np.zeros(len(seeds), dtype=SPREAD_SEED_DTYPE)
    for i, s in enumerate(seeds):
        if len(s) not in (3, 4):
            raise ValueError("world_spread: a seed is (x, y, z) or (x, y, z, start)")
        out[i]["voxel"] = [int(v) for v in s[:3]]
        out[i]["start"] = int(s[3]) if len(s) == 4 else 0
    return out


def _spread_tensor_ptr(tensor, box) -> int:
    lo, hi = box
    n = 1
    for a in range(3):
        n *= max(int(hi[a]) - int(lo[a]), 0)
    if str(getattr(tensor, "dtype", "")) != "torch.int32" or not tensor.is_contiguous() or tensor.numel() != n or not tensor.is_cuda:
        raise ValueError("world_spread_device: out_tensor is a contiguous int32 device tensor of X * Z * Y elements")
    return tensor.data_ptr()


def lifted_model(pieces, i: int, argb=None, solid=None):
    """The cvx_model fields of stored piece i of a world_lift_pieces result: (size (sx, sy, sz), argb, solid).  With numpy pools the arrays are
    views of shape (sx, sz, sy); with addresses (a device pool's data_ptr()) they are the addresses of the piece's first element, as
    Context.place_models_device takes them.  ValueError for a piece that is listed but not stored."""
    p = pieces[i]
    offset = int(p["offset"])
    if offset < 0:
        raise ValueError(f"lifted_model: piece {i} is listed but not stored")
    size = tuple(int(p["piece"]["max"][a]) - int(p["piece"]["min"][a]) for a in range(3))
    n = size[0] * size[1] * size[2]

    def part(pool, item_bytes):
        if pool is None:
            return None
        if isinstance(pool, int):
            return pool + offset * item_bytes if pool else 0
        return pool[offset:offset + n].reshape(size[0], size[2], size[1])
    return size, part(argb, 4), part(solid, 1)


def lifted_piece_mass(piece):
    """cvx_lifted_piece_mass of one LIFTED_PIECE_DTYPE element: (centre of mass (3,), inertia (Ixx, Iyy, Izz, Ixy, Iyz, Izx) about it) as float64
    arrays, for unit cubes of unit mass."""
    one = np.ascontiguousarray(np.asarray(piece, dtype=LIFTED_PIECE_DTYPE).reshape(1))
    centre, inertia = np.zeros(3), np.zeros(6)
    rc = lib().cvx_lifted_piece_mass(one.ctypes.data, centre.ctypes.data, inertia.ctypes.data)
    if rc != 0:
        raise ValueError("lifted_piece_mass: the piece has no voxels")
    return centre, inertia


def model_mass(result):
    """cvxd_model_mass of one MODEL_BRUSH_RESULT_DTYPE element (models_brush's): (centre of mass (3,), inertia (Ixx, Iyy, Izz, Ixy, Iyz, Izx)
    about it) as float64 arrays in MODEL coordinates, for unit cubes of unit mass: lifted_piece_mass' formula with min = 0.  A pure host call.
    ValueError for a model with no voxel left."""
    one = np.ascontiguousarray(np.asarray(result, dtype=MODEL_BRUSH_RESULT_DTYPE).reshape(1))
    centre, inertia = np.zeros(3), np.zeros(6)
    if lib().cvxd_model_mass(one.ctypes.data, centre.ctypes.data, inertia.ctypes.data) != 0:
        raise ValueError("model_mass: the model has no voxels")
    return centre, inertia


def contact_response(result):
    """cvxc_contact_response of one CONTACT_RESULT_DTYPE element: (centre of the overlap (3,), unit normal (3,) -- the way to push the body, 0
    when the faces cancel --, depth = overlap / |normal|) in float64; a body sunk k layers into flat ground gives depth k.  A pure host call.
    ValueError for a result without overlap."""
    one = np.ascontiguousarray(np.asarray(result, dtype=CONTACT_RESULT_DTYPE).reshape(1))
    centre, normal, depth = np.zeros(3), np.zeros(3), C.c_double()
    if lib().cvxc_contact_response(one.ctypes.data, centre.ctypes.data, normal.ctypes.data, C.byref(depth)) != 0:
        raise ValueError("contact_response: the result has no overlap")
    return centre, normal, depth.value


def _instance_array(instances):
    if isinstance(instances, C.Array) and instances._type_ is ModelInstance:
        return instances
    items = list(instances)
    if not all(isinstance(i, ModelInstance) for i in items):
        raise ValueError("instances are gpu.ModelInstance structures")
    return (ModelInstance * len(items))(*items)


def box_pairs(instances, margin: int = 0) -> np.ndarray:
    """cvxp_box_pairs, the broad phase of model_contacts: every (a, b), a < b, whose boxes intersect once each is widened by `margin` voxels on
    every side, as an (n, 2) int32 array in lexicographic order.  A pure host call."""
    inst = _instance_array(instances)
    found = C.c_int64()
    if lib().cvxp_box_pairs(C.addressof(inst) if len(inst) else None, len(inst), int(margin), None, 0, C.byref(found)) != 0:
        raise ValueError("box_pairs: margin is 0 .. 2^20")
    pairs = np.zeros((found.value, 2), dtype=np.int32)
    if found.value:
        lib().cvxp_box_pairs(C.addressof(inst), len(inst), int(margin), pairs.ctypes.data, found.value, C.byref(found))
    return pairs


def pair_response(result, which: int):
    """cvxp_pair_response of one PAIR_RESULT_DTYPE element: (centre of the overlap (3,), unit vector (3,) of pushA (which = 0: the way to move
    body a out of b) or pushB (which = 1), depth = overlap / |push|) in float64.  A pure host call.  ValueError for a result without overlap or
    another `which`."""
    one = np.ascontiguousarray(np.asarray(result, dtype=PAIR_RESULT_DTYPE).reshape(1))
    centre, normal, depth = np.zeros(3), np.zeros(3), C.c_double()
    if lib().cvxp_pair_response(one.ctypes.data, int(which), centre.ctypes.data, normal.ctypes.data, C.byref(depth)) != 0:
        raise ValueError("pair_response: the result has no overlap, or `which` is neither 0 nor 1")
    return centre, normal, depth.value


def bodies_array(bodies) -> np.ndarray:
    """A list of dicts {pos, size, delta (default 0), stepUp (default 0), flags (default 0)}, all in units of 1 / MOVE_UNIT voxel, or a
    MOVE_BODY_DTYPE array -> a contiguous MOVE_BODY_DTYPE array."""
    if isinstance(bodies, np.ndarray):
        return np.ascontiguousarray(bodies.astype(MOVE_BODY_DTYPE, copy=False))
    out = np.zeros(len(bodies), dtype=MOVE_BODY_DTYPE)
    for i, b in enumerate(bodies):
        out[i]["pos"], out[i]["size"] = b["pos"], b["size"]
        out[i]["delta"] = b.get("delta", (0, 0, 0))
        out[i]["stepUp"] = b.get("stepUp", 0)
        out[i]["flags"] = b.get("flags", 0)
    return out


def lamps_array(lamps):
    """A list of (pos, radius, level) or of dicts {pos, radius, level} -> a ctypes array of Lamp (cvx_world_light_lamps)."""
    out = (Lamp * len(lamps))()
    for i, lamp in enumerate(lamps):
        pos, radius, level = (lamp["pos"], lamp["radius"], lamp["level"]) if isinstance(lamp, dict) else lamp
        if len(pos) != 3:
            raise ValueError("a lamp's pos is three integers")
        out[i].pos[:] = [int(v) for v in pos]
        out[i].radius, out[i].level = int(radius), int(level)
    return out


def copy_placements_array(placements) -> np.ndarray:
    """A list of dicts {srcMin, srcMax, dst, transform (default 0), op (default COPY_REPLACE), move (default 0)} or a COPY_PLACEMENT_DTYPE array
    -> a contiguous COPY_PLACEMENT_DTYPE array."""
    if isinstance(placements, np.ndarray):
        return np.ascontiguousarray(placements.astype(COPY_PLACEMENT_DTYPE, copy=False))
    out = np.zeros(len(placements), dtype=COPY_PLACEMENT_DTYPE)
    for i, p in enumerate(placements):
        out[i]["srcMin"], out[i]["srcMax"], out[i]["dst"] = p["srcMin"], p["srcMax"], p["dst"]
        out[i]["transform"] = p.get("transform", 0)
        out[i]["op"] = p.get("op", COPY_REPLACE)
        out[i]["move"] = int(p.get("move", 0))
    return out


def screen_rays(camera, width: int, height: int, px, py):
    """(origins [N, 3], directions [N, 3]) of the rays through the centres of pixels (px, py) (row 0 = the bottom row, Unity screen space): the
    camera position and the inverse of its WorldToScreenMatrix (column-major, world -> 0..width x 0..height after the divide by w)."""
    m = np.array(camera.WorldToScreenMatrix[:], dtype=np.float64).reshape(4, 4).T  # (column-major storage)
    pos = np.array([camera.PositionXZ[0], camera.PositionY, camera.PositionXZ[1]], dtype=np.float64)
    inv = np.linalg.inv(m)
    # a point in front of the camera fixes the depth row: row 3 of the matrix is the view depth (w) of a point
    ahead = m @ np.append(pos + m[3, :3], 1.0)
    depth = ahead[2] / ahead[3]
    sx = np.asarray(px, dtype=np.float64) + 0.5
    sy = np.asarray(py, dtype=np.float64) + 0.5
    if sx.size and (sx.min() < 0 or sx.max() > width or sy.min() < 0 or sy.max() > height):
        raise ValueError(f"pixels outside the {width} x {height} screen")
    q = np.stack([sx, sy, np.full_like(sx, depth), np.ones_like(sx)], axis=-1) @ inv.T
    points = q[..., :3] / q[..., 3:4]
    directions = points - pos
    directions /= np.linalg.norm(directions, axis=-1, keepdims=True)
    return np.broadcast_to(pos, directions.shape).copy(), directions


def view_from_camera(camera, width: int, height: int, max_t: float = float("inf")) -> "DrawView":
    """cvxv_view_from_camera: the DrawView of a camera (host.CameraData, or anything with its WorldToScreenMatrix, PositionXZ and PositionY) at
    width x height -- what screen_rays computes, in doubles: the eye, the un-normalised direction through the centre of pixel (0, 0) and its
    change per pixel step in x and y.  A pure host call."""
    if isinstance(camera, CameraData):
        data = camera
    else:
        data = CameraData()
        data.WorldToScreenMatrix[:] = [float(v) for v in camera.WorldToScreenMatrix[:]]
        data.PositionXZ[:] = [float(v) for v in camera.PositionXZ[:]]
        data.PositionY = float(camera.PositionY)
    out = DrawView()
    if lib().cvxv_view_from_camera(C.addressof(data), int(width), int(height), float(max_t), C.addressof(out)) != 0:
        raise ValueError(f"view_from_camera: width and height are 1 .. {DRAW_MAX_SIZE} and the camera's matrix has an inverse")
    return out


def draw_view(origin, dir0, dir_x, dir_y, width: int, height: int, max_t: float = float("inf")) -> "DrawView":
    """A DrawView from a host's own camera: pixel (x, y)'s ray leaves `origin` along dir0 + x * dir_x + y * dir_y (row 0 = the bottom row)."""
    out = DrawView()
    out.origin[:], out.dir0[:], out.dirX[:], out.dirY[:] = [float(v) for v in origin], [float(v) for v in dir0], [float(v) for v in dir_x], [float(v) for v in dir_y]
    out.maxT, out.width, out.height = float(max_t), int(width), int(height)
    return out


def view_rays(view, x0: int = 0, y0: int = 0, w=None, h=None) -> np.ndarray:
    """cvxv_view_rays: the rays models_draw gives the pixels [x0, x0 + w) x [y0, y0 + h) of the view (default: all of it) as a PICK_RAY_DTYPE array
    of shape (h, w), byte for byte the rule's own; pick and model_pick take them.  A pure host call."""
    w = view.width - int(x0) if w is None else int(w)
    h = view.height - int(y0) if h is None else int(h)
    rays = np.zeros((max(h, 0), max(w, 0)), dtype=PICK_RAY_DTYPE)
    if lib().cvxv_view_rays(C.addressof(view), int(x0), int(y0), w, h, rays.ctypes.data if rays.size else None) != 0:
        raise ValueError("view_rays: the window lies inside the view and is not empty")
    return rays


def sweep_offset(motion, j: int):
    """cvxs_sweep_offset: (o_j as three ints, the axis of step j or -1 for j = 0) on the lattice path of `motion` (three integers of at most
    SWEEP_MAX_MOTION in magnitude): the k-th step of axis a has the parameter (2 k - 1) / (2 |v_a|), steps go in ascending parameter, ties to the
    lower axis.  A pure host call."""
    v = np.ascontiguousarray(motion, dtype=np.int64)
    if v.shape != (3,) or np.abs(v).max() > SWEEP_MAX_MOTION:
        raise ValueError(f"sweep_offset: motion is three integers of at most {SWEEP_MAX_MOTION} in magnitude")
    v, out, axis = v.astype(np.int32), np.zeros(3, dtype=np.int32), C.c_int(0)
    if not -(1 << 31) <= int(j) < 1 << 31 or lib().cvxs_sweep_offset(v.ctypes.data, int(j), out.ctypes.data, C.byref(axis)) != 0:
        raise ValueError(f"sweep_offset: j = {j} outside 0 .. {int(np.abs(v.astype(np.int64)).sum())}")
    return [int(c) for c in out], axis.value


def instance_moved(instance, offset) -> "ModelInstance":
    """cvxs_instance_moved: the instance whose body is `instance`'s shifted by the integer `offset`, voxel for voxel (the box shifted, toModel.t
    less toModel.m times the offset).  A pure host call."""
    o = np.ascontiguousarray(offset, dtype=np.int64)
    if not isinstance(instance, ModelInstance) or o.shape != (3,) or np.abs(o).max() >= 1 << 31:
        raise ValueError("instance_moved: a gpu.ModelInstance and three int32 offsets")
    o, out = o.astype(np.int32), ModelInstance()
    if lib().cvxs_instance_moved(C.addressof(instance), o.ctypes.data, C.addressof(out)) != 0:
        raise ValueError("instance_moved: the moved instance leaves the limits (a box coordinate beyond 2^30 or t beyond 2^46)")
    return out


class RaybufferLayout(C.Structure):
    _fields_ = [("width", C.c_int32), ("rayCapacity", C.c_int32), ("tileRays", C.c_int32),
                ("tileCapacity", C.c_int32), ("tileBytes", C.c_int64)]


_lib = None


def lib_path() -> str:
    # CVX_GPU_LIB selects another build of the same ABI (e.g. the diagnostic libcpuvox_gpu_prof.so); never a CPU path
    return os.environ.get("CVX_GPU_LIB") or os.path.join(_HERE, "libcpuvox_gpu.so")


def _load_torch_hip_runtime_first() -> None:
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64 under unversioned file names; its
    libraries ask for them by those names, so a copy of /opt/rocm's runtime that this library pulled in earlier (SONAME
    libamdhip64.so.7) is not recognised as the same thing, a second runtime is loaded and finds no GPU ("No HIP GPUs are
    available").  The other order works: the loader matches this library's libamdhip64.so.7 against the SONAME of torch's copy.
    Hosts that use both (bench.py, cpuvox_amd.dist, the tests that hand torch tensors to the C ABI) therefore need torch loaded
    first; without torch installed nothing happens.  CVX_NO_TORCH_PRELOAD=1 skips this (a host that never touches torch)."""
    import sys

    if "torch" in sys.modules or os.environ.get("CVX_NO_TORCH_PRELOAD"):
        return
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def lib() -> C.CDLL:
    """Load libcpuvox_gpu.so (built in-tree by cpuvox_amd/csrc/Makefile); fails loudly when missing."""
    global _lib
    if _lib is None:
        _lib = _bind(lib_path())
    return _lib


def use_library(path: str | None) -> None:
    """Diagnostics / tests: make another build of the same ABI (an experiment or profiling build) the library that contexts
    created FROM NOW ON talk to; None returns to the default.  Contexts of the previous library must be closed first."""
    global _lib
    _lib = _bind(path) if path else None


def _bind(path: str) -> C.CDLL:
    if not os.path.exists(path):
        raise RuntimeError(f"{path} missing: the HIP extension is required (build with `make -C cpuvox_amd/csrc`); there is no CPU fallback")
    _load_torch_hip_runtime_first()
    L = C.CDLL(path)
    L.cvx_version.restype = C.c_char_p
    L.cvx_last_error.restype = C.c_char_p
    L.cvx_last_error.argtypes = [C.c_void_p]
    L.cvx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.cvx_destroy.argtypes = [C.c_void_p]
    L.cvx_destroy.restype = None
    L.cvx_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.cvx_world_upload.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]
    L.cvx_set_resolution.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.cvx_set_buffer_count.argtypes = [C.c_void_p, C.c_int]
    L.cvx_draw_segments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.cvx_draw_segments_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.cvx_draw_segments_placed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int]
    L.cvx_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.cvx_set_latency_kernel.argtypes = [C.c_void_p, C.c_int]
    L.cvx_set_world_repeat.argtypes = [C.c_void_p, C.c_int]
    L.cvx_synchronize.argtypes = [C.c_void_p]
    L.cvx_clear_raybuffer.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32]
    L.cvx_read_raybuffer.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.cvx_blit_segments.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.cvx_blit_segments_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    L.cvx_raybuffer_device_ptr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.cvx_screen_device_ptr.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.cvx_last_draw_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.cvx_draw_time_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int]
    L.cvx_enable_counters.argtypes = [C.c_void_p, C.c_int]
    L.cvx_get_counters.argtypes = [C.c_void_p, C.POINTER(Counters)]
    L.cvx_get_raybuffer_layout.argtypes = [C.c_void_p, C.c_int, C.POINTER(RaybufferLayout)]
    L.cvx_bind_raybuffers.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    L.cvx_copy_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
    if hasattr(L, "cvx_selftest_math"):  # a diagnostics build (include/cpuvox_gpu_diag.h)
        L.cvx_debug_section_cycles.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        L.cvx_debug_section_histogram.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        L.cvx_debug_occupancy.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int)]
        L.cvx_debug_last_launch.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.cvx_debug_settle.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int64)]
        L.cvx_debug_cavities.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int64)]
        L.cvx_selftest_math.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cvx_selftest_scan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
        L.cvx_selftest_lone.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "cvxd_clip_census"):  # the counting / profiling / experiment builds; a name of its own family (cvxd_), so no row of DIAG_EXPORTS
        L.cvxd_clip_census.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
    L.cvx_world_downsample.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)]
    L.cvx_world_build_lods.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    L.cvx_free.argtypes = [C.c_void_p]
    L.cvx_free.restype = None
    L.cvx_world_set_columns.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int]
    L.cvx_world_edit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.cvx_world_edit_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.cvx_world_brush.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.cvx_world_pick.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.cvx_world_pick_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.cvx_world_read_region.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                        C.POINTER(C.c_int32)]
    L.cvx_world_read_level.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    L.cvx_world_compact.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_float)]
    L.cvx_world_stamp_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(C.c_float)]
    L.cvx_world_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.cvx_world_pieces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float)]
    L.cvx_world_settle.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                   C.POINTER(C.c_float)]
    L.cvx_world_cavities.argtypes = [C.c_void_p, C.POINTER(CavityParams), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float)]
    L.cvx_world_light.argtypes = [C.c_void_p, C.POINTER(LightParams), C.c_int, C.POINTER(C.c_float)]
    L.cvx_world_light_lamps.argtypes = [C.c_void_p, C.POINTER(LightParams), C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.cvx_world_move.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.cvx_world_move_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.cvx_world_nav_build.argtypes = [C.c_void_p, C.POINTER(NavParams), C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_float)]
    L.cvx_nav_field_goals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float)]
    L.cvx_nav_query.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.cvx_nav_query_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.cvx_nav_field_destroy.argtypes = [C.c_void_p]
    L.cvx_nav_field_destroy.restype = None
    L.cvx_world_surface.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_float)]
    L.cvx_world_surface_device.argtypes = L.cvx_world_surface.argtypes
    L.cvx_surface_triangles.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.cvx_world_read_voxels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    L.cvx_world_read_voxels_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.cvx_world_write_voxels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.cvx_world_write_voxels_device.argtypes = L.cvx_world_write_voxels.argtypes
    L.cvx_world_distance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float)]
    L.cvx_world_distance_device.argtypes = L.cvx_world_distance.argtypes
    L.cvx_world_read_heights.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    L.cvx_world_read_heights_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.cvx_world_write_heights.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(C.c_float)]
    L.cvx_world_write_heights_device.argtypes = L.cvx_world_write_heights.argtypes
    L.cvx_world_place_models.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.cvx_world_place_models_device.argtypes = L.cvx_world_place_models.argtypes
    L.cvx_world_read_model.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    L.cvx_world_read_model_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.cvx_model_instance_from_matrix.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.cvx_world_spread.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    L.cvx_world_spread_device.argtypes = L.cvx_world_spread.argtypes
    L.cvx_world_surface_rects.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_float)]
    L.cvx_world_surface_rects_device.argtypes = L.cvx_world_surface_rects.argtypes
    L.cvx_surface_rect_triangles.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.cvx_world_snapshot.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_float)]
    L.cvx_snapshot_info_get.argtypes = [C.c_void_p, C.POINTER(SnapshotInfo)]
    L.cvx_world_snapshot_restore.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    L.cvx_world_snapshot_diff.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_float)]
    L.cvx_world_snapshot_diff_device.argtypes = L.cvx_world_snapshot_diff.argtypes
    L.cvx_snapshot_destroy.argtypes = [C.c_void_p]
    L.cvx_snapshot_destroy.restype = None
    L.cvx_world_lift_pieces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                        C.POINTER(LiftSummary), C.POINTER(C.c_float)]
    L.cvx_world_lift_pieces_device.argtypes = L.cvx_world_lift_pieces.argtypes
    L.cvx_lifted_piece_mass.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.cvxc_world_contacts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(ContactsSummary),
                                      C.POINTER(C.c_float)]
    L.cvxc_world_contacts_device.argtypes = L.cvxc_world_contacts.argtypes
    L.cvxc_contact_response.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    L.cvxp_model_contacts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                      C.POINTER(PairsSummary), C.POINTER(C.c_float)]
    L.cvxp_model_contacts_device.argtypes = L.cvxp_model_contacts.argtypes
    L.cvxp_box_pairs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.cvxp_pair_response.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    L.cvxq_model_pick.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float)]
    L.cvxq_model_pick_device.argtypes = L.cvxq_model_pick.argtypes
    L.cvxv_view_from_camera.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]
    L.cvxv_view_rays.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.cvxv_models_draw.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(DrawSummary), C.POINTER(C.c_float)]
    L.cvxv_models_draw_device.argtypes = L.cvxv_models_draw.argtypes
    L.cvxs_world_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                   C.POINTER(SweepsSummary), C.POINTER(C.c_float)]
    L.cvxs_world_sweep_device.argtypes = L.cvxs_world_sweep.argtypes
    L.cvxs_sweep_offset.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    L.cvxs_instance_moved.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.cvxm_pair_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                  C.POINTER(PairSweepsSummary), C.POINTER(C.c_float)]
    L.cvxm_pair_sweep_device.argtypes = L.cvxm_pair_sweep.argtypes
    L.cvxd_models_brush.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(ModelBrushSummary),
                                    C.POINTER(C.c_float)]
    L.cvxd_models_brush_device.argtypes = L.cvxd_models_brush.argtypes
    L.cvxd_model_mass.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.cvx_shard_plan_create.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.cvx_shard_plan_destroy.argtypes = [C.c_void_p]
    L.cvx_shard_plan_destroy.restype = None
    L.cvx_shard_plan_tile_count.argtypes = [C.c_void_p]
    L.cvx_shard_plan_tile_count.restype = C.c_int64
    L.cvx_shard_plan_sections.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.cvx_shard_plan_tile_out.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.cvx_shard_plan_transfer.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.cvx_comm_unique_id.argtypes = [C.c_void_p]
    L.cvx_comm_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.cvx_comm_create_timeout.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_void_p)]
    L.cvx_comm_destroy.argtypes = [C.c_void_p]
    L.cvx_exchange.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.cvx_image_plan_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.cvx_image_plan_destroy.argtypes = [C.c_void_p]
    L.cvx_image_plan_destroy.restype = None
    L.cvx_image_plan_tile_count.argtypes = [C.c_void_p]
    L.cvx_image_plan_tile_count.restype = C.c_int64
    L.cvx_image_plan_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    L.cvx_image_plan_transfer.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.cvx_image_plan_tile_out.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.cvx_image_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.cvx_image_exchange.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.cvx_image_unpack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


class CvxError(RuntimeError):
    pass


def model_instance(forward, size, model: int = 0, op: int = COPY_REPLACE) -> ModelInstance:
    """cvx_model_instance_from_matrix: the instance that places a model of `size` (sx, sy, sz) under `forward`, the 3 x 4 matrix that takes model
    coordinates (voxel s is the cube [s, s + 1)) to world voxel coordinates: its toModel is the rounded inverse, its box the mapped model's
    bounds widened by a voxel.  For a read_model's to_world pass the INVERSE matrix and take the result's toModel."""
    f = np.ascontiguousarray(forward, dtype=np.float64)
    n = np.ascontiguousarray(size, dtype=np.int32)
    if f.shape != (3, 4) or n.shape != (3,):
        raise ValueError("model_instance: forward is a 3 x 4 matrix, size three integers")
    out = ModelInstance()
    if lib().cvx_model_instance_from_matrix(f.ctypes.data, n.ctypes.data, int(model), int(op), C.addressof(out)) != 0:
        raise CvxError("cvx_model_instance_from_matrix: a non-finite or singular matrix, or a map or box beyond the limits")
    return out


class Context:
    """What RenderManager owns on the GPU side (RenderManager.cs:12-56): the
    uploaded world LODs and the raybuffer pairs."""

    def __init__(self, device: int = 0, buffer_count: int = 2):
        self._h = C.c_void_p()
        rc = lib().cvx_create(device, C.byref(self._h))
        if rc != 0:
            raise CvxError(f"cvx_create({device}) failed ({rc}): {lib().cvx_last_error(None).decode()}")
        self.width = self.height = 0
        self.dims = None  # (dimX, dimY, dimZ) of the uploaded world
        if buffer_count != 2:
            self._check(lib().cvx_set_buffer_count(self._h, buffer_count))
        self.buffer_count = buffer_count
        self._nav_fields = []  # the NavFields still open: closed with the context, which they must not outlive
        self._snapshots = []   # ... and the Snapshots, under the same rule

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise CvxError(f"cpuvox_gpu error {rc}: {lib().cvx_last_error(self._h).decode()}")

    def close(self) -> None:
        if self._h:
            for field in list(getattr(self, "_nav_fields", ())):
                field.close()
            for snapshot in list(getattr(self, "_snapshots", ())):
                snapshot.close()
            lib().cvx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- setup ------------------------------------------------------------
    def set_stream(self, hip_stream: int | None) -> None:
        self._check(lib().cvx_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    def upload_world(self, world_set: WorldSet) -> None:
        """`fixed (World* worldPtr = worldLODs)` (RenderManager.cs:155): all LOD_LEVELS levels."""
        for lod in range(world_set.lod_count):
            i = world_set.info(lod)
            self._check(lib().cvx_world_upload(self._h, lod, i.storage, i.byteLength, i.dimX, i.dimY, i.dimZ, i.columnCount))
            self.dims = (i.dimX, i.dimY, i.dimZ)

    def downsample(self, world_set: WorldSet, lod: int, extra_lods: int):
        """World.DownSample(extraLods) (World.cs:45) of level `lod` on the device.  Returns (blob bytes in the reference's
        storage layout, ColumnCount of the new level, voxel count, device milliseconds)."""
        i = world_set.info(lod)
        out, nbytes, columns, voxels, ms = C.c_void_p(), C.c_int64(), C.c_int32(), C.c_int64(), C.c_float()
        self._check(lib().cvx_world_downsample(self._h, i.storage, i.byteLength, i.dimX, i.dimY, i.dimZ, i.lod, i.columnCount, extra_lods,
                                               C.byref(out), C.byref(nbytes), C.byref(columns), C.byref(voxels), C.byref(ms)))
        try:
            blob = C.string_at(out.value, nbytes.value)
        finally:
            lib().cvx_free(out)
        return blob, columns.value, voxels.value, ms.value

    def build_lods(self, world_set: WorldSet, levels: int = LOD_LEVELS) -> WorldSet:
        """UnityManager.cs:328-331 (`worldLODs[i] = worldLODs[0].DownSample(i)`) with the downsampling on the device:
        a new world set with LOD 0 taken from `world_set` and LOD 1..levels-1 built by cvx_world_downsample."""
        i = world_set.info(0)
        n = levels - 1
        outs, sizes, columns, ms = (C.c_void_p * n)(), (C.c_int64 * n)(), (C.c_int32 * n)(), C.c_float()
        self._check(lib().cvx_world_build_lods(self._h, i.storage, i.byteLength, i.dimX, i.dimY, i.dimZ, i.columnCount, n, outs, sizes, columns, C.byref(ms)))
        try:
            blobs = [world_set.storage(0)] + [C.string_at(outs[k], sizes[k]) for k in range(n)]
        finally:
            for k in range(n):
                lib().cvx_free(outs[k])
        self.last_build_lods_ms = ms.value
        return WorldSet.from_blobs(world_set.dims, blobs)

    # -- editing the uploaded world (World.SetVoxelColumn, World.cs:151) -------
    def set_columns(self, lod: int, x0: int, z0: int, size_x: int, size_z: int, blob, column_count: int) -> None:
        """Replaces a size_x x size_z rectangle of level `lod` (its own columns) with the columns of a sub-world blob
        (WorldSet.extract_region).  Ordered on the context's stream: earlier draws see the old world, later ones the new."""
        buf = np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else np.ascontiguousarray(blob, dtype=np.uint8)
        self._check(lib().cvx_world_set_columns(self._h, lod, x0, z0, size_x, size_z, buf.ctypes.data, buf.size, column_count))

    def edit(self, x0: int, z0: int, size_x: int, size_z: int, blob, column_count: int, level_count: int = LOD_LEVELS - 1) -> float:
        """Replaces a LOD-0 rectangle and rebuilds LOD 1..level_count over it on the device (x0, z0, size_x, size_z multiples of
        2^level_count).  Returns the device milliseconds of the edit."""
        buf = np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else np.ascontiguousarray(blob, dtype=np.uint8)
        ms = C.c_float()
        self._check(lib().cvx_world_edit(self._h, x0, z0, size_x, size_z, buf.ctypes.data, buf.size, column_count, level_count, C.byref(ms)))
        return ms.value

    def edit_stats(self):
        """(bytes of the arena in use, bytes edits left behind, bytes of headroom left in the edit tails)."""
        used, abandoned, spare = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(lib().cvx_world_edit_stats(self._h, C.byref(used), C.byref(abandoned), C.byref(spare)))
        return used.value, abandoned.value, spare.value

    # -- reading the uploaded world back, compacting its arena ----------------
    def _blob(self, call, *args):
        out, nbytes, columns = C.c_void_p(), C.c_int64(), C.c_int32()
        self._check(call(self._h, *args, C.byref(out), C.byref(nbytes), C.byref(columns)))
        try:
            return C.string_at(out.value, nbytes.value), columns.value
        finally:
            lib().cvx_free(out)

    def read_region(self, lod: int, x0: int, z0: int, size_x: int, size_z: int):
        """A rectangle of level `lod` (its own columns) as it is on the device now, as a sub-world blob in the builder's encoding: (blob
        bytes, column count), the shape of WorldSet.extract_region and what set_columns / edit take."""
        return self._blob(lib().cvx_world_read_region, lod, x0, z0, size_x, size_z)

    def read_level(self, lod: int):
        """The whole level `lod` as it is on the device now: (blob bytes, World.ColumnCount), the layout cvx_world_upload takes."""
        return self._blob(lib().cvx_world_read_level, lod)

    def download(self, level_count: int = LOD_LEVELS) -> WorldSet:
        """The uploaded world with every edit and brush, as a host world set (WorldSet.from_blobs) of its first level_count levels: e.g. to save it."""
        if self.dims is None:
            raise CvxError("no world has been uploaded to this context")
        return WorldSet.from_blobs(self.dims, [self.read_level(lod)[0] for lod in range(level_count)])

    def compact(self):
        """Lays the edited levels out again without the space edits left behind (on the device).  Returns (bytes reclaimed, device
        milliseconds)."""
        reclaimed, ms = C.c_int64(), C.c_float()
        self._check(lib().cvx_world_compact(self._h, C.byref(reclaimed), C.byref(ms)))
        return reclaimed.value, ms.value

    # -- voxel brushes and ray picking (cvx_world_brush, cvx_world_pick) ------
    def brush(self, strokes, level_count: int = LOD_LEVELS - 1) -> float:
        """Applies the strokes (a list of dicts {op, shape, a, b or radius, argb} or a STROKE_DTYPE array) in order to LOD 0 and rebuilds
        LOD 1..level_count over their footprint on the device.  Returns the device milliseconds.
        Shapes (strokes_array): SHAPE_BOX [a, b), SHAPE_SPHERE (centre a, radius), SHAPE_CAPSULE (the voxels within radius 0 .. 8191 of the segment
        from voxel a to voxel b, at most 8191 apart per axis, |a| <= 2^30) and SHAPE_ELLIPSOID (centre a, radii b = (rx, ry, rz), each 1 .. 1024)."""
        arr = strokes_array(strokes)
        ms = C.c_float()
        self._check(lib().cvx_world_brush(self._h, arr.ctypes.data if arr.size else None, arr.size, level_count, C.byref(ms)))
        return ms.value

    def stamp_mesh(self, mesh, op: int = BRUSH_FILL, level_count: int = LOD_LEVELS - 1) -> float:
        """Voxelises `mesh` (a cpuvox_amd.host.Mesh, positions in LOD-0 voxels: Mesh.rescale) on the device with the host voxeliser's rule and
        merges it into LOD 0 with op (BRUSH_FILL / CARVE / PAINT), then rebuilds LOD 1..level_count over its footprint.  Returns the device
        milliseconds (0 when the mesh stamps no voxel)."""
        v, idx = mesh.vertices, mesh.indices
        textures = (_TextureStruct * max(1, mesh.material_count))()
        for k in range(mesh.material_count):
            t = mesh.texture_struct(k)
            textures[k].width, textures[k].height, textures[k].rgba = t.width, t.height, t.rgba
        ms = C.c_float()
        self._check(lib().cvx_world_stamp_mesh(self._h, v.ctypes.data if v.size else None, v.size, idx.ctypes.data if idx.size else None, idx.size,
                                               C.cast(textures, C.c_void_p), mesh.material_count, op, level_count, C.byref(ms)))
        return ms.value

    def copy(self, placements, level_count: int = LOD_LEVELS - 1) -> float:
        """Copies, moves, turns or mirrors boxes of LOD-0 voxels inside the world (a list of dicts {srcMin, srcMax, dst, transform, op, move}
        or a COPY_PLACEMENT_DTYPE array; every source voxel is read from the world as it was before the call), then rebuilds
        LOD 1..level_count over the footprint.  Returns the device milliseconds (0 when nothing changes)."""
        arr = copy_placements_array(placements)
        ms = C.c_float()
        self._check(lib().cvx_world_copy(self._h, arr.ctypes.data if arr.size else None, arr.size, level_count, C.byref(ms)))
        return ms.value

    def world_pieces(self, box_min, box_max, anchors: int, op: int = PIECES_REPORT, level_count: int = LOD_LEVELS - 1, capacity: int = 1024):
        """The connected pieces (face contact) of the solid LOD-0 voxels inside [box_min, box_max) that none of the `anchors` bits (ANCHOR_GROUND /
        ANCHOR_OUTSIDE / ANCHOR_LARGEST) holds: (the first `capacity` floating pieces as a PIECE_DTYPE array in seed order, the four totals
        as a dict, device milliseconds).  op = PIECES_REMOVE turns all of them into air and rebuilds LOD 1..level_count over their footprint."""
        lo, hi = np.ascontiguousarray(box_min, dtype=np.int32), np.ascontiguousarray(box_max, dtype=np.int32)
        if lo.shape != (3,) or hi.shape != (3,):
            raise ValueError("world_pieces: box_min and box_max are three integers each")
        out = np.zeros(max(int(capacity), 0), dtype=PIECE_DTYPE)
        summary = np.zeros(1, dtype=PIECES_SUMMARY_DTYPE)
        ms = C.c_float()
        self._check(lib().cvx_world_pieces(self._h, lo.ctypes.data, hi.ctypes.data, anchors, op, level_count, out.ctypes.data if out.size else None,
                                           int(capacity), summary.ctypes.data, C.byref(ms)))
        totals = {name: int(summary[0][name]) for name in PIECES_SUMMARY_DTYPE.names}
        return out[:min(out.size, totals["floatingPieces"])].copy(), totals, ms.value

    def world_settle(self, box_min, box_max, anchors: int, max_drop: int = SETTLE_UNLIMITED, level_count: int = LOD_LEVELS - 1, capacity: int = 8192):
        """The floating pieces of world_pieces(box_min, box_max, anchors) fall straight down until they rest on something static or on each other,
        at most `max_drop` voxels (SETTLE_UNLIMITED: all the way), and LOD 1..level_count are rebuilt over the footprint of those that moved:
        (the first `capacity` floating pieces BEFORE the fall as a PIECE_DTYPE array in seed order, how far each fell as an int32 array, the totals
        of cvx_settle_summary as a dict, device milliseconds).  A piece that fell only part of the way is still floating for the next call."""
        lo, hi = np.ascontiguousarray(box_min, dtype=np.int32), np.ascontiguousarray(box_max, dtype=np.int32)
        if lo.shape != (3,) or hi.shape != (3,):
            raise ValueError("world_settle: box_min and box_max are three integers each")
        out = np.zeros(max(int(capacity), 0), dtype=PIECE_DTYPE)
        drops = np.zeros(max(int(capacity), 0), dtype=np.int32)
        summary = np.zeros(1, dtype=SETTLE_SUMMARY_DTYPE)
        ms = C.c_float()
        self._check(lib().cvx_world_settle(self._h, lo.ctypes.data, hi.ctypes.data, anchors, max_drop, level_count, out.ctypes.data if out.size else None,
                                           drops.ctypes.data if drops.size else None, int(capacity), summary.ctypes.data, C.byref(ms)))
        totals = {name: int(summary[0][name]) for name in SETTLE_SUMMARY_DTYPE.names if name != "pad_"}
        listed = min(out.size, totals["floatingPieces"])
        return out[:listed].copy(), drops[:listed].copy(), totals, ms.value

    def debug_settle(self, one_sweep_per_launch: int = -1) -> dict:
        """Diagnostics build only (include/cpuvox_gpu_diag.h): the last world_settle's device ms split (analysis, gap + relax, edit), its solid runs,
        relax sweeps and launches; one_sweep_per_launch 1 / 0 switches the comparison variant of the relax loop on / off for later calls."""
        ms, counts = (C.c_float * 3)(), (C.c_int64 * 4)()
        self._check(self._diag("cvx_debug_settle")(self._h, one_sweep_per_launch, ms, counts))
        return {"analysis_ms": ms[0], "relax_ms": ms[1], "edit_ms": ms[2], "nodes": counts[0], "sweeps": counts[1], "launches": counts[2], "single_workgroup": bool(counts[3])}

    def world_cavities(self, box_min, box_max, op: int = CAVITIES_REPORT, open_faces: int = CAVITY_OPEN_DEFAULT, max_voxels: int = 0, argb: int = 0,
                       level_count: int = LOD_LEVELS - 1, capacity: int = 1024):
        """The enclosed cavities of the LOD-0 air inside [box_min, box_max): the connected air regions (face contact) that reach no face of the
        clipped box whose bit is set in `open_faces` (bits 0..5 = -X,+X,-Y,+Y,-Z,+Z) with air across it: (the first `capacity` selected cavities
        -- the enclosed ones of at most `max_voxels` voxels, 0: all -- as a PIECE_DTYPE array in seed order, the six totals as a dict, device
        milliseconds).  op = CAVITIES_FILL makes all of them solid with `argb` and rebuilds LOD 1..level_count over their footprint."""
        if len(box_min) != 3 or len(box_max) != 3:
            raise ValueError("world_cavities: box_min and box_max are three integers each")
        p = CavityParams((C.c_int32 * 3)(*[int(v) for v in box_min]), (C.c_int32 * 3)(*[int(v) for v in box_max]), open_faces, op, argb & 0xFFFFFFFF, 0,
                         max_voxels)
        out = np.zeros(max(int(capacity), 0), dtype=PIECE_DTYPE)
        summary = np.zeros(1, dtype=CAVITIES_SUMMARY_DTYPE)
        ms = C.c_float()
        self._check(lib().cvx_world_cavities(self._h, C.byref(p), level_count, out.ctypes.data if out.size else None, int(capacity), summary.ctypes.data,
                                             C.byref(ms)))
        totals = {name: int(summary[0][name]) for name in CAVITIES_SUMMARY_DTYPE.names}
        return out[:min(out.size, totals["selectedCavities"])].copy(), totals, ms.value

    def _surface(self, entry, box_min, box_max, solid_outside, flags, quads_ptr, capacity):
        lo, hi = np.ascontiguousarray(box_min, dtype=np.int32), np.ascontiguousarray(box_max, dtype=np.int32)
        if lo.shape != (3,) or hi.shape != (3,):
            raise ValueError("world_surface: box_min and box_max are three integers each")
        summary = np.zeros(1, dtype=SURFACE_SUMMARY_DTYPE)
        ms = C.c_float()
        self._check(entry(self._h, lo.ctypes.data, hi.ctypes.data, solid_outside, flags, quads_ptr, int(capacity), summary.ctypes.data, C.byref(ms)))
        totals = {"quads": int(summary[0]["quads"]), "unitFaces": int(summary[0]["unitFaces"]), "quadsPerFace": [int(v) for v in summary[0]["quadsPerFace"]]}
        return totals, ms.value

    def world_surface(self, box_min, box_max, solid_outside: int = SURFACE_OUTSIDE_DEFAULT, flags: int = 0, capacity=None):
        """The exposed faces of the solid LOD-0 voxels inside [box_min, box_max) as coloured quads (maximal vertical runs of one colour per column
        and side face; SURFACE_IGNORE_COLOUR: of any colour; one quad per exposed -Y / +Y voxel face), in (x, z, face, descending y) order:
        (the first `capacity` quads as a SURFACE_QUAD_DTYPE array, the totals of cvx_surface_summary as a dict, device milliseconds).
        `solid_outside` bits 0..5 = -X,+X,-Y,+Y,-Z,+Z: what lies across a face of the world.  capacity=None asks for the count first and then
        for every quad (the milliseconds are the second call's)."""
        if capacity is None:
            totals, _ = self._surface(lib().cvx_world_surface, box_min, box_max, solid_outside, flags, None, 0)
            capacity = totals["quads"]
        out = np.zeros(max(int(capacity), 0), dtype=SURFACE_QUAD_DTYPE)
        totals, ms = self._surface(lib().cvx_world_surface, box_min, box_max, solid_outside, flags, out.ctypes.data if out.size else None, capacity)
        return (out if out.size <= totals["quads"] else out[:totals["quads"]].copy()), totals, ms

    def world_surface_device(self, box_min, box_max, quads_ptr: int, capacity: int, solid_outside: int = SURFACE_OUTSIDE_DEFAULT, flags: int = 0):
        """world_surface into device memory (the address of `capacity` cvx_surface_quad, e.g. a torch tensor's data_ptr()): the first min(capacity,
        quads) entries are written, the rest is left alone; returns (the totals, device milliseconds) once the summary is on the host."""
        return self._surface(lib().cvx_world_surface_device, box_min, box_max, solid_outside, flags, quads_ptr or None, capacity)

    def _surface_rects(self, entry, box_min, box_max, solid_outside, flags, rects_ptr, capacity):
        lo, hi = np.ascontiguousarray(box_min, dtype=np.int32), np.ascontiguousarray(box_max, dtype=np.int32)
        if lo.shape != (3,) or hi.shape != (3,):
            raise ValueError("world_surface_rects: box_min and box_max are three integers each")
        summary = np.zeros(1, dtype=SURFACE_RECTS_SUMMARY_DTYPE)
        ms = C.c_float()
        self._check(entry(self._h, lo.ctypes.data, hi.ctypes.data, solid_outside, flags, rects_ptr, int(capacity), summary.ctypes.data, C.byref(ms)))
        totals = {"rects": int(summary[0]["rects"]), "strips": int(summary[0]["strips"]), "unitFaces": int(summary[0]["unitFaces"]),
                  "rectsPerFace": [int(v) for v in summary[0]["rectsPerFace"]]}
        return totals, ms.value

    def world_surface_rects(self, box_min, box_max, solid_outside: int = SURFACE_OUTSIDE_DEFAULT, flags: int = 0, capacity=None):
        """world_surface's quads merged into rectangles (side faces along the wall, -Y / +Y faces into rows along x that stack along z; colours
        merge only with SURFACE_IGNORE_COLOUR), in (x, z, face, descending top) order of their lowest voxel: (the first `capacity` rectangles as a
        SURFACE_RECT_DTYPE array, the totals of cvx_surface_rects_summary as a dict, device milliseconds).  capacity=None asks for the count
        first and then for every rectangle (the milliseconds are the second call's)."""
        if capacity is None:
            totals, _ = self._surface_rects(lib().cvx_world_surface_rects, box_min, box_max, solid_outside, flags, None, 0)
            capacity = totals["rects"]
        out = np.zeros(max(int(capacity), 0), dtype=SURFACE_RECT_DTYPE)
        totals, ms = self._surface_rects(lib().cvx_world_surface_rects, box_min, box_max, solid_outside, flags, out.ctypes.data if out.size else None, capacity)
        return (out if out.size <= totals["rects"] else out[:totals["rects"]].copy()), totals, ms

    def world_surface_rects_device(self, box_min, box_max, rects_ptr: int, capacity: int, solid_outside: int = SURFACE_OUTSIDE_DEFAULT, flags: int = 0):
        """world_surface_rects into device memory (the address of `capacity` cvx_surface_rect, e.g. a torch tensor's data_ptr()): the first
        min(capacity, rects) entries are written, the rest is left alone; returns (the totals, device milliseconds) once the summary is on the host."""
        return self._surface_rects(lib().cvx_world_surface_rects_device, box_min, box_max, solid_outside, flags, rects_ptr or None, capacity)

    # -- dense voxel boxes in and out of the world (cvx_world_read_voxels, cvx_world_write_voxels) --
    @staticmethod
    def _box(box_min, box_max):
        lo, hi = np.ascontiguousarray(box_min, dtype=np.int32), np.ascontiguousarray(box_max, dtype=np.int32)
        if lo.shape != (3,) or hi.shape != (3,):
            raise ValueError("box_min and box_max are three integers each")
        return lo, hi

    def read_voxels(self, box_min, box_max, want_argb: bool = True, want_solid: bool = True):
        """The LOD-0 voxels of [box_min, box_max) (it may stick out of the world) as dense arrays of shape (X, Z, Y), y fastest: (argb uint32 --
        the colour word of a solid voxel, 0 for air and outside the world -- or None, solid bool or None)."""
        lo, hi = self._box(box_min, box_max)
        shape = tuple(max(int(hi[a]) - int(lo[a]), 0) for a in (0, 2, 1))
        if 0 < shape[0] * shape[1] * shape[2] < 1 << 31:  # (anything else: the call rejects it before it writes)
            argb = np.zeros(shape, dtype=np.uint32) if want_argb else None
            solid = np.zeros(shape, dtype=np.uint8) if want_solid else None
        else:
            argb = solid = None
        self._check(lib().cvx_world_read_voxels(self._h, lo.ctypes.data, hi.ctypes.data, argb.ctypes.data if argb is not None else None,
                                                solid.ctypes.data if solid is not None else None, None))
        return argb, (solid.view(np.bool_) if solid is not None else None)

    def read_voxels_device(self, box_min, box_max, argb_ptr: int, solid_ptr: int, stream: int | None = None) -> None:
        """read_voxels into device memory (addresses of X * Z * Y uint32 / uint8, e.g. a torch tensor's data_ptr(); either may be 0), enqueued
        on `stream` (None or 0: the context's) without waiting."""
        lo, hi = self._box(box_min, box_max)
        self._check(lib().cvx_world_read_voxels_device(self._h, lo.ctypes.data, hi.ctypes.data, argb_ptr or None, solid_ptr or None, stream or None))

    def write_voxels(self, box_min, argb, solid=None, op: int = COPY_REPLACE, level_count: int = LOD_LEVELS - 1) -> float:
        """Writes a dense box of voxels at box_min into LOD 0 and rebuilds LOD 1..level_count over its footprint.  `argb`: uint32 colour words of
        shape (X, Z, Y) (None for a BRUSH_CARVE with a mask); `solid` (optional, same shape): which voxels are set -- without it the voxels
        with a colour word other than 0.  op: COPY_REPLACE (the box replaces what is there, air included), BRUSH_FILL, BRUSH_CARVE, BRUSH_PAINT
        (the set voxels fill, carve or recolour).  Returns the device milliseconds (0 when the box lies outside the world)."""
        a = np.ascontiguousarray(argb, dtype=np.uint32) if argb is not None else None
        m = np.ascontiguousarray(solid).astype(np.bool_, copy=False).view(np.uint8) if solid is not None else None
        shape = a.shape if a is not None else (m.shape if m is not None else None)
        if shape is None or len(shape) != 3 or (a is not None and m is not None and a.shape != m.shape):
            raise ValueError("write_voxels: argb and solid are arrays of one shape (X, Z, Y)")
        lo = np.ascontiguousarray(box_min, dtype=np.int64)
        hi = lo + np.array([shape[0], shape[2], shape[1]], dtype=np.int64)
        lo, hi = self._box(np.clip(lo, -(1 << 31), (1 << 31) - 1), np.clip(hi, -(1 << 31), (1 << 31) - 1))
        ms = C.c_float()
        self._check(lib().cvx_world_write_voxels(self._h, lo.ctypes.data, hi.ctypes.data, a.ctypes.data if a is not None else None,
                                                 m.ctypes.data if m is not None else None, op, level_count, C.byref(ms)))
        return ms.value

    def write_voxels_device(self, box_min, box_max, argb_ptr: int, solid_ptr: int, op: int = COPY_REPLACE, level_count: int = LOD_LEVELS - 1) -> float:
        """write_voxels from device memory (addresses of X * Z * Y uint32 / uint8; solid_ptr may be 0, argb_ptr only for a BRUSH_CARVE), read
        on the context's stream: the arrays must be complete when the call is made.  Returns the device milliseconds."""
        lo, hi = self._box(box_min, box_max)
        ms = C.c_float()
        self._check(lib().cvx_world_write_voxels_device(self._h, lo.ctypes.data, hi.ctypes.data, argb_ptr or None, solid_ptr or None, op, level_count,
                                                        C.byref(ms)))
        return ms.value

    # -- terrain as height maps (cvx_world_read_heights, cvx_world_write_heights) --
    def read_heights(self, box_min, box_max, want_argb: bool = True, want_bottoms: bool = False):
        """The terrain of the footprint of [box_min, box_max) (it may stick out of the world) inside the window [box_min.y, box_max.y), as arrays
        of shape (X, Z), z fastest: (heights int32 -- 1 + the y of the highest solid voxel in the window, box_min.y when there is none --, argb
        uint32 -- that voxel's colour word, 0 when there is none -- or None, bottoms int32 -- how far down the solid goes from there -- or None)."""
        lo, hi = self._box(box_min, box_max)
        shape = tuple(max(int(hi[a]) - int(lo[a]), 0) for a in (0, 2))
        if 0 < shape[0] * shape[1] < 1 << 31:  # (anything else: the call rejects it before it writes)
            heights = np.zeros(shape, dtype=np.int32)
            argb = np.zeros(shape, dtype=np.uint32) if want_argb else None
            bottoms = np.zeros(shape, dtype=np.int32) if want_bottoms else None
        else:
            heights = argb = bottoms = None
        self._check(lib().cvx_world_read_heights(self._h, lo.ctypes.data, hi.ctypes.data, heights.ctypes.data if heights is not None else None,
                                                 argb.ctypes.data if argb is not None else None, bottoms.ctypes.data if bottoms is not None else None, None))
        return heights, argb, bottoms

    def read_heights_device(self, box_min, box_max, heights_ptr: int, argb_ptr: int = 0, bottoms_ptr: int = 0, stream: int | None = None) -> None:
        """read_heights into device memory (addresses of X * Z int32 / uint32 / int32, e.g. a torch tensor's data_ptr(); any may be 0, not all),
        enqueued on `stream` (None or 0: the context's) without waiting."""
        lo, hi = self._box(box_min, box_max)
        self._check(lib().cvx_world_read_heights_device(self._h, lo.ctypes.data, hi.ctypes.data, heights_ptr or None, argb_ptr or None, bottoms_ptr or None,
                                                        stream or None))

    def write_heights(self, box_min, y_max: int, heights, argb, side_argb=None, thickness: int = 1, flags: int = 0, op: int = COPY_REPLACE,
                      level_count: int = LOD_LEVELS - 1) -> float:
        """Writes terrain into the window [box_min.y, y_max) of the columns at box_min and rebuilds LOD 1..level_count over them.  `heights`:
        int32 of shape (X, Z), clamped into the window; a column's voxels from its crust's bottom up to its height are SET.  thickness 0: solid
        down to the window's bottom; t: a crust of t voxels, thicker where a neighbour is lower (HEIGHTS_WALLED in `flags`: the rim counts as a
        cliff down to the window's bottom).  `argb` (uint32, same shape; None for a BRUSH_CARVE): the top voxel's colour word, `side_argb`
        (optional) that of the voxels below it.  op: COPY_REPLACE (the window becomes this terrain), BRUSH_FILL, BRUSH_CARVE, BRUSH_PAINT.
        Returns the device milliseconds (0 when the box lies outside the world)."""
        h = np.asarray(heights)
        if h.ndim != 2 or h.dtype.kind not in "iu":
            raise ValueError("write_heights: heights is an integer array of shape (X, Z)")
        h = np.ascontiguousarray(h, dtype=np.int32)
        a = np.ascontiguousarray(argb, dtype=np.uint32) if argb is not None else None
        s = np.ascontiguousarray(side_argb, dtype=np.uint32) if side_argb is not None else None
        if any(c is not None and c.shape != h.shape for c in (a, s)):
            raise ValueError("write_heights: heights, argb and side_argb are arrays of one shape (X, Z)")
        lo = np.ascontiguousarray(box_min, dtype=np.int64)
        if lo.shape != (3,):
            raise ValueError("box_min is three integers")
        hi = np.array([lo[0] + h.shape[0], int(y_max), lo[2] + h.shape[1]], dtype=np.int64)
        lo, hi = self._box(np.clip(lo, -(1 << 31), (1 << 31) - 1), np.clip(hi, -(1 << 31), (1 << 31) - 1))
        ms = C.c_float()
        self._check(lib().cvx_world_write_heights(self._h, lo.ctypes.data, hi.ctypes.data, h.ctypes.data, a.ctypes.data if a is not None else None,
                                                  s.ctypes.data if s is not None else None, int(thickness), int(flags), int(op), int(level_count), C.byref(ms)))
        return ms.value

    def write_heights_device(self, box_min, box_max, heights_ptr: int, argb_ptr: int, side_argb_ptr: int = 0, thickness: int = 1, flags: int = 0,
                             op: int = COPY_REPLACE, level_count: int = LOD_LEVELS - 1) -> float:
        """write_heights from device memory (addresses of X * Z int32 / uint32 / uint32; side_argb_ptr may be 0, argb_ptr only for a
        BRUSH_CARVE), read on the context's stream: the arrays must be complete when the call is made.  Returns the device milliseconds."""
        lo, hi = self._box(box_min, box_max)
        ms = C.c_float()
        self._check(lib().cvx_world_write_heights_device(self._h, lo.ctypes.data, hi.ctypes.data, heights_ptr or None, argb_ptr or None, side_argb_ptr or None,
                                                         int(thickness), int(flags), int(op), int(level_count), C.byref(ms)))
        return ms.value

    # -- voxel models at any orientation and scale (cvx_world_place_models, cvx_world_read_model) --
    @staticmethod
    def _instances(instances):
        return _instance_array(instances)

    @staticmethod
    def _models(models, who):
        """The cvx_model descriptors of a list of (argb, solid) host arrays, and the arrays they point to."""
        keep, descriptors = [], (Model * max(len(models), 1))()
        for k, entry in enumerate(models):
            if not isinstance(entry, (tuple, list)) or len(entry) != 2:
                raise ValueError(f"{who}: a model is a pair (argb, solid)")
            argb, solid = entry
            if argb is not None and np.asarray(argb).dtype.kind not in "iu":
                raise ValueError(f"{who}: argb is an integer array of shape (X, Z, Y)")
            a = np.ascontiguousarray(argb, dtype=np.uint32) if argb is not None else None
            m = np.ascontiguousarray(solid).astype(np.bool_, copy=False).view(np.uint8) if solid is not None else None
            shape = a.shape if a is not None else (m.shape if m is not None else None)
            if shape is None or len(shape) != 3 or (a is not None and m is not None and a.shape != m.shape):
                raise ValueError(f"{who}: argb and solid are arrays of one shape (X, Z, Y)")
            keep += [a, m]
            descriptors[k].size[:] = [shape[0], shape[2], shape[1]]
            descriptors[k].argb = a.ctypes.data if a is not None else None
            descriptors[k].solid = m.ctypes.data if m is not None else None
        return descriptors, keep

    @staticmethod
    def _device_models(models, who):
        """The cvx_model descriptors of a list of ((sx, sy, sz), argb_ptr, solid_ptr)."""
        descriptors = (Model * max(len(models), 1))()
        for k, entry in enumerate(models):
            if not isinstance(entry, (tuple, list)) or len(entry) != 3 or len(tuple(entry[0])) != 3:
                raise ValueError(f"{who}: a model is ((sx, sy, sz), argb_ptr, solid_ptr)")
            descriptors[k].size[:] = [int(v) for v in entry[0]]
            descriptors[k].argb = entry[1] or None
            descriptors[k].solid = entry[2] or None
        return descriptors

    def place_models(self, models, instances, level_count: int = LOD_LEVELS - 1) -> float:
        """Places instances of voxel models into LOD 0, in order, and rebuilds LOD 1..level_count over their boxes.  `models`: a list of
        (argb, solid) -- uint32 colour words of shape (X, Z, Y) (None for a model only BRUSH_CARVE instances use) and an optional mask of the same
        shape (without it the voxels with a colour word other than 0 are set).  `instances`: gpu.ModelInstance structures (gpu.model_instance
        makes them from a matrix).  Returns the device milliseconds (0 when every box lies outside the world)."""
        descriptors, keep = self._models(models, "place_models")  # noqa: F841  (keep: the arrays the descriptors point to)
        inst = self._instances(instances)
        ms = C.c_float()
        self._check(lib().cvx_world_place_models(self._h, C.addressof(descriptors), len(models), C.addressof(inst), len(inst), int(level_count), C.byref(ms)))
        return ms.value

    def place_models_device(self, models, instances, level_count: int = LOD_LEVELS - 1) -> float:
        """place_models from device memory: `models` is a list of ((sx, sy, sz), argb_ptr, solid_ptr), the addresses of sx * sz * sy uint32 /
        uint8 laid out (X, Z, Y) (e.g. a torch tensor's data_ptr(); either may be 0, not both), read on the context's stream: the arrays must
        be complete when the call is made."""
        descriptors = self._device_models(models, "place_models_device")
        inst = self._instances(instances)
        ms = C.c_float()
        self._check(lib().cvx_world_place_models_device(self._h, C.addressof(descriptors), len(models), C.addressof(inst), len(inst), int(level_count),
                                                        C.byref(ms)))
        return ms.value

    # -- where placed models touch the world (cvxc_world_contacts, include/cpuvox_gpu_contacts.h) --
    def _contacts(self, entry, descriptors, model_count, instances, solid_outside, results_ptr, points_ptr, capacity):
        inst = self._instances(instances)
        summary, ms = ContactsSummary(), C.c_float()
        self._check(entry(self._h, C.addressof(descriptors), model_count, C.addressof(inst), len(inst), int(solid_outside), results_ptr, points_ptr or None,
                          int(capacity), C.byref(summary), C.byref(ms)))
        return {name: int(getattr(summary, name)) for name in CONTACTS_SUMMARY_DTYPE.names}, ms.value

    def world_contacts(self, models, instances, solid_outside: int = SURFACE_OUTSIDE_DEFAULT, capacity=None):
        """Where every instance, placed as place_models would place it, touches the world: (one CONTACT_RESULT_DTYPE element per instance, the first
        `capacity` contact points as a CONTACT_POINT_DTYPE array in (instance, x, z, descending y) order, the totals of cvxc_contacts_summary
        as a dict, device milliseconds).  The overlap of an instance is exactly the voxels a BRUSH_FILL of it would write that are already
        solid; `normal` sums the open faces of those voxels and points out of the world's solid.  `models` and `instances` as place_models'
        (an instance's op is not read); `solid_outside` bits 0..5 = -X,+X,-Y,+Y,-Z,+Z: what lies across a face of the world.  capacity=0 asks
        for the results alone; capacity=None asks for them first and then for every point (the milliseconds are the second call's)."""
        descriptors, keep = self._models(models, "world_contacts")  # noqa: F841  (keep: the arrays the descriptors point to)
        inst = self._instances(instances)
        results = np.zeros(len(inst), dtype=CONTACT_RESULT_DTYPE)
        call = lib().cvxc_world_contacts
        if capacity is None:
            totals, _ = self._contacts(call, descriptors, len(models), inst, solid_outside, results.ctypes.data if len(inst) else None, None, 0)
            capacity = totals["points"]
        points = np.zeros(max(int(capacity), 0), dtype=CONTACT_POINT_DTYPE)
        totals, ms = self._contacts(call, descriptors, len(models), inst, solid_outside, results.ctypes.data if len(inst) else None,
                                    points.ctypes.data if points.size else None, capacity)
        return results, (points if points.size <= totals["points"] else points[:totals["points"]].copy()), totals, ms

    @staticmethod
    def _checked_tensor(who, tensor, item_bytes, at_least):
        """(the device pointer, the items it holds) of a contiguous device tensor of at least `at_least` items of `item_bytes` bytes."""
        nbytes = tensor.numel() * tensor.element_size()
        if not tensor.is_cuda or not tensor.is_contiguous() or nbytes < at_least * item_bytes:
            raise ValueError(f"{who}: a contiguous device tensor of at least {at_least} x {item_bytes} bytes")
        return tensor.data_ptr(), nbytes // item_bytes

    def world_contacts_device(self, models, instances, results_tensor, points_tensor=None, solid_outside: int = SURFACE_OUTSIDE_DEFAULT):
        """world_contacts on device memory: `models` is a list of ((sx, sy, sz), argb_ptr, solid_ptr) as place_models_device's (gpu.lifted_model of
        device pools gives one), `results_tensor` a contiguous device tensor of at least 120 bytes per instance, `points_tensor` (or None: the
        results alone) one whose bytes / 24 are the capacity; entries beyond the points found are left alone.  Returns (the totals as a dict,
        device milliseconds) once the summary is on the host: the tensors are complete then."""
        descriptors = self._device_models(models, "world_contacts_device")
        inst = self._instances(instances)
        results_ptr, _ = self._checked_tensor("world_contacts_device", results_tensor, C.sizeof(ContactResult), len(inst))
        points_ptr, capacity = self._checked_tensor("world_contacts_device", points_tensor, C.sizeof(ContactPoint), 0) if points_tensor is not None else (None, 0)
        return self._contacts(lib().cvxc_world_contacts_device, descriptors, len(models), inst, solid_outside, results_ptr, points_ptr if capacity else None, capacity)

    # -- where placed models touch each other (cvxp_model_contacts, include/cpuvox_gpu_pair_contacts.h) --
    @staticmethod
    def _pairs(pairs, inst, who):
        p = box_pairs(inst) if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32)
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError(f"{who}: pairs is an (n, 2) integer array of indices into instances")
        return p

    def _pair_contacts(self, entry, descriptors, model_count, inst, pairs, results_ptr, points_ptr, capacity):
        summary, ms = PairsSummary(), C.c_float()
        self._check(entry(self._h, C.addressof(descriptors), model_count, C.addressof(inst), len(inst), pairs.ctypes.data if len(pairs) else None, len(pairs),
                          results_ptr, points_ptr or None, int(capacity), C.byref(summary), C.byref(ms)))
        return {name: int(getattr(summary, name)) for name in PAIRS_SUMMARY_DTYPE.names}, ms.value

    def model_contacts(self, models, instances, pairs=None, capacity=None):
        """Where placed instances touch EACH OTHER; no world is read and none need be uploaded: (one PAIR_RESULT_DTYPE element per pair, the first
        `capacity` contact points as a PAIR_POINT_DTYPE array in (pair, x, z, descending y) order, the totals of cvxp_pairs_summary as a dict,
        device milliseconds).  `models` and `instances` as world_contacts'; `pairs` an (n, 2) array of indices into instances, or None: the pairs
        gpu.box_pairs finds.  A pair's overlap is the voxels in both bodies; pushA sums the open faces of body b over them (the way to move a),
        pushB those of body a.  capacity=0 asks for the results alone; capacity=None asks for them first and then for every point (the
        milliseconds are the second call's)."""
        descriptors, keep = self._models(models, "model_contacts")  # noqa: F841  (keep: the arrays the descriptors point to)
        inst = self._instances(instances)
        p = self._pairs(pairs, inst, "model_contacts")
        results = np.zeros(len(p), dtype=PAIR_RESULT_DTYPE)
        call = lib().cvxp_model_contacts
        results_ptr = results.ctypes.data if len(p) else None
        if capacity is None:
            totals, _ = self._pair_contacts(call, descriptors, len(models), inst, p, results_ptr, None, 0)
            capacity = totals["points"]
        points = np.zeros(max(int(capacity), 0), dtype=PAIR_POINT_DTYPE)
        totals, ms = self._pair_contacts(call, descriptors, len(models), inst, p, results_ptr, points.ctypes.data if points.size else None, capacity)
        return results, (points if points.size <= totals["points"] else points[:totals["points"]].copy()), totals, ms

    def model_contacts_device(self, models, instances, pairs, results_tensor, points_tensor=None):
        """model_contacts on device memory: `models` is a list of ((sx, sy, sz), argb_ptr, solid_ptr) as place_models_device's, `pairs` an (n, 2)
        host array (None: gpu.box_pairs), `results_tensor` a contiguous device tensor of at least 144 bytes per pair, `points_tensor` (or None:
        the results alone) one whose bytes / 32 are the capacity; entries beyond the points found are left alone.  Returns (the totals as a
        dict, device milliseconds) once the summary is on the host: the tensors are complete then."""
        descriptors = self._device_models(models, "model_contacts_device")
        inst = self._instances(instances)
        p = self._pairs(pairs, inst, "model_contacts_device")
        results_ptr, _ = self._checked_tensor("model_contacts_device", results_tensor, C.sizeof(PairResult), len(p))
        points_ptr, capacity = self._checked_tensor("model_contacts_device", points_tensor, C.sizeof(PairPoint), 0) if points_tensor is not None else (None, 0)
        return self._pair_contacts(lib().cvxp_model_contacts_device, descriptors, len(models), inst, p, results_ptr, points_ptr if capacity else None, capacity)

    # -- first-hit rays against placed models (cvxq_model_pick, include/cpuvox_gpu_model_pick.h) --
    def model_pick(self, models, instances, origins, directions, max_t):
        """The first voxel of any placed instance along each ray; no world is read and none need be uploaded: (a MODEL_HIT_DTYPE array, one
        element per ray: the world voxel, the face as pick's, the model's colour word, t, the instance and the model's voxel; a miss has
        voxel -1, face -1, argb 0, t = max_t, instance -1 -- device milliseconds).  `models` and `instances` as world_contacts' (an instance's op
        is not read); origins, directions, max_t as pick's.  For the first of world or bodies pass pick's t as max_t."""
        descriptors, keep = self._models(models, "model_pick")  # noqa: F841  (keep: the arrays the descriptors point to)
        inst = self._instances(instances)
        o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        if d.shape[0] != n:
            raise ValueError("model_pick: one direction per origin")
        rays = np.zeros(n, dtype=PICK_RAY_DTYPE)
        rays["origin"], rays["direction"] = o, d
        rays["maxT"] = np.broadcast_to(np.asarray(max_t, dtype=np.float32), (n,))
        hits = np.zeros(n, dtype=MODEL_HIT_DTYPE)
        ms = C.c_float()
        self._check(lib().cvxq_model_pick(self._h, C.addressof(descriptors), len(models), C.addressof(inst), len(inst), rays.ctypes.data if n else None, n,
                                          hits.ctypes.data if n else None, C.byref(ms)))
        return hits, ms.value

    def model_pick_device(self, models, instances, rays_tensor, hits_tensor, ray_count=None):
        """model_pick on device memory: `models` is a list of ((sx, sy, sz), argb_ptr, solid_ptr) as place_models_device's, `rays_tensor` a
        contiguous device tensor of 32 bytes per ray (cvx_pick_ray: the array cvx_world_pick_device reads), `hits_tensor` one of at least 48
        bytes per ray; ray_count: the rays to pick (None: all of rays_tensor).  Returns the device milliseconds once the hits are complete."""
        descriptors = self._device_models(models, "model_pick_device")
        inst = self._instances(instances)
        rays_ptr, n = self._checked_tensor("model_pick_device", rays_tensor, C.sizeof(PickRay), 0 if ray_count is None else int(ray_count))
        n = n if ray_count is None else int(ray_count)
        hits_ptr, _ = self._checked_tensor("model_pick_device", hits_tensor, C.sizeof(ModelHit), n)
        ms = C.c_float()
        self._check(lib().cvxq_model_pick_device(self._h, C.addressof(descriptors), len(models), C.addressof(inst), len(inst), rays_ptr, n, hits_ptr, C.byref(ms)))
        return ms.value

    # -- placed models drawn into the rendered frame (cvxv_models_draw, include/cpuvox_gpu_model_draw.h) --
    def _models_draw(self, entry, descriptors, model_count, instances, view, flags, image_ptr, depth_ptr, ids_ptr):
        inst = self._instances(instances)
        if not isinstance(view, DrawView):
            raise ValueError("models_draw: view is a gpu.DrawView (gpu.view_from_camera or gpu.draw_view makes one)")
        summary, ms = DrawSummary(), C.c_float()
        self._check(entry(self._h, C.addressof(descriptors), model_count, C.addressof(inst), len(inst), C.addressof(view), int(flags), image_ptr or None,
                          depth_ptr or None, ids_ptr or None, C.byref(summary), C.byref(ms)))
        return {name: int(getattr(summary, name)) for name in DRAW_SUMMARY_DTYPE.names if name != "pad_"}, ms.value

    def models_draw(self, models, instances, view, flags: int = 0, image=None, depth=None, ids=None):
        """Draws the nearest placed instance of every pixel of `view` (a gpu.DrawView) into host arrays of shape (height, width), row 0 the bottom
        row: image uint32 (the model's colour word), depth float32 (distance in voxels) and ids int32 (the instance's index).  An array
        that is None is made here (image 0, depth +inf, ids -1); the arrays given are copied, and every pixel no body shows in keeps what it
        held.  flags: DRAW_WORLD -- the uploaded world occludes --, DRAW_DEPTH_TEST -- a pixel's ray ends at the depth it holds.  `models` and
        `instances` as world_contacts' (an instance's op is not read).  Returns (image, depth, ids, the counts of cvxv_draw_summary as a dict,
        device milliseconds)."""
        descriptors, keep = self._models(models, "models_draw")  # noqa: F841  (keep: the arrays the descriptors point to)
        if not isinstance(view, DrawView):
            raise ValueError("models_draw: view is a gpu.DrawView (gpu.view_from_camera or gpu.draw_view makes one)")
        shape = (view.height, view.width)

        def own(array, dtype, fill, name):
            if array is None:
                return np.full(shape, fill, dtype=dtype)
            a = np.array(array, dtype=dtype, order="C")
            if a.shape != shape:
                raise ValueError(f"models_draw: {name} has the shape (height, width) = {shape}")
            return a
        image, depth, ids = own(image, np.uint32, 0, "image"), own(depth, np.float32, np.inf, "depth"), own(ids, np.int32, -1, "ids")
        summary, ms = self._models_draw(lib().cvxv_models_draw, descriptors, len(models), instances, view, flags, image.ctypes.data, depth.ctypes.data, ids.ctypes.data)
        return image, depth, ids, summary, ms

    def models_draw_device(self, models, instances, view, flags, image_tensor, depth_tensor=None, ids_tensor=None):
        """models_draw on device memory: `models` is a list of ((sx, sy, sz), argb_ptr, solid_ptr) as place_models_device's (gpu.lifted_model of
        device pools gives one); image_tensor, depth_tensor and ids_tensor are contiguous device tensors of at least width * height 4-byte
        elements, or None (not all three) -- or plain device addresses, as screen_device_ptr's, which are taken as they are.  Returns (the
        counts of cvxv_draw_summary as a dict, device milliseconds) once the outputs are complete."""
        descriptors = self._device_models(models, "models_draw_device")
        if not isinstance(view, DrawView):
            raise ValueError("models_draw_device: view is a gpu.DrawView (gpu.view_from_camera or gpu.draw_view makes one)")
        pixels = view.width * view.height

        def pointer(tensor):
            if tensor is None or isinstance(tensor, int):
                return tensor
            return self._checked_tensor("models_draw_device", tensor, 4, pixels)[0]
        return self._models_draw(lib().cvxv_models_draw_device, descriptors, len(models), instances, view, flags, pointer(image_tensor), pointer(depth_tensor),
                                 pointer(ids_tensor))

    # -- how far placed models can move before they touch the world (cvxs_world_sweep, include/cpuvox_gpu_sweep.h) --
    def _sweep(self, entry, who, descriptors, model_count, instances, motions, solid_outside, contacts_ptr, points_ptr, capacity):
        inst = self._instances(instances)
        v = np.asarray(motions)
        if v.dtype.kind not in "iu" or v.shape != (len(inst), 3) or (v.size and np.abs(v.astype(np.int64)).max() >= 1 << 31):
            raise ValueError(f"{who}: motions is an integer array of shape (instances, 3)")
        v = np.ascontiguousarray(v, dtype=np.int32)
        sweeps = np.zeros(len(inst), dtype=SWEEP_RESULT_DTYPE)
        summary, ms = SweepsSummary(), C.c_float()
        self._check(entry(self._h, C.addressof(descriptors), model_count, C.addressof(inst), len(inst), v.ctypes.data if len(inst) else None, int(solid_outside),
                          sweeps.ctypes.data if len(inst) else None, contacts_ptr or None, points_ptr or None, int(capacity), C.byref(summary), C.byref(ms)))
        return sweeps, {name: int(getattr(summary, name)) for name in SWEEPS_SUMMARY_DTYPE.names}, ms.value

    def world_sweep(self, models, instances, motions, solid_outside: int = SURFACE_OUTSIDE_DEFAULT, point_capacity=None):
        """How far every instance can move along its integer motion (`motions`: shape (instances, 3), components of at most SWEEP_MAX_MOTION in
        magnitude) before it touches the world: (one SWEEP_RESULT_DTYPE element per instance -- the first touching step `hit` of gpu.sweep_offset's
        path or -1, its axis and sign, the last free offset and the touching one --, the CONTACT_RESULT_DTYPE results of world_contacts for the
        instances moved to `at`, the first `point_capacity` contact points of those, the totals of cvxs_sweeps_summary as a dict, device
        milliseconds).  `models`, `instances` and `solid_outside` as world_contacts'.  point_capacity=0 asks for no points; None asks for the
        results first and then for every point (the milliseconds are the second call's)."""
        descriptors, keep = self._models(models, "world_sweep")  # noqa: F841  (keep: the arrays the descriptors point to)
        inst = self._instances(instances)
        contacts = np.zeros(len(inst), dtype=CONTACT_RESULT_DTYPE)
        call = lib().cvxs_world_sweep
        if point_capacity is None:
            _, totals, _ = self._sweep(call, "world_sweep", descriptors, len(models), inst, motions, solid_outside, contacts.ctypes.data if len(inst) else None, None, 0)
            point_capacity = totals["points"]
        points = np.zeros(max(int(point_capacity), 0), dtype=CONTACT_POINT_DTYPE)
        sweeps, totals, ms = self._sweep(call, "world_sweep", descriptors, len(models), inst, motions, solid_outside, contacts.ctypes.data if len(inst) else None,
                                         points.ctypes.data if points.size else None, point_capacity)
        return sweeps, contacts, (points if points.size <= totals["points"] else points[:totals["points"]].copy()), totals, ms

    def world_sweep_device(self, models, instances, motions, contacts_tensor=None, points_tensor=None, solid_outside: int = SURFACE_OUTSIDE_DEFAULT):
        """world_sweep on device memory: `models` is a list of ((sx, sy, sz), argb_ptr, solid_ptr) as world_contacts_device's, `contacts_tensor` (or
        None: the sweeps alone) a contiguous device tensor of at least 120 bytes per instance, `points_tensor` (or None) one whose bytes / 24 are
        the capacity; entries beyond the points found are left alone.  Returns (the sweeps, a host array, the totals as a dict, device
        milliseconds) once the tensors are complete."""
        descriptors = self._device_models(models, "world_sweep_device")
        inst = self._instances(instances)
        contacts_ptr = self._checked_tensor("world_sweep_device", contacts_tensor, C.sizeof(ContactResult), len(inst))[0] if contacts_tensor is not None else None
        points_ptr, capacity = self._checked_tensor("world_sweep_device", points_tensor, C.sizeof(ContactPoint), 0) if points_tensor is not None else (None, 0)
        return self._sweep(lib().cvxs_world_sweep_device, "world_sweep_device", descriptors, len(models), inst, motions, solid_outside, contacts_ptr,
                           points_ptr if capacity else None, capacity)

    # -- how far placed models can move before they touch each other (cvxm_pair_sweep, include/cpuvox_gpu_pair_sweep.h) --
    def _pair_sweep(self, entry, who, descriptors, model_count, inst, pairs, motions, contacts_ptr):
        p = self._pairs(pairs, inst, who)
        v = np.asarray(motions)
        if v.dtype.kind not in "iu" or v.shape != (len(p), 3) or (v.size and np.abs(v.astype(np.int64)).max() >= 1 << 31):
            raise ValueError(f"{who}: motions is an integer array of shape (pairs, 3)")
        v = np.ascontiguousarray(v, dtype=np.int32)
        sweeps = np.zeros(len(p), dtype=PAIR_SWEEP_RESULT_DTYPE)
        summary, ms = PairSweepsSummary(), C.c_float()
        self._check(entry(self._h, C.addressof(descriptors), model_count, C.addressof(inst), len(inst), p.ctypes.data if len(p) else None, v.ctypes.data if len(p) else None,
                          len(p), sweeps.ctypes.data if len(p) else None, contacts_ptr or None, C.byref(summary), C.byref(ms)))
        return sweeps, {name: int(getattr(summary, name)) for name in PAIR_SWEEPS_SUMMARY_DTYPE.names if name != "pad_"}, ms.value

    def model_sweep(self, models, instances, pairs, motions, want_contacts=True):
        """How far body a of every pair (a, b) can move along its integer motion RELATIVE TO b (`motions`: shape (pairs, 3), components of at most
        SWEEP_MAX_MOTION in magnitude; for two moving bodies pass v_a - v_b) before the two bodies share a voxel; no world is read and none
        need be uploaded: (one PAIR_SWEEP_RESULT_DTYPE element per pair -- `sweep` as world_sweep's: the first touching step `hit` of
        gpu.sweep_offset's path or -1, its axis and sign, the last free offset and the touching one; then the pair --, the PAIR_RESULT_DTYPE
        results of model_contacts with body a of every pair moved to its `at` (None without want_contacts), the totals of
        cvxm_pair_sweeps_summary as a dict, device milliseconds).  `models`, `instances` and `pairs` as model_contacts' (pairs None:
        gpu.box_pairs)."""
        descriptors, keep = self._models(models, "model_sweep")  # noqa: F841  (keep: the arrays the descriptors point to)
        inst = self._instances(instances)
        p = self._pairs(pairs, inst, "model_sweep")
        contacts = np.zeros(len(p), dtype=PAIR_RESULT_DTYPE) if want_contacts else None
        sweeps, totals, ms = self._pair_sweep(lib().cvxm_pair_sweep, "model_sweep", descriptors, len(models), inst, p, motions,
                                              contacts.ctypes.data if want_contacts and len(p) else None)
        return sweeps, contacts, totals, ms

    def model_sweep_device(self, models, instances, pairs, motions, contacts_tensor=None):
        """model_sweep on device memory: `models` is a list of ((sx, sy, sz), argb_ptr, solid_ptr) as model_contacts_device's, `contacts_tensor`
        (or None: the sweeps alone) a contiguous device tensor of at least 144 bytes per pair.  Returns (the sweeps, a host array, the totals
        as a dict, device milliseconds) once the tensor is complete."""
        descriptors = self._device_models(models, "model_sweep_device")
        inst = self._instances(instances)
        p = self._pairs(pairs, inst, "model_sweep_device")
        contacts_ptr = self._checked_tensor("model_sweep_device", contacts_tensor, C.sizeof(PairResult), len(p))[0] if contacts_tensor is not None else None
        return self._pair_sweep(lib().cvxm_pair_sweep_device, "model_sweep_device", descriptors, len(models), inst, p, motions, contacts_ptr)

    # -- brush strokes that carve and paint placed models (cvxd_models_brush, include/cpuvox_gpu_model_brush.h) --
    def _models_brush(self, entry, descriptors, model_count, instances, strokes):
        inst = self._instances(instances)
        k = strokes_array(strokes)
        results = np.zeros(model_count, dtype=MODEL_BRUSH_RESULT_DTYPE)
        hit = np.zeros(len(inst), dtype=MODEL_BRUSH_INSTANCE_RESULT_DTYPE)
        summary, ms = ModelBrushSummary(), C.c_float()
        self._check(entry(self._h, C.addressof(descriptors), model_count, C.addressof(inst), len(inst), k.ctypes.data if len(k) else None, len(k),
                          results.ctypes.data if model_count else None, hit.ctypes.data if len(inst) else None, C.byref(summary), C.byref(ms)))
        return results, hit, {name: int(getattr(summary, name)) for name in MODEL_BRUSH_SUMMARY_DTYPE.names}, ms.value

    def models_brush(self, models, instances, strokes):
        """World-space brush strokes (strokes_array's; BRUSH_CARVE and BRUSH_PAINT only) applied to the MODELS through the instances that place
        them; no world is read and none need be uploaded.  A CARVE unsets the model voxels of the body voxels inside its shape, a PAINT recolours
        them, in stroke order; every instance of a model contributes, so a shared model changes for all of them.  `models` and `instances` as
        world_contacts'; the caller's arrays are left alone: (the models after the call, a list of (argb, solid) copies of shape (X, Z, Y), one
        MODEL_BRUSH_RESULT_DTYPE element per model -- voxels left, carved, painted, the mass sums gpu.model_mass takes, the tight box --, one
        MODEL_BRUSH_INSTANCE_RESULT_DTYPE element per instance -- the body voxels inside a CARVE, and of the others those inside a PAINT --, the
        totals of cvxd_brush_summary as a dict, device milliseconds)."""
        copies = []
        for entry in models:
            if not isinstance(entry, (tuple, list)) or len(entry) != 2:
                raise ValueError("models_brush: a model is a pair (argb, solid)")
            argb, solid = entry
            if argb is not None and np.asarray(argb).dtype.kind not in "iu":
                raise ValueError("models_brush: argb is an integer array of shape (X, Z, Y)")
            copies.append((np.array(argb, dtype=np.uint32, order="C") if argb is not None else None,
                           np.array(np.asarray(solid) != 0, dtype=np.bool_, order="C") if solid is not None else None))
        descriptors, keep = self._models(copies, "models_brush")  # noqa: F841  (keep: views of the copies, which the call writes in place)
        results, hit, totals, ms = self._models_brush(lib().cvxd_models_brush, descriptors, len(models), instances, strokes)
        return copies, results, hit, totals, ms

    def models_brush_device(self, device_models, instances, strokes):
        """models_brush in place on device memory: `device_models` is a list of (argb, solid) torch tensors on the context's device -- uint32 /
        int32 colour words and a uint8 / bool mask of one shape (X, Z, Y), contiguous, either may be None, not both --, written in place; two
        models may not share memory.  Returns (the model results, the instance results, the totals as a dict, device milliseconds) once the
        tensors are complete."""
        entries = []
        for entry in device_models:
            if not isinstance(entry, (tuple, list)) or len(entry) != 2 or (entry[0] is None and entry[1] is None):
                raise ValueError("models_brush_device: a model is a pair (argb, solid) of device tensors, not both None")
            argb, solid = entry
            shape = tuple((argb if argb is not None else solid).shape)
            for tensor, item_bytes in ((argb, 4), (solid, 1)):
                if tensor is not None and (not tensor.is_cuda or not tensor.is_contiguous() or tensor.element_size() != item_bytes or tuple(tensor.shape) != shape
                                           or len(shape) != 3):
                    raise ValueError("models_brush_device: argb (4-byte items) and solid (1-byte items) are contiguous device tensors of one shape (X, Z, Y)")
            entries.append(((shape[0], shape[2], shape[1]), argb.data_ptr() if argb is not None else 0, solid.data_ptr() if solid is not None else 0))
        descriptors = self._device_models(entries, "models_brush_device")
        return self._models_brush(lib().cvxd_models_brush_device, descriptors, len(entries), instances, strokes)

    @staticmethod
    def _model_read(size, to_world):
        n = np.ascontiguousarray(size, dtype=np.int32)
        if n.shape != (3,):
            raise ValueError("size is three integers (sx, sy, sz)")
        if not isinstance(to_world, ModelMap):
            raise ValueError("to_world is a gpu.ModelMap")
        return n

    def read_model(self, size, to_world, want_argb: bool = True, want_solid: bool = True):
        """The world sampled as a model of `size` (sx, sy, sz): element (x, z, y) of the arrays, of shape (sx, sz, sy), is the LOD-0 voxel at
        to_world(x, y, z) (a gpu.ModelMap), air outside the world: (argb uint32 or None, solid bool or None)."""
        n = self._model_read(size, to_world)
        shape = (max(int(n[0]), 0), max(int(n[2]), 0), max(int(n[1]), 0))
        if 0 < shape[0] * shape[1] * shape[2] < 1 << 31:  # (anything else: the call rejects it before it writes)
            argb = np.zeros(shape, dtype=np.uint32) if want_argb else None
            solid = np.zeros(shape, dtype=np.uint8) if want_solid else None
        else:
            argb = solid = None
        self._check(lib().cvx_world_read_model(self._h, n.ctypes.data, C.addressof(to_world), argb.ctypes.data if argb is not None else None,
                                               solid.ctypes.data if solid is not None else None, None))
        return argb, (solid.view(np.bool_) if solid is not None else None)

    def read_model_device(self, size, to_world, argb_ptr: int, solid_ptr: int, stream: int | None = None) -> None:
        """read_model into device memory (addresses of sx * sz * sy uint32 / uint8; either may be 0), enqueued on `stream` (None or 0: the
        context's) without waiting."""
        n = self._model_read(size, to_world)
        self._check(lib().cvx_world_read_model_device(self._h, n.ctypes.data, C.addressof(to_world), argb_ptr or None, solid_ptr or None, stream or None))

    # -- exact squared-distance fields (cvx_world_distance) --
    def distance(self, box_min, box_max, max_distance: int, mode: int = DISTANCE_TO_SOLID, solid_outside: int = SURFACE_OUTSIDE_DEFAULT):
        """The squared Euclidean distance, in LOD-0 voxels, of every voxel of [box_min, box_max) (it may stick out of the world) to the nearest
        solid voxel (DISTANCE_TO_SOLID), the nearest air voxel (DISTANCE_TO_AIR) or both (DISTANCE_SIGNED: negative inside the solid), as an
        int32 array of shape (X, Z, Y), y fastest; DISTANCE_FAR where nothing lies within max_distance (1 .. 255).  `solid_outside` bits
        0..5 = -X,+X,-Y,+Y,-Z,+Z: what lies beyond a face of the world."""
        lo, hi = self._box(box_min, box_max)
        shape = tuple(max(int(hi[a]) - int(lo[a]), 0) for a in (0, 2, 1))
        out = np.zeros(shape, dtype=np.int32) if 0 < shape[0] * shape[1] * shape[2] < 1 << 31 else None  # (anything else: the call rejects it)
        self._check(lib().cvx_world_distance(self._h, lo.ctypes.data, hi.ctypes.data, int(max_distance), int(mode), int(solid_outside),
                                             out.ctypes.data if out is not None else None, None))
        return out

    def distance_device(self, box_min, box_max, max_distance: int, out_ptr: int, mode: int = DISTANCE_TO_SOLID,
                        solid_outside: int = SURFACE_OUTSIDE_DEFAULT) -> float:
        """distance into device memory (the address of X * Z * Y int32, e.g. a torch tensor's data_ptr()), ordered on the context's stream; the
        field is complete when the call returns.  Returns the device milliseconds."""
        lo, hi = self._box(box_min, box_max)
        ms = C.c_float()
        self._check(lib().cvx_world_distance_device(self._h, lo.ctypes.data, hi.ctypes.data, int(max_distance), int(mode), int(solid_outside),
                                                    out_ptr or None, C.byref(ms)))
        return ms.value

    # -- snapshots that stay on the device (include/cpuvox_gpu_snapshot.h) --
    def world_snapshot(self, x0: int, z0: int, size_x: int, size_z: int, level_count: int = 5) -> "Snapshot":
        """cvx_world_snapshot: the columns of the rectangle (rounded outward to 2^level_count, clipped) at LOD 0 .. level_count, kept in device
        memory -> a Snapshot (.info, .restore(), .diff(), .diff_device(), .close(); a context manager)."""
        handle, ms = C.c_void_p(), C.c_float()
        self._check(lib().cvx_world_snapshot(self._h, int(x0), int(z0), int(size_x), int(size_z), int(level_count), C.byref(handle), C.byref(ms)))
        snapshot = Snapshot(self, handle, ms.value)
        self._snapshots.append(snapshot)
        return snapshot

    # -- the floating pieces as models with mass moments (include/cpuvox_gpu_lift.h) --
    def _lift(self, fn, box_min, box_max, anchors, op, level_count, capacity, argb_ptr, solid_ptr, voxel_capacity):
        lo, hi = np.ascontiguousarray(box_min, dtype=np.int32), np.ascontiguousarray(box_max, dtype=np.int32)
        if lo.shape != (3,) or hi.shape != (3,):
            raise ValueError("world_lift_pieces: box_min and box_max are three integers each")
        out = np.zeros(max(int(capacity), 0), dtype=LIFTED_PIECE_DTYPE)
        summary, ms = LiftSummary(), C.c_float()
        self._check(fn(self._h, lo.ctypes.data, hi.ctypes.data, int(anchors), int(op), int(level_count), out.ctypes.data if out.size else None, int(capacity),
                       argb_ptr or None, solid_ptr or None, int(voxel_capacity), C.byref(summary), C.byref(ms)))
        totals = {name: int(getattr(summary.pieces, name)) for name, _ in PiecesSummary._fields_}
        totals.update({name: int(getattr(summary, name)) for name in ("storedPieces", "storedVoxels", "neededVoxels")})
        return out[:min(out.size, totals["floatingPieces"])].copy(), totals, ms.value

    def world_lift_pieces(self, box_min, box_max, anchors: int, op: int = LIFT_COPY, level_count: int = LOD_LEVELS - 1, capacity: int = 1024,
                          voxel_capacity: int = 0, want_argb: bool = True, want_solid: bool = True, argb=None, solid=None):
        """cvx_world_lift_pieces: the floating pieces of world_pieces(box_min, box_max, anchors) as models.  Returns (the first `capacity` pieces
        as a LIFTED_PIECE_DTYPE array -- cvx_piece, offset, sum, moment --, the totals as a dict: cvx_pieces_summary's four and storedPieces,
        storedVoxels, neededVoxels, the argb pool (uint32, voxel_capacity elements, or None), the solid pool (uint8 or None), device
        milliseconds).  The longest prefix of the listed pieces whose box volumes fit voxel_capacity is stored: lifted_model(pieces, i, argb,
        solid) gives piece i's arrays.  op = LIFT_REMOVE turns the stored pieces into air and rebuilds LOD 1..level_count over their footprint.
        With the capacities 0 the call is a report whose neededVoxels sizes the pools.  `argb` / `solid`: the caller's own pools (contiguous
        uint32 / uint8 arrays of at least voxel_capacity elements) instead of fresh ones; elements from storedVoxels on keep what they held."""
        n = max(int(voxel_capacity), 0)
        for pool, dtype in ((argb, np.uint32), (solid, np.uint8)):
            if pool is not None and (not isinstance(pool, np.ndarray) or pool.dtype != dtype or not pool.flags.c_contiguous or pool.size < n):
                raise ValueError("world_lift_pieces: a pool is a contiguous uint32 / uint8 array of at least voxel_capacity elements")
        if argb is None:
            argb = np.zeros(n, dtype=np.uint32) if want_argb and n else None
        if solid is None:
            solid = np.zeros(n, dtype=np.uint8) if want_solid and n else None
        pieces, totals, ms = self._lift(lib().cvx_world_lift_pieces, box_min, box_max, anchors, op, level_count, capacity,
                                        argb.ctypes.data if argb is not None else None, solid.ctypes.data if solid is not None else None, voxel_capacity)
        return pieces, totals, argb, solid, ms

    def world_lift_pieces_device(self, box_min, box_max, anchors: int, argb_tensor, solid_tensor, op: int = LIFT_COPY, level_count: int = LOD_LEVELS - 1,
                                 capacity: int = 1024, voxel_capacity: int | None = None):
        """world_lift_pieces into device memory: argb_tensor / solid_tensor are contiguous torch tensors on the context's device, int32 (the colour
        words' bits) and uint8 (either may be None), or addresses of such memory; voxel_capacity defaults to the smaller tensor's length.  The
        pools are complete when the call returns.  Returns (pieces, totals, device milliseconds)."""
        sizes, ptrs = [], []
        for tensor, dtypes in ((argb_tensor, ("torch.int32", "torch.uint32")), (solid_tensor, ("torch.uint8",))):
            if tensor is None or isinstance(tensor, int):
                ptrs.append(tensor or None)
                continue
            if str(getattr(tensor, "dtype", "")) not in dtypes or not tensor.is_contiguous() or not tensor.is_cuda:
                raise ValueError("world_lift_pieces_device: the pools are contiguous int32 / uint8 device tensors")
            sizes.append(tensor.numel())
            ptrs.append(tensor.data_ptr() if tensor.numel() else None)
        if voxel_capacity is None:
            if not sizes and any(ptrs):
                raise ValueError("world_lift_pieces_device: voxel_capacity is needed with raw addresses")
            voxel_capacity = min(sizes) if sizes else 0
        elif sizes and voxel_capacity > min(sizes):
            raise ValueError("world_lift_pieces_device: voxel_capacity exceeds a pool")
        return self._lift(lib().cvx_world_lift_pieces_device, box_min, box_max, anchors, op, level_count, capacity, ptrs[0], ptrs[1], voxel_capacity)

    # -- travel-distance fields through air or solid (cvx_world_spread) --
    def _spread(self, fn, box_min, box_max, seeds, medium, step_faces, max_steps, out_ptr):
        lo, hi = self._box(box_min, box_max)
        p = SpreadParams((C.c_int32 * 3)(*lo.tolist()), (C.c_int32 * 3)(*hi.tolist()), int(medium), int(step_faces), int(max_steps), 0)
        s = seeds_array(seeds)
        summary, ms = SpreadSummary(), C.c_float()
        self._check(fn(self._h, C.addressof(p), s.ctypes.data if s.size else None, s.size, out_ptr or None, C.addressof(summary), C.byref(ms)))
        return {name: getattr(summary, name) for name, _ in SpreadSummary._fields_ if name != "pad_"}, ms.value

    def world_spread(self, box_min, box_max, seeds, *, medium: int, step_faces: int = 0x3F, max_steps: int):
        """The travel distance from `seeds` -- (x, y, z) or (x, y, z, start) each, or a SPREAD_SEED_DTYPE array -- to every voxel of [box_min,
        box_max) (it may stick out of the world) through SPREAD_AIR or SPREAD_SOLID: steps of cost 1 between passable face neighbours, in the
        directions `step_faces` allows (bits 0..5 = -X,+X,-Y,+Y,-Z,+Z: 0x3F all, 0x37 water, 0x3B smoke), cut at max_steps (1 .. 65534).
        Returns (the field, int32 of shape (X, Z, Y), y fastest: the distance, SPREAD_UNREACHED, or SPREAD_BLOCKED where the voxel is not
        passable; the summary as a dict: passable, reached, largestDistance, seedsUsed, launches, tileVisits; the device milliseconds)."""
        lo, hi = self._box(box_min, box_max)
        shape = tuple(max(int(hi[a]) - int(lo[a]), 0) for a in (0, 2, 1))
        out = np.zeros(shape, dtype=np.int32) if 0 < shape[0] * shape[1] * shape[2] < 1 << 31 else None  # (anything else: the call rejects it)
        summary, ms = self._spread(lib().cvx_world_spread, lo, hi, seeds, medium, step_faces, max_steps, out.ctypes.data if out is not None else None)
        return out, summary, ms

    def world_spread_device(self, box_min, box_max, seeds, out_tensor, *, medium: int, step_faces: int = 0x3F, max_steps: int):
        """world_spread into device memory: `out_tensor` is a contiguous int32 torch tensor of X * Z * Y elements on the context's device (or the
        address of such memory); the field is complete when the call returns.  `seeds` stays a host array.  Returns (summary, device ms)."""
        ptr = out_tensor if isinstance(out_tensor, int) else _spread_tensor_ptr(out_tensor, self._box(box_min, box_max))
        return self._spread(lib().cvx_world_spread_device, box_min, box_max, seeds, medium, step_faces, max_steps, ptr)

    def debug_cavities(self) -> dict:
        """Diagnostics build only (include/cpuvox_gpu_diag.h): the last world_cavities' device ms split (analysis, edit), its air intervals and
        hook rounds."""
        ms, counts = (C.c_float * 2)(), (C.c_int64 * 2)()
        self._check(self._diag("cvx_debug_cavities")(self._h, ms, counts))
        return {"analysis_ms": ms[0], "edit_ms": ms[1], "nodes": counts[0], "rounds": counts[1]}

    def world_light(self, box_min, box_max, *, sun_dir=(0, 0, 0), sun_level: int = 0, sun_range: int = 0, sky_level: int = 0, sky_range: int = 0,
                    floor_level: int = 0, target: int = LIGHT_TO_RGB, level_count: int = LOD_LEVELS - 1) -> float:
        """Bakes sky occlusion and a sun shadow into the solid LOD-0 voxels inside [box_min, box_max): shade = min(255, floor_level + sky_level *
        open sky / 26 + (lit ? sun_level * facing / den : 0)), multiplied into R, G, B (LIGHT_TO_RGB, one-shot) or stored in A (LIGHT_TO_ALPHA),
        then rebuilds LOD 1..level_count over the footprint.  sun_dir points TOWARDS the sun (integers, |.| <= 1024).  Returns the device
        milliseconds (0 when the box lies outside the world)."""
        if len(box_min) != 3 or len(box_max) != 3 or len(sun_dir) != 3:
            raise ValueError("world_light: box_min, box_max and sun_dir are three integers each")
        p = LightParams((C.c_int32 * 3)(*[int(v) for v in box_min]), (C.c_int32 * 3)(*[int(v) for v in box_max]), (C.c_int32 * 3)(*[int(v) for v in sun_dir]),
                        sun_level, sun_range, sky_level, sky_range, floor_level, target, 0)
        ms = C.c_float()
        self._check(lib().cvx_world_light(self._h, C.byref(p), level_count, C.byref(ms)))
        return ms.value

    def world_light_lamps(self, box_min, box_max, lamps, *, sun_dir=(0, 0, 0), sun_level: int = 0, sun_range: int = 0, sky_level: int = 0,
                          sky_range: int = 0, floor_level: int = 0, target: int = LIGHT_TO_RGB, level_count: int = LOD_LEVELS - 1) -> float:
        """world_light with point lights in the same bake: `lamps` is a list of (pos, radius, level) or of dicts {pos, radius, level} -- pos the
        LOD-0 voxel at whose centre the lamp sits (anywhere, also outside the world), radius 1 .. LAMP_MAX_RADIUS voxels, level 0 .. 255, at most
        LIGHT_MAX_LAMPS of them.  A lit voxel with an air face towards a lamp it sees gains level * (1 - (d / radius)^2) * facing / den; the terms of
        all lamps are summed before the one min(255, ...).  No lamps: exactly world_light.  Returns the device milliseconds."""
        if len(box_min) != 3 or len(box_max) != 3 or len(sun_dir) != 3:
            raise ValueError("world_light_lamps: box_min, box_max and sun_dir are three integers each")
        p = LightParams((C.c_int32 * 3)(*[int(v) for v in box_min]), (C.c_int32 * 3)(*[int(v) for v in box_max]), (C.c_int32 * 3)(*[int(v) for v in sun_dir]),
                        sun_level, sun_range, sky_level, sky_range, floor_level, target, 0)
        arr = lamps_array(lamps)
        ms = C.c_float()
        self._check(lib().cvx_world_light_lamps(self._h, C.byref(p), arr if len(arr) else None, len(arr), level_count, C.byref(ms)))
        return ms.value

    def world_move(self, bodies) -> np.ndarray:
        """Moves boxes through LOD 0 with collision, sliding and step-up (include/cpuvox_gpu.h, cvx_world_move): `bodies` is a list of dicts
        {pos, size, delta, stepUp, flags} or a MOVE_BODY_DTYPE array, in units of 1 / MOVE_UNIT voxel.  Returns a MOVE_RESULT_DTYPE array: the
        new min corner and the MOVED_* flags of every body.  The world is not changed."""
        arr = bodies_array(bodies)
        out = np.zeros(arr.size, dtype=MOVE_RESULT_DTYPE)
        self._check(lib().cvx_world_move(self._h, arr.size, arr.ctypes.data if arr.size else None, out.ctypes.data if out.size else None))
        return out

    def world_move_device(self, body_count: int, bodies_ptr: int, results_ptr: int, lanes_per_body: int = 0, stream: int = 0) -> None:
        """cvx_world_move on device arrays (addresses of body_count cvx_move_body / cvx_move_result, e.g. a torch tensor's data_ptr()): enqueues
        on `stream` (a hipStream_t as an integer; 0 = the context's stream) and does not wait.  lanes_per_body: 0 (= 16), 1, 4, 16 or 64 lanes
        of a wave share a body; the results do not depend on it."""
        self._check(lib().cvx_world_move_device(self._h, int(body_count), C.c_void_p(int(bodies_ptr)), C.c_void_p(int(results_ptr)), int(lanes_per_body),
                                                C.c_void_p(int(stream)) if stream else None))

    def nav_build(self, box_min, box_max, goals, *, width: int = 1, height: int = 2, step_up: int = 1, max_drop: int = 3, max_steps: int = 0) -> "NavField":
        """A walking-distance field (include/cpuvox_gpu.h, cvx_world_nav_build) over the places a width x height x width box can stand inside
        [box_min, box_max), towards `goals` (int triples; each resolves to the floor below it): a NavField with .summary (dict), .ms, .goals(),
        .query(), .query_device() and .close().  The field is a snapshot of the world as it is now; the context closes the fields it still owns."""
        if len(box_min) != 3 or len(box_max) != 3:
            raise ValueError("nav_build: box_min and box_max are three integers each")
        g = np.ascontiguousarray(np.asarray(goals, dtype=np.int32).reshape(-1, 3))
        p = NavParams((C.c_int32 * 3)(*[int(v) for v in box_min]), (C.c_int32 * 3)(*[int(v) for v in box_max]), width, height, step_up, max_drop, max_steps, 0)
        handle, ms = C.c_void_p(), C.c_float()
        summary = np.zeros(1, dtype=NAV_SUMMARY_DTYPE)
        self._check(lib().cvx_world_nav_build(self._h, C.byref(p), g.ctypes.data if g.size else None, len(g), C.byref(handle), summary.ctypes.data, C.byref(ms)))
        field = NavField(self, handle)
        field._took(summary, ms)
        self._nav_fields.append(field)
        return field

    def pick(self, origins, directions, max_t):
        """First solid LOD-0 voxel along each ray -> (voxel int32[N, 3], face int32[N], argb uint32[N], t float32[N]).  max_t: a scalar or
        one per ray.  Misses: voxel -1, face -1, argb 0, t = max_t."""
        o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        rays = np.zeros(n, dtype=PICK_RAY_DTYPE)
        rays["origin"], rays["direction"] = o, d
        rays["maxT"] = np.broadcast_to(np.asarray(max_t, dtype=np.float32), (n,))
        hits = np.zeros(n, dtype=PICK_HIT_DTYPE)
        self._check(lib().cvx_world_pick(self._h, n, rays.ctypes.data, hits.ctypes.data))
        return hits["voxel"].copy(), hits["face"].copy(), hits["argb"].copy(), hits["t"].copy()

    def pick_screen(self, camera, width: int, height: int, px, py, max_t: float):
        """pick() through the centres of pixels (px, py) of a width x height screen (row 0 = the bottom row) of `camera` (a cvx_camera_data):
        the voxel under the cursor."""
        o, d = screen_rays(camera, width, height, px, py)
        return self.pick(o, d, max_t)

    def set_resolution(self, width: int, height: int) -> None:
        """RenderManager.SetResolution (RenderManager.cs:94-109)."""
        self._check(lib().cvx_set_resolution(self._h, width, height))
        self.width, self.height = width, height

    def set_shard(self, index: int, count: int) -> None:
        self._check(lib().cvx_set_shard(self._h, index, count))

    def set_latency_kernel(self, mode: int) -> None:
        """Which kernel a draw goes to: LATENCY_AUTO (few rays -> one wave per ray), LATENCY_NEVER, LATENCY_ALWAYS (include/cpuvox_gpu.h)."""
        self._check(lib().cvx_set_latency_kernel(self._h, mode))

    def set_world_repeat(self, repeat: bool) -> None:
        """False: the bounded world (default); True: the world repeats in X and Z (World.REPEAT_WORLD; include/cpuvox_gpu.h cvx_set_world_repeat).
        Applies to the draws and picks enqueued from now on; pair it with host.setup_lods(..., repeat=True) for the reference's 10x far clip."""
        if not isinstance(repeat, (bool, int)) or int(repeat) not in (0, 1):
            raise ValueError(f"set_world_repeat: expected a bool, got {repeat!r}")
        self._check(lib().cvx_set_world_repeat(self._h, int(repeat)))

    def enable_counters(self, enable: bool) -> None:
        self._check(lib().cvx_enable_counters(self._h, int(enable)))

    # -- the hot path -------------------------------------------------------
    def draw_segments(self, frame: Frame, buffer_index: int = 0, flags: int = DRAW_SYNC) -> None:
        """RenderManager.DrawSegments (RenderManager.cs:258-372)."""
        vp = (C.c_float * 2)(*frame.vanishingPointScreenSpace)
        self._check(lib().cvx_draw_segments(self._h, C.addressof(frame.segments), C.addressof(frame.camera), self.width, self.height,
                                            C.addressof(vp), buffer_index, flags))

    def draw_segments_batch(self, frames, first_buffer_index: int = 0, flags: int = DRAW_SYNC) -> None:
        n = len(frames)
        segs = (SegmentData * (4 * n))()
        cams = (CameraData * n)()
        vps = (C.c_float * (2 * n))()
        for i, f in enumerate(frames):
            for s in range(4):
                segs[4 * i + s] = f.segments[s]
            cams[i] = f.camera
            vps[2 * i] = f.vanishingPointScreenSpace[0]
            vps[2 * i + 1] = f.vanishingPointScreenSpace[1]
        self._batch_keepalive = (segs, cams, vps)
        self._check(lib().cvx_draw_segments_batch(self._h, n, C.addressof(segs), C.addressof(cams), self.width, self.height,
                                                  C.addressof(vps), first_buffer_index, flags))

    def pack_batch(self, frames):
        """Marshal frames once; returns an opaque object for draw_packed (keeps bench loops free of Python overhead)."""
        return pack_frames(frames)

    def draw_packed(self, packed, first_buffer_index: int = 0, flags: int = DRAW_SYNC) -> None:
        n, segs, cams, vps = packed
        self._check(lib().cvx_draw_segments_batch(self._h, n, C.addressof(segs), C.addressof(cams), self.width, self.height,
                                                  C.addressof(vps), first_buffer_index, flags))

    def draw_placed(self, packed, tile_out: np.ndarray, flags: int = DRAW_SYNC) -> None:
        """cvx_draw_segments_placed: packed = pack_batch(frames), tile_out = uint64 device address per tile (0 = skip)."""
        n, segs, cams, vps = packed
        tile_out = np.ascontiguousarray(tile_out, dtype=np.uint64)
        self._check(lib().cvx_draw_segments_placed(self._h, n, C.addressof(segs), C.addressof(cams), self.width, self.height,
                                                   C.addressof(vps), tile_out.size, tile_out.ctypes.data, flags))

    def synchronize(self) -> None:
        self._check(lib().cvx_synchronize(self._h))

    def last_draw_ms(self) -> float:
        ms = C.c_float()
        self._check(lib().cvx_last_draw_ms(self._h, C.byref(ms)))
        return ms.value

    def draw_time_stats(self, reset: bool = False):
        """(total kernel ms, draws) since the last reset; HIP events on the context's stream."""
        ms = C.c_double()
        n = C.c_int()
        self._check(lib().cvx_draw_time_stats(self._h, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def counters(self) -> Counters:
        out = Counters()
        self._check(lib().cvx_get_counters(self._h, C.byref(out)))
        return out

    # -- raybuffers ---------------------------------------------------------
    def clear_raybuffer(self, buffer_index: int, which: int, argb: int = 0) -> None:
        """RenderManager.ClearRayBuffer (RenderManager.cs:58-92)."""
        self._check(lib().cvx_clear_raybuffer(self._h, buffer_index, which, argb & 0xFFFFFFFF))

    def clear_raybuffers(self, buffer_index: int = 0, argb: int = 0) -> None:
        self.clear_raybuffer(buffer_index, RAYBUFFER_TOPDOWN, argb)
        self.clear_raybuffer(buffer_index, RAYBUFFER_LEFTRIGHT, argb)

    def read_raybuffer(self, buffer_index: int, which: int, first_ray: int = 0, ray_count: int | None = None) -> np.ndarray:
        """Rows of a raybuffer in the reference's ray-major layout (RayBuffer.cs:121-128)."""
        W, H = self.width, self.height
        width = H if which == RAYBUFFER_TOPDOWN else W
        cap = W + 2 * H if which == RAYBUFFER_TOPDOWN else 2 * W + H
        if ray_count is None:
            ray_count = cap - first_ray
        out = np.empty((ray_count, width), dtype=np.uint32)
        self._check(lib().cvx_read_raybuffer(self._h, buffer_index, which, first_ray, ray_count, out.ctypes.data))
        return out

    def blit_segments(self, buffer_index: int = 0, to_host: bool = True):
        """RenderManager.BlitSegments + RayBufferBlit.shader (Phase 2) -> image[H, W] uint32, row 0 = bottom."""
        if not to_host:
            self._check(lib().cvx_blit_segments(self._h, buffer_index, None))
            return None
        out = np.empty((self.height, self.width), dtype=np.uint32)
        self._check(lib().cvx_blit_segments(self._h, buffer_index, out.ctypes.data))
        return out

    def blit_segments_batch(self, first_buffer: int, frame_count: int, dst_device: int | None = None) -> int:
        """Phase 2 of `frame_count` frames (buffers first_buffer ..) in ONE launch, asynchronous on the context's stream.  Image f goes to
        dst_device + f * H * W * 4 (a device address, e.g. a torch tensor's data_ptr()), or into an array the context owns; returns
        the device address of image 0."""
        p = C.c_void_p()
        self._check(lib().cvx_blit_segments_batch(self._h, first_buffer, frame_count, C.c_void_p(dst_device) if dst_device else None, C.byref(p)))
        return p.value

    def screen_device_ptr(self):
        """cvx_screen_device_ptr: (the device address of the image blit_segments(to_host=False) left on the device, its bytes);
        models_draw_device takes the address as its image."""
        p = C.c_void_p()
        n = C.c_int64()
        self._check(lib().cvx_screen_device_ptr(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def raybuffer_device_ptr(self, buffer_index: int, which: int):
        p = C.c_void_p()
        n = C.c_int64()
        self._check(lib().cvx_raybuffer_device_ptr(self._h, buffer_index, which, C.byref(p), C.byref(n)))
        return p.value, n.value

    def bind_raybuffers(self, td_ptr: int, td_bytes: int, lr_ptr: int, lr_bytes: int) -> None:
        """Render into caller-owned device memory (e.g. torch tensors used by a RCCL exchange)."""
        self._check(lib().cvx_bind_raybuffers(self._h, C.c_void_p(td_ptr), td_bytes, C.c_void_p(lr_ptr), lr_bytes))

    def copy_rows(self, hip_stream: int | None, to_packed: bool, span_count: int, spans_ptr: int, packed_ptr: int) -> None:
        """Pack / unpack tile pixel rows between the pools and a staging buffer (multi-GPU exchange payload)."""
        self._check(lib().cvx_copy_rows(self._h, C.c_void_p(hip_stream or 0), int(to_packed), span_count, C.c_void_p(spans_ptr), C.c_void_p(packed_ptr)))

    def raybuffer_layout(self, which: int) -> RaybufferLayout:
        out = RaybufferLayout()
        self._check(lib().cvx_get_raybuffer_layout(self._h, which, C.byref(out)))
        return out

    @staticmethod
    def _diag(name: str):
        """An entry point of include/cpuvox_gpu_diag.h: present in the experiment / profiling builds only."""
        if not hasattr(lib(), name):
            raise RuntimeError(f"{name} is a diagnostic of libcpuvox_gpu_exp.so / the profiling builds (include/cpuvox_gpu_diag.h); "
                               "the product library does not export it: cpuvox_amd.gpu.use_library(<diagnostics build>) first")
        return getattr(lib(), name)

    def debug_occupancy(self, lds_bytes: int) -> int:
        n = C.c_int()
        self._diag("cvx_debug_occupancy")
        self._check(lib().cvx_debug_occupancy(self._h, lds_bytes, C.byref(n)))
        return n.value

    def debug_last_launch(self) -> dict:
        """Experiment build only: the shape of the last draw's launch, LAUNCH_FIELDS -> value (include/cpuvox_gpu_diag.h)."""
        out = (C.c_int64 * 8)()
        self._check(self._diag("cvx_debug_last_launch")(self._h, out))
        return dict(zip(LAUNCH_FIELDS, list(out)))

    def set_buffer_count(self, buffer_count: int) -> None:
        """cvx_set_buffer_count: raybuffer pairs of the context (the pools are allocated anew; the world stays)."""
        self._check(lib().cvx_set_buffer_count(self._h, buffer_count))
        self.buffer_count = buffer_count

    def debug_section_cycles(self, reset: bool = False):
        """Diagnostic build only: wave cycles per render-kernel section (include/cpuvox_gpu_diag.h)."""
        out = (C.c_uint64 * 32)()
        self._check(self._diag("cvx_debug_section_cycles")(self._h, out, int(reset)))
        return list(out)

    def debug_section_histogram(self, reset: bool = False):
        """Counting diagnostic build only: [section][bucket of 8 lanes] executions (include/cpuvox_gpu_diag.h)."""
        out = (C.c_uint64 * 128)()
        self._check(self._diag("cvx_debug_section_histogram")(self._h, out, int(reset)))
        return [list(out[i * 8:(i + 1) * 8]) for i in range(16)]

    def debug_clip_census(self, reset: bool = False) -> dict:
        """Counting diagnostic build only: the census of the frustum clip's general instance (include/cpuvox_gpu_diag.h).  "pairs": {(class at Last,
        class at Next): executions whose lanes all share it} (indices into CLIP_CLASSES), "mixed_pairs", "executions", "predicates": {name of
        CLIP_PREDICATES: {"all", "some", "some_lanes"}}, "arms": executions of the "inverted_straddle" and the "general" instance, of the latter with an
        inverted-straddling lane in it ("general_mixed") and those lanes ("general_mixed_lanes")."""
        out = (C.c_uint64 * 96)()
        self._check(self._diag("cvxd_clip_census")(self._h, out, int(reset)))
        n = len(CLIP_CLASSES)
        return {"pairs": {(cl, cn): int(out[cl * n + cn]) for cl in range(n) for cn in range(n)}, "mixed_pairs": int(out[n * n]), "executions": int(out[n * n + 1]),
                "predicates": {name: {"all": int(out[51 + 3 * k]), "some": int(out[52 + 3 * k]), "some_lanes": int(out[53 + 3 * k])}
                               for k, (name, _) in enumerate(CLIP_PREDICATES)},
                "arms": {"inverted_straddle": int(out[72]), "general": int(out[73]), "general_mixed": int(out[74]), "general_mixed_lanes": int(out[75])}}

    def selftest_math(self, op: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        out = np.empty_like(a)
        self._check(self._diag("cvx_selftest_math")(self._h, op, a.size, a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out

    def selftest_lone(self, op: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
        """The latency kernel's inline-assembly primitives on the caller's values (diagnostics build): op 0 the crossing chains, op 1 v_writelane."""
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        waves = b.size
        out = np.empty(waves * (128 if op == 0 else 64), dtype=np.float32)
        self._check(self._diag("cvx_selftest_lone")(self._h, op, waves, a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out

    def selftest_scan(self, values: np.ndarray):
        """Diagnostics build only: (exclusive prefix sums modulo 2^32, 64-bit total) of uint32 values by the device scan of cvx_world_downsample."""
        v = np.ascontiguousarray(values, dtype=np.uint32).copy()
        total = C.c_uint64()
        self._check(self._diag("cvx_selftest_scan")(self._h, v.size, v.ctypes.data, C.byref(total)))
        return v, int(total.value)


class Snapshot:
    """A cvx_snapshot: made by Context.world_snapshot, closed by .close(), by leaving its `with` block, or with its context.  It keeps its
    context alive and must be destroyed before it (cvx_snapshot_destroy before cvx_destroy): Context.close() closes the snapshots still open."""

    def __init__(self, ctx: "Context", handle, ms: float):
        self._ctx, self._h, self.ms = ctx, handle, ms
        info = SnapshotInfo()
        ctx._check(lib().cvx_snapshot_info_get(handle, C.byref(info)))
        self.info = {name: int(getattr(info, name)) for name, _ in SnapshotInfo._fields_}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def restore(self) -> float:
        """cvx_world_snapshot_restore: every held level back over its rectangle -> device milliseconds."""
        ms = C.c_float()
        self._ctx._check(lib().cvx_world_snapshot_restore(self._ctx._h, self._h, C.byref(ms)))
        return ms.value

    def _diff(self, fn, flags, ptr, capacity):
        summary, ms = SnapshotDiffSummary(), C.c_float()
        self._ctx._check(fn(self._ctx._h, self._h, int(flags), C.c_void_p(ptr) if ptr else None, int(capacity), C.byref(summary), C.byref(ms)))
        self.ms = ms.value
        return {"changedColumns": int(summary.changedColumns), "changedVoxels": int(summary.changedVoxels), "min": tuple(summary.min), "max": tuple(summary.max)}

    def diff(self, flags: int = 0, capacity: int | None = None):
        """cvx_world_snapshot_diff: LOD 0 as it is now against the snapshot's -> (a SNAPSHOT_CHANGE_DTYPE array of the first min(capacity, changed
        columns) changed columns in the rectangle's column order, the summary as a dict).  capacity None: every column of the rectangle."""
        if capacity is None:
            capacity = self.info["sizeX"] * self.info["sizeZ"]
        changes = np.zeros(int(capacity), dtype=SNAPSHOT_CHANGE_DTYPE)
        summary = self._diff(lib().cvx_world_snapshot_diff, flags, changes.ctypes.data if capacity else None, capacity)
        return changes[:min(int(capacity), summary["changedColumns"])], summary

    def diff_device(self, tensor_ptr, capacity: int, flags: int = 0) -> dict:
        """cvx_world_snapshot_diff_device: the list goes to device memory at `tensor_ptr` (an address, e.g. a torch tensor's data_ptr(), with room for
        `capacity` entries of 16 bytes; None with capacity 0) -> the summary."""
        return self._diff(lib().cvx_world_snapshot_diff_device, flags, int(tensor_ptr) if tensor_ptr else None, capacity)

    def close(self) -> None:
        if self._h:
            lib().cvx_snapshot_destroy(self._h)
            self._h = C.c_void_p()
            if self in self._ctx._snapshots:
                self._ctx._snapshots.remove(self)

    def __del__(self):
        try:
            if self._ctx._h:  # (a context that is gone has closed its snapshots)
                self.close()
        except Exception:
            pass


class NavField:
    """A cvx_nav_field: made by Context.nav_build, closed by .close() or with its context."""

    def __init__(self, ctx: "Context", handle):
        self._ctx, self._h = ctx, handle
        self.summary, self.ms = {}, 0.0

    def _took(self, summary, ms) -> None:
        self.summary = {name: int(summary[0][name]) for name in NAV_SUMMARY_DTYPE.names if name != "pad_"}
        self.ms = ms.value

    def goals(self, goals, max_steps: int = 0) -> dict:
        """Solves the same nodes and steps for new goals (cvx_nav_field_goals) -> the new summary."""
        g = np.ascontiguousarray(np.asarray(goals, dtype=np.int32).reshape(-1, 3))
        summary, ms = np.zeros(1, dtype=NAV_SUMMARY_DTYPE), C.c_float()
        self._ctx._check(lib().cvx_nav_field_goals(self._ctx._h, self._h, g.ctypes.data if g.size else None, len(g), int(max_steps), summary.ctypes.data, C.byref(ms)))
        self._took(summary, ms)
        return self.summary

    def query(self, cells) -> np.ndarray:
        """cvx_nav_query: positions (int triples) -> a NAV_STEP_DTYPE array, one cvx_nav_step each."""
        c = np.ascontiguousarray(np.asarray(cells, dtype=np.int32).reshape(-1, 3))
        out = np.zeros(len(c), dtype=NAV_STEP_DTYPE)
        self._ctx._check(lib().cvx_nav_query(self._ctx._h, self._h, len(c), c.ctypes.data if len(c) else None, out.ctypes.data if len(c) else None))
        return out

    def query_device(self, count: int, cells_ptr: int, steps_ptr: int, stream: int = 0) -> None:
        """cvx_nav_query on device arrays (addresses of 3 * count int32 and count cvx_nav_step): enqueues on `stream` (a hipStream_t as an
        integer; 0 = the context's stream) and does not wait."""
        self._ctx._check(lib().cvx_nav_query_device(self._ctx._h, self._h, int(count), C.c_void_p(int(cells_ptr)), C.c_void_p(int(steps_ptr)),
                                                    C.c_void_p(int(stream)) if stream else None))

    def close(self) -> None:
        if self._h:
            lib().cvx_nav_field_destroy(self._h)
            self._h = C.c_void_p()
            if self in self._ctx._nav_fields:
                self._ctx._nav_fields.remove(self)

    def __del__(self):
        try:
            if self._ctx._h:  # (a context that is gone has closed its fields)
                self.close()
        except Exception:
            pass


def pack_frames(frames):
    """(n, SegmentData[4 n], CameraData[n], float[2 n]) of a list of host frames: the argument arrays of cvx_draw_segments_batch /
    cvx_shard_plan_create.  Needs no context and no GPU."""
    n = len(frames)
    segs = (SegmentData * (4 * n))()
    cams = (CameraData * n)()
    vps = (C.c_float * (2 * n))()
    for i, f in enumerate(frames):
        for s in range(4):
            segs[4 * i + s] = f.segments[s]
        cams[i] = f.camera
        vps[2 * i] = f.vanishingPointScreenSpace[0]
        vps[2 * i + 1] = f.vanishingPointScreenSpace[1]
    return (n, segs, cams, vps)


class NativeShardPlan:
    """cvx_shard_plan_* (include/cpuvox_gpu.h): the shard plan of one batch of frames as the library computes it -- host
    arithmetic only, no GPU needed.  `packed` = Context.pack_batch(frames) or (n, segments, cameras, vps)."""

    def __init__(self, packed, width: int, height: int, rank: int, world_size: int):
        n, segs, _cams, vps = packed
        self._keep = packed
        self._h = C.c_void_p()
        rc = lib().cvx_shard_plan_create(n, C.addressof(segs), C.addressof(vps), width, height, rank, world_size, C.byref(self._h))
        if rc != 0:
            raise CvxError(f"cvx_shard_plan_create failed ({rc}): {lib().cvx_last_error(None).decode()}")
        self.rank, self.N = rank, world_size
        self.tile_count = int(lib().cvx_shard_plan_tile_count(self._h))
        self.send_start = np.zeros(world_size + 1, dtype=np.int64)
        self.disp_start = np.zeros(world_size + 1, dtype=np.int64)
        lib().cvx_shard_plan_sections(self._h, self.send_start.ctypes.data, self.disp_start.ctypes.data)
        self.send_total, self.disp_total = int(self.send_start[-1]), int(self.disp_start[-1])

    def tile_out(self, send_ptr: int, disp_ptr: int) -> np.ndarray:
        out = np.zeros(max(1, self.tile_count), dtype=np.uint64)
        lib().cvx_shard_plan_tile_out(self._h, C.c_void_p(send_ptr), C.c_void_p(disp_ptr), out.ctypes.data)
        return out[: self.tile_count]

    def transfer(self, peer: int):
        """(send row, send rows, receive row, receive rows) between this rank and `peer` -- what cvx_exchange moves."""
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        rc = lib().cvx_shard_plan_transfer(self._h, peer, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        if rc != 0:
            raise CvxError(f"cvx_shard_plan_transfer failed ({rc})")
        return a.value, b.value, c.value, d.value

    def exchange(self, ctx: "Context", comm: int, hip_stream: int | None, send_ptr: int, disp_ptr: int) -> None:
        """cvx_exchange: grouped ncclSend / ncclRecv of this batch's sections, enqueued on hip_stream."""
        ctx._check(lib().cvx_exchange(ctx._h, self._h, C.c_void_p(comm), C.c_void_p(hip_stream or 0), C.c_void_p(send_ptr), C.c_void_p(disp_ptr)))

    def close(self) -> None:
        if self._h:
            lib().cvx_shard_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ImagePlan:
    """cvx_image_plan_* (include/cpuvox_gpu.h): the IMAGE gather of one batch of frames -- every rank blits the pixels of the tiles it
    rendered, the display rank receives W * H pixels per frame in total.  Needs the GPU (pixel counts per rank are made on the device)."""

    def __init__(self, ctx: "Context", packed, width: int, height: int, rank: int, world_size: int):
        n, segs, _cams, vps = packed
        self._keep = packed
        self._h = C.c_void_p()
        ctx._check(lib().cvx_image_plan_create(ctx._h, n, C.addressof(segs), C.addressof(vps), width, height, rank, world_size, C.byref(self._h)))
        self.rank, self.N, self.frames = rank, world_size, n
        self.tile_count = int(lib().cvx_image_plan_tile_count(self._h))
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        lib().cvx_image_plan_sizes(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        self.local_store_bytes, self.send_pixels, self.recv_pixels, self.images = a.value, b.value, c.value, d.value

    def tile_out(self, local_store_ptr: int) -> np.ndarray:
        out = np.zeros(max(1, self.tile_count), dtype=np.uint64)
        lib().cvx_image_plan_tile_out(self._h, C.c_void_p(local_store_ptr), out.ctypes.data)
        return out[: self.tile_count]

    def transfer(self, peer: int):
        """(first send pixel, send pixels, first receive pixel, receive pixels) between this rank and `peer`."""
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        if lib().cvx_image_plan_transfer(self._h, peer, C.byref(a), C.byref(b), C.byref(c), C.byref(d)) != 0:
            raise CvxError("cvx_image_plan_transfer failed")
        return a.value, b.value, c.value, d.value

    def pack(self, ctx: "Context", hip_stream: int | None, local_store_ptr: int, send_ptr: int, images_ptr: int) -> None:
        ctx._check(lib().cvx_image_pack(ctx._h, self._h, C.c_void_p(hip_stream or 0), C.c_void_p(local_store_ptr), C.c_void_p(send_ptr), C.c_void_p(images_ptr)))

    def exchange(self, ctx: "Context", comm: int, hip_stream: int | None, send_ptr: int, recv_ptr: int) -> None:
        ctx._check(lib().cvx_image_exchange(ctx._h, self._h, C.c_void_p(comm), C.c_void_p(hip_stream or 0), C.c_void_p(send_ptr), C.c_void_p(recv_ptr)))

    def unpack(self, ctx: "Context", hip_stream: int | None, recv_ptr: int, images_ptr: int) -> None:
        ctx._check(lib().cvx_image_unpack(ctx._h, self._h, C.c_void_p(hip_stream or 0), C.c_void_p(recv_ptr), C.c_void_p(images_ptr)))

    def close(self) -> None:
        if self._h:
            lib().cvx_image_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    rc = lib().cvx_comm_unique_id(buf)
    if rc != 0:
        raise CvxError(f"cvx_comm_unique_id failed ({rc}): {lib().cvx_last_error(None).decode()}")
    return buf.raw


def comm_create(ctx: Context, unique_id: bytes, rank: int, world_size: int, timeout_s: float = 180.0) -> int:
    """ncclCommInitRank through the C ABI; raises (CVX_ERR_TIMEOUT) when the clique is not complete after `timeout_s`."""
    comm = C.c_void_p()
    ctx._check(lib().cvx_comm_create_timeout(ctx._h, unique_id, rank, world_size, float(timeout_s), C.byref(comm)))
    return comm.value


def comm_destroy(comm: int) -> None:
    lib().cvx_comm_destroy(C.c_void_p(comm))
