"""evplp_amd -- Python binding (ctypes) of libevplp_hip.so, the MI355X implementation of evplp's
radiance-accumulation hot path.

The product is the C-ABI library (include/evplp.h) plus the C++ host side above it
(evplp_amd/csrc/host); this module only exposes that ABI to tests, bench.py and the multi-GPU
strip renderer.  It never computes anything itself and has no CPU fallback: if the shared
library is missing the import fails loudly, and without a HIP device `Context()` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# EVPLP_LIB: developer override (e.g. the -DEVPLP_TRAVERSAL_STATS=1 diagnostic build of tools/traversal_stats.py)
LIB_PATH = os.environ.get("EVPLP_LIB") or os.path.join(_HERE, "lib", "libevplp_hip.so")
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

ABI_VERSION = 5

# evplp_status
OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_IO, ERR_PARSE, ERR_OOM = 0, -1, -2, -3, -4, -5, -6
# flags (rt/rtcomphoton/rtphotonrecord.h:9-15)
USABLE_VPL, USABLE_PHOTON, LAMBERT_ONLY, PHONG_ONLY = 1, 2, 4, 8
# EMis (rtcomphoton.h:64-72, string map :1199-1206)
MIS_MODES = {"one": 0, "balance": 1, "max": 2, "power2": 3, "geometryClamp": 4, "geometryBrdfClamp": 5}
BVH_LBVH, BVH_SAH, BVH_SBVH, BVH_LBVH_GPU, BVH_PLOC_GPU = 0, 1, 2, 3, 4
PLOC_RADIUS, PLOC_MAX_RADIUS, PLOC_SEARCH_ITERATIONS = 16, 32, 128      # csrc/evplp_types.h
(BUF_RECORDS, BUF_GBUF_POSITION, BUF_GBUF_NORMAL, BUF_GBUF_DIFFUSE, BUF_GBUF_PHONG, BUF_LIGHT,
 BUF_VPL_ACCUM, BUF_PHOTON_ACCUM, BUF_COUNT) = range(9)
(PASS_PRIMARY, PASS_LIGHT_TRACE, PASS_GATHER_VPL, PASS_GATHER_VSL, PASS_SPLAT, PASS_RESOLVE, PASS_PATH_TRACE,
 PASS_GATHER_LVC, PASS_COUNT) = range(9)

RECORD_DTYPE = np.dtype([
    ("pos", np.float32, 3), ("flags", np.uint32),
    ("normal", np.float32, 3), ("p_select_lambert", np.float32),
    ("flux", np.float32, 3), ("pad1", np.float32),
    ("flux_dir", np.float32, 3), ("pad2", np.float32),
    ("rho_d", np.float32, 3), ("pad3", np.float32),
    ("rho_s", np.float32, 3), ("phong_exp", np.float32),
])
assert RECORD_DTYPE.itemsize == 96
# ray queries (evplp_ray: origin, tmin, direction, tmax as 8 floats; evplp_hit)
HIT_DTYPE = np.dtype([("t", np.float32), ("beta", np.float32), ("gamma", np.float32), ("triangle", np.int32)])
assert HIT_DTYPE.itemsize == 16
QUERY_CHUNK_RAYS, QUERY_ORDER = 262144, 1
# probe gather (evplp_probe_sh: nine SH coefficients x rgb, then the number of lit pairs, -1 for an invalid probe)
PROBE_SH_DTYPE = np.dtype([("c", np.float32, (9, 3)), ("lit", np.float32)])
assert PROBE_SH_DTYPE.itemsize == 112
PROBE_CHUNK, PROBE_SLICE_SLOTS = 16384, 256
# surface gather (evplp_surface_point: the four float4 of a G-buffer pixel; evplp_surface_light: the VPL sum and the lit pairs, the photon
# estimate and the pairs inside the radius; lit = photons = -1 for a point or an eye that is not finite)
SURFACE_POINT_DTYPE = np.dtype([("pos", np.float32, 3), ("valid", np.float32), ("normal", np.float32, 3), ("pad0", np.float32),
                                ("rho_d", np.float32, 3), ("pad1", np.float32), ("rho_s", np.float32, 3), ("phong_exp", np.float32)])
SURFACE_LIGHT_DTYPE = np.dtype([("vpl", np.float32, 3), ("lit", np.float32), ("pm", np.float32, 3), ("photons", np.float32)])
assert SURFACE_POINT_DTYPE.itemsize == 64 and SURFACE_LIGHT_DTYPE.itemsize == 32
SURFACE_VPL, SURFACE_PHOTONS, SURFACE_CHUNK = 1, 2, 16384
# progressive surface gather (evplp_surface_state: a point's unnormalised photon flux, squared radius, running VPL sums and counts; 48 zero
# bytes are a fresh state)
SURFACE_STATE_DTYPE = np.dtype([("tau", np.float32, 3), ("radius2", np.float32), ("vpl", np.float32, 3), ("n", np.float32),
                                ("lit_sum", np.float32), ("vpl_calls", np.uint32), ("pm_calls", np.uint32), ("flags", np.uint32)])
assert SURFACE_STATE_DTYPE.itemsize == 48
STATE_INVALID = 1
# lightmap baking (evplp_lightmap_texel: the resolved VPL sum, the coverage -- count / S^2, -d for a texel the gutter's pass d filled --, the
# photon estimate and the mean pair count)
LIGHTMAP_TEXEL_DTYPE = np.dtype([("vpl", np.float32, 3), ("coverage", np.float32), ("pm", np.float32, 3), ("photons", np.float32)])
assert LIGHTMAP_TEXEL_DTYPE.itemsize == 32
POINTS_WHITE, POINTS_FACE_EYES, LIGHTMAP_CHUNK = 1, 2, 262144
# trace_closest / trace_occluded's default for `order`: off.  On the furnished stand-in scene the ordering pass did not pay for its keys
# and its sort on shuffled camera rays by more than the spread of the unordered runs (profiles/ray_query_times.txt)
QUERY_ORDER_DEFAULT = False


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("res_x", C.c_int32), ("res_y", C.c_int32),
                ("strip_rank", C.c_int32), ("strip_count", C.c_int32), ("strip_rows", C.c_int32),
                ("num_light_paths", C.c_uint32), ("num_vpl_light_paths", C.c_uint32), ("photons_per_path", C.c_uint32),
                ("bvh_builder", C.c_int32), ("deterministic", C.c_int32), ("gather_splits_per_wave", C.c_int32),
                ("overlap_light_tracing", C.c_int32), ("cut_scratch_bytes", C.c_uint64), ("vsl_mask_bytes", C.c_uint64), ("strip_capacity_rows", C.c_int32)]


class Material(C.Structure):
    _fields_ = [("kd", C.c_float * 3), ("ks", C.c_float * 3), ("ns", C.c_float),
                ("tex_kd", C.c_int32), ("tex_ks", C.c_int32), ("tex_ns", C.c_int32)]


class Camera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("lookat", C.c_float * 3), ("up", C.c_float * 3),
                ("fovy", C.c_float), ("aspect", C.c_float)]


class FrameParams(C.Structure):
    _fields_ = [("camera_pos", C.c_float * 3), ("mis_mode", C.c_uint32), ("pdf_mc", C.c_float),
                ("clamping_value", C.c_float), ("photon_radius", C.c_float), ("vsl_radius", C.c_float),
                ("vsl_inv_pi_radius2", C.c_float), ("num_light_paths", C.c_uint32),
                ("num_vpl_light_paths", C.c_uint32), ("photons_per_path", C.c_uint32),
                ("do_accumulate", C.c_uint32), ("rng_seed", C.c_uint32), ("jitter", C.c_float * 2),
                ("splat_footprint", C.c_uint32), ("reserved", C.c_uint32)]


FOOTPRINT_IDEAL, FOOTPRINT_PROXY = 0, 1
FOOTPRINTS = {"ideal": FOOTPRINT_IDEAL, "proxy": FOOTPRINT_PROXY}


class GroupConfig(C.Structure):
    _fields_ = [("n_ranks", C.c_int32), ("devices", C.POINTER(C.c_int32)), ("strip_rows", C.c_int32), ("use_rccl", C.c_int32),
                ("partition", C.c_int32), ("strip_capacity_pct", C.c_int32), ("split_light_paths", C.c_int32), ("reserved", C.c_int32)]


PARTITION_STRIPS, PARTITION_ITERATIONS = 0, 2
PARTITIONS = {"strips": PARTITION_STRIPS, "iterations": PARTITION_ITERATIONS}


class DenoiseParams(C.Structure):
    """evplp_denoise_params: a zero field is the library's default (levels 5, sigma_luminance 4, sigma_normal 128, sigma_position 0.01)"""
    _fields_ = [("levels", C.c_int32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_position", C.c_float),
                ("reserved", C.c_int32 * 4)]


class TemporalParams(C.Structure):
    """evplp_temporal_params: a zero field is the library's default (max_history 16, normal_cos 0.9)"""
    _fields_ = [("max_history", C.c_int32), ("normal_cos", C.c_float), ("reserved", C.c_int32 * 6)]


class TemporalInfo(C.Structure):
    """evplp_temporal_info"""
    _fields_ = [("filtered", C.c_int64), ("reprojected", C.c_int64), ("disoccluded", C.c_int64), ("history_sum", C.c_int64),
                ("frames_since_reset", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


# evplp_temporal_download's planes
TEMPORAL_HISTORY_U, TEMPORAL_HISTORY_POS, TEMPORAL_HISTORY_NRM, TEMPORAL_PREV_POS, TEMPORAL_PREV_NRM, TEMPORAL_DEBUG_HIT = range(6)


class PassStats(C.Structure):
    _fields_ = [("ms", C.c_float), ("pairs", C.c_uint64), ("rays", C.c_uint64), ("usable", C.c_uint64),
                ("dominant_kernel_ms", C.c_float), ("reserved", C.c_uint32 * 3), ("shaded", C.c_uint64), ("launches", C.c_uint32),
                ("pad", C.c_uint32)]


class AccelQuality(C.Structure):
    """struct evplp_accel_quality"""
    _fields_ = [("cost", C.c_double), ("root_area", C.c_double), ("inner_area", C.c_double), ("leaf_pair_area", C.c_double), ("leaf_tri_area", C.c_double),
                ("built_cost", C.c_double), ("reached_nodes", C.c_int32), ("leaf_refs", C.c_int32), ("refits_since_build", C.c_int32),
                ("policy_rebuilds", C.c_int32), ("last_action", C.c_int32), ("pad", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad"}


# the weights of evplp_accel_quality's cost (csrc/evplp_types.h): vector instructions of a node visit and of a pair test
COST_NODE_VISIT, COST_PAIR_TEST = 15.0, 40.0

# evplp_debug_accel's records (csrc/evplp_types.h BvhNode, LeafBlock, TriFlat, BvhNode4)
ACCEL_NODE = np.dtype([("ctr", np.float32, (3, 2)), ("hal", np.float32, (3, 2)), ("c0", np.int32), ("c1", np.int32), ("pad", np.int32, 2)])
ACCEL_PAIR = np.dtype([("p0", np.float32, (3, 2)), ("e0", np.float32, (3, 2)), ("e1", np.float32, (3, 2)), ("n", np.float32, (3, 2))])
ACCEL_LEAF = np.dtype([("pair", ACCEL_PAIR, 2)])
ACCEL_TRI = np.dtype([("p0", np.float32, 3), ("e0", np.float32, 3), ("e1", np.float32, 3), ("n", np.float32, 3)])
ACCEL_NODE4 = np.dtype([("lo", np.float32, (3, 4)), ("hi", np.float32, (3, 4)), ("child", np.int32, 4), ("pad", np.int32, 4)])
NO_CHILD = -2 ** 31

# every symbol include/evplp.h declares: (restype, argtypes)
_P = C.c_void_p
_SIGNATURES = {
    "evplp_create": (C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    "evplp_destroy": (None, [_P]),
    "evplp_last_error": (C.c_char_p, [_P]),
    "evplp_abi_version": (C.c_int, []),
    "evplp_set_stream": (C.c_int, [_P, _P]),
    "evplp_synchronize": (C.c_int, [_P]),
    "evplp_add_texture": (C.c_int, [_P, C.c_int32, C.c_int32, _P]),
    "evplp_add_material": (C.c_int, [_P, C.POINTER(Material)]),
    "evplp_add_mesh": (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, C.c_int32]),
    "evplp_set_arealight": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_float * 4)]),
    "evplp_set_camera": (C.c_int, [_P, C.POINTER(Camera)]),
    "evplp_load_scene_json": (C.c_int, [_P, C.c_char_p]),
    "evplp_get_camera": (C.c_int, [_P, C.POINTER(Camera)]),
    "evplp_build_accel": (C.c_int, [_P]),
    "evplp_update_mesh": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),
    "evplp_refit_accel": (C.c_int, [_P]),
    "evplp_transform_mesh": (C.c_int, [_P, C.c_int32, _P]),
    "evplp_transform_points": (C.c_int, [_P, _P, _P, C.c_int32]),
    "evplp_group_transform_mesh": (C.c_int, [_P, C.c_int32, _P]),
    "evplp_set_mesh_skin": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, C.c_int32]),
    "evplp_pose_mesh": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),
    "evplp_skin_points": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, C.c_int32]),
    "evplp_mesh_count": (C.c_int, [_P]),
    "evplp_mesh_info": (C.c_int, [_P, C.c_int32, _P, _P, _P]),
    "evplp_mesh_vertices": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32]),
    "evplp_group_set_mesh_skin": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, C.c_int32]),
    "evplp_group_pose_mesh": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),
    "evplp_set_mesh_morph": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32]),
    "evplp_morph_mesh": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),
    "evplp_morph_points": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P]),
    "evplp_group_set_mesh_morph": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32]),
    "evplp_group_morph_mesh": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),
    "evplp_refit_info": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "evplp_refit_levels": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32]),
    "evplp_debug_accel": (C.c_int, [_P, C.c_int32, _P, C.c_size_t]),
    "evplp_group_update_mesh": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),
    "evplp_group_refit_accel": (C.c_int, [_P]),
    "evplp_accel_cost": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double)]),
    "evplp_accel_quality": (C.c_int, [_P, C.POINTER(AccelQuality)]),
    "evplp_trace_closest": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "evplp_trace_occluded": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    "evplp_trace_closest_device": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "evplp_trace_occluded_device": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    "evplp_triangle_info": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "evplp_gather_probes": (C.c_int, [_P, _P, _P, C.c_int32, _P]),
    "evplp_gather_probes_device": (C.c_int, [_P, _P, _P, C.c_int32, _P]),
    "evplp_probe_pair": (None, [_P, _P, C.c_float, _P]),
    "evplp_sh_basis": (None, [_P, _P]),
    "evplp_sh_irradiance": (None, [_P, _P, _P]),
    "evplp_gather_surface": (C.c_int, [_P, _P, C.c_uint32, _P, _P, C.c_int32, _P]),
    "evplp_gather_surface_device": (C.c_int, [_P, _P, C.c_uint32, _P, _P, C.c_int32, _P]),
    "evplp_surface_points": (C.c_int, [_P, _P, C.c_int32, C.c_uint32, _P, _P]),
    "evplp_surface_points_device": (C.c_int, [_P, _P, C.c_int32, C.c_uint32, _P, _P]),
    "evplp_lightmap_samples": (C.c_int, [_P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "evplp_lightmap_samples_device": (C.c_int, [_P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "evplp_lightmap_cover": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "evplp_bake_lightmap": (C.c_int, [_P, _P, C.c_uint32, _P, _P, _P]),
    "evplp_bake_lightmap_device": (C.c_int, [_P, _P, C.c_uint32, _P, _P, _P]),
    "evplp_gather_surface_progressive": (C.c_int, [_P, _P, C.c_uint32, C.c_float, _P, _P, C.c_int32, _P]),
    "evplp_gather_surface_progressive_device": (C.c_int, [_P, _P, C.c_uint32, C.c_float, _P, _P, C.c_int32, _P]),
    "evplp_surface_resolve": (C.c_int, [_P, _P, C.c_int32, _P]),
    "evplp_surface_resolve_device": (C.c_int, [_P, _P, C.c_int32, _P]),
    "evplp_bake_lightmap_progressive_device": (C.c_int, [_P, _P, C.c_uint32, C.c_float, _P, _P, _P]),
    "evplp_bake_lightmap_resolve": (C.c_int, [_P, _P, _P, _P]),
    "evplp_bake_lightmap_resolve_device": (C.c_int, [_P, _P, _P, _P]),
    "evplp_surface_state_update": (C.c_int, [_P, C.c_uint32, _P, C.c_float, C.c_float]),
    "evplp_surface_state_resolve": (C.c_int, [_P, _P]),
    "evplp_gather_surface_knn": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P]),
    "evplp_gather_surface_knn_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P]),
    "evplp_bake_lightmap_knn_device": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "evplp_knn_radius2": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "evplp_surface_state_seed": (C.c_int, [_P, C.c_float, C.c_uint32, _P, C.c_float, C.c_float]),
    "evplp_photon_grid_plan": (C.c_int, [C.c_float, _P, _P, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "evplp_photon_grid_cell": (C.c_uint32, [_P, _P, C.c_float, C.c_uint32, _P]),
    "evplp_photon_grid_range": (C.c_int, [_P, C.c_float, _P, _P, C.c_float, _P, _P]),
    "evplp_group_trace_closest": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "evplp_group_trace_occluded": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    "evplp_ploc_tree": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.POINTER(C.c_int32)]),
    "evplp_set_refit_policy": (C.c_int, [_P, C.c_double, C.c_int32]),
    "evplp_group_accel_quality": (C.c_int, [_P, C.POINTER(AccelQuality)]),
    "evplp_group_set_refit_policy": (C.c_int, [_P, C.c_double, C.c_int32]),
    "evplp_optimize_accel": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32)]),
    "evplp_set_refit_rotations": (C.c_int, [_P, C.c_int32]),
    "evplp_rotation_info": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, C.POINTER(C.c_int32)]),
    "evplp_rotate_tree": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P, _P, C.POINTER(C.c_int32)]),
    "evplp_group_optimize_accel": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32)]),
    "evplp_group_set_refit_rotations": (C.c_int, [_P, C.c_int32]),
    "evplp_scene_metrics": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "evplp_primary": (C.c_int, [_P, C.POINTER(C.c_float * 2), C.c_int32]),
    "evplp_trace_light_paths": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32]),
    "evplp_gather_vpl": (C.c_int, [_P, C.POINTER(FrameParams)]),
    "evplp_gather_vsl": (C.c_int, [_P, C.POINTER(FrameParams)]),
    "evplp_gather_lvc": (C.c_int, [_P, C.POINTER(FrameParams)]),
    "evplp_path_trace": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_int32]),
    "evplp_path_trace_batch": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_uint32]),
    "evplp_path_trace_batch_scratch": (C.c_int, [_P, C.c_uint64]),
    "evplp_splat_photons": (C.c_int, [_P, C.POINTER(FrameParams), C.c_int32]),
    "evplp_set_splat_proxy": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32]),
    "evplp_group_set_splat_proxy": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32]),
    "evplp_default_splat_proxy": (C.c_int, [_P, _P]),
    "evplp_resolve": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, _P]),
    "evplp_present": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32]),
    "evplp_set_error_reference": (C.c_int, [_P, _P, _P]),
    "evplp_frame_error": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, C.POINTER(C.c_double * 3)]),
    "evplp_noise_track": (C.c_int, [_P, C.c_int32, _P]),
    "evplp_noise_fold": (C.c_int, [_P, C.c_int32]),
    "evplp_noise_estimate": (C.c_int, [_P, C.c_float, C.c_float, C.c_int32, C.POINTER(C.c_double * 3)]),
    "evplp_noise_variance": (C.c_int, [_P, C.c_float, _P]),
    "evplp_denoise": (C.c_int, [_P, C.c_float, C.c_float, C.c_int32, C.POINTER(DenoiseParams), _P]),
    "evplp_temporal_enable": (C.c_int, [_P, C.c_int32]),
    "evplp_temporal_reset": (C.c_int, [_P]),
    "evplp_denoise_temporal": (C.c_int, [_P, C.c_float, C.c_float, C.c_int32, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), _P, C.POINTER(TemporalInfo)]),
    "evplp_temporal_download": (C.c_int, [_P, C.c_int32, _P]),
    "evplp_project_points": (C.c_int, [C.POINTER(Camera), C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    "evplp_adaptive_enable": (C.c_int, [_P, C.c_int32]),
    "evplp_adaptive_enable_pt": (C.c_int, [_P, C.c_int32]),
    "evplp_adaptive_retire": (C.c_int, [_P, C.c_float, C.c_float, C.c_int32, C.c_double, C.c_int32]),
    "evplp_adaptive_tiles": (C.c_int, [_P, _P, C.c_int32]),
    "evplp_adaptive_set_budgets": (C.c_int, [_P, _P, C.c_int32]),
    "evplp_adaptive_budgets": (C.c_int, [_P, _P, C.c_int32]),
    "evplp_adaptive_budget_window": (C.c_int, [_P, C.c_int32]),
    "evplp_adaptive_tile_noise": (C.c_int, [_P, C.c_float, C.c_float, C.c_int32, _P, C.c_int32]),
    "evplp_plan_budgets": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _P]),
    "evplp_clear_accumulators": (C.c_int, [_P]),
    "evplp_set_blocks": (C.c_int, [_P, _P, C.c_int32]),
    "evplp_get_blocks": (C.c_int, [_P, _P, C.c_int32]),
    "evplp_calibrate_blocks": (C.c_int, [_P, C.c_int32]),
    "evplp_block_costs": (C.c_int, [_P, _P, C.c_int32]),
    "evplp_deal_blocks": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "evplp_rank_blocks": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32]),
    "evplp_local_rows": (C.c_int, [_P]),
    "evplp_buffer_info": (C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "evplp_bind_buffer": (C.c_int, [_P, C.c_int32, _P, C.c_size_t]),
    "evplp_download": (C.c_int, [_P, C.c_int32, _P, C.c_size_t]),
    "evplp_upload": (C.c_int, [_P, C.c_int32, _P, C.c_size_t]),
    "evplp_pass_stats_get": (C.c_int, [_P, C.c_int32, C.POINTER(PassStats)]),
    "evplp_profile_kernels": (C.c_int, [_P, C.c_int32]),
    "evplp_profile_passes": (C.c_int, [_P, C.c_int32]),
    "evplp_group_profile_passes": (C.c_int, [_P, C.c_int32]),
    "evplp_debug_counters": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),
    "evplp_debug_splat_bins": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32]),
    "evplp_accel_info": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "evplp_accel_builder": (C.c_int, [_P]),
    "evplp_accel_stack_entries": (C.c_int, [_P]),
    "evplp_selftest": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),
    "evplp_debug_ev_math": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, _P, _P]),
    "evplp_group_create": (C.c_int, [C.POINTER(Config), _P, C.POINTER(_P)]),
    "evplp_group_destroy": (None, [_P]),
    "evplp_group_last_error": (C.c_char_p, [_P]),
    "evplp_group_size": (C.c_int, [_P]),
    "evplp_group_context": (_P, [_P, C.c_int32]),
    "evplp_group_load_scene_json": (C.c_int, [_P, C.c_char_p]),
    "evplp_group_clear_accumulators": (C.c_int, [_P]),
    "evplp_group_primary": (C.c_int, [_P, C.POINTER(C.c_float * 2), C.c_int32]),
    "evplp_group_trace_light_paths": (C.c_int, [_P, C.c_uint32]),
    "evplp_group_gather": (C.c_int, [_P, C.POINTER(FrameParams), C.c_int32]),
    "evplp_group_splat_photons": (C.c_int, [_P, C.POINTER(FrameParams), C.c_int32]),
    "evplp_group_path_trace": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_int32]),
    "evplp_group_path_trace_batch": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_uint32]),
    "evplp_group_path_trace_batch_scratch": (C.c_int, [_P, C.c_uint64]),
    "evplp_group_synchronize": (C.c_int, [_P]),
    "evplp_group_select_rank": (C.c_int, [_P, C.c_int32]),
    "evplp_group_synchronize_rank": (C.c_int, [_P, C.c_int32]),
    "evplp_group_host_stats": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double * 3)]),
    "evplp_group_rebalance": (C.c_int, [_P]),
    "evplp_group_calibrate": (C.c_int, [_P, C.c_int32]),
    "evplp_group_split_model": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(C.c_double * 2)]),
    "evplp_group_block_owners": (C.c_int, [_P, _P, C.c_int32]),
    "evplp_group_resolve": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, _P]),
    "evplp_group_present": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32]),
    "evplp_group_present_ex": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_int32]),
    "evplp_group_set_error_reference": (C.c_int, [_P, _P, _P]),
    "evplp_group_frame_error": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, C.POINTER(C.c_double * 3)]),
    "evplp_group_noise_track": (C.c_int, [_P, C.c_int32, _P]),
    "evplp_group_noise_fold": (C.c_int, [_P, C.c_int32]),
    "evplp_group_noise_estimate": (C.c_int, [_P, C.c_float, C.c_float, C.c_int32, C.POINTER(C.c_double * 3)]),
    "evplp_group_noise_variance": (C.c_int, [_P, C.c_float, _P]),
    "evplp_group_denoise": (C.c_int, [_P, C.c_float, C.c_float, C.c_int32, C.POINTER(DenoiseParams), _P]),
    "evplp_group_temporal_enable": (C.c_int, [_P, C.c_int32]),
    "evplp_group_temporal_reset": (C.c_int, [_P]),
    "evplp_group_denoise_temporal": (C.c_int, [_P, C.c_float, C.c_float, C.c_int32, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), _P, C.POINTER(TemporalInfo)]),
    "evplp_group_temporal_download": (C.c_int, [_P, C.c_int32, _P]),
    "evplp_group_adaptive_enable": (C.c_int, [_P, C.c_int32]),
    "evplp_group_adaptive_enable_pt": (C.c_int, [_P, C.c_int32]),
    "evplp_group_adaptive_retire": (C.c_int, [_P, C.c_float, C.c_float, C.c_int32, C.c_double, C.c_int32]),
    "evplp_group_adaptive_tiles": (C.c_int, [_P, _P, C.c_int32]),
    "evplp_group_adaptive_set_budgets": (C.c_int, [_P, _P, C.c_int32]),
    "evplp_group_adaptive_budgets": (C.c_int, [_P, _P, C.c_int32]),
    "evplp_group_adaptive_budget_window": (C.c_int, [_P, C.c_int32]),
    "evplp_group_adaptive_tile_noise": (C.c_int, [_P, C.c_float, C.c_float, C.c_int32, _P, C.c_int32]),
    "evplp_jitter_sequence": (C.c_int, [C.c_uint32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "evplp_json_query": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int32, C.POINTER(C.c_double), C.c_char_p, C.c_int32]),
    "evplp_progressive_step": (None, [C.c_int32, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.POINTER(C.c_float),
                                      C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "evplp_save_image": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32, _P]),
    "evplp_load_pfm": (C.c_int, [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, C.c_size_t]),
    "evplp_load_image": (C.c_int, [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, C.c_size_t]),
    "evplp_image_error_heat": (C.c_int, [C.c_int32, _P, _P, C.c_float, C.c_int32, _P]),
    "evplp_decode_image": (C.c_int, [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, C.c_size_t]),
    "evplp_image_mse": (C.c_double, [C.c_int32, _P, _P]),
    "evplp_image_rel_mse": (C.c_double, [C.c_int32, _P, _P]),
    "evplp_image_rel_mse_masked": (C.c_double, [C.c_int32, _P, _P, _P]),
    "evplp_synth_scene": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int32, C.c_uint32, C.c_int32, C.c_int32]),
    "evplp_synth_scene_ex": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32]),
    "evplp_render_json": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int32, C.c_char_p, C.c_size_t]),
}

_lib = None


class EvplpError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"evplp status {status}: {message}")
        self.status = status


def lib() -> C.CDLL:
    """Load libevplp_hip.so (built in-tree by `make` / __graft_entry__.build()).  Fails loudly."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `make` (or __graft_entry__.build()) first; "
                              "evplp_amd has no fallback implementation")
        l = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(l, name)  # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        if l.evplp_abi_version() != ABI_VERSION:
            raise ImportError("libevplp_hip.so ABI version mismatch")
        _lib = l
    return _lib


class ProbeParams(C.Structure):
    """evplp_probe_params"""
    _fields_ = [("num_vpl_light_paths", C.c_uint32), ("photons_per_path", C.c_uint32), ("min_distance", C.c_float), ("flags", C.c_uint32)]


def probe_pair(record, x, min_distance: float) -> np.ndarray:
    """evplp_probe_pair (host only): the term of one RECORD_DTYPE record at point x with visibility 1, float32 [9, 3], not divided"""
    r = np.ascontiguousarray(np.asarray(record, dtype=RECORD_DTYPE).reshape(1))
    p = _f32(x).reshape(3)
    out = np.zeros((9, 3), np.float32)
    lib().evplp_probe_pair(_ptr(r), _ptr(p), float(min_distance), _ptr(out))
    return out


def sh_basis(direction) -> np.ndarray:
    """evplp_sh_basis (host only): Y_0 .. Y_8 of a direction (not normalised), float32 [9]"""
    d = _f32(direction).reshape(3)
    y = np.zeros(9, np.float32)
    lib().evplp_sh_basis(_ptr(d), _ptr(y))
    return y


def sh_irradiance(sh, normal) -> np.ndarray:
    """evplp_sh_irradiance (host only): the irradiance (rgb, float32 [3]) of one PROBE_SH_DTYPE element on a surface of unit normal"""
    s = np.ascontiguousarray(np.asarray(sh, dtype=PROBE_SH_DTYPE).reshape(1))
    n = _f32(normal).reshape(3)
    rgb = np.zeros(3, np.float32)
    lib().evplp_sh_irradiance(_ptr(s), _ptr(n), _ptr(rgb))
    return rgb


class LightmapParams(C.Structure):
    """evplp_lightmap_params"""
    _fields_ = [("mesh", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("samples", C.c_int32), ("gutter", C.c_int32), ("flags", C.c_uint32)]


class KnnParams(C.Structure):
    """evplp_knn_params"""
    _fields_ = [("k", C.c_uint32), ("r_min", C.c_float), ("alpha", C.c_float), ("flags", C.c_uint32)]


def lightmap_cover(uv6, width: int, height: int, samples: int, x: int, y: int, i: int, j: int):
    """evplp_lightmap_cover (host only): (beta, gamma) where sample (i, j) of texel (x, y) is covered by the triangle uv6 (u0 v0 u1 v1 u2 v2), else None"""
    uv = _f32(uv6).reshape(6)
    b, g = C.c_float(), C.c_float()
    if not lib().evplp_lightmap_cover(_ptr(uv), int(width), int(height), int(samples), int(x), int(y), int(i), int(j), C.byref(b), C.byref(g)):
        return None
    return b.value, g.value


def _is_device(t) -> bool:
    return getattr(t, "is_cuda", False) and hasattr(t, "data_ptr")


def _device_uvs(uvs, device):
    """uvs for a _device form: None, or a contiguous float32 tensor [k, 6] on `device`"""
    if uvs is None:
        return None
    import torch
    if not _is_device(uvs):
        uvs = torch.as_tensor(np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 6), device=device)
    if uvs.dtype != torch.float32 or uvs.dim() != 2 or uvs.shape[1] != 6:
        raise ValueError(f"uvs must be a float32 tensor [triangles, 6], not {uvs.dtype} {tuple(uvs.shape)}")
    return uvs.contiguous()


def photon_grid_plan(radius: float, box_lo, box_hi, usable_photons: int):
    """evplp_photon_grid_plan (host only): (edge, bits) of the surface gather's photon grid, or None where the call refuses"""
    lo, hi = _f32(box_lo).reshape(3), _f32(box_hi).reshape(3)
    edge, bits = C.c_float(), C.c_uint32()
    if lib().evplp_photon_grid_plan(float(radius), _ptr(lo), _ptr(hi), int(usable_photons), C.byref(edge), C.byref(bits)) != OK:
        return None
    return edge.value, bits.value


def photon_grid_cell(p, box_lo, edge: float, bits: int):
    """evplp_photon_grid_cell (host only): (cell int32 [3], bucket) of a position"""
    x, lo = _f32(p).reshape(3), _f32(box_lo).reshape(3)
    cell = np.zeros(3, np.int32)
    bucket = lib().evplp_photon_grid_cell(_ptr(x), _ptr(lo), float(edge), int(bits), _ptr(cell))
    return cell, int(bucket)


def photon_grid_range(x, radius: float, box_lo, box_hi, edge: float):
    """evplp_photon_grid_range (host only): (walked, cell_lo int32 [3], cell_hi int32 [3]) of a point; walked False: farther than the
    reach from the box on some axis, no cell is visited"""
    p, lo, hi = _f32(x).reshape(3), _f32(box_lo).reshape(3), _f32(box_hi).reshape(3)
    c0, c1 = np.zeros(3, np.int32), np.zeros(3, np.int32)
    walked = lib().evplp_photon_grid_range(_ptr(p), float(radius), _ptr(lo), _ptr(hi), float(edge), _ptr(c0), _ptr(c1))
    return bool(walked), c0, c1


def surface_state_update(state, m: int, phi, alpha: float, r0sq: float) -> np.ndarray:
    """evplp_surface_state_update (host only): one SURFACE_STATE_DTYPE element after one photon half that found m photons of summed value
    phi (float32 [3]) -- flagged and otherwise unchanged where its radius2 is out of range for r0sq -- as a new one-element array"""
    s = np.array(np.asarray(state, dtype=SURFACE_STATE_DTYPE).reshape(1), copy=True)
    p = _f32(phi).reshape(3)
    if lib().evplp_surface_state_update(_ptr(s), int(m), _ptr(p), float(alpha), float(r0sq)) != OK:
        raise ValueError("evplp_surface_state_update refused its arguments")
    return s


def surface_state_resolve(state) -> np.ndarray:
    """evplp_surface_state_resolve (host only): one SURFACE_STATE_DTYPE element as a one-element SURFACE_LIGHT_DTYPE array"""
    s = np.ascontiguousarray(np.asarray(state, dtype=SURFACE_STATE_DTYPE).reshape(1))
    out = np.zeros(1, SURFACE_LIGHT_DTYPE)
    if lib().evplp_surface_state_resolve(_ptr(s), _ptr(out)) != OK:
        raise ValueError("evplp_surface_state_resolve refused its arguments")
    return out


def knn_radius2(d2, k: int, rminsq: float, r0sq: float):
    """evplp_knn_radius2 (host only): (radius2, m) -- the k-th smallest of the float32 values d2 that pass !(d2 > r0sq), clamped into
    [rminsq, r0sq] (r0sq where there are fewer than k), as a numpy float32 scalar, and the number of them that pass !(d2 > radius2)"""
    a = _f32(d2).reshape(-1)
    r, m = C.c_float(), C.c_uint32()
    if lib().evplp_knn_radius2(_ptr(a) if a.size else None, a.size, int(k), float(rminsq), float(r0sq), C.byref(r), C.byref(m)) != OK:
        raise ValueError("evplp_knn_radius2 refused its arguments")
    return np.float32(r.value), int(m.value)


def surface_state_seed(state, radius2: float, m: int, phi, alpha: float, r0sq: float) -> np.ndarray:
    """evplp_surface_state_seed (host only): one SURFACE_STATE_DTYPE element with pm_calls == 0 after a first photon half at radius2 that
    found m photons of summed value phi (float32 [3]), as a new one-element array; ValueError for a state that is not fresh in that sense"""
    s = np.array(np.asarray(state, dtype=SURFACE_STATE_DTYPE).reshape(1), copy=True)
    p = _f32(phi).reshape(3)
    if lib().evplp_surface_state_seed(_ptr(s), float(radius2), int(m), _ptr(p), float(alpha), float(r0sq)) != OK:
        raise ValueError("evplp_surface_state_seed refused its arguments")
    return s


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _host_rays(rays) -> np.ndarray:
    """a batch of evplp_ray as a contiguous float32 array [n, 8]: origin, tmin, direction, tmax"""
    r = np.ascontiguousarray(rays, dtype=np.float32)
    if r.ndim != 2 or r.shape[1] != 8:
        raise ValueError(f"rays must be [n, 8] float32 (origin, tmin, direction, tmax), not {r.shape}")
    return r


def _device_rays(rays):
    """a torch tensor on the device as a batch of evplp_ray (contiguous float32 [n, 8]), or None for anything else"""
    if not (getattr(rays, "is_cuda", False) and hasattr(rays, "data_ptr")):
        return None
    import torch
    if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8:
        raise ValueError(f"rays must be a float32 tensor [n, 8] (origin, tmin, direction, tmax), not {rays.dtype} {tuple(rays.shape)}")
    return rays.contiguous()


def _error_reference(rgb, mask, W: int, H: int):
    """The arguments of set_error_reference, checked before any C call: rgb float32 (H, W, 3) top-down (None releases), mask uint8 (H, W, 3)."""
    if rgb is None:
        if mask is not None:
            raise ValueError("set_error_reference: a mask without a reference image")
        return None, None
    if not isinstance(rgb, np.ndarray) or rgb.dtype != np.float32 or rgb.shape != (H, W, 3):
        raise ValueError(f"set_error_reference: the reference must be float32 of shape {(H, W, 3)}, got "
                         f"{getattr(rgb, 'dtype', type(rgb).__name__)} {getattr(rgb, 'shape', None)}")
    if mask is not None and (not isinstance(mask, np.ndarray) or mask.dtype != np.uint8 or mask.shape != (H, W, 3)):
        raise ValueError(f"set_error_reference: the mask must be uint8 of shape {(H, W, 3)}, got "
                         f"{getattr(mask, 'dtype', type(mask).__name__)} {getattr(mask, 'shape', None)}")
    return np.ascontiguousarray(rgb), None if mask is None else np.ascontiguousarray(mask)


def _noise_track_args(on, mask, W: int, H: int):
    """The arguments of noise_track, checked before any C call: on a bool, mask uint8 (H, W, 3) top-down or None (only with on)."""
    if not isinstance(on, (bool, int, np.bool_)):
        raise ValueError(f"noise_track: on must be a bool, got {type(on).__name__}")
    if mask is not None:
        if not on:
            raise ValueError("noise_track: a mask without tracking")
        if not isinstance(mask, np.ndarray) or mask.dtype != np.uint8 or mask.shape != (H, W, 3):
            raise ValueError(f"noise_track: the mask must be uint8 of shape {(H, W, 3)}, got "
                             f"{getattr(mask, 'dtype', type(mask).__name__)} {getattr(mask, 'shape', None)}")
        mask = np.ascontiguousarray(mask)
    return int(bool(on)), mask


def _denoise_params(levels, sigma_luminance, sigma_normal, sigma_position) -> DenoiseParams:
    """evplp_denoise_params from the keyword arguments of denoise (0 = the default; the library checks the ranges)"""
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)):
        raise ValueError(f"denoise: levels must be an int, got {levels!r}")
    return DenoiseParams(int(levels), float(sigma_luminance), float(sigma_normal), float(sigma_position))


def _temporal_params(max_history, normal_cos) -> TemporalParams:
    """evplp_temporal_params from the keyword arguments of denoise_temporal (0 = the default; the library checks the ranges)"""
    if isinstance(max_history, bool) or not isinstance(max_history, (int, np.integer)):
        raise ValueError(f"denoise_temporal: max_history must be an int, got {max_history!r}")
    return TemporalParams(int(max_history), float(normal_cos))


def _camera(origin, lookat, up, fovy, aspect) -> Camera:
    cam = Camera()
    cam.origin = (C.c_float * 3)(*[float(x) for x in origin]); cam.lookat = (C.c_float * 3)(*[float(x) for x in lookat])
    cam.up = (C.c_float * 3)(*[float(x) for x in up]); cam.fovy = float(fovy); cam.aspect = float(aspect)
    return cam


def project_points(origin, lookat, up, fovy, aspect, W: int, H: int, pts) -> np.ndarray:
    """evplp_project_points: the world points (n, 3) on the screen of a camera (set_camera's arguments) at W x H pixels -> (n, 3) float32
    (x, y, view depth) in pixel-centre coordinates, y from the bottom; depth <= 0: at or behind the eye, x = y = 0.  No GPU."""
    p = _f32(pts).reshape(-1, 3)
    out = np.empty_like(p)
    cam = _camera(origin, lookat, up, fovy, aspect)
    rc = lib().evplp_project_points(C.byref(cam), int(W), int(H), _ptr(p), p.shape[0], _ptr(out))
    if rc < 0:
        raise EvplpError(rc, "evplp_project_points: bad arguments")
    return out


def _fold_iterations(iterations) -> int:
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or iterations < 1:
        raise ValueError(f"noise_fold: iterations must be an int >= 1, got {iterations!r}")
    return int(iterations)


def _adaptive_retire_args(tile_rel_mse, min_batches):
    """adaptive_retire's thresholds, checked before any C call: tile_rel_mse a number >= 0, min_batches an int >= 2"""
    if isinstance(tile_rel_mse, (bool, np.bool_)) or not isinstance(tile_rel_mse, (int, float, np.integer, np.floating)) or not tile_rel_mse >= 0.0:
        raise ValueError(f"adaptive_retire: tile_rel_mse must be a number >= 0, got {tile_rel_mse!r}")
    if isinstance(min_batches, (bool, np.bool_)) or not isinstance(min_batches, (int, np.integer)) or min_batches < 2:
        raise ValueError(f"adaptive_retire: min_batches must be an int >= 2, got {min_batches!r}")
    return float(tile_rel_mse), int(min_batches)


def frame_params(camera_pos, mis_mode=0, pdf_mc=0.0, clamping_value=0.0, photon_radius=0.0, vsl_radius=0.0,
                 vsl_inv_pi_radius2=0.0, num_light_paths=1, num_vpl_light_paths=1, photons_per_path=1,
                 do_accumulate=0, rng_seed=0, jitter=(0.0, 0.0), splat_footprint=0) -> FrameParams:
    fp = FrameParams()
    fp.camera_pos = (C.c_float * 3)(*[float(x) for x in camera_pos])
    fp.mis_mode = MIS_MODES[mis_mode] if isinstance(mis_mode, str) else int(mis_mode)
    fp.pdf_mc = pdf_mc; fp.clamping_value = clamping_value; fp.photon_radius = photon_radius
    fp.vsl_radius = vsl_radius; fp.vsl_inv_pi_radius2 = vsl_inv_pi_radius2
    fp.num_light_paths = num_light_paths; fp.num_vpl_light_paths = num_vpl_light_paths
    fp.photons_per_path = photons_per_path; fp.do_accumulate = do_accumulate; fp.rng_seed = rng_seed
    fp.jitter = (C.c_float * 2)(float(jitter[0]), float(jitter[1]))
    fp.splat_footprint = FOOTPRINTS[splat_footprint] if isinstance(splat_footprint, str) else int(splat_footprint)
    return fp


def default_splat_proxy():
    """(vertices float32 [42, 3], triangles int32 [80, 3]) of the proxy EVPLP_FOOTPRINT_PROXY uses when no mesh was given."""
    v = np.zeros((42, 3), dtype=np.float32); t = np.zeros((80, 3), dtype=np.int32)
    n = lib().evplp_default_splat_proxy(_ptr(v), _ptr(t))
    assert n == 80
    return v, t


def _batch_arrays(jitters, rng_seeds):
    """(samples, jitters [S][2] float32, seeds [S] uint32) of a path_trace_batch call; the C side checks the count"""
    j = np.ascontiguousarray(np.asarray(jitters, np.float32).reshape(-1, 2))
    r = np.ascontiguousarray(np.asarray(rng_seeds, np.uint32).reshape(-1))
    if len(j) != len(r):
        raise ValueError(f"path_trace_batch: {len(j)} jitters but {len(r)} seeds")
    return len(r), j, r


class Context:
    """One GPU's share of a frame (thin RAII wrapper over evplp_context)."""

    def __init__(self, res_x: int, res_y: int, num_light_paths: int, num_vpl_light_paths: int, photons_per_path: int,
                 device: int = 0, strip_rank: int = 0, strip_count: int = 1, strip_rows: int = 16,
                 bvh_builder: int = BVH_SAH, deterministic: bool = False, gather_splits_per_wave: int = 0, overlap_light_tracing: bool = False,
                 strip_capacity_rows: int = 0, cut_scratch_bytes: int = 0, vsl_mask_bytes: int = 0):
        self._lib = lib()
        cfg = Config()
        cfg.abi_version = ABI_VERSION; cfg.device = device; cfg.res_x = res_x; cfg.res_y = res_y
        cfg.strip_rank = strip_rank; cfg.strip_count = strip_count; cfg.strip_rows = strip_rows
        cfg.num_light_paths = num_light_paths; cfg.num_vpl_light_paths = num_vpl_light_paths
        cfg.photons_per_path = photons_per_path; cfg.bvh_builder = bvh_builder; cfg.deterministic = int(deterministic)
        cfg.gather_splits_per_wave = gather_splits_per_wave
        cfg.overlap_light_tracing = int(overlap_light_tracing); cfg.strip_capacity_rows = int(strip_capacity_rows)
        cfg.cut_scratch_bytes = int(cut_scratch_bytes); cfg.vsl_mask_bytes = int(vsl_mask_bytes)
        self.cfg = cfg
        h = C.c_void_p()
        rc = self._lib.evplp_create(C.byref(cfg), C.byref(h))
        if rc != OK:
            raise EvplpError(rc, self._lib.evplp_last_error(None).decode())
        self._h = h
        self.W, self.H = res_x, res_y
        self.local_rows = self._lib.evplp_local_rows(h)
        self.num_records = num_light_paths * photons_per_path

    @classmethod
    def borrowed(cls, handle, res_x: int, res_y: int, strip_rank: int = 0, strip_count: int = 1, strip_rows: int = 8,
                 num_light_paths: int = 0, num_vpl_light_paths: int = 0, photons_per_path: int = 0):
        """A view of a context somebody else owns (a rank of an evplp_group): statistics and buffers; close() does not destroy it."""
        self = cls.__new__(cls)
        self._lib = lib(); self._h = C.c_void_p(handle); self._borrowed = True
        self.cfg = Config(); self.cfg.strip_rank = strip_rank; self.cfg.strip_count = strip_count; self.cfg.strip_rows = strip_rows
        self.cfg.abi_version = ABI_VERSION; self.cfg.res_x = res_x; self.cfg.res_y = res_y
        self.cfg.num_light_paths = num_light_paths; self.cfg.num_vpl_light_paths = num_vpl_light_paths; self.cfg.photons_per_path = photons_per_path
        self.num_records = num_light_paths * photons_per_path
        self.W, self.H = res_x, res_y
        self.local_rows = self._lib.evplp_local_rows(self._h)
        return self

    # -- plumbing
    def _check(self, rc: int) -> int:
        if rc < 0:
            raise EvplpError(rc, self._lib.evplp_last_error(self._h).decode())
        return rc

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                self._lib.evplp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- scene
    def add_texture(self, rgba: np.ndarray) -> int:
        rgba = _f32(rgba)
        h, w = rgba.shape[:2]
        return self._check(self._lib.evplp_add_texture(self._h, w, h, _ptr(rgba)))

    def add_material(self, kd, ks, ns, tex_kd=-1, tex_ks=-1, tex_ns=-1) -> int:
        m = Material()
        m.kd = (C.c_float * 3)(*[float(x) for x in kd]); m.ks = (C.c_float * 3)(*[float(x) for x in ks]); m.ns = float(ns)
        m.tex_kd, m.tex_ks, m.tex_ns = tex_kd, tex_ks, tex_ns
        return self._check(self._lib.evplp_add_material(self._h, C.byref(m)))

    def add_mesh(self, vertices, indices, material: int, texcoords=None) -> int:
        v = _f32(vertices).reshape(-1, 3)
        i = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
        t = None if texcoords is None else _f32(texcoords).reshape(-1, 2)
        return self._check(self._lib.evplp_add_mesh(self._h, _ptr(v), _ptr(t), v.shape[0], _ptr(i), i.shape[0], material))

    def set_arealight(self, mesh: int, intensity: Sequence[float]):
        arr = (C.c_float * 4)(*[float(x) for x in intensity])
        self._check(self._lib.evplp_set_arealight(self._h, mesh, C.byref(arr)))

    def set_camera(self, origin, lookat, up, fovy: float, aspect: float):
        cam = Camera()
        cam.origin = (C.c_float * 3)(*[float(x) for x in origin]); cam.lookat = (C.c_float * 3)(*[float(x) for x in lookat])
        cam.up = (C.c_float * 3)(*[float(x) for x in up]); cam.fovy = float(fovy); cam.aspect = float(aspect)
        self._check(self._lib.evplp_set_camera(self._h, C.byref(cam)))

    def build_accel(self):
        self._check(self._lib.evplp_build_accel(self._h))

    def update_mesh(self, mesh: int, vertices):
        """evplp_update_mesh: new positions (n, 3) for mesh `mesh` (same vertex count); every pass is refused until refit_accel / build_accel"""
        v = _f32(vertices).reshape(-1, 3)
        self._check(self._lib.evplp_update_mesh(self._h, int(mesh), _ptr(v), v.shape[0]))

    def transform_mesh(self, mesh: int, m):
        """evplp_transform_mesh: mesh `mesh` = its rest pose under the row-major 3 x 4 matrix m (12 numbers; transforms do not compose);
        dirty like update_mesh, but the refit uploads the matrix alone"""
        m = _f32(m).reshape(12)
        self._check(self._lib.evplp_transform_mesh(self._h, int(mesh), _ptr(m)))

    def set_mesh_skin(self, mesh: int, nbones: int, bone_index=None, weight=None):
        """evplp_set_mesh_skin: four bone indices (n, 4) and four weights (n, 4) per vertex of mesh `mesh` over nbones bones; constant for the
        topology, moves nothing, marks nothing dirty; nbones = 0 removes the skin"""
        if int(nbones) == 0 and bone_index is None and weight is None:
            return self._check(self._lib.evplp_set_mesh_skin(self._h, int(mesh), 0, None, None, 0))
        b = np.ascontiguousarray(bone_index, np.int32).reshape(-1, 4)
        w = _f32(weight).reshape(-1, 4)
        if b.shape != w.shape:
            raise ValueError("set_mesh_skin: bone_index and weight must both be (nverts, 4)")
        self._check(self._lib.evplp_set_mesh_skin(self._h, int(mesh), int(nbones), _ptr(b), _ptr(w), b.shape[0]))

    def pose_mesh(self, mesh: int, bone_matrices):
        """evplp_pose_mesh: mesh `mesh` = its rest pose skinned under the palette (nbones, 12) of row-major 3 x 4 matrices (poses do not
        compose); dirty like update_mesh, but the refit uploads the palette alone"""
        m = _f32(bone_matrices).reshape(-1, 12)
        self._check(self._lib.evplp_pose_mesh(self._h, int(mesh), _ptr(m), m.shape[0]))

    def set_mesh_morph(self, mesh: int, deltas=None):
        """evplp_set_mesh_morph: morph targets (T, nverts, 3) for mesh `mesh`, T = 1 .. 64; constant for the topology, moves nothing, marks
        nothing dirty; None removes the targets.  Refused while weights are in force on the mesh"""
        if deltas is None:
            return self._check(self._lib.evplp_set_mesh_morph(self._h, int(mesh), 0, None, 0))
        d = _f32(deltas)
        if d.ndim != 3 or d.shape[2] != 3:
            raise ValueError("set_mesh_morph: deltas must be (ntargets, nverts, 3)")
        self._check(self._lib.evplp_set_mesh_morph(self._h, int(mesh), d.shape[0], _ptr(d), d.shape[1]))

    def morph_mesh(self, mesh: int, weights=None):
        """evplp_morph_mesh: the base of mesh `mesh` = its rest pose + the weighted deltas (weights do not compose), and its positions that
        base under the matrix or the pose in force; dirty like update_mesh, but the refit uploads the weights alone.  None takes the weights away"""
        if weights is None:
            return self._check(self._lib.evplp_morph_mesh(self._h, int(mesh), None, 0))
        w = _f32(weights).reshape(-1)
        self._check(self._lib.evplp_morph_mesh(self._h, int(mesh), _ptr(w), w.shape[0]))

    def mesh_count(self) -> int:
        return self._check(self._lib.evplp_mesh_count(self._h))

    def mesh_info(self, mesh: int) -> dict:
        """evplp_mesh_info: nverts, ntris, material of mesh `mesh` as the host copy holds it"""
        nv, nt, mat = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._lib.evplp_mesh_info(self._h, int(mesh), C.byref(nv), C.byref(nt), C.byref(mat)))
        return dict(nverts=nv.value, ntris=nt.value, material=mat.value)

    def mesh_vertices(self, mesh: int, which: int = 0):
        """evplp_mesh_vertices: the positions (nverts, 3) of mesh `mesh` in the numbering update_mesh expects; which = 0 current, 1 rest pose, 2 the morphed base"""
        out = np.empty((self.mesh_info(mesh)["nverts"], 3), np.float32)
        self._check(self._lib.evplp_mesh_vertices(self._h, int(mesh), int(which), _ptr(out), out.shape[0]))
        return out

    def refit_accel(self):
        """evplp_refit_accel: the tree, the triangle operands and the scene's figures follow the updated vertices, on the device; the topology stays"""
        self._check(self._lib.evplp_refit_accel(self._h))

    def trace_closest(self, rays, filter: int = 0, order: bool = QUERY_ORDER_DEFAULT):
        """evplp_trace_closest: the closest hit of every ray of a float32 array [n, 8] (origin, tmin, direction, tmax) as a HIT_DTYPE array
        (triangle -1: a miss, -2: an invalid ray); filter 0 all, 1 without the light mesh, 2 the light mesh only; order: the ordering pass.
        A torch tensor on the device goes through evplp_trace_closest_device instead: enqueued on the context's stream, not waited for
        (synchronize() before another stream reads it), and the result is an int32 tensor [n, 4] on the same device holding the hits' bytes
        (t, beta, gamma as float bits: .view(torch.float32))."""
        flags = QUERY_ORDER if order else 0
        d = _device_rays(rays)
        if d is not None:
            import torch
            hits = torch.empty((d.shape[0], 4), dtype=torch.int32, device=d.device)
            self._check(self._lib.evplp_trace_closest_device(self._h, C.c_void_p(d.data_ptr()), int(d.shape[0]), int(filter), flags, C.c_void_p(hits.data_ptr())))
            self._query_inputs = d          # (the launch reads it after this call returns)
            return hits
        r = _host_rays(rays)
        hits = np.zeros(r.shape[0], HIT_DTYPE)
        self._check(self._lib.evplp_trace_closest(self._h, _ptr(r), r.shape[0], int(filter), flags, _ptr(hits)))
        return hits

    def trace_occluded(self, rays, order: bool = QUERY_ORDER_DEFAULT):
        """evplp_trace_occluded: uint8 per ray of a float32 array [n, 8] -- 1 a triangle lies in (tmin, tmax), 0 none does, 2 an invalid ray.
        A torch tensor on the device goes through evplp_trace_occluded_device (see trace_closest) and gives a uint8 tensor."""
        flags = QUERY_ORDER if order else 0
        d = _device_rays(rays)
        if d is not None:
            import torch
            out = torch.empty((d.shape[0],), dtype=torch.uint8, device=d.device)
            self._check(self._lib.evplp_trace_occluded_device(self._h, C.c_void_p(d.data_ptr()), int(d.shape[0]), flags, C.c_void_p(out.data_ptr())))
            self._query_inputs = d
            return out
        r = _host_rays(rays)
        out = np.zeros(r.shape[0], np.uint8)
        self._check(self._lib.evplp_trace_occluded(self._h, _ptr(r), r.shape[0], flags, _ptr(out)))
        return out

    def gather_probes(self, positions, num_vpl_light_paths: int, photons_per_path: int, min_distance: float, flags: int = 0):
        """evplp_gather_probes: the indirect light of the record slots [0, num_vpl_light_paths * photons_per_path) at every point of a
        float32 array [n, 3], as a PROBE_SH_DTYPE array (c[i][rgb] the order-2 SH coefficients of the incident radiance, lit the number of
        lit pairs, -1 for a point with a coordinate that is not finite).  A torch tensor on the device goes through
        evplp_gather_probes_device instead: enqueued on the context's stream, not waited for, and the result is a float32 tensor [n, 28]
        on the same device holding the probes' bytes (27 coefficients, then lit)."""
        prm = ProbeParams(int(num_vpl_light_paths), int(photons_per_path), float(min_distance), int(flags))
        if getattr(positions, "is_cuda", False) and hasattr(positions, "data_ptr"):
            import torch
            if positions.dtype != torch.float32 or positions.dim() != 2 or positions.shape[1] != 3:
                raise ValueError(f"positions must be a float32 tensor [n, 3], not {positions.dtype} {tuple(positions.shape)}")
            d = positions.contiguous()
            out = torch.empty((d.shape[0], 28), dtype=torch.float32, device=d.device)
            self._check(self._lib.evplp_gather_probes_device(self._h, C.byref(prm), C.c_void_p(d.data_ptr()), int(d.shape[0]), C.c_void_p(out.data_ptr())))
            self._query_inputs = d          # (the launch reads it after this call returns)
            return out
        x = np.ascontiguousarray(positions, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != 3:
            raise ValueError(f"positions must be [n, 3] float32, not {x.shape}")
        out = np.zeros(x.shape[0], PROBE_SH_DTYPE)
        self._check(self._lib.evplp_gather_probes(self._h, C.byref(prm), _ptr(x), x.shape[0], _ptr(out)))
        return out

    def gather_surface(self, points, fp: FrameParams, eyes=None, what: int = SURFACE_VPL | SURFACE_PHOTONS):
        """evplp_gather_surface: the VPL sum and the photon estimate at the surface points of a SURFACE_POINT_DTYPE array, as a
        SURFACE_LIGHT_DTYPE array; eyes: float32 [n, 3], or None for fp.camera_pos at every point.  A float32 torch tensor [n, 16] on the
        device (eyes, if any, a tensor [n, 3] there too) goes through evplp_gather_surface_device instead: enqueued on the context's
        stream, not waited for, and the result is a float32 tensor [n, 8] on the same device holding the results' bytes."""
        if getattr(points, "is_cuda", False) and hasattr(points, "data_ptr"):
            import torch
            if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 16:
                raise ValueError(f"points must be a float32 tensor [n, 16], not {points.dtype} {tuple(points.shape)}")
            d = points.contiguous()
            e = None
            if eyes is not None:
                if not getattr(eyes, "is_cuda", False) or eyes.dtype != torch.float32 or tuple(eyes.shape) != (d.shape[0], 3):
                    raise ValueError("eyes must be a float32 tensor [n, 3] on the points' device")
                e = eyes.contiguous()
            out = torch.empty((d.shape[0], 8), dtype=torch.float32, device=d.device)
            self._check(self._lib.evplp_gather_surface_device(self._h, C.byref(fp), int(what), C.c_void_p(d.data_ptr()),
                                                              C.c_void_p(e.data_ptr()) if e is not None else None, int(d.shape[0]), C.c_void_p(out.data_ptr())))
            self._query_inputs = (d, e)     # (the launches read them after this call returns)
            return out
        x = np.ascontiguousarray(points, dtype=SURFACE_POINT_DTYPE).reshape(-1)
        e = None
        if eyes is not None:
            e = np.ascontiguousarray(eyes, dtype=np.float32)
            if e.shape != (x.shape[0], 3):
                raise ValueError(f"eyes must be [n, 3] float32, not {e.shape}")
        out = np.zeros(x.shape[0], SURFACE_LIGHT_DTYPE)
        self._check(self._lib.evplp_gather_surface(self._h, C.byref(fp), int(what), _ptr(x), _ptr(e), x.shape[0], _ptr(out)))
        return out

    def surface_points(self, hits, flags: int = 0, eyes=None):
        """evplp_surface_points: the G-buffer's four float4 at every hit of a HIT_DTYPE array, as a SURFACE_POINT_DTYPE array (valid = 0 and
        zeros for a miss, an invalid ray, a triangle outside the scene or without area, a beta or gamma that is not finite); flags:
        POINTS_WHITE, POINTS_FACE_EYES (then eyes: float32 [n, 3]).  An int32 torch tensor [n, 4] on the device (trace_closest's result;
        eyes a float32 tensor [n, 3] there too) goes through evplp_surface_points_device instead: enqueued on the context's stream, not
        waited for, and the result is a float32 tensor [n, 16] on the same device -- what gather_surface takes."""
        if _is_device(hits):
            import torch
            if hits.dtype not in (torch.int32, torch.float32) or hits.dim() != 2 or hits.shape[1] != 4:
                raise ValueError(f"hits must be an int32 (or float32) tensor [n, 4], not {hits.dtype} {tuple(hits.shape)}")
            d = hits.contiguous()
            e = None
            if eyes is not None:
                if not _is_device(eyes) or eyes.dtype != torch.float32 or tuple(eyes.shape) != (d.shape[0], 3):
                    raise ValueError("eyes must be a float32 tensor [n, 3] on the hits' device")
                e = eyes.contiguous()
            out = torch.empty((d.shape[0], 16), dtype=torch.float32, device=d.device)
            self._check(self._lib.evplp_surface_points_device(self._h, C.c_void_p(d.data_ptr()), int(d.shape[0]), int(flags),
                                                              C.c_void_p(e.data_ptr()) if e is not None else None, C.c_void_p(out.data_ptr())))
            self._query_inputs = (d, e)     # (the launches read them after this call returns)
            return out
        h = np.ascontiguousarray(hits, dtype=HIT_DTYPE).reshape(-1)
        e = None
        if eyes is not None:
            e = np.ascontiguousarray(eyes, dtype=np.float32)
            if e.shape != (h.shape[0], 3):
                raise ValueError(f"eyes must be [n, 3] float32, not {e.shape}")
        out = np.zeros(h.shape[0], SURFACE_POINT_DTYPE)
        self._check(self._lib.evplp_surface_points(self._h, _ptr(h), h.shape[0], int(flags), _ptr(e), _ptr(out)))
        return out

    def surface_points_device(self, hits, flags: int = 0, eyes=None):
        """surface_points for tensors on the device (evplp_surface_points_device); a tensor is required"""
        if not _is_device(hits):
            raise ValueError("hits must be a tensor on the device")
        return self.surface_points(hits, flags, eyes)

    def lightmap_samples(self, width: int, height: int, samples: int = 1, mesh: int = -1, uvs=None):
        """evplp_lightmap_samples: for every sample of a width x height atlas the covering triangle of mesh `mesh` (-1: of the scene) as a
        HIT_DTYPE array [height, width, samples, samples] (row 0 at v = 0; triangle -1: uncovered; t = 0); uvs: float32 [triangles of the
        selection, 6], or None for the meshes' own texcoords"""
        u = None if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 6)
        out = np.zeros((int(height), int(width), int(samples), int(samples)), HIT_DTYPE) if min(int(width), int(height), int(samples)) > 0 else np.zeros((0, 0, 0, 0), HIT_DTYPE)
        self._check(self._lib.evplp_lightmap_samples(self._h, int(mesh), _ptr(u), int(width), int(height), int(samples), _ptr(out) if out.size else None))
        return out

    def lightmap_samples_device(self, width: int, height: int, samples: int = 1, mesh: int = -1, uvs=None, device=None):
        """evplp_lightmap_samples_device: as lightmap_samples, the result an int32 tensor [height * width * samples^2, 4] on the device holding
        the hits' bytes (surface_points takes it); uvs: None, an array, or a float32 tensor [triangles, 6] on the device.  Waits once per
        band for the size of the tiles' lists, and for nothing else."""
        import torch
        dev = device if device is not None else (uvs.device if _is_device(uvs) else torch.device("cuda", self.cfg.device))
        u = _device_uvs(uvs, dev)
        n = max(int(width), 0) * max(int(height), 0) * max(int(samples), 0) ** 2
        out = torch.empty((n, 4), dtype=torch.int32, device=dev)
        self._check(self._lib.evplp_lightmap_samples_device(self._h, int(mesh), C.c_void_p(u.data_ptr()) if u is not None else None, int(width), int(height),
                                                            int(samples), C.c_void_p(out.data_ptr()) if n else None))
        self._query_inputs = u
        return out

    def bake_lightmap(self, fp: FrameParams, width: int, height: int, samples: int = 1, mesh: int = -1, gutter: int = 0, flags: int = 0, uvs=None,
                      what: int = SURFACE_VPL | SURFACE_PHOTONS):
        """evplp_bake_lightmap: the atlas of mesh `mesh` (-1: of the scene) lit by the records, as a LIGHTMAP_TEXEL_DTYPE array [height, width]
        (row 0 at v = 0): per texel the mean of the surface gather's two estimates over its covered samples, coverage = their share
        (-d where the gutter's pass d filled the texel); flags: POINTS_WHITE or 0"""
        prm = LightmapParams(int(mesh), int(width), int(height), int(samples), int(gutter), int(flags))
        u = None if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 6)
        out = np.zeros((max(int(height), 0), max(int(width), 0)), LIGHTMAP_TEXEL_DTYPE)
        self._check(self._lib.evplp_bake_lightmap(self._h, C.byref(fp), int(what), C.byref(prm), _ptr(u), _ptr(out) if out.size else None))
        return out

    def bake_lightmap_device(self, fp: FrameParams, width: int, height: int, samples: int = 1, mesh: int = -1, gutter: int = 0, flags: int = 0, uvs=None,
                             what: int = SURFACE_VPL | SURFACE_PHOTONS, device=None):
        """evplp_bake_lightmap_device: as bake_lightmap, the result a float32 tensor [height, width, 8] on the device holding the texels' bytes;
        enqueued on the context's stream behind one wait per band (the tiles' lists), not waited for at the end"""
        import torch
        dev = device if device is not None else (uvs.device if _is_device(uvs) else torch.device("cuda", self.cfg.device))
        u = _device_uvs(uvs, dev)
        prm = LightmapParams(int(mesh), int(width), int(height), int(samples), int(gutter), int(flags))
        out = torch.empty((max(int(height), 0), max(int(width), 0), 8), dtype=torch.float32, device=dev)
        self._check(self._lib.evplp_bake_lightmap_device(self._h, C.byref(fp), int(what), C.byref(prm), C.c_void_p(u.data_ptr()) if u is not None else None,
                                                         C.c_void_p(out.data_ptr()) if out.numel() else None))
        self._query_inputs = u
        return out

    def gather_surface_progressive(self, points, fp: FrameParams, states, alpha: float = 2.0 / 3.0, eyes=None, what: int = SURFACE_VPL | SURFACE_PHOTONS):
        """evplp_gather_surface_progressive: one iteration of the records into the points' states (mis_mode 0, 4, 5).  points, eyes as
        gather_surface takes them; states: a SURFACE_STATE_DTYPE array (np.zeros is fresh), returned as a new array -- or, with points a
        float32 tensor [n, 16] on the device, a float32 tensor [n, 12] there holding the states' bytes (torch.zeros is fresh), updated IN
        PLACE through evplp_gather_surface_progressive_device: enqueued on the context's stream, not waited for, and returned."""
        if _is_device(points):
            import torch
            if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 16:
                raise ValueError(f"points must be a float32 tensor [n, 16], not {points.dtype} {tuple(points.shape)}")
            d = points.contiguous()
            if not _is_device(states) or states.dtype != torch.float32 or tuple(states.shape) != (d.shape[0], 12) or not states.is_contiguous():
                raise ValueError("states must be a contiguous float32 tensor [n, 12] on the points' device")
            e = None
            if eyes is not None:
                if not _is_device(eyes) or eyes.dtype != torch.float32 or tuple(eyes.shape) != (d.shape[0], 3):
                    raise ValueError("eyes must be a float32 tensor [n, 3] on the points' device")
                e = eyes.contiguous()
            self._check(self._lib.evplp_gather_surface_progressive_device(self._h, C.byref(fp), int(what), float(alpha), C.c_void_p(d.data_ptr()),
                                                                          C.c_void_p(e.data_ptr()) if e is not None else None, int(d.shape[0]),
                                                                          C.c_void_p(states.data_ptr()) if d.shape[0] else None))
            self._query_inputs = (d, e, states)     # (the launches read them after this call returns)
            return states
        x = np.ascontiguousarray(points, dtype=SURFACE_POINT_DTYPE).reshape(-1)
        e = None
        if eyes is not None:
            e = np.ascontiguousarray(eyes, dtype=np.float32)
            if e.shape != (x.shape[0], 3):
                raise ValueError(f"eyes must be [n, 3] float32, not {e.shape}")
        s = np.array(np.asarray(states, dtype=SURFACE_STATE_DTYPE).reshape(-1), copy=True)
        if s.shape[0] != x.shape[0]:
            raise ValueError(f"{s.shape[0]} states for {x.shape[0]} points")
        self._check(self._lib.evplp_gather_surface_progressive(self._h, C.byref(fp), int(what), float(alpha), _ptr(x), _ptr(e), x.shape[0], _ptr(s)))
        return s

    def gather_surface_knn(self, points, fp: FrameParams, states, k: int, r_min: float, alpha: float = 2.0 / 3.0, eyes=None, flags: int = 0):
        """evplp_gather_surface_knn: the first photon half of the states with pm_calls == 0, each at the distance of its point's k-th nearest
        photon within fp.photon_radius (not below r_min).  points, eyes, states and what is returned as gather_surface_progressive: numpy
        arrays give a new array; a float32 tensor [n, 16] on the device with a float32 tensor [n, 12] of states there goes through
        evplp_gather_surface_knn_device, in place, enqueued and not waited for."""
        prm = KnnParams(int(k), float(r_min), float(alpha), int(flags))
        if _is_device(points):
            import torch
            if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 16:
                raise ValueError(f"points must be a float32 tensor [n, 16], not {points.dtype} {tuple(points.shape)}")
            d = points.contiguous()
            if not _is_device(states) or states.dtype != torch.float32 or tuple(states.shape) != (d.shape[0], 12) or not states.is_contiguous():
                raise ValueError("states must be a contiguous float32 tensor [n, 12] on the points' device")
            e = None
            if eyes is not None:
                if not _is_device(eyes) or eyes.dtype != torch.float32 or tuple(eyes.shape) != (d.shape[0], 3):
                    raise ValueError("eyes must be a float32 tensor [n, 3] on the points' device")
                e = eyes.contiguous()
            self._check(self._lib.evplp_gather_surface_knn_device(self._h, C.byref(fp), C.byref(prm), C.c_void_p(d.data_ptr()),
                                                                  C.c_void_p(e.data_ptr()) if e is not None else None, int(d.shape[0]),
                                                                  C.c_void_p(states.data_ptr()) if d.shape[0] else None))
            self._query_inputs = (d, e, states)     # (the launches read them after this call returns)
            return states
        x = np.ascontiguousarray(points, dtype=SURFACE_POINT_DTYPE).reshape(-1)
        e = None
        if eyes is not None:
            e = np.ascontiguousarray(eyes, dtype=np.float32)
            if e.shape != (x.shape[0], 3):
                raise ValueError(f"eyes must be [n, 3] float32, not {e.shape}")
        s = np.array(np.asarray(states, dtype=SURFACE_STATE_DTYPE).reshape(-1), copy=True)
        if s.shape[0] != x.shape[0]:
            raise ValueError(f"{s.shape[0]} states for {x.shape[0]} points")
        self._check(self._lib.evplp_gather_surface_knn(self._h, C.byref(fp), C.byref(prm), _ptr(x), _ptr(e), x.shape[0], _ptr(s)))
        return s

    def bake_lightmap_knn(self, fp: FrameParams, states, width: int, height: int, samples: int = 1, k: int = 8, r_min: float = 0.0, alpha: float = 2.0 / 3.0,
                          mesh: int = -1, flags: int = 0, uvs=None):
        """evplp_bake_lightmap_knn_device: gather_surface_knn over the atlas' samples into their states, a contiguous float32 tensor
        [height * width * samples^2, 12] on the device (torch.zeros is fresh), updated in place and returned; waits once per band"""
        import torch
        n = max(int(width), 0) * max(int(height), 0) * max(int(samples), 0) ** 2
        if not _is_device(states) or states.dtype != torch.float32 or tuple(states.shape) != (n, 12) or not states.is_contiguous():
            raise ValueError(f"states must be a contiguous float32 tensor [{n}, 12] on the device")
        u = _device_uvs(uvs, states.device)
        prm = LightmapParams(int(mesh), int(width), int(height), int(samples), 0, int(flags))
        knn = KnnParams(int(k), float(r_min), float(alpha), 0)
        self._check(self._lib.evplp_bake_lightmap_knn_device(self._h, C.byref(fp), C.byref(knn), C.byref(prm),
                                                             C.c_void_p(u.data_ptr()) if u is not None else None, C.c_void_p(states.data_ptr()) if n else None))
        self._query_inputs = (u, states)
        return states

    def surface_resolve(self, states):
        """evplp_surface_resolve: a SURFACE_STATE_DTYPE array as a SURFACE_LIGHT_DTYPE array; a float32 tensor [n, 12] on the device goes
        through evplp_surface_resolve_device (enqueued, not waited for) and gives a float32 tensor [n, 8] there"""
        if _is_device(states):
            import torch
            if states.dtype != torch.float32 or states.dim() != 2 or states.shape[1] != 12:
                raise ValueError(f"states must be a float32 tensor [n, 12], not {states.dtype} {tuple(states.shape)}")
            d = states.contiguous()
            out = torch.empty((d.shape[0], 8), dtype=torch.float32, device=d.device)
            self._check(self._lib.evplp_surface_resolve_device(self._h, C.c_void_p(d.data_ptr()), int(d.shape[0]), C.c_void_p(out.data_ptr())))
            self._query_inputs = d
            return out
        s = np.ascontiguousarray(states, dtype=SURFACE_STATE_DTYPE).reshape(-1)
        out = np.zeros(s.shape[0], SURFACE_LIGHT_DTYPE)
        self._check(self._lib.evplp_surface_resolve(self._h, _ptr(s), s.shape[0], _ptr(out)))
        return out

    def bake_lightmap_progressive_device(self, fp: FrameParams, states, width: int, height: int, samples: int = 1, alpha: float = 2.0 / 3.0, mesh: int = -1,
                                         flags: int = 0, uvs=None, what: int = SURFACE_VPL | SURFACE_PHOTONS):
        """evplp_bake_lightmap_progressive_device: one iteration of the records into the atlas' states, a contiguous float32 tensor
        [height * width * samples^2, 12] on the device (torch.zeros is fresh), updated in place and returned; waits once per band"""
        import torch
        n = max(int(width), 0) * max(int(height), 0) * max(int(samples), 0) ** 2
        if not _is_device(states) or states.dtype != torch.float32 or tuple(states.shape) != (n, 12) or not states.is_contiguous():
            raise ValueError(f"states must be a contiguous float32 tensor [{n}, 12] on the device")
        u = _device_uvs(uvs, states.device)
        prm = LightmapParams(int(mesh), int(width), int(height), int(samples), 0, int(flags))
        self._check(self._lib.evplp_bake_lightmap_progressive_device(self._h, C.byref(fp), int(what), float(alpha), C.byref(prm),
                                                                     C.c_void_p(u.data_ptr()) if u is not None else None, C.c_void_p(states.data_ptr()) if n else None))
        self._query_inputs = (u, states)
        return states

    def bake_lightmap_resolve(self, states, width: int, height: int, samples: int = 1, gutter: int = 0):
        """evplp_bake_lightmap_resolve: the atlas of the states (on the device) as a LIGHTMAP_TEXEL_DTYPE array [height, width]; waits"""
        prm = LightmapParams(-1, int(width), int(height), int(samples), int(gutter), 0)
        out = np.zeros((max(int(height), 0), max(int(width), 0)), LIGHTMAP_TEXEL_DTYPE)
        self._check(self._lib.evplp_bake_lightmap_resolve(self._h, C.byref(prm), C.c_void_p(states.data_ptr()), _ptr(out) if out.size else None))
        return out

    def bake_lightmap_resolve_device(self, states, width: int, height: int, samples: int = 1, gutter: int = 0):
        """evplp_bake_lightmap_resolve_device: as bake_lightmap_resolve, the result a float32 tensor [height, width, 8] on the states' device;
        enqueued, not waited for"""
        import torch
        prm = LightmapParams(-1, int(width), int(height), int(samples), int(gutter), 0)
        out = torch.empty((max(int(height), 0), max(int(width), 0), 8), dtype=torch.float32, device=states.device)
        self._check(self._lib.evplp_bake_lightmap_resolve_device(self._h, C.byref(prm), C.c_void_p(states.data_ptr()), C.c_void_p(out.data_ptr()) if out.numel() else None))
        self._query_inputs = states
        return out

    def triangle_info(self, triangle: int):
        """evplp_triangle_info: (mesh, index within the mesh) of a hit's scene triangle"""
        m, i = C.c_int32(), C.c_int32()
        self._check(self._lib.evplp_triangle_info(self._h, int(triangle), C.byref(m), C.byref(i)))
        return m.value, i.value

    def accel_quality(self) -> dict:
        """evplp_accel_quality: the SAH cost of the tree as it is on the device (cost, root_area, inner_area, leaf_pair_area, leaf_tri_area),
        built_cost, reached_nodes, leaf_refs, refits_since_build, policy_rebuilds, last_action (0 none, 1 refit kept, 2 rebuilt); waits"""
        q = AccelQuality()
        self._check(self._lib.evplp_accel_quality(self._h, C.byref(q)))
        return q.as_dict()

    def set_refit_policy(self, max_cost_ratio: float, rebuild_builder: int = -1):
        """evplp_set_refit_policy: refit_accel rebuilds when the cost exceeds max_cost_ratio x the built tree's (0: off, the default);
        rebuild_builder: a BVH_* value, or -1 for the context's own"""
        self._check(self._lib.evplp_set_refit_policy(self._h, float(max_cost_ratio), int(rebuild_builder)))

    def optimize_accel(self, passes: int = 1) -> int:
        """evplp_optimize_accel: `passes` (1 .. 8) refit sweeps with tree rotations over the tree as it is, then the four-wide nodes; waits.
        Returns the rotations taken."""
        n = C.c_int32(0)
        self._check(self._lib.evplp_optimize_accel(self._h, int(passes), C.byref(n)))
        return n.value

    def set_refit_rotations(self, passes: int):
        """evplp_set_refit_rotations: refit_accel's own sweeps rotate, `passes` of them (0: off, the default); the refit then waits once"""
        self._check(self._lib.evplp_set_refit_rotations(self._h, int(passes)))

    def rotation_info(self) -> dict:
        """evplp_rotation_info: rotations since the build, in the last sweeping call, per pass of it, and the refit's setting"""
        a, b, p, per = C.c_int32(0), C.c_int32(0), C.c_int32(0), np.zeros(8, np.int32)
        self._check(self._lib.evplp_rotation_info(self._h, C.byref(a), C.byref(b), _ptr(per), C.byref(p)))
        return {"since_build": a.value, "last_call": b.value, "per_pass": [int(x) for x in per], "refit_passes": p.value}

    def refit_info(self):
        n, l, ms = C.c_int32(), C.c_int32(), C.c_float()
        self._check(self._lib.evplp_refit_info(self._h, C.byref(n), C.byref(l), C.byref(ms)))
        return {"refits": n.value, "levels": l.value, "last_refit_ms": ms.value}

    def debug_accel(self, which: int) -> np.ndarray:
        """evplp_debug_accel (tests): 0 nodes, 1 leaf blocks, 2 flat triangle operands, 3 slot -> triangle, 4 four-wide nodes (structured arrays
        / int32), 5 the box pad (a float), 6 the last refit's four stage times in ms, 7 the last cost measurement's time in ms (a float)"""
        info = self.accel_info()
        nn, nl = max(info["nodes"], 1), max(info["leaves"], 1)
        out = {0: lambda: np.zeros(nn, ACCEL_NODE), 1: lambda: np.zeros(nl, ACCEL_LEAF), 2: lambda: np.zeros(4 * nl, ACCEL_TRI), 3: lambda: np.zeros(4 * nl, np.int32),
               4: lambda: np.zeros(nn, ACCEL_NODE4), 5: lambda: np.zeros(1, np.float32), 6: lambda: np.zeros(4, np.float32), 7: lambda: np.zeros(1, np.float32)}[which]()
        self._check(self._lib.evplp_debug_accel(self._h, which, _ptr(out), out.nbytes))
        return out[0] if which in (5, 7) else out

    def load_scene_json(self, json_path: str):
        rc = self._lib.evplp_load_scene_json(self._h, json_path.encode())
        if rc < 0:
            raise EvplpError(rc, f"evplp_load_scene_json({json_path}): " + self._lib.evplp_last_error(self._h).decode())

    def camera(self) -> Camera:
        cam = Camera()
        self._check(self._lib.evplp_get_camera(self._h, C.byref(cam)))
        return cam

    def scene_metrics(self):
        r, t, l = C.c_float(), C.c_float(), C.c_float()
        self._check(self._lib.evplp_scene_metrics(self._h, C.byref(r), C.byref(t), C.byref(l)))
        return r.value, t.value, l.value

    def accel_info(self):
        n, l, d, ms = C.c_int32(), C.c_int32(), C.c_int32(), C.c_float()
        self._check(self._lib.evplp_accel_info(self._h, C.byref(n), C.byref(l), C.byref(d), C.byref(ms)))
        b = self._lib.evplp_accel_builder(self._h)
        return {"nodes": n.value, "leaves": l.value, "depth": d.value, "build_ms": ms.value,
                "builder": {0: "lbvh", 1: "sah", 2: "sbvh", 3: "gpu", 4: "ploc"}.get(b, "none"), "stack4_entries": self._lib.evplp_accel_stack_entries(self._h)}

    def selftest(self, which: int = 0) -> np.ndarray:
        """evplp_selftest: 0 the exact reciprocal, 1 the hardware pow, 2 the hand-written triangle-pair test against tri_pair_test
        (mismatches, cases, hits, then the hits of classes 0|1, 2|3, 4|5 packed 32 bits each), 3 the in-place visit of a synthetic
        node of an entry cut against the scalar-operand node visit (differences, cases, entered lanes, then the entered lanes of
        classes 0|1, 2|3, 4|5 packed 32 bits each), 4 the hardware primitives of the VSL estimators against double precision, maxima
        in units of 1e-12 (absolute: v_sin, v_cos, the Phong samples' cos_t; relative: v_rcp, v_rsq, v_sqrt), 5 the whole hand-written
        packet walk against the C++ walk for eight patterns of live lanes (mismatches, cases, occluded lanes, then the occluded lanes of
        classes 0-2, 3-5, 6-7 packed 21 bits each)"""
        out = np.zeros(8, dtype=np.uint64)
        n = self._check(self._lib.evplp_selftest(self._h, which, _ptr(out), 8))
        return out[:n]

    # -- passes
    def ev_math(self, which: int, x, y=None):
        """ev_math.h on the device: which 0 -> (sin x, cos x), 1 -> x ** y (evplp_debug_ev_math)"""
        x = _f32(x).reshape(-1); y = None if y is None else _f32(y).reshape(-1)
        o0 = np.empty_like(x); o1 = np.empty_like(x)
        self._check(self._lib.evplp_debug_ev_math(self._h, which, _ptr(x), _ptr(y), x.size, _ptr(o0), _ptr(o1)))
        return (o0, o1) if which == 0 else o0

    def set_stream(self, stream_ptr: int):
        self._check(self._lib.evplp_set_stream(self._h, C.c_void_p(stream_ptr)))

    def synchronize(self):
        self._check(self._lib.evplp_synchronize(self._h))

    def primary(self, jitter=(0.0, 0.0), clear_light=False, light_unoccluded=False, light_skip=False):
        """clear_light / light_unoccluded / light_skip = EVPLP_LIGHT_CLEAR / _UNOCCLUDED / _SKIP (include/evplp.h)."""
        j = (C.c_float * 2)(float(jitter[0]), float(jitter[1]))
        flags = (1 if clear_light else 0) | (2 if light_unoccluded else 0) | (4 if light_skip else 0)
        self._check(self._lib.evplp_primary(self._h, C.byref(j), flags))

    def trace_light_paths(self, rng_seed: int, path_begin: int = 0, path_count: Optional[int] = None):
        if path_count is None:
            path_count = self.cfg.num_light_paths - path_begin
        self._check(self._lib.evplp_trace_light_paths(self._h, rng_seed, path_begin, path_count))

    def gather_vpl(self, fp: FrameParams):
        self._check(self._lib.evplp_gather_vpl(self._h, C.byref(fp)))

    def gather_vsl(self, fp: FrameParams):
        self._check(self._lib.evplp_gather_vsl(self._h, C.byref(fp)))

    def gather_lvc(self, fp: FrameParams):
        self._check(self._lib.evplp_gather_lvc(self._h, C.byref(fp)))

    def path_trace(self, camera_pos, rng_seed: int, max_bounces: int, accumulate=True):
        cp = (C.c_float * 3)(*[float(v) for v in camera_pos])
        self._check(self._lib.evplp_path_trace(self._h, C.byref(cp), rng_seed, max_bounces, int(accumulate)))

    def path_trace_batch(self, camera_pos, jitters, rng_seeds, max_bounces: int):
        """S accumulating iterations in one call: primary(jitters[s], 0) + path_trace(camera_pos, rng_seeds[s], max_bounces) for every s,
        over the active tiles only (evplp_path_trace_batch)"""
        cp = (C.c_float * 3)(*[float(v) for v in camera_pos])
        n, j, r = _batch_arrays(jitters, rng_seeds)
        self._check(self._lib.evplp_path_trace_batch(self._h, C.byref(cp), n, j.ctypes.data, r.ctypes.data, max_bounces))

    def path_trace_batch_scratch(self, nbytes: int):
        """bound of the batch's staging buffer in bytes (default 1 GiB); smaller bounds mean more chunks, never other bits"""
        self._check(self._lib.evplp_path_trace_batch_scratch(self._h, int(nbytes)))

    def splat_photons(self, fp: FrameParams, clear=False):
        self._check(self._lib.evplp_splat_photons(self._h, C.byref(fp), int(clear)))

    def set_splat_proxy(self, vertices=None, triangles=None):
        """The proxy mesh of FOOTPRINT_PROXY (None: the generated icosphere); refused unless closed and convex around the origin."""
        if vertices is None:
            self._check(self._lib.evplp_set_splat_proxy(self._h, None, 0, None, 0)); return
        v = _f32(vertices).reshape(-1, 3); t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        self._check(self._lib.evplp_set_splat_proxy(self._h, _ptr(v), v.shape[0], _ptr(t), t.shape[0]))

    def resolve(self, vpl_scale=1.0, photon_scale=1.0, light_scale=1.0, mask_emitter=False, gamma=False) -> np.ndarray:
        out = np.empty((self.local_rows, self.W, 3), dtype=np.float32)
        self._check(self._lib.evplp_resolve(self._h, vpl_scale, photon_scale, light_scale, int(mask_emitter), int(gamma), _ptr(out)))
        return out

    def present(self, vpl_scale=1.0, photon_scale=1.0, light_scale=1.0, mask_emitter=True, gamma=False):
        """The per-iteration composite (rtcomphoton.h:997-1004): the strip's RGB stays on the device."""
        self._check(self._lib.evplp_present(self._h, vpl_scale, photon_scale, light_scale, int(mask_emitter), int(gamma)))

    def clear_accumulators(self):
        self._check(self._lib.evplp_clear_accumulators(self._h))

    def set_error_reference(self, rgb: Optional[np.ndarray], mask: Optional[np.ndarray] = None):
        """The reference of frame_error(): float32 (H, W, 3) rows top to bottom, an optional uint8 (H, W, 3) mask; rgb=None releases it."""
        rgb, mask = _error_reference(rgb, mask, self.W, self.H)
        self._check(self._lib.evplp_set_error_reference(self._h, _ptr(rgb), _ptr(mask)))

    def frame_error(self, vpl_scale=1.0, photon_scale=1.0, light_scale=1.0, mask_emitter=False, gamma=False):
        """(mse, rel_mse, rel_mse_masked) of the composite against the reference, reduced on the device over the rows this context holds"""
        out = (C.c_double * 3)()
        self._check(self._lib.evplp_frame_error(self._h, vpl_scale, photon_scale, light_scale, int(mask_emitter), int(gamma), C.byref(out)))
        return out[0], out[1], out[2]

    def noise_track(self, on=True, mask: Optional[np.ndarray] = None):
        """Start (again) or stop tracking per-pixel noise from the running sums; mask: optional uint8 (H, W, 3) top-down (include/evplp.h)"""
        on, mask = _noise_track_args(on, mask, self.W, self.H)
        self._check(self._lib.evplp_noise_track(self._h, on, _ptr(mask)))

    def noise_fold(self, iterations=1):
        """close a batch of `iterations` accumulating iterations"""
        k = _fold_iterations(iterations)
        self._check(self._lib.evplp_noise_fold(self._h, k))

    def noise_estimate(self, scale, light_scale=1.0, mask_emitter=False):
        """(mse, rel_mse, rel_mse_masked) estimated from the spread of the folded batches for the composite scale * sums + light_scale * light"""
        out = (C.c_double * 3)()
        self._check(self._lib.evplp_noise_estimate(self._h, float(scale), float(light_scale), int(mask_emitter), C.byref(out)))
        return out[0], out[1], out[2]

    def noise_variance(self, scale):
        """per-pixel variance of scale * sums, float32 (local_rows, W, 3), y = 0 at the bottom"""
        out = np.empty((self.local_rows, self.W, 3), dtype=np.float32)
        self._check(self._lib.evplp_noise_variance(self._h, float(scale), _ptr(out)))
        return out

    def denoise(self, scale, light_scale=1.0, mask_emitter=False, levels=0, sigma_luminance=0, sigma_normal=0, sigma_position=0) -> np.ndarray:
        """the composite of noise_estimate's arguments, filtered by the variance-guided a-trous denoiser (include/evplp.h evplp_denoise):
        float32 (local_rows, W, 3), y = 0 at the bottom, linear.  0 = the library's default for levels and every sigma."""
        p = _denoise_params(levels, sigma_luminance, sigma_normal, sigma_position)
        out = np.empty((self.local_rows, self.W, 3), dtype=np.float32)
        self._check(self._lib.evplp_denoise(self._h, float(scale), float(light_scale), int(mask_emitter), C.byref(p), _ptr(out)))
        return out

    def temporal_enable(self, on=True):
        """evplp_temporal_enable: the previous pose (36 B per triangle) and the previous-pose texels (32 B per plane pixel); False releases them
        and the history"""
        self._check(self._lib.evplp_temporal_enable(self._h, int(bool(on))))

    def temporal_reset(self):
        """evplp_temporal_reset: the next denoise_temporal behaves as a first call"""
        self._check(self._lib.evplp_temporal_reset(self._h))

    def denoise_temporal(self, scale, light_scale=1.0, mask_emitter=False, levels=0, sigma_luminance=0, sigma_normal=0, sigma_position=0,
                         max_history=0, normal_cos=0.0):
        """denoise() with the temporal accumulation stage in front of the passes (include/evplp.h evplp_denoise_temporal; frames must be
        independent samples): (float32 (local_rows, W, 3), the dict of evplp_temporal_info)"""
        p = _denoise_params(levels, sigma_luminance, sigma_normal, sigma_position)
        t = _temporal_params(max_history, normal_cos)
        out = np.empty((self.local_rows, self.W, 3), dtype=np.float32)
        info = TemporalInfo()
        self._check(self._lib.evplp_denoise_temporal(self._h, float(scale), float(light_scale), int(mask_emitter), C.byref(p), C.byref(t), _ptr(out), C.byref(info)))
        return out, info.as_dict()

    def temporal_download(self, which: int) -> np.ndarray:
        """evplp_temporal_download: plane TEMPORAL_* of the last denoise_temporal, float32 (local_rows, W, 4), y = 0 at the bottom"""
        out = np.empty((self.local_rows, self.W, 4), dtype=np.float32)
        self._check(self._lib.evplp_temporal_download(self._h, int(which), _ptr(out)))
        return out

    def adaptive_enable(self, on=True, path_trace=False, budget=False, gather_budget=False):
        """Switch the adaptive gather on or off (before the first accumulating gather since the last clear; needs noise tracking; include/evplp.h).
        path_trace=True: path-trace mode instead (evplp_adaptive_enable_pt) -- path_trace() honours retirement and the gathers are refused"""
        if budget:        # budget mode (evplp_adaptive_enable_pt(.., 2)): every tile takes its own number of samples of a path_trace_batch call
            self._check(self._lib.evplp_adaptive_enable_pt(self._h, 2 if on else 0)); return
        if gather_budget:     # gather budget mode (evplp_adaptive_enable(.., 2)): every tile takes the first b_t of every window of gather calls
            self._check(self._lib.evplp_adaptive_enable(self._h, 2 if on else 0)); return
        f = self._lib.evplp_adaptive_enable_pt if path_trace else self._lib.evplp_adaptive_enable
        self._check(f(self._h, int(bool(on))))

    def adaptive_retire(self, scale, tile_rel_mse, min_batches=2, light_scale=1.0, mask_emitter=False) -> int:
        """retire the active tiles whose mean relative variance of scale * sums + light_scale * light is <= tile_rel_mse; returns how many"""
        tau, mb = _adaptive_retire_args(tile_rel_mse, min_batches)
        return self._check(self._lib.evplp_adaptive_retire(self._h, float(scale), float(light_scale), int(mask_emitter), tau, mb))

    def adaptive_tiles(self) -> np.ndarray:
        """int32 (ceil(H / 8), ceil(W / 8)), tile rows from the bottom: n_t of a retired tile, N of an active one (0: another rank's)"""
        out = np.zeros(((self.H + 7) // 8, (self.W + 7) // 8), dtype=np.int32)
        self._check(self._lib.evplp_adaptive_tiles(self._h, _ptr(out), out.size))
        return out

    def adaptive_set_budgets(self, samples_per_tile):
        """budget mode: samples of the next path_trace_batch calls per image tile, int32 (ceil(H / 8), ceil(W / 8)) in adaptive_tiles' layout, 0 .. 64"""
        b = np.ascontiguousarray(samples_per_tile, dtype=np.int32)
        self._check(self._lib.evplp_adaptive_set_budgets(self._h, _ptr(b), b.size))

    def adaptive_budgets(self) -> np.ndarray:
        """int32 (ceil(H / 8), ceil(W / 8)): the tiles' budgets, -1 = every sample of a call (0: another rank's)"""
        out = np.zeros(((self.H + 7) // 8, (self.W + 7) // 8), dtype=np.int32)
        self._check(self._lib.evplp_adaptive_budgets(self._h, _ptr(out), out.size))
        return out

    def adaptive_budget_window(self, window: int):
        """gather budget mode: the window S (1 .. 64) -- a tile with budget b takes the first min(b, S) of every S accumulating gather calls"""
        self._check(self._lib.evplp_adaptive_budget_window(self._h, int(window)))

    def adaptive_tile_noise(self, scale, light_scale=1.0, mask_emitter=False) -> np.ndarray:
        """float64 (ceil(H / 8), ceil(W / 8)): the mean relative variance of every tile, the figure adaptive_retire compares with tile_rel_mse"""
        out = np.zeros(((self.H + 7) // 8, (self.W + 7) // 8), dtype=np.float64)
        self._check(self._lib.evplp_adaptive_tile_noise(self._h, float(scale), float(light_scale), int(mask_emitter), _ptr(out), out.size))
        return out

    def set_blocks(self, image_blocks=None):
        """row-strip context: own these image blocks (in this local order) instead of the blocks b % strip_count == strip_rank; None = back to that"""
        if image_blocks is None:
            self._check(self._lib.evplp_set_blocks(self._h, None, 0)); return
        b = np.ascontiguousarray(image_blocks, dtype=np.int32)
        self._check(self._lib.evplp_set_blocks(self._h, _ptr(b), b.size))

    def blocks(self) -> np.ndarray:
        """the image blocks this context owns, in local order"""
        n = self._check(self._lib.evplp_get_blocks(self._h, None, 0))
        out = np.zeros(n, dtype=np.int32)
        self._check(self._lib.evplp_get_blocks(self._h, _ptr(out), n))
        return out

    def calibrate_blocks(self, on: bool = True):
        self._check(self._lib.evplp_calibrate_blocks(self._h, int(on)))

    def block_costs(self) -> np.ndarray:
        """clock ticks the gathers' wavefronts spent in every IMAGE block since calibrate_blocks(True) (0 for other ranks' blocks)"""
        sr = self.cfg.strip_rows if self.cfg.strip_count > 1 else (self.H + 7) // 8 * 8
        out = np.zeros((self.H + sr - 1) // sr, dtype=np.uint64)
        self._check(self._lib.evplp_block_costs(self._h, _ptr(out), out.size))
        return out

    # -- buffers
    def buffer_info(self, which: int):
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._lib.evplp_buffer_info(self._h, which, C.byref(p), C.byref(n)))
        return p.value, n.value

    def bind_buffer(self, which: int, device_ptr: int, nbytes: int):
        self._check(self._lib.evplp_bind_buffer(self._h, which, C.c_void_p(device_ptr), nbytes))

    def buffer_bytes(self, which: int) -> int:
        n = C.c_size_t()
        self._check(self._lib.evplp_buffer_info(self._h, which, None, C.byref(n)))   # (no pointer taken: see evplp_buffer_info)
        return n.value

    def download(self, which: int) -> np.ndarray:
        n = self.buffer_bytes(which)
        if which == BUF_RECORDS:
            out = np.empty(n // 96, dtype=RECORD_DTYPE)
        else:
            out = np.empty((self.local_rows, self.W, 4), dtype=np.float32)
        self._check(self._lib.evplp_download(self._h, which, _ptr(out), n))
        return out

    def upload(self, which: int, data: np.ndarray):
        data = np.ascontiguousarray(data)
        self._check(self._lib.evplp_upload(self._h, which, _ptr(data), data.nbytes))

    def pass_stats(self, which: int) -> dict:
        s = PassStats()
        self._check(self._lib.evplp_pass_stats_get(self._h, which, C.byref(s)))
        return {"ms": s.ms, "pairs": s.pairs, "rays": s.rays, "usable": s.usable, "dominant_kernel_ms": s.dominant_kernel_ms,
                "nodes": s.reserved[0] | (s.reserved[1] << 32), "shaded": s.shaded, "launches": s.launches,
                # VSL gather: the same two words carry the sample-iterations of the estimators (lighttracing.cu:632-640)
                "samples": (s.reserved[0] | (s.reserved[1] << 32)) if which == PASS_GATHER_VSL else 0}

    def profile_kernels(self, on: bool = True):
        """Record the events around the photon splat's dominant kernel (pass_stats()["dominant_kernel_ms"]); they sit between its launches."""
        self._check(self._lib.evplp_profile_kernels(self._h, int(on)))

    def profile_passes(self, on: bool = True):
        """Record the two events per pass that pass_stats()["ms"] needs (default on); off, a loop of sub-millisecond iterations runs
        without them and pass_stats reports ms = 0 for passes run meanwhile."""
        self._check(self._lib.evplp_profile_passes(self._h, int(on)))

    def debug_counters(self, which: int) -> np.ndarray:
        out = np.zeros(256, dtype=np.uint64)
        n = self._check(self._lib.evplp_debug_counters(self._h, which, _ptr(out), out.size))
        return out[:n]

    def debug_splat_bins(self):
        """evplp_debug_splat_bins (tests): (big_count uint32 [bin groups of 256 records], tile_cursor uint32 [local tile rows, tile columns])
        of the last photon splat, settled: the photons of every group that went through the large-rectangle list, and the entries every
        tile's bin wanted."""
        big = np.zeros((self.num_records + 255) // 256, dtype=np.uint32)
        cur = np.zeros((self.local_rows // 8, (self.W + 7) // 8), dtype=np.uint32)
        self._check(self._lib.evplp_debug_splat_bins(self._h, _ptr(big), big.size, _ptr(cur), cur.size))
        return big, cur

    # -- strips
    def global_rows(self) -> np.ndarray:
        """Global image row of every local row (>= H for padding rows)."""
        from . import strips
        if self.cfg.strip_count <= 1:
            return strips.global_rows(self.H, self.cfg.strip_rank, self.cfg.strip_count, self.cfg.strip_rows)
        return strips.rows_of_blocks(self.H, self.blocks(), self.cfg.strip_rows, self.local_rows)      # (the library's table: dealt or round-robin)


def refit_levels(nodes, level_capacity: int = 64):
    """evplp_refit_levels: (height per node, nodes by height, level offsets [levels + 1]) of a flattened tree (ACCEL_NODE records or raw 64-byte
    nodes); host only, deterministic.  EvplpError for an array that is not a tree of at most level_capacity heights."""
    raw = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1, 64)
    n = raw.shape[0]
    height, order, begin = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(level_capacity, 0) + 1, np.int32)
    rc = lib().evplp_refit_levels(_ptr(raw), n, _ptr(height), _ptr(order), _ptr(begin), int(level_capacity))
    if rc < 0:
        raise EvplpError(rc, "evplp_refit_levels: not a tree (a child index out of range, a node reached twice, a cycle), or more heights than level_capacity")
    return height[:n], order[:int(begin[rc])], begin[:rc + 1]


def transform_points(m, pts):
    """evplp_transform_points: the points (n, 3) under the row-major 3 x 4 matrix m, by the function evplp_transform_mesh moves a mesh with
    (fp32, every product and sum rounded on its own; host only)"""
    m = _f32(m).reshape(12)
    p = _f32(pts).reshape(-1, 3)
    out = np.empty_like(p)
    rc = lib().evplp_transform_points(_ptr(m), _ptr(p), _ptr(out), p.shape[0])
    if rc < 0:
        raise EvplpError(rc, "evplp_transform_points: a null pointer")
    return out


def skin_points(bone_matrices, bone_index, weight, pts):
    """evplp_skin_points: the points (n, 3) under the palette (nbones, 12) with four bone indices (n, 4) and weights (n, 4) each, by the
    function evplp_pose_mesh moves a mesh with (fp32, every product and sum rounded on its own; host only)"""
    m = _f32(bone_matrices).reshape(-1, 12)
    p = _f32(pts).reshape(-1, 3)
    b = np.ascontiguousarray(bone_index, np.int32).reshape(-1, 4)
    w = _f32(weight).reshape(-1, 4)
    if b.shape[0] != p.shape[0] or w.shape[0] != p.shape[0]:
        raise ValueError("skin_points: bone_index and weight must be (n, 4) for (n, 3) points")
    out = np.empty_like(p)
    rc = lib().evplp_skin_points(_ptr(m), m.shape[0], _ptr(b), _ptr(w), _ptr(p), _ptr(out), p.shape[0])
    if rc < 0:
        raise EvplpError(rc, "evplp_skin_points: a null pointer, nbones outside 1 .. 1024, a bone index out of range, a bad weight, or a matrix entry or result that is not finite")
    return out


def morph_points(pts, deltas, weights):
    """evplp_morph_points: the points (n, 3) + the weighted deltas (T, n, 3), by the function evplp_morph_mesh makes a mesh's base with (fp32,
    every product and sum rounded on its own, in index order; host only)"""
    p = _f32(pts).reshape(-1, 3)
    d = _f32(deltas)
    w = _f32(weights).reshape(-1)
    if d.ndim != 3 or d.shape[1:] != p.shape or d.shape[0] != w.shape[0]:
        raise ValueError("morph_points: deltas must be (T, n, 3) for (n, 3) points and T weights")
    out = np.empty_like(p)
    rc = lib().evplp_morph_points(_ptr(p), _ptr(d), _ptr(w), w.shape[0], p.shape[0], _ptr(out))
    if rc < 0:
        raise EvplpError(rc, "evplp_morph_points: a null pointer, ntargets outside 1 .. 64, or a point, a delta, a weight or a result that is not finite")
    return out


def accel_cost(nodes) -> dict:
    """evplp_accel_cost: the SAH cost of a flattened tree (ACCEL_NODE records or raw 64-byte nodes) on the host, in the order and shape of
    the device's sums -- evplp_accel_quality's reference.  EvplpError for an array that is not a tree."""
    raw = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1, 64)
    out = (C.c_double * 5)()
    rc = lib().evplp_accel_cost(_ptr(raw), raw.shape[0], out)
    if rc < 0:
        raise EvplpError(rc, "evplp_accel_cost: not a tree (a child index out of range, a node reached twice, a cycle), or no nodes")
    return {"cost": out[0], "root_area": out[1], "inner_area": out[2], "leaf_pair_area": out[3], "leaf_tri_area": out[4], "reached_nodes": rc}


def ploc_tree(verts9, radius: int = PLOC_RADIUS, search_iterations: int = PLOC_SEARCH_ITERATIONS):
    """evplp_ploc_tree: the tree the device PLOC builder makes, on the host (deterministic).  verts9: 9 floats per triangle.  Returns (order [n]: the
    valid triangles in Morton order, children [n - 1, 2]: inner index or ~position, iterations)."""
    v = np.ascontiguousarray(verts9, dtype=np.float32).reshape(-1, 9)
    ntri = v.shape[0]
    order, children, it = np.zeros(max(ntri, 1), np.int32), np.zeros((max(ntri - 1, 1), 2), np.int32), C.c_int32(0)
    n = lib().evplp_ploc_tree(_ptr(v), ntri, int(radius), int(search_iterations), _ptr(order), _ptr(children), C.byref(it))
    if n < 0:
        raise EvplpError(n, "evplp_ploc_tree: a null pointer, or a radius outside 1 .. 32, or search_iterations outside 0 .. 128")
    return order[:n].copy(), children[:max(n - 1, 0)].copy(), it.value


def rotate_tree(nodes, tri_index, verts9, passes: int = 1, level=None) -> dict:
    """evplp_rotate_tree: the rotating refit sweep on the host (deterministic), the twin of evplp_optimize_accel.  nodes: ACCEL_NODE records or
    raw 64-byte nodes (the child references alone are read); tri_index: 4 ints per leaf block; verts9: 9 floats per original triangle; level:
    the plan's level per node, or None for evplp_refit_levels' heights of `nodes`.  Returns children [nnodes, 2], boxes [nnodes, 6] (lo, hi),
    rotations (per pass), need0 (the root's four-wide stack need), levels, and nodes: a copy of the records with the new references (its
    padded boxes are NOT updated)."""
    raw = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1, 64)
    n = raw.shape[0]
    ti = np.ascontiguousarray(tri_index, dtype=np.int32).reshape(-1)
    v = np.ascontiguousarray(verts9, dtype=np.float32).reshape(-1, 9)
    lv = None if level is None else np.ascontiguousarray(level, dtype=np.int32).reshape(-1)
    if lv is not None and lv.shape[0] != n:
        raise ValueError("rotate_tree: one level per node")
    children, boxes = np.zeros((max(n, 1), 2), np.int32), np.zeros((max(n, 1), 6), np.float32)
    rot, need0 = np.zeros(8, np.int32), C.c_int32(0)
    rc = lib().evplp_rotate_tree(_ptr(raw), n, _ptr(ti) if ti.size else None, ti.shape[0], _ptr(v) if v.size else None, v.shape[0], None if lv is None else _ptr(lv), int(passes),
                                 _ptr(children), _ptr(boxes), _ptr(rot), C.byref(need0))
    if rc < 0:
        raise EvplpError(rc, "evplp_rotate_tree: not a tree, passes outside 1 .. 8, or levels that put an inner child at or above its parent")
    out = raw.copy()
    out[:, 48:56] = children[:n].view(np.uint8).reshape(n, 8)
    return {"children": children[:n], "boxes": boxes[:n], "rotations": [int(x) for x in rot[:int(passes)]], "need0": need0.value, "levels": rc, "nodes": out.reshape(-1).view(ACCEL_NODE)}


Context.refit_levels = staticmethod(refit_levels)      # (the plan needs no context; it is listed with the calls it serves)


def deal_blocks(costs, n_ranks: int, capacity_blocks: int) -> np.ndarray:
    """evplp_deal_blocks: owner rank of every image block for these per-block costs (host only, deterministic)"""
    c = np.ascontiguousarray(costs, dtype=np.uint64)
    owner = np.zeros(c.size, dtype=np.int32)
    rc = lib().evplp_deal_blocks(_ptr(c), c.size, n_ranks, capacity_blocks, _ptr(owner))
    if rc < 0:
        raise EvplpError(rc, "evplp_deal_blocks: the blocks do not fit the ranks' capacity")
    return owner


def plan_budgets(rel, n_t, samples: int, min_samples: int = 1, tile_rel_mse: float = 0.0, reference_quantile: float = 1.0) -> np.ndarray:
    """evplp_plan_budgets: samples of the next call per tile from the tiles' noise (adaptive_tile_noise) and sample counts (adaptive_tiles),
    in the shape of n_t (host only, deterministic)"""
    r = np.ascontiguousarray(rel, dtype=np.float64)
    n = np.ascontiguousarray(n_t, dtype=np.int32)
    if r.size != n.size:
        raise ValueError(f"plan_budgets: {r.size} noise figures but {n.size} sample counts")
    out = np.zeros(n.shape, dtype=np.int32)
    rc = lib().evplp_plan_budgets(_ptr(r), _ptr(n), n.size, int(samples), int(min_samples), float(tile_rel_mse), float(reference_quantile), _ptr(out))
    if rc < 0:
        raise EvplpError(rc, "evplp_plan_budgets: samples 1 .. 64, min_samples 0 .. samples, reference_quantile in (0, 1], finite rel >= 0, >= 1 tile")
    return out


def split_model(num_light_paths: int, photons_per_path: int, n_ranks: int):
    """evplp_group_split_model: (split expected to be faster?, ms with every rank tracing all paths, ms with a share + the record exchange)"""
    out = (C.c_double * 2)()
    rc = lib().evplp_group_split_model(num_light_paths, photons_per_path, n_ranks, C.byref(out))
    return bool(rc == 1), out[0], out[1]


def rank_blocks(costs, owner, rank: int) -> np.ndarray:
    """evplp_rank_blocks: the blocks a deal gives `rank`, in the order it stores and launches them (most expensive first; costs=None: image order)"""
    o = np.ascontiguousarray(owner, dtype=np.int32)
    c = None if costs is None else np.ascontiguousarray(costs, dtype=np.uint64)
    out = np.zeros(o.size, dtype=np.int32)
    n = lib().evplp_rank_blocks(_ptr(c), _ptr(o), o.size, rank, _ptr(out), out.size)
    if n < 0:
        raise EvplpError(n, "evplp_rank_blocks")
    return out[:n]


class Group:
    """evplp_group: n ranks driven by one thread (RCCL across distinct GPUs, device copies for virtual ranks) that share out the image
    (partition "strips") or the iterations of a progressive run ("iterations": select_rank() picks the rank the passes go to,
    present() / resolve() sum the ranks' accumulators on the GPUs)."""

    def __init__(self, res_x, res_y, num_light_paths, num_vpl_light_paths, photons_per_path, n_ranks, devices=None, strip_rows=0,
                 use_rccl=False, deterministic=False, bvh_builder=BVH_SAH, overlap_light_tracing=False, partition="strips", strip_capacity_pct=0, split_light_paths=0, cut_scratch_bytes=0, vsl_mask_bytes=0):
        """strip_rows = 0: the library's choice (16 rows)"""
        self._lib = lib()
        cfg = Config()
        cfg.abi_version = ABI_VERSION; cfg.res_x = res_x; cfg.res_y = res_y
        cfg.num_light_paths = num_light_paths; cfg.num_vpl_light_paths = num_vpl_light_paths; cfg.photons_per_path = photons_per_path
        cfg.bvh_builder = bvh_builder; cfg.deterministic = int(deterministic); cfg.overlap_light_tracing = int(overlap_light_tracing)
        cfg.cut_scratch_bytes = int(cut_scratch_bytes); cfg.vsl_mask_bytes = int(vsl_mask_bytes)
        gc = GroupConfig(); gc.n_ranks = n_ranks; gc.strip_rows = strip_rows; gc.use_rccl = int(use_rccl)
        if partition not in PARTITIONS:
            raise ValueError(f"partition: one of {sorted(PARTITIONS)}, got {partition!r}")
        gc.partition = PARTITIONS[partition]; gc.strip_capacity_pct = int(strip_capacity_pct); gc.split_light_paths = int(split_light_paths)
        self.partition = partition
        self._devs = (C.c_int32 * n_ranks)(*devices) if devices is not None else None
        gc.devices = C.cast(self._devs, C.POINTER(C.c_int32)) if self._devs is not None else None
        h = C.c_void_p()
        rc = self._lib.evplp_group_create(C.byref(cfg), C.byref(gc), C.byref(h))
        if rc != OK:
            raise EvplpError(rc, self._lib.evplp_group_last_error(None).decode())
        self._h = h; self.W, self.H, self.n = res_x, res_y, n_ranks
        self.strip_rows = strip_rows if strip_rows > 0 else 16
        self._paths = (num_light_paths, num_vpl_light_paths, photons_per_path)

    def _check(self, rc):
        if rc < 0:
            raise EvplpError(rc, self._lib.evplp_group_last_error(self._h).decode())
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self._lib.evplp_group_destroy(self._h); self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def load_scene_json(self, path):
        self._check(self._lib.evplp_group_load_scene_json(self._h, path.encode()))

    def clear_accumulators(self):
        self._check(self._lib.evplp_group_clear_accumulators(self._h))

    def primary(self, jitter=(0.0, 0.0), light_flags=0):
        j = (C.c_float * 2)(float(jitter[0]), float(jitter[1]))
        self._check(self._lib.evplp_group_primary(self._h, C.byref(j), light_flags))

    def trace_light_paths(self, seed):
        self._check(self._lib.evplp_group_trace_light_paths(self._h, seed))

    def gather(self, fp, kind=0):
        self._check(self._lib.evplp_group_gather(self._h, C.byref(fp), kind))

    def path_trace(self, camera_pos, rng_seed: int, max_bounces: int, accumulate=True):
        cp = (C.c_float * 3)(*[float(v) for v in camera_pos])
        self._check(self._lib.evplp_group_path_trace(self._h, C.byref(cp), rng_seed, max_bounces, int(accumulate)))

    def path_trace_batch(self, camera_pos, jitters, rng_seeds, max_bounces: int):
        """S accumulating iterations in one call: primary(jitters[s], 0) + path_trace(camera_pos, rng_seeds[s], max_bounces) for every s,
        over the active tiles only (evplp_group_path_trace_batch)"""
        cp = (C.c_float * 3)(*[float(v) for v in camera_pos])
        n, j, r = _batch_arrays(jitters, rng_seeds)
        self._check(self._lib.evplp_group_path_trace_batch(self._h, C.byref(cp), n, j.ctypes.data, r.ctypes.data, max_bounces))

    def path_trace_batch_scratch(self, nbytes: int):
        """bound of the batch's staging buffer in bytes (default 1 GiB); smaller bounds mean more chunks, never other bits"""
        self._check(self._lib.evplp_group_path_trace_batch_scratch(self._h, int(nbytes)))

    def splat_photons(self, fp, clear=False):
        self._check(self._lib.evplp_group_splat_photons(self._h, C.byref(fp), int(clear)))

    def update_mesh(self, mesh: int, vertices):
        v = _f32(vertices).reshape(-1, 3)
        self._check(self._lib.evplp_group_update_mesh(self._h, int(mesh), _ptr(v), v.shape[0]))

    def transform_mesh(self, mesh: int, m):
        m = _f32(m).reshape(12)
        self._check(self._lib.evplp_group_transform_mesh(self._h, int(mesh), _ptr(m)))

    def set_mesh_skin(self, mesh: int, nbones: int, bone_index=None, weight=None):
        if int(nbones) == 0 and bone_index is None and weight is None:
            return self._check(self._lib.evplp_group_set_mesh_skin(self._h, int(mesh), 0, None, None, 0))
        b = np.ascontiguousarray(bone_index, np.int32).reshape(-1, 4)
        w = _f32(weight).reshape(-1, 4)
        if b.shape != w.shape:
            raise ValueError("set_mesh_skin: bone_index and weight must both be (nverts, 4)")
        self._check(self._lib.evplp_group_set_mesh_skin(self._h, int(mesh), int(nbones), _ptr(b), _ptr(w), b.shape[0]))

    def pose_mesh(self, mesh: int, bone_matrices):
        m = _f32(bone_matrices).reshape(-1, 12)
        self._check(self._lib.evplp_group_pose_mesh(self._h, int(mesh), _ptr(m), m.shape[0]))

    def set_mesh_morph(self, mesh: int, deltas=None):
        if deltas is None:
            return self._check(self._lib.evplp_group_set_mesh_morph(self._h, int(mesh), 0, None, 0))
        d = _f32(deltas)
        if d.ndim != 3 or d.shape[2] != 3:
            raise ValueError("set_mesh_morph: deltas must be (ntargets, nverts, 3)")
        self._check(self._lib.evplp_group_set_mesh_morph(self._h, int(mesh), d.shape[0], _ptr(d), d.shape[1]))

    def morph_mesh(self, mesh: int, weights=None):
        if weights is None:
            return self._check(self._lib.evplp_group_morph_mesh(self._h, int(mesh), None, 0))
        w = _f32(weights).reshape(-1)
        self._check(self._lib.evplp_group_morph_mesh(self._h, int(mesh), _ptr(w), w.shape[0]))

    def refit_accel(self):
        self._check(self._lib.evplp_group_refit_accel(self._h))

    def accel_quality(self) -> dict:
        """evplp_group_accel_quality: rank 0's figures; an error if any rank's differ"""
        q = AccelQuality()
        self._check(self._lib.evplp_group_accel_quality(self._h, C.byref(q)))
        return q.as_dict()

    def set_refit_policy(self, max_cost_ratio: float, rebuild_builder: int = -1):
        self._check(self._lib.evplp_group_set_refit_policy(self._h, float(max_cost_ratio), int(rebuild_builder)))

    def trace_closest(self, rays, filter: int = 0, order: bool = QUERY_ORDER_DEFAULT):
        """evplp_group_trace_closest: Context.trace_closest of a numpy batch, the rays dealt over the ranks by index; the same bytes"""
        r = _host_rays(rays)
        hits = np.zeros(r.shape[0], HIT_DTYPE)
        self._check(self._lib.evplp_group_trace_closest(self._h, _ptr(r), r.shape[0], int(filter), QUERY_ORDER if order else 0, _ptr(hits)))
        return hits

    def trace_occluded(self, rays, order: bool = QUERY_ORDER_DEFAULT):
        """evplp_group_trace_occluded: Context.trace_occluded of a numpy batch, the rays dealt over the ranks by index; the same bytes"""
        r = _host_rays(rays)
        out = np.zeros(r.shape[0], np.uint8)
        self._check(self._lib.evplp_group_trace_occluded(self._h, _ptr(r), r.shape[0], QUERY_ORDER if order else 0, _ptr(out)))
        return out

    def optimize_accel(self, passes: int = 1) -> int:
        """evplp_group_optimize_accel: on every rank; rank 0's rotation count, an error if any rank's differs"""
        n = C.c_int32(0)
        self._check(self._lib.evplp_group_optimize_accel(self._h, int(passes), C.byref(n)))
        return n.value

    def set_refit_rotations(self, passes: int):
        self._check(self._lib.evplp_group_set_refit_rotations(self._h, int(passes)))

    def set_splat_proxy(self, vertices=None, triangles=None):
        if vertices is None:
            self._check(self._lib.evplp_group_set_splat_proxy(self._h, None, 0, None, 0)); return
        v = _f32(vertices).reshape(-1, 3); t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        self._check(self._lib.evplp_group_set_splat_proxy(self._h, _ptr(v), v.shape[0], _ptr(t), t.shape[0]))

    def synchronize(self):
        self._check(self._lib.evplp_group_synchronize(self._h))

    def select_rank(self, r: int):
        """iterations partition: the rank the pass calls go to from now on"""
        self._check(self._lib.evplp_group_select_rank(self._h, r))

    def synchronize_rank(self, r: int):
        """wait for rank r's worker and its context's streams only"""
        self._check(self._lib.evplp_group_synchronize_rank(self._h, r))

    def rebalance(self) -> None:
        """strips partition: deal the blocks by the cost clocked since calibrate() (clears the accumulators; block_owners() has the result)"""
        self._check(self._lib.evplp_group_rebalance(self._h))

    def calibrate(self, on: bool = True):
        """strips partition: the gathers clock their blocks until rebalance() deals them by cost"""
        self._check(self._lib.evplp_group_calibrate(self._h, int(on)))

    def block_owners(self) -> np.ndarray:
        n = self._check(self._lib.evplp_group_block_owners(self._h, None, 0))
        out = np.zeros(n, dtype=np.int32)
        self._check(self._lib.evplp_group_block_owners(self._h, _ptr(out), n))
        return out

    def profile_passes(self, on: bool = True):
        self._check(self._lib.evplp_group_profile_passes(self._h, int(on)))

    def host_stats(self, r: int) -> dict:
        """host time of rank r's worker thread (ms inside pass calls, ms inside exchanges, commands run)"""
        out = (C.c_double * 3)()
        self._check(self._lib.evplp_group_host_stats(self._h, r, C.byref(out)))
        return {"calls_ms": out[0], "exchange_ms": out[1], "commands": int(out[2])}

    def present(self, vpl_scale=1.0, photon_scale=1.0, light_scale=1.0, mask_emitter=False, gamma=False, exchange=True):
        """composite + all-gather of the strips on the devices (the per-frame exchange; iterations partition: the reduction); nothing comes to the host.
        exchange=False: the composite alone (iterations partition: of the selected rank's own accumulators)"""
        self._check(self._lib.evplp_group_present_ex(self._h, vpl_scale, photon_scale, light_scale, int(mask_emitter), int(gamma), int(exchange)))

    def rank(self, r: int) -> "Context":
        """rank r's context (borrowed): pass statistics, buffers"""
        self._lib.evplp_group_context.restype = C.c_void_p
        h = self._lib.evplp_group_context(self._h, r)
        if not h:
            raise EvplpError(ERR_INVALID, "evplp_group_context: bad rank")
        whole = self.partition == "iterations"       # (every rank holds the whole image)
        c = Context.borrowed(h, self.W, self.H, strip_rank=0 if whole else r, strip_count=1 if whole else self.n, strip_rows=self.strip_rows,
                             num_light_paths=self._paths[0], num_vpl_light_paths=self._paths[1], photons_per_path=self._paths[2])
        return c

    context = rank

    def resolve(self, vpl_scale=1.0, photon_scale=1.0, light_scale=1.0, mask_emitter=False, gamma=False):
        out = np.empty((self.H, self.W, 3), dtype=np.float32)
        self._check(self._lib.evplp_group_resolve(self._h, vpl_scale, photon_scale, light_scale, int(mask_emitter), int(gamma), _ptr(out)))
        return out

    def set_error_reference(self, rgb: Optional[np.ndarray], mask: Optional[np.ndarray] = None):
        """Context.set_error_reference on every rank"""
        rgb, mask = _error_reference(rgb, mask, self.W, self.H)
        self._check(self._lib.evplp_group_set_error_reference(self._h, _ptr(rgb), _ptr(mask)))

    def frame_error(self, vpl_scale=1.0, photon_scale=1.0, light_scale=1.0, mask_emitter=False, gamma=False):
        """(mse, rel_mse, rel_mse_masked) of the whole frame against the reference (strips: no all-gather; equal to one context's, bit for bit)"""
        out = (C.c_double * 3)()
        self._check(self._lib.evplp_group_frame_error(self._h, vpl_scale, photon_scale, light_scale, int(mask_emitter), int(gamma), C.byref(out)))
        return out[0], out[1], out[2]

    def noise_track(self, on=True, mask: Optional[np.ndarray] = None):
        """Start (again) or stop tracking per-pixel noise from the running sums; mask: optional uint8 (H, W, 3) top-down (include/evplp.h)"""
        on, mask = _noise_track_args(on, mask, self.W, self.H)
        self._check(self._lib.evplp_group_noise_track(self._h, on, _ptr(mask)))

    def noise_fold(self, iterations=1):
        """close a batch of `iterations` accumulating iterations"""
        k = _fold_iterations(iterations)
        self._check(self._lib.evplp_group_noise_fold(self._h, k))

    def noise_estimate(self, scale, light_scale=1.0, mask_emitter=False):
        """(mse, rel_mse, rel_mse_masked) estimated from the spread of the folded batches for the composite scale * sums + light_scale * light"""
        out = (C.c_double * 3)()
        self._check(self._lib.evplp_group_noise_estimate(self._h, float(scale), float(light_scale), int(mask_emitter), C.byref(out)))
        return out[0], out[1], out[2]

    def noise_variance(self, scale):
        """per-pixel variance of scale * sums, float32 (H, W, 3), y = 0 at the bottom"""
        out = np.empty((self.H, self.W, 3), dtype=np.float32)
        self._check(self._lib.evplp_group_noise_variance(self._h, float(scale), _ptr(out)))
        return out

    def denoise(self, scale, light_scale=1.0, mask_emitter=False, levels=0, sigma_luminance=0, sigma_normal=0, sigma_position=0) -> np.ndarray:
        """Context.denoise for the whole frame, float32 (H, W, 3), y = 0 at the bottom (strips: equal to one context's, bit for bit)"""
        p = _denoise_params(levels, sigma_luminance, sigma_normal, sigma_position)
        out = np.empty((self.H, self.W, 3), dtype=np.float32)
        self._check(self._lib.evplp_group_denoise(self._h, float(scale), float(light_scale), int(mask_emitter), C.byref(p), _ptr(out)))
        return out

    def temporal_enable(self, on=True):
        """evplp_group_temporal_enable: Context.temporal_enable on every rank"""
        self._check(self._lib.evplp_group_temporal_enable(self._h, int(bool(on))))

    def temporal_reset(self):
        self._check(self._lib.evplp_group_temporal_reset(self._h))

    def denoise_temporal(self, scale, light_scale=1.0, mask_emitter=False, levels=0, sigma_luminance=0, sigma_normal=0, sigma_position=0,
                         max_history=0, normal_cos=0.0):
        """Context.denoise_temporal for the whole frame: (float32 (H, W, 3), the info dict); strips: one context's bits for any block table"""
        p = _denoise_params(levels, sigma_luminance, sigma_normal, sigma_position)
        t = _temporal_params(max_history, normal_cos)
        out = np.empty((self.H, self.W, 3), dtype=np.float32)
        info = TemporalInfo()
        self._check(self._lib.evplp_group_denoise_temporal(self._h, float(scale), float(light_scale), int(mask_emitter), C.byref(p), C.byref(t), _ptr(out), C.byref(info)))
        return out, info.as_dict()

    def temporal_download(self, which: int) -> np.ndarray:
        """evplp_group_temporal_download: a history or previous-pose plane of the last denoise_temporal, float32 (H, W, 4)"""
        out = np.empty((self.H, self.W, 4), dtype=np.float32)
        self._check(self._lib.evplp_group_temporal_download(self._h, int(which), _ptr(out)))
        return out

    def adaptive_enable(self, on=True, path_trace=False, budget=False, gather_budget=False):
        """Switch the adaptive gather on or off (before the first accumulating gather since the last clear; needs noise tracking; include/evplp.h).
        path_trace=True: path-trace mode instead (evplp_group_adaptive_enable_pt) -- path_trace() honours retirement and gather() is refused"""
        if budget:        # budget mode (evplp_group_adaptive_enable_pt(.., 2)): every tile takes its own number of samples of a path_trace_batch call
            self._check(self._lib.evplp_group_adaptive_enable_pt(self._h, 2 if on else 0)); return
        if gather_budget:     # gather budget mode (evplp_group_adaptive_enable(.., 2)): every tile takes the first b_t of every window of gather calls
            self._check(self._lib.evplp_group_adaptive_enable(self._h, 2 if on else 0)); return
        f = self._lib.evplp_group_adaptive_enable_pt if path_trace else self._lib.evplp_group_adaptive_enable
        self._check(f(self._h, int(bool(on))))

    def adaptive_retire(self, scale, tile_rel_mse, min_batches=2, light_scale=1.0, mask_emitter=False) -> int:
        """retire the active tiles whose mean relative variance of scale * sums + light_scale * light is <= tile_rel_mse; returns how many"""
        tau, mb = _adaptive_retire_args(tile_rel_mse, min_batches)
        return self._check(self._lib.evplp_group_adaptive_retire(self._h, float(scale), float(light_scale), int(mask_emitter), tau, mb))

    def adaptive_tiles(self) -> np.ndarray:
        """int32 (ceil(H / 8), ceil(W / 8)), tile rows from the bottom: n_t of a retired tile, N of an active one (0: another rank's)"""
        out = np.zeros(((self.H + 7) // 8, (self.W + 7) // 8), dtype=np.int32)
        self._check(self._lib.evplp_group_adaptive_tiles(self._h, _ptr(out), out.size))
        return out

    def adaptive_set_budgets(self, samples_per_tile):
        """budget mode: samples of the next path_trace_batch calls per image tile, int32 (ceil(H / 8), ceil(W / 8)) in adaptive_tiles' layout, 0 .. 64"""
        b = np.ascontiguousarray(samples_per_tile, dtype=np.int32)
        self._check(self._lib.evplp_group_adaptive_set_budgets(self._h, _ptr(b), b.size))

    def adaptive_budgets(self) -> np.ndarray:
        """int32 (ceil(H / 8), ceil(W / 8)): the tiles' budgets, -1 = every sample of a call (0: another rank's)"""
        out = np.zeros(((self.H + 7) // 8, (self.W + 7) // 8), dtype=np.int32)
        self._check(self._lib.evplp_group_adaptive_budgets(self._h, _ptr(out), out.size))
        return out

    def adaptive_budget_window(self, window: int):
        """gather budget mode: the window S (1 .. 64) -- a tile with budget b takes the first min(b, S) of every S accumulating gather calls"""
        self._check(self._lib.evplp_group_adaptive_budget_window(self._h, int(window)))

    def adaptive_tile_noise(self, scale, light_scale=1.0, mask_emitter=False) -> np.ndarray:
        """float64 (ceil(H / 8), ceil(W / 8)): the mean relative variance of every tile, the figure adaptive_retire compares with tile_rel_mse"""
        out = np.zeros(((self.H + 7) // 8, (self.W + 7) // 8), dtype=np.float64)
        self._check(self._lib.evplp_group_adaptive_tile_noise(self._h, float(scale), float(light_scale), int(mask_emitter), _ptr(out), out.size))
        return out


def jitter_sequence(rng_offset: int, count: int, res_x: int, res_y: int) -> np.ndarray:
    out = np.zeros((count, 2), dtype=np.float32)
    rc = lib().evplp_jitter_sequence(rng_offset, count, res_x, res_y, _ptr(out))
    if rc != OK:
        raise EvplpError(rc, "evplp_jitter_sequence")
    return out


def progressive_step(n: int, alpha: float, clamp_start: float, n_vpl: int, n_light: int, radius: float, clamp: float,
                     pdf_mc: float, force_vsl=False, vsl_radius=0.0, vsl_inv_pi_r2=0.0):
    r, c, p, vr, vi = C.c_float(radius), C.c_float(clamp), C.c_float(pdf_mc), C.c_float(vsl_radius), C.c_float(vsl_inv_pi_r2)
    lib().evplp_progressive_step(n, alpha, clamp_start, n_vpl, n_light, C.byref(r), C.byref(c), C.byref(p), int(force_vsl), C.byref(vr), C.byref(vi))
    return r.value, c.value, p.value, vr.value, vi.value


def save_image(path: str, rgb_top_down: np.ndarray):
    a = _f32(rgb_top_down)
    h, w = a.shape[:2]
    rc = lib().evplp_save_image(path.encode(), w, h, _ptr(a))
    if rc != OK:
        raise EvplpError(rc, f"evplp_save_image({path})")


def load_pfm(path: str) -> np.ndarray:
    w, h = C.c_int32(), C.c_int32()
    rc = lib().evplp_load_pfm(path.encode(), C.byref(w), C.byref(h), None, 0)
    if rc != OK:
        raise EvplpError(rc, f"evplp_load_pfm({path})")
    out = np.empty((h.value, w.value, 3), dtype=np.float32)
    rc = lib().evplp_load_pfm(path.encode(), C.byref(w), C.byref(h), _ptr(out), out.size)
    if rc != OK:
        raise EvplpError(rc, f"evplp_load_pfm({path})")
    return out


def load_image(path: str) -> np.ndarray:
    """FloatImage::LoadPFM / LoadHDR by extension: float32 [h, w, 3], rows top to bottom."""
    w, h = C.c_int32(), C.c_int32()
    rc = lib().evplp_load_image(path.encode(), C.byref(w), C.byref(h), None, 0)
    if rc != OK:
        raise EvplpError(rc, f"evplp_load_image({path})")
    out = np.empty((h.value, w.value, 3), dtype=np.float32)
    rc = lib().evplp_load_image(path.encode(), C.byref(w), C.byref(h), _ptr(out), out.size)
    if rc != OK:
        raise EvplpError(rc, f"evplp_load_image({path})")
    return out


def error_heat(img: np.ndarray, ref: np.ndarray, max_error: float, relative: bool = False) -> np.ndarray:
    a, b = _f32(img), _f32(ref)
    out = np.empty_like(a)
    rc = lib().evplp_image_error_heat(a.shape[0] * a.shape[1], _ptr(a), _ptr(b), max_error, int(relative), _ptr(out))
    if rc != OK:
        raise EvplpError(rc, "evplp_image_error_heat")
    return out


def decode_image(path: str):
    """stbi_load(path, .., 3) of the reference (rt/rtcommon.h:144): (pixels uint8 [h, w, 3] top-down, channels in file)."""
    w, h, ch = C.c_int32(), C.c_int32(), C.c_int32()
    rc = lib().evplp_decode_image(path.encode(), C.byref(w), C.byref(h), C.byref(ch), None, C.c_size_t(0))
    if rc != OK:
        raise EvplpError(rc, f"evplp_decode_image({path})")
    out = np.empty((h.value, w.value, 3), dtype=np.uint8)
    rc = lib().evplp_decode_image(path.encode(), C.byref(w), C.byref(h), C.byref(ch), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes))
    if rc != OK:
        raise EvplpError(rc, f"evplp_decode_image({path})")
    return out, ch.value


SCENE_STYLES = {"easy": 0, "hard": 1, "textured": 2}


def synth_scene(out_dir: str, name: str = "conference_synth", target_triangles: int = 331000, seed: int = 1234,
                res_x: int = 1024, res_y: int = 1024, style=0) -> str:
    """style: 0 / "easy" = tessellated boxes, 1 / "hard" = furnished with curved and thin parts."""
    style = SCENE_STYLES[style] if isinstance(style, str) else int(style)
    rc = lib().evplp_synth_scene_ex(out_dir.encode(), name.encode(), target_triangles, seed, res_x, res_y, style)
    if rc < 0:
        raise EvplpError(rc, "evplp_synth_scene failed")
    return os.path.join(out_dir, name + ".json")


def render_json(json_path: str, overrides: Optional[str] = None, device: int = 0):
    err = C.create_string_buffer(1024)
    rc = lib().evplp_render_json(json_path.encode(), overrides.encode() if overrides else None, device, err, 1024)
    if rc != OK:
        raise EvplpError(rc, err.value.decode())
