"""ctypes binding of libhns.so (include/hns.h). Fails loudly when the library is missing: no fallback."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# HNS_LIBRARY: another build of the same library (A/B measurements of kernel variants, profiles/micro/exp)
_LIB_PATH = os.environ.get("HNS_LIBRARY") or os.path.join(_HERE, "lib", "libhns.so")

HNS_OK = 0
HNS_ERR_INVALID_ARGUMENT = -1
HNS_ERR_RUNTIME = -2
HNS_ERR_HIP = -3
HNS_ERR_NO_DEVICE = -4
HNS_ERR_TOPOLOGY = -5

HNS_GRID_DEFAULT = 0
HNS_GRID_HOST_ONLY = 1
HNS_GRID_SKIP_VALIDATE = 2


class HNSError(RuntimeError):
    """A libhns call returned a negative code. ``code`` is the HNS_ERR_* value."""

    def __init__(self, code: int, message: str):
        super().__init__(f"libhns error {code}: {message}")
        self.code = code
        self.message = message


class hns_field(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ncomp", C.c_int), ("host", C.POINTER(C.c_float))]


class hns_dist_stats(C.Structure):
    _fields_ = [("world", C.c_int), ("rank", C.c_int), ("peers", C.c_int), ("sweeps_per_exchange", C.c_int),
                ("boundary_leaves", C.c_uint64), ("interior_leaves", C.c_uint64), ("ghost_leaves", C.c_uint64),
                ("region_voxels_sent", C.c_uint64 * 4), ("bytes_sent", C.c_uint64 * 4), ("messages_sent", C.c_uint64), ("exchanges", C.c_uint64),
                ("halo_peers", C.c_uint64), ("packed_exchanges", C.c_uint64), ("chained", C.c_uint64)]


HNS_DIST_IPC_BLOB_BYTES = 2048
HNS_DIST_PLAN_ONLY = 1
HNS_DIST_LEAF_ORDER = 2


class hns_leaf_source(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ncomp", C.c_int), ("origins", C.c_void_p), ("n_leaves", C.c_uint64), ("masks", C.c_void_p), ("values", C.c_void_p)]


class hns_activity_field(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ncomp", C.c_int), ("tolerance", C.c_float)]


class hns_stats(C.Structure):
    _fields_ = [("count", C.c_uint64), ("nan_count", C.c_uint64), ("min", C.c_float), ("max", C.c_float), ("max_abs", C.c_float), ("reserved", C.c_uint32),
                ("sum", C.c_double), ("sum_sq", C.c_double)]


class hns_stats_field(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ncomp", C.c_int)]


class hns_solve_control(C.Structure):
    _fields_ = [("rel_tol", C.c_float), ("abs_tol", C.c_float), ("check_every", C.c_int)]


class hns_solve_report(C.Structure):
    _fields_ = [("iterations", C.c_int), ("checks", C.c_int), ("converged", C.c_int), ("initial", hns_stats), ("final", hns_stats)]


class hns_solve_method(C.Structure):
    _fields_ = [("method", C.c_int), ("pre", C.c_int), ("post", C.c_int), ("coarse_iterations", C.c_int), ("max_levels", C.c_int), ("omega", C.c_float)]


class hns_splat_spec(C.Structure):
    _fields_ = [("kernel", C.c_int), ("mode", C.c_int), ("radius", C.c_float), ("d_radius", C.c_void_p), ("min_weight", C.c_float)]


class hns_point_collision(C.Structure):
    _fields_ = [("mode", C.c_int), ("threshold", C.c_float), ("skin", C.c_float), ("iterations", C.c_int)]


HNS_COLLIDE_STOP, HNS_COLLIDE_PUSH, HNS_COLLIDE_KILL = 1, 2, 3


class hns_point_motion_info(C.Structure):
    _fields_ = [("capacity", C.c_uint64), ("xyz", C.c_void_p), ("vel", C.c_void_p), ("age", C.c_void_p), ("status", C.c_void_p), ("hit", C.c_void_p)]


class hns_point_motion_spec(C.Structure):
    _fields_ = [("mode", C.c_int), ("gravity", C.c_float * 3), ("drag", C.c_float), ("restitution", C.c_float), ("friction", C.c_float), ("max_age", C.c_float),
                ("threshold", C.c_float), ("skin", C.c_float), ("iterations", C.c_int)]


HNS_MOTION_FREE, HNS_MOTION_STICK, HNS_MOTION_BOUNCE, HNS_MOTION_KILL = 0, 1, 2, 3


class hns_turbulence_spec(C.Structure):
    _fields_ = [("amplitude", C.c_float), ("frequency", C.c_float), ("offset", C.c_float * 3), ("octaves", C.c_int), ("lacunarity", C.c_float), ("gain", C.c_float),
                ("seed", C.c_uint), ("control", C.c_char_p), ("control_lo", C.c_float), ("control_hi", C.c_float)]


class hns_decay_spec(C.Structure):
    _fields_ = [("name", C.c_char_p), ("rate", C.c_float), ("target", C.c_float)]


class hns_shaping_curl(C.Structure):
    _fields_ = [("c", C.c_float * 3)]


class hns_diffusion_term(C.Structure):
    _fields_ = [("name", C.c_char_p), ("coefficient", C.c_float)]


class hns_diffusion_spec(C.Structure):
    _fields_ = [("iterations", C.c_int), ("method", C.c_int), ("viscosity", C.c_float), ("collide", C.c_int), ("threshold", C.c_float)]


class hns_diffusion_schedule(C.Structure):
    _fields_ = [("a", C.c_float), ("r", C.c_float * 7), ("rho", C.c_float), ("omega", C.c_float * 256)]


HNS_DIFFUSION_JACOBI, HNS_DIFFUSION_CHEBYSHEV = 0, 1


class hns_point_order_info(C.Structure):
    _fields_ = [("perm", C.c_void_p), ("keys", C.c_void_p), ("leaf_start", C.c_void_p), ("n", C.c_uint64), ("n_leaves", C.c_uint64), ("capacity", C.c_uint64),
                ("level", C.c_int)]


class hns_birth_spec(C.Structure):
    _fields_ = [("threshold", C.c_float), ("rate", C.c_float), ("max_per_voxel", C.c_uint32), ("seed", C.c_uint32), ("fill", C.c_int)]


class hns_point_population_info(C.Structure):
    _fields_ = [("slot", C.c_void_p), ("counters", C.c_void_p), ("n", C.c_uint64), ("capacity", C.c_uint64)]


class hns_combustion_params(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("expansionRate", "temperatureRelease", "buoyancyStrength", "ambientTemp", "vorticityScale", "factorScale")]


_vp, _i, _u64, _f = C.c_void_p, C.c_int, C.c_uint64, C.c_float
_fp = C.c_void_p  # device or host float* passed as an address
_ip = C.POINTER(C.c_int)

# name -> (restype, argtypes): every symbol include/hns.h declares
SIGNATURES = {
    "hns_last_error": (C.c_char_p, []),
    "hns_version": (_i, []),
    "hns_device_count": (_i, []),
    "hns_trim_memory": (_i, []),
    "hns_set_option": (_i, [C.c_char_p, C.c_char_p]),
    "hns_get_option": (C.c_char_p, [C.c_char_p]),
    "hns_grid_create": (_vp, [_vp, _u64, _f, C.c_uint, _ip]),
    "hns_grid_create_from_leaves": (_vp, [_vp, _u64, _f, C.c_uint, _ip]),
    "hns_grid_destroy": (None, [_vp]),
    "hns_grid_leaf_count": (_u64, [_vp]),
    "hns_grid_voxel_count": (_u64, [_vp]),
    "hns_grid_voxel_size": (_f, [_vp]),
    "hns_grid_set_active_leaves": (_i, [_vp, _u64]),
    "hns_grid_set_active_range": (_i, [_vp, _u64, _u64]),
    "hns_grid_active_leaves": (_u64, [_vp]),
    "hns_grid_set_outside_element": (_i, [_vp, _u64]),
    "hns_grid_offsets": (_i, [_vp, _vp, _u64, _vp]),
    "hns_grid_neighbor_table": (_i, [_vp, _vp]),
    "hns_grid_coords": (_i, [_vp, _vp]),
    "hns_grid_release_cache": (_i, [_vp]),
    "hns_grid_matches": (_i, [_vp, _vp, _u64, C.c_uint]),
    "hns_grid_export_nanovdb": (_i, [_vp, _vp, _u64, _vp]),
    "hns_grid_launch_tables": (_i, [_vp, _vp]),
    "hns_gather_leaves": (_i, [_vp, _u64, _vp, _u64, _vp, _i, _i, _vp]),
    "hns_scatter_leaves": (_i, [_vp, _u64, _i, C.POINTER(C.c_void_p)]),
    "hns_dilate_leaves": (_i, [_vp, _u64, _vp, _i, _vp, _u64, C.POINTER(C.c_uint64)]),
    "hns_dilate_leaf_masks": (_i, [_vp, _u64, _vp, _i, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "hns_union_leaves": (_i, [_vp, _u64, _vp, _u64, _vp, _u64, C.POINTER(C.c_uint64)]),
    "hns_add_leaves": (_i, [_vp, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _i, _vp, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "hns_deactivate_leaf_masks": (_i, [_u64, _vp, C.POINTER(hns_activity_field), C.POINTER(C.c_void_p), _i, _vp, C.POINTER(C.c_uint64)]),
    "hns_leaf_stats": (_i, [_u64, _vp, _vp, _i, _vp]),
    "hns_compute_sim": (_i, [_vp, C.POINTER(hns_field), _i, _i, _f, _f, C.POINTER(hns_combustion_params), _i, _vp]),
    "hns_compute_sim_resident": (_i, [_vp, C.POINTER(hns_field), _i, C.c_char_p, C.POINTER(C.c_int), _i, _f, _f, C.POINTER(hns_combustion_params), _i, _vp]),
    "hns_advect_index_grid": (_i, [_vp, C.POINTER(hns_field), _i, _f, _f, _vp]),
    "hns_advect_index_grid_velocity": (_i, [_vp, C.POINTER(hns_field), _i, _f, _f, _vp]),
    "hns_project_non_divergent": (_i, [_vp, C.POINTER(hns_field), _i, _u64, _f, _vp]),
    "hns_divergence": (_i, [_vp, C.POINTER(hns_field), _i, _f, _vp]),
    "hns_sim_create": (_vp, [_vp, C.POINTER(C.c_char_p), _i, _ip]),
    "hns_sim_destroy": (None, [_vp]),
    "hns_sim_upload": (_i, [_vp, C.POINTER(hns_field), _i, _vp]),
    "hns_sim_download": (_i, [_vp, C.POINTER(hns_field), _i, _vp]),
    "hns_sim_substep": (_i, [_vp, _i, _f, _f, C.POINTER(hns_combustion_params), _i, _vp]),
    "hns_sim_core_substep": (_i, [_vp, _i, _f, _f, _vp]),
    "hns_sim_advect": (_i, [_vp, C.POINTER(C.c_char_p), _i, _i, _f, _f, _vp]),
    "hns_sim_sample_points": (_i, [_vp, C.POINTER(C.c_char_p), _i, _i, _fp, _u64, C.POINTER(C.c_void_p), _vp]),
    "hns_sim_trace_points": (_i, [_vp, _fp, _u64, _f, _f, _i, _i, _vp, _vp]),
    "hns_sim_splat_points": (_i, [_vp, C.POINTER(C.c_char_p), _i, _fp, _fp, C.POINTER(C.c_void_p), _u64, _i, _i, _vp, _vp, _vp]),
    "hns_sim_pressure_solve": (_i, [_vp, _i, _f, _vp]),
    "hns_sim_timing": (_i, [_vp, _i]),
    "hns_sim_pressure_time": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_longlong)]),
    "hns_sim_stage_timing": (_i, [_vp, _i]),
    "hns_sim_stage_times": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_longlong)]),
    "hns_sim_lookahead_counts": (_i, [_vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "hns_sim_substep_plan": (_i, [_vp, C.POINTER(hns_combustion_params), _i, C.c_char_p, C.c_uint64]),
    "hns_sim_velocity_ptr": (_vp, [_vp]),
    "hns_sim_field_ptr": (_vp, [_vp, C.c_char_p]),
    "hns_sim_divergence_ptr": (_vp, [_vp]),
    "hns_sim_pressure_ptr": (_vp, [_vp]),
    "hns_sim_set_active_masks": (_i, [_vp, _vp, _vp]),
    "hns_sim_active_masks": (_i, [_vp, _vp, _vp]),
    "hns_sim_regrid": (_vp, [_vp, _i, _vp, _u64, _vp, _vp, _vp, _ip]),
    "hns_sim_regrid_times": (_i, [_vp, C.POINTER(C.c_float)]),
    "hns_sim_regrid_sourced": (_vp, [_vp, _i, C.POINTER(hns_leaf_source), _i, _vp, _u64, _vp, _vp, _vp, _ip]),
    "hns_sim_regrid_seeded": (_vp, [_vp, _i, C.POINTER(hns_leaf_source), _i, _fp, _u64, C.POINTER(C.c_uint64), _vp, _u64, _vp, _vp, _vp, _ip]),
    "hns_sim_deactivate": (_i, [_vp, C.POINTER(hns_activity_field), _i, C.POINTER(C.c_uint64), _vp]),
    "hns_sim_stats": (_i, [_vp, C.POINTER(hns_stats_field), _i, _i, _vp, _vp]),
    "hns_sim_residual": (_i, [_vp, _f, C.POINTER(hns_stats), _vp]),
    "hns_sim_set_solve_control": (_i, [_vp, C.POINTER(hns_solve_control)]),
    "hns_sim_solve_report": (_i, [_vp, C.POINTER(hns_solve_report), _vp, _i, _ip]),
    "hns_sim_set_solve_method": (_i, [_vp, C.POINTER(hns_solve_method)]),
    "hns_sim_solve_levels": (_i, [_vp, _ip, C.POINTER(C.c_uint64), _i]),
    "hns_dev_advect_vector": (_i, [_vp, _fp, _fp, _fp, _i, _f, _f, _vp]),
    "hns_dev_advect_scalar": (_i, [_vp, _fp, _fp, _fp, _fp, _i, _f, _f, _vp]),
    "hns_dev_advect_scalars": (_i, [_vp, _fp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _i, _fp, _i, _f, _f, _vp]),
    "hns_dev_advect_scalar_multi": (_i, [_vp, _fp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _i, _fp, _i, _f, _f, _vp]),
    "hns_dev_advect_scalars_ahead": (_i, [_vp, _fp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _i, _fp, _f, _f, _vp]),
    "hns_dev_sample_points": (_i, [_vp, C.POINTER(C.c_void_p), _ip, _i, _fp, _u64, C.POINTER(C.c_void_p), _vp]),
    "hns_dev_trace_points": (_i, [_vp, _fp, _fp, _u64, _f, _f, _i, _i, _vp, _vp]),
    "hns_dev_trace_points_collide": (_i, [_vp, _fp, _fp, _fp, _u64, _f, _f, _i, _i, C.POINTER(hns_point_collision), _vp, _vp, _vp]),
    "hns_sim_trace_points_collide": (_i, [_vp, _fp, _u64, _f, _f, _i, _i, C.POINTER(hns_point_collision), _vp, _vp, _vp]),
    "hns_point_motion_create": (_vp, [_u64, _ip]),
    "hns_point_motion_destroy": (None, [_vp]),
    "hns_point_motion_set_stream": (_i, [_vp, _vp]),
    "hns_point_motion_get": (_i, [_vp, C.POINTER(hns_point_motion_info)]),
    "hns_point_motion_step": (_i, [_vp, _vp, _u64, _f, _f, _i, C.POINTER(hns_point_motion_spec)]),
    "hns_shaping_create": (_vp, [_ip]),
    "hns_shaping_destroy": (None, [_vp]),
    "hns_shaping_set_stream": (_i, [_vp, _vp]),
    "hns_shaping_apply": (_i, [_vp, _vp, _f, C.POINTER(hns_turbulence_spec), C.POINTER(hns_decay_spec), _i]),
    "hns_shaping_curl_host": (_i, [C.POINTER(hns_turbulence_spec), _i, _i, _i, C.POINTER(hns_shaping_curl)]),
    "hns_diffusion_create": (_vp, [_ip]),
    "hns_diffusion_destroy": (None, [_vp]),
    "hns_diffusion_set_stream": (_i, [_vp, _vp]),
    "hns_diffusion_apply": (_i, [_vp, _vp, _f, _f, C.POINTER(hns_diffusion_spec), C.POINTER(hns_diffusion_term), _i]),
    "hns_diffusion_schedule_host": (_i, [_f, _f, _f, _i, C.POINTER(hns_diffusion_schedule)]),
    "hns_dev_splat_points": (_i, [_vp, C.POINTER(C.c_void_p), _ip, _i, _fp, C.POINTER(C.c_void_p), _u64, _i, _vp, _vp, _vp]),
    "hns_grid_splat_points": (_i, [_vp, C.POINTER(C.c_void_p), _ip, _i, _fp, C.POINTER(C.c_void_p), _u64, _i, _vp, _i, _vp, C.POINTER(C.c_uint64)]),
    "hns_grid_set_splat_spec": (_i, [_vp, C.POINTER(hns_splat_spec)]),
    "hns_sim_set_splat_spec": (_i, [_vp, C.POINTER(hns_splat_spec)]),
    "hns_grid_get_splat_spec": (_i, [_vp, C.POINTER(hns_splat_spec)]),
    "hns_sim_get_splat_spec": (_i, [_vp, C.POINTER(hns_splat_spec)]),
    "hns_grid_splat_points_spec": (_i, [_vp, C.POINTER(hns_splat_spec), C.POINTER(C.c_void_p), _ip, _i, _fp, C.POINTER(C.c_void_p), _u64, _i, _vp, _i, _vp,
                                        C.POINTER(C.c_uint64)]),
    "hns_point_leaves": (_i, [_fp, _u64, _vp, _vp, _u64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hns_dev_point_leaves": (_i, [_i, _fp, _u64, _vp, _vp, _u64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _vp]),
    "hns_point_order_create": (_vp, [_vp, _u64, _ip]),
    "hns_point_order_destroy": (None, [_vp]),
    "hns_point_order_set_stream": (_i, [_vp, _vp]),
    "hns_point_order_sort": (_i, [_vp, _fp, _u64, _i]),
    "hns_point_order_get": (_i, [_vp, C.POINTER(hns_point_order_info)]),
    "hns_point_order_gather": (_i, [_vp, _vp, _vp, _i]),
    "hns_point_order_scatter": (_i, [_vp, _vp, _vp, _i]),
    "hns_point_order_splat": (_i, [_vp, C.POINTER(C.c_void_p), _ip, _i, _fp, C.POINTER(C.c_void_p), _i, _i, _vp, _vp]),
    "hns_point_order_splat_sim": (_i, [_vp, _vp, C.POINTER(C.c_char_p), _i, _fp, _fp, C.POINTER(C.c_void_p), _i, _i, _i, _vp, _vp]),
    "hns_grid_sort_points": (_i, [_vp, _fp, _u64, _i, _vp, _vp, _vp]),
    "hns_point_order_cells": (_i, [_vp, C.POINTER(C.c_void_p)]),
    "hns_point_order_neighbours": (_i, [_vp, _fp, _i, _f, _vp, _fp, _fp]),
    "hns_grid_point_neighbours": (_i, [_vp, _fp, _u64, _f, _vp, _fp, _fp]),
    "hns_point_population_create": (_vp, [_vp, _u64, _ip]),
    "hns_point_population_destroy": (None, [_vp]),
    "hns_point_population_set_stream": (_i, [_vp, _vp]),
    "hns_point_population_set_live": (_i, [_vp, _u64]),
    "hns_point_population_select": (_i, [_vp, _vp, _u64, _i]),
    "hns_point_population_compact": (_i, [_vp, _vp, _vp, _i, C.POINTER(C.c_uint32)]),
    "hns_point_population_birth": (_i, [_vp, _fp, _vp, C.POINTER(hns_birth_spec), _fp, _vp, _u64, _i]),
    "hns_point_population_birth_sim": (_i, [_vp, _vp, C.c_char_p, _i, C.POINTER(hns_birth_spec), _fp, _vp, _u64, _i]),
    "hns_point_population_get": (_i, [_vp, C.POINTER(hns_point_population_info)]),
    "hns_point_population_counts": (_i, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hns_grid_birth_points": (_i, [_vp, _fp, _vp, C.POINTER(hns_birth_spec), _u64, _fp, _vp, _u64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hns_dev_divergence": (_i, [_vp, _fp, _fp, _f, _vp]),
    "hns_dev_rbgs_color": (_i, [_vp, _fp, _fp, _f, _f, _i, _vp]),
    "hns_dev_rbgs_iterate": (_i, [_vp, _fp, _fp, _fp, _f, _f, _i, _ip, _vp]),
    "hns_dev_subtract_pressure_gradient": (_i, [_vp, _fp, _fp, _fp, _fp, _i, _f, _vp]),
    "hns_dev_combustion_oxygen": (_i, [_fp] * 9 + [_f, _f, _u64, _vp]),
    "hns_dev_temperature_buoyancy": (_i, [_fp, _fp, _fp, _f, _f, _f, _u64, _vp]),
    "hns_dev_vorticity_confinement": (_i, [_vp, _fp, _fp, _f, _f, _f, _f, _vp]),
    "hns_dev_enforce_collision_boundaries": (_i, [_vp, _fp, _fp, _f, _vp]),
    "hns_dev_pack_leaves": (_i, [_fp, _vp, _u64, _fp, _i, _vp]),
    "hns_dev_unpack_leaves": (_i, [_fp, _vp, _u64, _fp, _i, _vp]),
    "hns_dev_field_stats": (_i, [_vp, _fp, _i, _vp, _vp, _vp]),
    "hns_dev_residual": (_i, [_vp, _fp, _fp, _f, _fp, _vp, _vp]),
    "hns_dist_create": (_vp, [_vp, _u64, _i, _i, _f, _i, _i, C.c_uint, _ip]),
    "hns_dist_destroy": (None, [_vp]),
    "hns_dist_unique_id": (_i, [_vp]),
    "hns_dist_connect_rccl": (_i, [_vp, _vp]),
    "hns_dist_connect_local": (_i, [C.POINTER(C.c_void_p), _i]),
    "hns_dist_connect_loopback": (_i, [_vp]),
    "hns_dist_connect_loopback_rccl": (_i, [_vp]),
    "hns_dist_ipc_export": (_i, [_vp, _vp]),
    "hns_dist_connect_ipc": (_i, [_vp, _vp]),
    "hns_dist_owned_leaves": (_u64, [_vp]),
    "hns_dist_first_owned_leaf": (_u64, [_vp]),
    "hns_dist_owned_leaf_ids": (_i, [_vp, _vp]),
    "hns_dist_partition_axis": (_i, [_vp]),
    "hns_dist_one_sided_sweeps": (_i, [_u64, _i]),
    "hns_dist_info": (_i, [_vp, C.POINTER(hns_dist_stats)]),
    "hns_dist_local_leaves": (_i, [_vp, _vp]),
    "hns_dist_peer_rank": (_i, [_vp, _i]),
    "hns_dist_peer_region": (_i, [_vp, _i, _i, _i, _vp, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hns_dist_upload": (_i, [_vp, _vp, C.POINTER(C.c_void_p), _vp]),
    "hns_dist_download": (_i, [_vp, _vp, C.POINTER(C.c_void_p), _vp, _vp]),
    "hns_dist_download_local": (_i, [_vp, _i, _vp, _vp]),
    "hns_dist_core_substep": (_i, [_vp, _i, _f, _vp]),
    "hns_dist_local_core_substep": (_i, [C.POINTER(C.c_void_p), _i, _i, _f, _vp]),
    "hns_dist_sim_substep": (_i, [_vp, _i, _f, _vp, _ip, _i, _vp]),
    "hns_dist_local_sim_substep": (_i, [C.POINTER(C.c_void_p), _i, _i, _f, _vp, _ip, _i, _vp]),
    "hns_dist_timing": (_i, [_vp, _i]),
    "hns_dist_pressure_time": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_longlong)]),
    "hns_dist_synchronize": (_i, [_vp, _vp]),
    "hns_dev_time_rbgs": (_i, [_vp, _fp, _fp, _fp, _f, _f, _i, _i, C.POINTER(C.c_float), _vp]),
    "hns_grid_rbgs_plan": (_i, [_vp, _i, C.c_char_p, C.c_uint64, _ip, _ip]),
}

_lib = None


def library_path() -> str:
    return _LIB_PATH


def load_library() -> C.CDLL:
    """Load libhns.so and declare every signature. Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise FileNotFoundError(
            f"{_LIB_PATH} is missing: build it with `make -C hnanosolver_amd/csrc` (or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "hnanosolver_amd has no CPU fallback."
        )
    lib_ = C.CDLL(_LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib_, name)  # AttributeError here means the .so and include/hns.h disagree
        fn.restype = res
        fn.argtypes = args
    _lib = lib_
    return lib_


class _LazyLib:
    def __getattr__(self, name):
        return getattr(load_library(), name)


lib = _LazyLib()


def set_option(name: str, value=None) -> None:
    """hns_set_option: switch an alternative kernel form / data-movement strategy (include/hns.h); value None = default."""
    check(load_library().hns_set_option(name.encode(), None if value is None else str(value).encode()))


def get_option(name: str):
    v = load_library().hns_get_option(name.encode())
    return None if v is None else v.decode()


def check(code: int) -> None:
    if code < 0:
        raise HNSError(code, load_library().hns_last_error().decode("utf-8", "replace"))
