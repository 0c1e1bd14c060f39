"""ctypes loader for liborbhip.so (the C ABI declared in include/orbhip.h).

The library is built in-tree by `__graft_entry__.build()` / `make -C
orb_slam2_comment_amd/csrc`.  There is no CPU fallback: if the shared object is
missing or fails to load, importing a compute entry point raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liborbhip.so")

OK, E_ARG, E_HIP, E_CAPACITY, E_SIZE, E_NODEVICE = 0, -1, -2, -3, -4, -5
MAX_LEVELS = 16

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
NO_NODE = 0xFFFFFFFF   # ORBHIP_NO_NODE
QUERY_DTYPE = np.dtype([("valid", "<i4"), ("u", "<f4"), ("v", "<f4"), ("radius", "<f4"),
                        ("min_level", "<i4"), ("max_level", "<i4"), ("ur", "<f4"),
                        ("level_aux", "<i4"), ("angle", "<f4"), ("observed", "<i4")])
assert KP_DTYPE.itemsize == 28 and QUERY_DTYPE.itemsize == 40


class FrameView(C.Structure):
    _fields_ = [("n", C.c_int32), ("keys", C.c_void_p), ("desc", C.c_void_p),
                ("u_right", C.c_void_p), ("min_x", C.c_float), ("min_y", C.c_float),
                ("max_x", C.c_float), ("max_y", C.c_float), ("grid_inv_w", C.c_float),
                ("grid_inv_h", C.c_float), ("n_levels", C.c_int32),
                ("scale_factors", C.c_void_p)]


class Camera(C.Structure):
    """orbhip_camera: the Frame statics the projection prologues read."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("mbf", C.c_float),
                ("mb", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float),
                ("max_y", C.c_float), ("n_levels", C.c_int32), ("log_scale_factor", C.c_float),
                ("scale_factors", C.c_float * MAX_LEVELS)]


class LocalMapTables(C.Structure):
    """orbhip_local_map_tables: the bank, graph and map-point tables of orbhip_update_local_map* (read only)."""
    _fields_ = [(k, C.c_void_p) for k in ("slot_point", "n", "kf_bad", "covis", "child_start", "child", "parent", "obs_start",
                                          "obs_kf", "flags", "world", "normal", "max_dist", "min_dist", "point_desc")]


class LocalMapIO(C.Structure):
    """orbhip_local_map_io: the in/out lists and the outputs of orbhip_update_local_map*."""
    _fields_ = [(k, C.c_void_p) for k in ("frame_point", "frame_n", "local_kf", "n_local_kf", "votes", "local_point", "world_l",
                                          "normal_l", "max_dist_l", "min_dist_l", "desc_l", "flags_l", "np_l", "taken",
                                          "report")]


class LocalMapTrack(C.Structure):
    """orbhip_local_map_track: the current frames and the search outputs of orbhip_track_local_map_device."""
    _fields_ = [(k, C.c_void_p) for k in ("Tcw", "kps", "desc", "u_right", "q", "assign", "nmatches")]


class CovisTables(C.Structure):
    """orbhip_covis_tables: the bank and map-point tables orbhip_update_connections* reads."""
    _fields_ = [(k, C.c_void_p) for k in ("slot_point", "n", "obs_start", "obs_kf", "flags")]


class CovisState(C.Structure):
    """orbhip_covis_state: the covisibility graph orbhip_update_connections* maintains (in/out)."""
    _fields_ = [(k, C.c_void_p) for k in ("conn_w", "ord_kf", "ord_w", "n_ord", "covis", "first_conn", "parent")]


class CullTables(C.Structure):
    """orbhip_cull_tables: what orbhip_cull_map_points* / orbhip_cull_key_frames* read."""
    _fields_ = [(k, C.c_void_p) for k in ("kps", "u_right", "depth", "n", "obs_start", "obs_kf", "obs_idx", "ref_obs",
                                          "not_erase")]


class CullIO(C.Structure):
    """orbhip_cull_io: the tables the culling entries maintain (in/out) and the observation table out."""
    _fields_ = [(k, C.c_void_p) for k in ("slot_point", "flags", "kf_bad", "to_be_erased", "child_start", "child",
                                          "obs_start_out", "obs_kf_out", "obs_idx_out", "ref_obs_out")]


class Sim3Tables(C.Structure):
    """orbhip_sim3_tables: the bank and map-point tables orbhip_sim3_setup_device / orbhip_sim3_ransac read."""
    _fields_ = [(k, C.c_void_p) for k in ("slot_point", "obs_start", "obs_kf", "obs_idx", "flags", "world", "Tcw", "kps", "n")]


class Sim3Solvers(C.Structure):
    """orbhip_sim3_solvers: the per-candidate solver state on the device (written by setup, advanced by iterate)."""
    _fields_ = [(k, C.c_void_p) for k in ("x1", "x2", "p1", "p2", "max_err1", "max_err2", "slot1", "n_corr", "n1", "limit",
                                          "state")]


class LbaTables(C.Structure):
    """orbhip_lba_tables: what orbhip_local_bundle_adjustment* reads; Tcw and world are in/out."""
    _fields_ = [(k, C.c_void_p) for k in ("slot_point", "n", "kf_bad", "obs_start", "obs_kf", "obs_idx", "flags", "kps", "u_right",
                                          "ord_kf", "n_ord", "Tcw", "world")]


class LbaOut(C.Structure):
    """orbhip_lba_out: the three lists, the erase rows and the report of orbhip_local_bundle_adjustment*."""
    _fields_ = [(k, C.c_void_p) for k in ("local_kf", "fixed_kf", "local_point", "erase", "report")]


class EgTables(C.Structure):
    """orbhip_eg_tables: what orbhip_optimize_essential_graph* reads; Tcw and world are in/out."""
    _fields_ = [(k, C.c_void_p) for k in ("kf_bad", "kf_id", "parent", "conn_w", "ord_kf", "ord_w", "n_ord", "loop_start", "loop_kf",
                                          "lc_start", "lc_kf", "corrected", "non_corrected", "in_corrected", "in_non_corrected", "flags",
                                          "ref_kf", "corrected_by_kf", "corrected_ref", "Tcw", "world")]


class EgOut(C.Structure):
    """orbhip_eg_out: the point list, vScw, vCorrectedSwc and the report of orbhip_optimize_essential_graph*."""
    _fields_ = [(k, C.c_void_p) for k in ("point_list", "Scw", "Swc", "report")]


class GbaTables(C.Structure):
    """orbhip_gba_tables: what orbhip_global_bundle_adjustment* reads; Tcw and world are in/out (ORBHIP_GBA_IN_PLACE)."""
    _fields_ = [(k, C.c_void_p) for k in ("kf_bad", "kf_id", "obs_start", "obs_kf", "obs_idx", "flags", "kps", "u_right", "Tcw", "world")]


class GbaOut(C.Structure):
    """orbhip_gba_out: the staged poses and points with their marks, the point list and the report."""
    _fields_ = [(k, C.c_void_p) for k in ("TcwGBA", "posGBA", "kf_mark", "pt_mark", "point_list", "report")]


class GbaApply(C.Structure):
    """orbhip_gba_apply: the arrays of orbhip_apply_global_ba*."""
    _fields_ = [(k, C.c_void_p) for k in ("origins", "parent", "kf_bad", "pt_mark", "posGBA", "flags", "ref_kf", "kf_mark", "TcwGBA",
                                          "Tcw", "world", "TcwBefGBA", "report")]


class PnpParams(C.Structure):
    """orbhip_pnp_params: the arguments of PnPsolver::SetRansacParameters."""
    _fields_ = [("prob", C.c_double), ("min_inliers", C.c_int32), ("max_its", C.c_int32), ("min_set", C.c_int32),
                ("epsilon", C.c_float), ("th2", C.c_float)]


class PnpMap(C.Structure):
    """orbhip_pnp_map: the map-point tables (and, for slot matches, the bank's slot_point) the PnP setup reads."""
    _fields_ = [(k, C.c_void_p) for k in ("flags", "world", "slot_point")]


class PnpSolvers(C.Structure):
    """orbhip_pnp_solvers: the per-candidate solver record on the device (written by setup, advanced by iterate)."""
    _fields_ = [(k, C.c_void_p) for k in ("p2d", "p3d", "max_err", "kp_index", "n_corr", "min_inliers", "limit", "state",
                                          "best_inliers", "best_Tcw")]


POINT_PRESENT, POINT_OBSERVED = 1, 2
COLOR_BGR, COLOR_RGB = 0, 1
DEPTH_U16, DEPTH_F32 = 0, 1
SEED_ALL, SEED_CLOSEST = 0, 1
# ORBHIP_NEWPOINT_*: d_status of orbhip_create_new_map_points*, one code per way out of the loop body
(NEWPOINT_CREATED, NEWPOINT_NO_MATCH, NEWPOINT_LOW_PARALLAX, NEWPOINT_W_ZERO, NEWPOINT_BEHIND_1, NEWPOINT_BEHIND_2,
 NEWPOINT_REPROJ_1, NEWPOINT_REPROJ_2, NEWPOINT_ZERO_DIST, NEWPOINT_SCALE) = range(10)
# ORBHIP_UPDATE_* (the `what` mask) and ORBHIP_MAPPOINT_* (d_status) of orbhip_update_map_points*
UPDATE_DESCRIPTOR, UPDATE_NORMAL_DEPTH = 1, 2
(MAPPOINT_UPDATED, MAPPOINT_BAD, MAPPOINT_NO_OBSERVATION, MAPPOINT_NO_DESCRIPTOR, MAPPOINT_BAD_REF,
 MAPPOINT_TOO_MANY) = range(6)
# ORBHIP_LOCALMAP_*: report[0] (status) and report[5] (walk_end) of orbhip_update_local_map*
LOCALMAP_OK, LOCALMAP_NO_VOTES, LOCALMAP_ALL_BAD = range(3)
LOCALMAP_WALK_EXHAUSTED, LOCALMAP_WALK_LIMIT, LOCALMAP_WALK_PARENT = range(3)
# ORBHIP_CONNECTIONS_*: report[0] of orbhip_update_connections*
CONNECTIONS_OK, CONNECTIONS_EMPTY = range(2)
CONNECTIONS_REPORT = ("status", "n_voted", "n_ordered", "max_row", "max_votes", "parent_set", "n_resorted", "fallback")
# ORBHIP_CULLPOINT_*: d_status of orbhip_cull_map_points*; ORBHIP_CULLKF_*: report[0] of orbhip_cull_key_frames*
CULLPOINT_KEPT, CULLPOINT_ALREADY_BAD, CULLPOINT_BAD_RATIO, CULLPOINT_BAD_OBS, CULLPOINT_DROPPED_OLD = range(5)
CULLKF_NOT_CULLED, CULLKF_CULLED, CULLKF_SKIPPED_ID0, CULLKF_SKIPPED_ENTRY, CULLKF_NOT_ERASE = range(5)
CULLKF_REPORT = ("status", "n_mps", "n_redundant", "n_erased", "n_bad", "n_resorted", "n_children", "fallback")
# ORBHIP_SIM3_MATCH_*: what d_matched12 of orbhip_sim3_setup_device holds; ORBHIP_SIM3_*: report[0] of orbhip_sim3_iterate_device
SIM3_MATCH_POINTS, SIM3_MATCH_SLOTS = range(2)
SIM3_RETURNED, SIM3_CONTINUE, SIM3_NO_MORE, SIM3_TOO_FEW = range(4)
SIM3_REPORT = ("status", "n_corr", "limit", "iterations", "best_inliers", "returned_iteration", "n_inliers", "reserved")
# ORBHIP_PNP_MATCH_*: what d_matches of orbhip_pnp_setup_device holds; ORBHIP_PNP_*: report[0] of orbhip_pnp_iterate_device
PNP_MATCH_POINTS, PNP_MATCH_SLOTS = range(2)
PNP_REFINED, PNP_BEST, PNP_NO_MORE, PNP_TOO_FEW = range(4)
PNP_REPORT = ("status", "n_corr", "limit", "iterations", "best_inliers", "returned_iteration", "n_inliers", "min_inliers")
# ORBHIP_POSEOPT_*: mode and flags of orbhip_pose_optimization_device, report[0]
POSEOPT_PLAIN, POSEOPT_DISCARD, POSEOPT_LOCAL_MAP = range(3)
POSEOPT_ONLY_TRACKING, POSEOPT_STEREO = 1, 2
POSEOPT_OK, POSEOPT_TOO_FEW, POSEOPT_ONE_ROUND = range(3)
POSEOPT_REPORT = ("status", "n_initial", "n_bad", "returned", "rounds", "iterations", "count_a", "count_b")
# ORBHIP_SIM3OPT_*: report[0] of orbhip_optimize_sim3_device
SIM3OPT_OK, SIM3OPT_TOO_FEW, SIM3OPT_SKIPPED = range(3)
SIM3OPT_REPORT = ("status", "n_correspondences", "n_bad", "n_in", "iterations_1", "iterations_2", "reserved_0", "reserved_1")
# ORBHIP_LBA_*: report[0] of orbhip_local_bundle_adjustment_device
LBA_OK, LBA_STOPPED, LBA_ONE_ROUND, LBA_CAPACITY = range(4)
LBA_MAX_LOCAL = 128
LBA_REPORT = ("status", "n_local_kf", "n_fixed_kf", "n_local_points", "n_mono", "n_stereo", "n_level1", "n_erase", "iterations_1",
              "trials_1", "iterations_2", "trials_2", "poses_1", "poses_2", "reserved_0", "stop_samples")
# ORBHIP_EG_*: report[0] of orbhip_optimize_essential_graph_device
EG_OK, EG_CAPACITY, EG_SINGULAR = range(3)
EG_MAX_KF = 512
EG_REPORT = ("status", "n_vertices", "n_loop_connection", "n_spanning_tree", "n_old_loop", "n_covisibility", "skipped_inserted",
             "skipped_weight", "iterations", "trials", "unknowns", "n_points", "skipped_null", "reserved_0", "reserved_1", "reserved_2")
# ORBHIP_GBA_*: mode and report[0] of orbhip_global_bundle_adjustment_device
GBA_IN_PLACE, GBA_STAGED = range(2)
GBA_OK, GBA_STOPPED, GBA_CAPACITY = range(3)
GBA_MAX_KF = 512
GBA_REPORT = ("status", "n_vertices", "n_free", "n_points", "n_removed", "n_mono", "n_stereo", "skipped_bad_or_new", "skipped_null",
              "iterations", "trials", "unknowns", "n_listed", "reserved_0", "reserved_1", "stop_samples")
GBA_APPLY_REPORT = ("n_visited", "n_propagated", "n_from_gba", "n_moved", "n_left", "n_present", "reserved_0", "reserved_1")
REMAP_TABLE_SIZE = 4096

# every symbol include/orbhip.h declares: (name, restype, argtypes)
_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_pi = C.POINTER(C.c_int)
_d = C.c_double
SYMBOLS = [
    ("orbhip_last_error", C.c_char_p, []),
    ("orbhip_device_count", _i, [_pi]),
    ("orbhip_extractor_create", _i, [_i, _f, _i, _i, _i, _i, C.POINTER(_vp)]),
    ("orbhip_extractor_destroy", None, [_vp]),
    ("orbhip_extractor_levels", _i, [_vp]),
    ("orbhip_extractor_tables", _i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    ("orbhip_extractor_capacity", _i, [_vp, _i, _i, _pi]),
    ("orbhip_extractor_set_blur_kernel", _i, [_vp, _vp]),
    ("orbhip_extractor_set_lazy_level0", _i, [_vp, _i]),
    ("orbhip_extractor_set_stage_gate", _i, [_vp, _i, _vp, _vp]),
    ("orbhip_extract", _i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _pi]),
    ("orbhip_extract_batch", _i, [_vp, _vp, _i, _i, _i, _i, _sz, _vp, _vp, _i, _vp]),
    ("orbhip_extract_batch_device", _i, [_vp, _vp, _i, _i, _i, _i, _sz, _vp, _vp, _i, _vp, _vp]),
    ("orbhip_extractor_set_gray_weights", _i, [_vp, _vp, _i]),
    ("orbhip_extract_color", _i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _pi]),
    ("orbhip_extract_color_batch", _i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _sz, _vp, _vp, _i, _vp]),
    ("orbhip_extract_color_batch_device", _i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _sz, _vp, _vp, _i, _vp, _vp]),
    ("orbhip_init_undistort_rectify_map", _i, [_vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp]),
    ("orbhip_extractor_set_remap", _i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    ("orbhip_extractor_set_remap_table", _i, [_vp, _vp]),
    ("orbhip_extract_remap", _i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _pi]),
    ("orbhip_extract_remap_batch", _i, [_vp, _vp, _i, _i, _i, _i, _i, _sz, _vp, _vp, _i, _vp]),
    ("orbhip_extract_remap_batch_device", _i, [_vp, _vp, _i, _i, _i, _i, _i, _sz, _vp, _vp, _i, _vp, _vp]),
    ("orbhip_extractor_sync", _i, [_vp]),
    ("orbhip_extractor_stream", _vp, [_vp]),
    ("orbhip_extractor_set_stream", _i, [_vp, _vp]),
    ("orbhip_pyramid_level", _i, [_vp, _i, _i, _pi, _pi, _pi, C.POINTER(_vp)]),
    ("orbhip_pyramid_level_download", _i, [_vp, _i, _i, _i, _vp, _i]),
    ("orbhip_blurred_level_download", _i, [_vp, _i, _i, _vp, _i]),
    ("orbhip_level_candidates", _i, [_vp, _i, _i, _vp, _vp, _vp, _i, _pi]),
    ("orbhip_fast_cell_table", _i, [_i, _f, _i, _i, _i, _vp, _i, _pi, _pi]),
    ("orbhip_extractor_set_profiling", _i, [_vp, _i]),
    ("orbhip_extractor_stage_times", _i, [_vp, _vp]),
    ("orbhip_matcher_create", _i, [_i, C.POINTER(_vp)]),
    ("orbhip_matcher_destroy", None, [_vp]),
    ("orbhip_descriptor_distance", _i, [_vp, _vp, _i, _vp, _i, _vp]),
    ("orbhip_search_for_initialization", _i, [_vp, C.POINTER(FrameView), C.POINTER(FrameView), _vp,
                                              _vp, _i, _f, _i, _pi]),
    ("orbhip_search_by_projection_frame", _i, [_vp, C.POINTER(FrameView), _vp, _vp, _i, _vp, _vp,
                                               _i, _pi]),
    ("orbhip_search_by_projection_points", _i, [_vp, C.POINTER(FrameView), _vp, _vp, _i, _vp, _vp,
                                                _f, _pi]),
    ("orbhip_search_by_projection_keyframe", _i, [_vp, C.POINTER(FrameView), _vp, _vp, _i, _vp, _vp, _i, _i, _pi]),
    ("orbhip_search_by_projection_sim3", _i, [_vp, C.POINTER(FrameView), _vp, _vp, _i, _vp, _vp, _pi]),
    ("orbhip_search_best_in_window", _i, [_vp, C.POINTER(FrameView), _vp, _vp, _i, _i, _vp, _vp, _vp]),
    ("orbhip_search_by_bow", _i, [_vp, C.POINTER(FrameView), _vp, _vp, C.POINTER(FrameView), _vp, _vp, _i, _f, _i, _vp, _pi]),
    ("orbhip_search_by_bow_device", _i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i,
                                         _f, _i, _vp, _vp]),
    ("orbhip_search_for_triangulation", _i, [_vp, C.POINTER(FrameView), _vp, _vp, C.POINTER(FrameView), _vp, _vp, _vp, _f,
                                             _f, _vp, _i, _i, _vp, _pi]),
    ("orbhip_undistort_keypoints", _i, [_vp, _vp, _i, _f, _f, _f, _f, _vp, _vp]),
    ("orbhip_undistort_keypoints_device", _i, [_vp, _i, _vp, _vp, _i, _f, _f, _f, _f, _vp, _vp]),
    ("orbhip_assign_features_to_grid", _i, [_vp, C.POINTER(FrameView), _vp, _vp, _vp]),
    ("orbhip_assign_features_to_grid_device", _i, [_vp, _i, _vp, _vp, _i, _f, _f, _f, _f, _vp, _vp, _vp]),
    ("orbhip_compute_stereo_from_rgbd", _i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _f, _vp, _vp]),
    ("orbhip_compute_stereo_from_rgbd_device", _i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _sz, _f, _vp, _vp]),
    ("orbhip_compute_stereo_from_rgbd_raw", _i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _f, _f, _vp, _vp]),
    ("orbhip_compute_stereo_from_rgbd_raw_device", _i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _sz, _f, _f, _vp,
                                                        _vp]),
    ("orbhip_distinctive_descriptors", _i, [_vp, _vp, _vp, _i, _vp]),
    ("orbhip_vocabulary_load_text", _i, [C.c_char_p, _i, C.POINTER(_vp)]),
    ("orbhip_vocabulary_create", _i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, C.POINTER(_vp)]),
    ("orbhip_vocabulary_destroy", None, [_vp]),
    ("orbhip_vocabulary_info", _i, [_vp, _pi, _pi, _pi, _pi, _pi, _pi]),
    ("orbhip_vocabulary_set_stream", _i, [_vp, _vp]),
    ("orbhip_vocabulary_sync", _i, [_vp]),
    ("orbhip_vocabulary_transform", _i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _pi]),
    ("orbhip_vocabulary_transform_device", _i, [_vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("orbhip_search_by_projection_frame_device", _i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _f, _f, _f, _f, _vp, _vp,
                                                      _vp, _i, _i, _vp, _vp]),
    ("orbhip_search_by_projection_points_device", _i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _f, _f, _f, _f, _vp, _vp,
                                                       _vp, _i, _f, _vp, _vp]),
    ("orbhip_search_for_initialization_device", _i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _f, _i, _vp, _i,
                                                     _f, _i, _vp, _vp]),
    ("orbhip_project_last_frame", _i, [_vp, C.POINTER(Camera), _vp, _vp, _i, _vp, _vp, _vp, _f, _i, _vp]),
    ("orbhip_frustum_queries", _i, [_vp, C.POINTER(Camera), _vp, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp]),
    ("orbhip_keyframe_queries", _i, [_vp, C.POINTER(Camera), _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp]),
    ("orbhip_fuse", _i, [_vp, C.POINTER(FrameView), C.POINTER(Camera), _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp,
                         _vp]),
    ("orbhip_fuse_device", _i, [_vp, _i, _vp, C.POINTER(Camera), _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp,
                                _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp]),
    ("orbhip_fuse_batch", _i, [_vp, _i, _vp, C.POINTER(Camera), _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp]),
    ("orbhip_create_new_map_points_device", _i, [_vp, _i, _i, _vp, C.POINTER(Camera), _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp,
                                                 _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("orbhip_create_new_map_points", _i, [_vp, C.POINTER(FrameView), _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                          C.POINTER(Camera), _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("orbhip_search_by_sim3", _i, [_vp, C.POINTER(FrameView), C.POINTER(FrameView), C.POINTER(Camera), _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _pi]),
    ("orbhip_project_last_frame_device", _i, [_vp, _i, C.POINTER(Camera), _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _f, _i,
                                              _vp, _vp]),
    ("orbhip_track_last_frame_device", _i, [_vp, _i, C.POINTER(Camera), _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp,
                                            _vp, _vp, _vp, _f, _i, _i, _vp, _vp]),
    ("orbhip_frustum_queries_device", _i, [_vp, _i, C.POINTER(Camera), _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp,
                                           _vp]),
    ("orbhip_seed_stereo_points", _i, [_vp, C.POINTER(Camera), _vp, _vp, _vp, _i, _f, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    ("orbhip_seed_stereo_points_device", _i, [_vp, _i, C.POINTER(Camera), _vp, _vp, _vp, _i, _i, _i, _vp, _f, _i, _i, _vp, _vp,
                                              _vp, _vp, _vp]),
    ("orbhip_count_close_points", _i, [_vp, _vp, _vp, _i, _f, _pi, _pi]),
    ("orbhip_count_close_points_device", _i, [_vp, _i, _vp, _vp, _vp, _i, _f, _vp]),
    ("orbhip_update_map_points_device", _i, [_vp, C.POINTER(Camera), _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp,
                                             _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("orbhip_update_map_points", _i, [_vp, C.POINTER(Camera), _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp, _vp]),
    ("orbhip_update_local_map_device", _i, [_vp, _i, _i, _i, _i, _i, C.POINTER(LocalMapTables), C.POINTER(LocalMapIO)]),
    ("orbhip_track_local_map_device", _i, [_vp, _i, _i, _i, _i, _i, C.POINTER(LocalMapTables), C.POINTER(LocalMapIO),
                                           C.POINTER(Camera), C.POINTER(LocalMapTrack), _f, _f, _f]),
    ("orbhip_update_local_map", _i, [_vp, _i, _i, _i, _i, _i, C.POINTER(LocalMapTables), C.POINTER(LocalMapIO)]),
    ("orbhip_update_connections_device", _i, [_vp, _i, _i, _i, _i, C.POINTER(CovisTables), C.POINTER(CovisState), _i, _i, _vp,
                                              _vp]),
    ("orbhip_update_connections", _i, [_vp, _i, _i, _i, _i, C.POINTER(CovisTables), C.POINTER(CovisState), _i, _i, _vp, _vp]),
    ("orbhip_covisible_targets_device", _i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp]),
    ("orbhip_covisible_targets", _i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp]),
    ("orbhip_children_from_parents_device", _i, [_vp, _i, _vp, _vp, _vp, _vp]),
    ("orbhip_cull_map_points_device", _i, [_vp, _i, _i, _i, _i, _i, C.POINTER(CullTables), C.POINTER(CullIO), _i, _vp, _vp, _vp,
                                           _vp, _i, _i, _vp, _vp, _vp]),
    ("orbhip_cull_map_points", _i, [_vp, _i, _i, _i, _i, _i, C.POINTER(CullTables), C.POINTER(CullIO), _i, _vp, _vp, _vp, _vp, _i,
                                    _i, _vp, _vp, _vp]),
    ("orbhip_cull_key_frames_device", _i, [_vp, _i, _i, _i, _i, _i, C.POINTER(CullTables), C.POINTER(CullIO),
                                           C.POINTER(CovisState), _i, _i, _vp, _i, _f, _vp]),
    ("orbhip_cull_key_frames", _i, [_vp, _i, _i, _i, _i, _i, C.POINTER(CullTables), C.POINTER(CullIO), C.POINTER(CovisState), _i,
                                    _i, _vp, _i, _f, _vp]),
    ("orbhip_sim3_setup_device", _i, [_vp, _i, _i, _vp, C.POINTER(Camera), _i, _i, _i, _i, C.POINTER(Sim3Tables), _vp, _i, _vp, _d,
                                      _i, _i, C.POINTER(Sim3Solvers)]),
    ("orbhip_sim3_iterate_device", _i, [_vp, _i, _i, C.POINTER(Camera), C.POINTER(Sim3Solvers), _vp, _i, _i, _i, _i, _vp, _vp,
                                        _vp]),
    ("orbhip_sim3_ransac", _i, [_vp, _i, _i, _vp, C.POINTER(Camera), _i, _i, _i, _i, C.POINTER(Sim3Tables), _vp, _i, _vp, _d, _i,
                                _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    ("orbhip_pnp_setup_device", _i, [_vp, _i, _vp, _i, _i, _vp, _i, _vp, _i, _i, _i, C.POINTER(PnpMap), C.POINTER(Camera), _vp,
                                     C.POINTER(PnpParams), C.POINTER(PnpSolvers)]),
    ("orbhip_pnp_iterate_device", _i, [_vp, _i, _i, _i, C.POINTER(Camera), C.POINTER(PnpParams), C.POINTER(PnpSolvers), _vp, _i,
                                       _i, _vp, _vp, _vp]),
    ("orbhip_pnp_ransac", _i, [_vp, _i, _vp, _i, _i, _vp, _i, _vp, _i, _i, _i, C.POINTER(PnpMap), C.POINTER(Camera), _vp,
                               C.POINTER(PnpParams), _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("orbhip_pose_optimization_device", _i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, C.POINTER(Camera), _vp, _i, _i,
                                             _vp, _vp, _vp, _vp, _vp]),
    ("orbhip_pose_optimization", _i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, C.POINTER(Camera), _vp, _i, _i,
                                      _vp, _vp, _vp, _vp, _vp]),
    ("orbhip_optimize_sim3_device", _i, [_vp, _i, _i, _vp, C.POINTER(Camera), _i, _i, _i, _i, C.POINTER(Sim3Tables), _i, _vp, _f, _i,
                                         _vp, _vp, _vp, _vp, _vp, _vp]),
    ("orbhip_optimize_sim3", _i, [_vp, _i, _i, _vp, C.POINTER(Camera), _i, _i, _i, _i, C.POINTER(Sim3Tables), _i, _vp, _f, _i,
                                  _vp, _vp, _vp, _vp, _vp, _vp]),
    ("orbhip_local_bundle_adjustment_device", _i, [_vp, _i, _i, C.POINTER(Camera), _i, _i, _i, _i, C.POINTER(LbaTables), _vp, _i, _i,
                                                   _vp, C.POINTER(LbaOut)]),
    ("orbhip_local_bundle_adjustment", _i, [_vp, _i, _i, C.POINTER(Camera), _i, _i, _i, _i, C.POINTER(LbaTables), _vp, _i, _i, _vp,
                                            C.POINTER(LbaOut)]),
    ("orbhip_optimize_essential_graph_device", _i, [_vp, _i, _i, _i, _i, C.POINTER(EgTables), _i, _i, C.POINTER(EgOut)]),
    ("orbhip_optimize_essential_graph", _i, [_vp, _i, _i, _i, _i, C.POINTER(EgTables), _i, _i, C.POINTER(EgOut)]),
    ("orbhip_optimize_essential_graph_counters", _i, [_vp, _vp]),
    ("orbhip_global_bundle_adjustment_device", _i, [_vp, C.POINTER(Camera), _i, _i, _i, _i, C.POINTER(GbaTables), _vp, _vp, _i, _vp, _i,
                                                    _i, _i, _i, _i, _i, _vp, C.POINTER(GbaOut)]),
    ("orbhip_global_bundle_adjustment", _i, [_vp, C.POINTER(Camera), _i, _i, _i, _i, C.POINTER(GbaTables), _vp, _vp, _i, _vp, _i, _i,
                                             _i, _i, _i, _i, _vp, C.POINTER(GbaOut)]),
    ("orbhip_global_bundle_adjustment_counters", _i, [_vp, _vp]),
    ("orbhip_apply_global_ba_device", _i, [_vp, _i, _i, _i, C.POINTER(GbaApply)]),
    ("orbhip_apply_global_ba", _i, [_vp, _i, _i, _i, C.POINTER(GbaApply)]),
    ("orbhip_matcher_set_stream", _i, [_vp, _vp]),
    ("orbhip_matcher_sync", _i, [_vp]),
    ("orbhip_matcher_fill_scratch", _i, [_vp, _i, C.POINTER(C.c_ulonglong)]),
    ("orbhip_compute_stereo_matches_device", _i, [_vp, _vp, _i, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i,
                                                  _f, _f, _vp, _vp, _vp]),
    ("orbhip_compute_stereo_matches", _i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _f,
                                           _f, _vp, _vp, _pi]),
]

_LIB = None


class OrbHipError(RuntimeError):
    def __init__(self, code, where):
        msg = lib().orbhip_last_error()
        super().__init__("%s failed with status %d: %s" % (where, code, (msg or b"").decode()))
        self.code = code


def use_library(path):
    """Point the loader at another build of the library (tools/: the -DORBHIP_DEVTOOLS build).  Before the first lib()."""
    global LIB_PATH
    if _LIB is not None:
        raise RuntimeError("liborbhip is already loaded")
    LIB_PATH = path


def lib():
    """Load liborbhip.so and bind every declared symbol.  Raises if it is missing."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'`"
                              % LIB_PATH)
        # torch bundles its own libamdhip64.so.7 (same soname as /opt/rocm's).  Whichever copy is
        # loaded first serves the whole process, and torch cannot see the GPU through the system
        # copy -- so when torch is installed, let it load its runtime before liborbhip.so binds.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)  # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def check(code, where):
    if code != OK:
        raise OrbHipError(code, where)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None
