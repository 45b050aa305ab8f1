"""ctypes binding of the C-ABI declared in include/gmmloc_hip.h."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GMMLOC_HIP_LIB", os.path.join(_HERE, "libgmmloc_hip.so"))  # override: A/B builds


class gl_camera(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("bf", C.c_double), ("width", C.c_int32), ("height", C.c_int32)]


class gl_params(C.Structure):
    _fields_ = [("neighbor_dist_thresh", C.c_double), ("tri_lambda2", C.c_float),
                ("tri_str_thresh", C.c_float), ("ba_lambda2", C.c_float),
                ("tri_check_str_chi2", C.c_int32), ("ba_first_as_prior", C.c_int32),
                ("sigma2_inv", C.c_float * 8)]


class gl_track_anchor(C.Structure):
    _fields_ = [("prior_dev", C.c_void_p), ("F", C.c_int32), ("fixed_pose_dev", C.c_void_p), ("fixed_obs_dev", C.c_void_p),
                ("fixed_oct_dev", C.c_void_p), ("fixed_erase_dev", C.c_void_p)]


class gl_map_view(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("NMP", "NKF", "NFK", "NOBS")] +
                [(k, C.c_void_p) for k in ("mp_valid", "obs_ptr", "obs_kf", "kf_valid", "kf_mp", "mp_pos", "mp_normal", "mp_max_dist",
                                           "mp_min_dist", "mp_desc")])


class gl_local_map_io(C.Structure):
    _fields_ = ([("last_mp", C.c_void_p), ("kf_feat_mp", C.c_void_p), ("feat_mp", C.c_void_p), ("KFcap", C.c_int32), ("reserved_", C.c_int32)] +
                [(k, C.c_void_p) for k in ("local_kf", "n_local_kf", "local_mp", "n_local_mp", "ref_kf", "kf_count", "status")])


class gl_map_ba_view(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("kf_pose", "kf_twc", "kf_uvr", "kf_oct", "obs_feat", "mp_assoc")] +
                [("kf_first", C.c_int32), ("reserved_", C.c_int32)])


BA_WINDOW_ARRAYS = ("poses", "prior", "points", "assoc", "obs_ptr", "obs_pose", "obs_uvr", "obs_oct", "win_kf", "win_mp", "win_obs", "sizes",
                    "status")


class gl_map_edit(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf", "obs_feat", "mp_ref_kf")]


class gl_map_remove_lists(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("rm_mp", "n_rm_mp", "erase_obs", "n_erase", "rm_kf", "n_rm_kf")] +
                [(k, C.c_int32) for k in ("rm_mp_cap", "erase_cap", "rm_kf_cap", "reserved_")])


class gl_map_remove_out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("result", "dead_mp", "obs_new_pos")] + [("dead_cap", C.c_int32), ("reserved_", C.c_int32)]


class gl_map_add_lists(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("new_pos", "new_assoc", "new_ref_kf", "n_new_mp", "new_kf", "n_new_kf", "att_mp", "att_kf", "att_feat",
                                           "n_attach", "walk_kf", "n_walk")] +
                [(k, C.c_int32) for k in ("new_mp_cap", "new_kf_cap", "attach_cap", "walk_cap")])


class gl_map_add_out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("result", "already_mp", "obs_new_pos")] + [("already_cap", C.c_int32), ("reserved_", C.c_int32)]


class gl_map_fuse_out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("result", "repl_src", "repl_tgt", "obs_new_pos")] + [("repl_cap", C.c_int32), ("reserved_", C.c_int32)]


class gl_map_stats(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("mp_visible", "mp_found", "mp_ref_idx", "kf_idx", "cand", "n_cand")] +
                [("cand_cap", C.c_int32), ("reserved_", C.c_int32)])


class gl_map_covis(C.Structure):
    _fields_ = [("NKFcap", C.c_int32), ("Wcap", C.c_int32)] + [(k, C.c_void_p) for k in ("cov_kf", "cov_w", "cov_n", "cov_nord", "best_cov")]


class gl_stereo_points_in(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("pose", "feat_uv", "feat_ur", "feat_depth", "feat_oct", "cand", "ncand", "held", "kf_row")]


class gl_stereo_points_out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("pts0", "new_feat", "new_pos", "new_assoc", "new_ref_kf", "att_mp", "att_kf", "att_feat", "n_new",
                                          "feat_new", "stats")]


class gl_temporal_points_in(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("pose", "feat_uv", "feat_depth", "feat_oct", "held", "last_outlier", "feat_desc")]


class gl_temporal_points_out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("temp_flag", "n_temp", "last_pt", "last_observed", "last_valid", "last_desc", "stats", "last_mp")]


class gl_stereo_in(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("feat_uv", "feat_oct", "feat_desc", "r_uv", "r_oct", "r_desc", "n_left", "n_right")]


class gl_image_pyramid(C.Structure):
    _fields_ = [("nlevels", C.c_int32), ("reserved_", C.c_int32), ("width", C.c_int32 * 8), ("height", C.c_int32 * 8), ("stride", C.c_int64 * 8),
                ("offset", C.c_int64 * 8), ("frame_stride", C.c_int64), ("data", C.c_void_p)]


class gl_stereo_out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("feat_ur", "feat_depth", "match_r", "sad", "stat")]


class gl_orb_in(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("kp_xy", "kp_oct", "n_kp", "kp_angle", "pattern")] + [("blur_w", C.POINTER(C.c_int32)), ("scale_factor", C.c_double)]


class gl_orb_out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("desc", "angle", "moments", "uv32", "uv64", "stat")]


class gl_orb_detect_out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("kp_xy", "kp_oct", "n_kp", "kp_response", "level_count", "stat", "cand_xy", "cand_resp", "cand_count")]


class gl_frame_end_in(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("feat_mp", "match_last", "match_local", "match_kf", "outlier", "local_mp", "n_local_mp", "counts2", "ref_kf",
                                          "last_observed", "feat_depth")]


class gl_kf_rule(C.Structure):
    _fields_ = [("num_kfs", C.c_int32), ("frame_idx", C.c_int32), ("kf_frame_idx", C.c_int32), ("fps", C.c_float), ("is_idle", C.c_int32),
                ("n_queue", C.c_int32)]


class gl_frame_end_out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("held_mp", "held", "stat", "ratio_map")]


class gl_frame_next_in(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("pose_tracked", "pose_prev", "ref_kf", "feat_new", "mp_replaced")] +
                [("mp_base", C.c_int32), ("NMPcap", C.c_int32)])


class gl_frame_next_out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("t_rc", "t_cr", "pose_lw", "pose_cw", "held_mp", "last_pt", "last_valid", "last_observed", "held", "status",
                                          "last_desc")]


class gl_map_kf_tables(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("kf_angle", "kf_desc", "kf_depth", "kf_nnode", "kf_node_id", "kf_node_ptr", "kf_node_idx", "kf_cand",
                                           "kf_ncand")] + [("NNcap", C.c_int32), ("k", C.c_int32)])


class gl_bow_out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("word_id", "node", "weight", "nnode", "node_id", "node_ptr", "node_idx", "status")]


TRI_POINTS_ARRAYS = ("new_pos", "new_assoc", "new_ref_kf", "new_type", "new_nb", "new_feat1", "new_feat2", "att_mp", "att_kf", "att_feat", "n_new",
                     "n_attach", "feat_new", "nb_stats", "fmat", "epipole", "status")


class gl_tri_points_out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in TRI_POINTS_ARRAYS] + [("new_cap", C.c_int32), ("reserved_", C.c_int32)]


class gl_ba_window(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("Pcap", "Fcap", "Lcap", "Ocap")] + [(k, C.c_void_p) for k in BA_WINDOW_ARRAYS])


_lib = None


def load():
    """Load libgmmloc_hip.so.  Fails loudly when the extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    try:  # make torch's bundled libamdhip64.so.7 the one the loader binds (same SONAME)
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "gmmloc_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    P = C.POINTER
    sig = {
        "gl_default_params": (None, [P(gl_params)]),
        "gl_last_error_string": (C.c_char_p, []),
        "gl_device_count": (i32, []),
        "gl_ctx_create": (i32, [i32, vp, P(vp)]),
        "gl_ctx_destroy": (i32, [vp]),
        "gl_ctx_synchronize": (i32, [vp]),
        "gl_ctx_stream": (vp, [vp]),
        "gl_ctx_set_option": (i32, [vp, C.c_char_p, C.c_double]),
        "gl_ctx_get_option": (i32, [vp, C.c_char_p, P(C.c_double)]),
        "gl_ctx_timing_enable": (i32, [vp, i32]),
        "gl_ctx_timing_read": (i32, [vp, i32, P(C.c_double), P(i64), i32]),
        "gl_ctx_set_stats_buffer": (i32, [vp, vp, i32]),
        "gl_ctx_set_stats_buffers": (i32, [vp, vp, vp, i32]),
        "gl_ctx_set_edge_stats_buffer": (i32, [vp, vp, i32]),
        "gl_ctx_counter_read": (i32, [vp, i32, P(i64), i32]),
        "gl_gmm_create": (i32, [vp, vp, vp, i32, P(gl_params), P(vp)]),
        "gl_gmm_load_file": (i32, [vp, C.c_char_p, P(gl_params), P(vp)]),
        "gl_gmm_save_file": (i32, [vp, C.c_char_p]),
        "gl_gmm_destroy": (i32, [vp]),
        "gl_gmm_count": (i32, [vp]),
        "gl_gmm_file_read": (i32, [C.c_char_p, vp, vp, i32, P(i32)]),
        "gl_gmm_file_write": (i32, [C.c_char_p, vp, vp, vp, i32]),
        "gl_write_tum_trajectory": (i32, [C.c_char_p, vp, vp, i32]),
        "gl_gmm_get": (i32, [vp, i32, vp, C.c_size_t]),
        "gl_gmm_nbs_count": (i32, [vp]),
        "gl_associate3d": (i32, [vp, vp, vp, i32, i32, vp, vp]),
        "gl_gmm_index_info": (i32, [vp, P(C.c_double)]),
        "gl_gmm_index_bytes": (i32, [vp, P(C.c_double)]),
        "gl_assoc_index_work": (i32, [vp, vp, vp, i32, vp]),
        "gl_knn3d": (i32, [vp, vp, vp, i32, i32, vp, vp]),
        "gl_search2d": (i32, [vp, vp, P(gl_camera), i32, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp]),
        "gl_search_by_projection": (i32, [vp, P(gl_camera), C.c_float, i32, i32, i32] + [vp] * 10 + [C.c_float, C.c_float, vp, vp]),
        "gl_search_by_projection_frame": (i32, [vp, P(gl_camera), C.c_float, i32, i32, i32] + [vp] * 13 + [C.c_float, i32, i32, vp, vp]),
        "gl_search_for_triangulation": (i32, [vp, C.c_float, i32, i32, i32, i32, i32] + [vp] * 22 + [i32, i32, vp, vp]),
        "gl_search_by_bow": (i32, [vp, C.c_float, i32, i32, i32, i32, i32, i32] + [vp] * 15),
        "gl_voc_file_read": (i32, [C.c_char_p, vp, vp, vp, vp, i32, P(i32), P(i32)]),
        "gl_voc_create": (i32, [vp, i32, vp, vp, vp, vp, i32, i32, P(vp)]),
        "gl_voc_load_file": (i32, [vp, C.c_char_p, P(vp)]),
        "gl_voc_destroy": (i32, [vp]),
        "gl_voc_info": (i32, [vp, P(C.c_double)]),
        "gl_bow_transform": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, P(gl_bow_out)]),
        "gl_fuse_search": (i32, [vp, vp, C.c_float, i32, i32, i32] + [vp] * 8 + [C.c_float, vp, vp]),
        "gl_project_map_points": (i32, [vp, vp, C.c_float, i32, i32] + [vp] * 12),
        "gl_level_steps": (i32, [C.c_float, vp]),
        "gl_update_map_points": (i32, [vp, C.c_float, i32, i32, i32, i32, i32] + [vp] * 14),
        "gl_track_frame_chain": (i32, [vp, vp, vp, C.c_float, i32, i32, i32, i32, vp, C.c_float, C.c_float, C.c_float, i32]),
        "gl_track_frame_chain_front": (i32, [vp, vp, vp, C.c_float, i32, i32, i32, i32, vp, C.c_float, i32]),
        "gl_track_frame_chain_back": (i32, [vp, vp, vp, C.c_float, i32, i32, i32, i32, vp, C.c_float, C.c_float]),
        "gl_update_local_map": (i32, [vp, vp, i32, i32, i32, i32] + [vp] * 8),
        "gl_track_frame_chain_map": (i32, [vp, vp, vp, C.c_float, i32, i32, i32, i32, vp, vp, vp, C.c_float, C.c_float, C.c_float, i32]),
        "gl_update_connections": (i32, [vp, vp, i32, vp, i32] + [vp] * 5),
        "gl_ba_window_build": (i32, [vp, vp, vp, i32, vp, vp]),
        "gl_ba_window_apply": (i32, [vp, vp, vp, vp, i32, vp] + [vp] * 5),
        "gl_cull_keyframes": (i32, [vp, vp, vp, vp, C.c_float, i32, i32] + [vp] * 8),
        "gl_map_remove": (i32, [vp, i32, i32, i32, i32, vp, vp, i32, vp, vp]),
        "gl_map_add": (i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
        "gl_map_fuse": (i32, [vp, i32, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp]),
        "gl_map_stats_track": (i32, [vp, i32, vp, i32, i32, i32] + [vp] * 7),
        "gl_map_stats_new_points": (i32, [vp, i32, i32, vp, i32, i32, vp, vp, vp]),
        "gl_map_cand_append": (i32, [vp, vp, vp, i32, i32, vp, vp]),
        "gl_map_stats_merge": (i32, [vp, i32, vp, vp, vp, i32, vp]),
        "gl_cull_map_points": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp]),
        "gl_covis_update": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp]),
        "gl_covis_remove": (i32, [vp, i32, vp, i32, vp, vp, i32, vp]),
        "gl_covis_best": (i32, [vp, i32, vp, i32, vp, i32, i32, vp, vp, vp, vp]),
        "gl_fuse_targets": (i32, [vp, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
        "gl_fuse_candidates": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]),
        "gl_track_frame_end": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, C.c_float, vp, vp]),
        "gl_map_note_replaced": (i32, [vp, i32, vp, vp, vp, i32, vp]),
        "gl_track_frame_next": (i32, [vp, vp, vp, i32, i32, vp, vp]),
        "gl_search_local_points": (i32, [vp, vp, C.c_float, i32, i32, i32] + [vp] * 13 + [C.c_float, C.c_float, vp, vp, vp]),
        "gl_gather_triangulation_matches": (i32, [vp, i32, i32, i32, i32, i32] + [vp] * 32),
        "gl_optimize_point": (i32, [vp, vp, P(gl_camera), P(gl_params), i32] + [vp] * 10),
        "gl_check_map_association": (i32, [vp, vp, P(gl_camera), P(gl_params), i32, i32] + [vp] * 6 + [i32, vp]),
        "gl_optimize_triangulation": (i32, [vp, vp, P(gl_camera), P(gl_params), i32] + [vp] * 11 + [i32, vp]),
        "gl_create_map_points": (i32, [vp, vp, P(gl_camera), P(gl_params), C.c_float, i32] + [vp] * 12 + [i32, vp, vp, vp]),
        "gl_tri_pair_setup": (i32, [vp, P(gl_camera), i32, vp, vp, vp, i32, vp, vp, i32, i32, i32, C.c_float, vp, vp, vp]),
        "gl_create_map_points_from_map": (i32, [vp, vp, P(gl_camera), P(gl_params), C.c_float, vp, vp, vp, i32, vp, vp, i32, i32, i32, C.c_float,
                                                i32, vp]),
        "gl_create_stereo_points": (i32, [vp, vp, P(gl_camera), P(gl_params), i32, i32, i32, vp, i32, i32, C.c_float, vp]),
        "gl_create_temporal_points": (i32, [vp, P(gl_camera), i32, i32, vp, C.c_float, vp]),
        "gl_stereo_matches": (i32, [vp, P(gl_camera), C.c_double, i32, i32, i32, P(gl_stereo_in), P(gl_image_pyramid), P(gl_image_pyramid),
                                    P(gl_stereo_out)]),
        "gl_orb_describe": (i32, [vp, i32, i32, P(gl_orb_in), P(gl_image_pyramid), P(gl_orb_out)]),
        "gl_orb_default_blur": (i32, [C.c_double, P(C.c_int32)]),
        "gl_orb_pyramid_layout": (i32, [i32, i32, i32, C.c_double, i32, i64, P(gl_image_pyramid)]),
        "gl_orb_pyramid": (i32, [vp, i32, P(gl_image_pyramid), C.c_double]),
        "gl_orb_features_per_level": (i32, [i32, i32, C.c_double, P(C.c_int32)]),
        "gl_orb_detect_bound": (i32, [P(gl_image_pyramid), i32, C.c_double, P(C.c_int32)]),
        "gl_orb_detect": (i32, [vp, i32, i32, P(gl_image_pyramid), i32, C.c_double, i32, i32, i32, P(gl_orb_detect_out)]),
        "gl_optimize_current_pose": (i32, [vp, P(gl_camera), P(gl_params), i32, i32, vp, vp, vp, vp, vp, vp]),
        "gl_joint_optimization": (i32, [vp, vp, P(gl_camera), P(gl_params), i32, i32, i32, i32, i32] + [vp] * 11),
        "gl_joint_optimization_stoppable": (i32, [vp, vp, P(gl_camera), P(gl_params), i32, i32, i32, i32, i32] + [vp] * 12),
        "gl_track_frames": (i32, [vp, vp, P(gl_camera), P(gl_params), i32, i32, vp, vp, vp, vp, vp, vp]),
        "gl_track_frames_anchored": (i32, [vp, vp, P(gl_camera), P(gl_params), i32, i32, vp, vp, vp, vp, vp, vp, P(gl_track_anchor)]),
        "gl_track_frame_host_anchored": (i32, [vp, vp, P(gl_camera), P(gl_params), i32, vp, vp, vp, vp, vp]),
        "gl_malloc": (i32, [vp, C.c_size_t, P(vp)]),
        "gl_free": (i32, [vp, vp]),
        "gl_memcpy_h2d": (i32, [vp, vp, vp, C.c_size_t]),
        "gl_memcpy_d2h": (i32, [vp, vp, vp, C.c_size_t]),
        "gl_track_frame_host": (i32, [vp, vp, P(gl_camera), P(gl_params), i32, vp, vp, vp, vp, vp]),
        "gl_malloc_host": (i32, [vp, C.c_size_t, P(vp)]),
        "gl_free_host": (i32, [vp, vp]),
        "gl_memcpy_h2d_async": (i32, [vp, vp, vp, C.c_size_t]),
        "gl_memcpy_d2h_async": (i32, [vp, vp, vp, C.c_size_t]),
    }
    missing = []
    for name, (res, args) in sig.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    lib._gl_missing = missing
    lib._gl_signatures = sig
    _lib = lib
    return lib
