"""ctypes binding of libse3icp.so (include/se3icp.h).

The product path: every call goes to the HIP engine.  If the shared library is
missing or no HIP device is visible, calls raise — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)  # se3-icp_amd/
LIB_PATH = os.environ.get("SE3ICP_LIB") or os.path.join(_ROOT, "lib", "libse3icp.so")

OK = 0
ERR_INVALID_ARG = -1
ERR_INVALID_METHOD = -2
ERR_EMPTY_CLOUD = -3
ERR_K_TOO_LARGE = -4
ERR_NO_DEVICE = -5
ERR_HIP = -6
ERR_NONFINITE = -7
ERR_OUT_OF_MEMORY = -8
ERR_INTERNAL = -9

METHODS = ["pt2pt", "pt2pl", "gicp", "se3_pt2pt", "se3_pt2pl", "se3_gicp", "se3_gicp_with_cf",
           "se3_pure_pt2pt", "se3_pure_pt2pl", "se3_pure_gicp"]

# every symbol include/se3icp.h declares
EXPORTED_SYMBOLS = [
    "se3icp_abi_version", "se3icp_status_string", "se3icp_method_from_name", "se3icp_method_name",
    "se3icp_default_params", "se3icp_device_count",
    "se3icp_registration_new", "se3icp_registration_free", "se3icp_set_source_cloud", "se3icp_set_target_cloud",
    "se3icp_params_of", "se3icp_run_icp", "se3icp_run_se3_icp", "se3icp_run_se3_icp_with_cf", "se3icp_run_se3_pure",
    "se3icp_get_result",
    "se3icp_register_batch", "se3icp_register_batch_device", "se3icp_register",
    "se3icp_register_sweep", "se3icp_register_sweep_device",
    "se3icp_register_graph", "se3icp_register_graph_device", "se3icp_register_graph_report",
    "se3icp_register_graph_report_device", "se3icp_last_graph_stats", "se3icp_set_batch_sharing",
    "se3icp_set_lrf_seeding", "se3icp_last_seed_stats", "se3icp_set_tree_sharing", "se3icp_last_tree_stats",
    "se3icp_set_lrf_taking", "se3icp_last_take_stats",
    "se3icp_report_version", "se3icp_register_batch_report", "se3icp_register_batch_report_device",
    "se3icp_register_sweep_report", "se3icp_register_sweep_report_device",
    "se3icp_request_report", "se3icp_get_report",
    "se3icp_toldi_frames", "se3icp_knn_self", "se3icp_estimate_normals", "se3icp_nn",
    "se3icp_nn_sequence_version", "se3icp_nn_sequence",
    "se3icp_synthetic_pairs", "se3icp_synthetic_reference", "se3icp_synthetic_reference_device",
    "se3icp_random_downsample",
    "se3icp_voxel_version", "se3icp_voxel_downsample_device", "se3icp_voxel_downsample",
    "se3icp_init_version", "se3icp_register_graph_init", "se3icp_register_graph_init_device",
    "se3icp_set_initial_transform", "se3icp_set_pose_seeding", "se3icp_last_init_stats",
    "se3icp_transform_points", "se3icp_transform_device",
    "se3icp_set_profiling", "se3icp_last_kernel_times", "se3icp_last_kernel_times_n", "se3icp_set_trace", "se3icp_set_lrf_exact",
    "se3icp_set_nn_events", "se3icp_setup_record_version", "se3icp_set_setup_record",
    "se3icp_tree_record_version", "se3icp_set_tree_record",
    # include/se3icp_cc.h: metrics and pose files of the benchmark drivers (host only)
    "se3icp_cc_rot_3d", "se3icp_cc_angular_error_so3", "se3icp_cc_angular_error_so3_alt",
    "se3icp_cc_error_filterreg", "se3icp_cc_rot2euler", "se3icp_cc_avg_eul_error",
    "se3icp_cc_evaluate_lrf_quality", "se3icp_cc_evaluate_trajectory",
    "se3icp_cc_read_trajectory", "se3icp_cc_read_kitti_poses", "se3icp_cc_read_redwood_log",
    "se3icp_cc_write_trajectory", "se3icp_cc_write_redwood_log",
]


class Params(C.Structure):
    _fields_ = [
        ("max_num_iterations", C.c_int32),
        ("max_num_se3_iterations", C.c_int32),
        ("number_of_nn_for_LRF", C.c_int32),
        ("_reserved", C.c_int32),
        ("mse", C.c_double),
        ("mse_switch_error", C.c_double),
        ("estimated_overlap", C.c_double),
        ("alpha_rot", C.c_double),
        ("beta_transl", C.c_double),
        ("scale_preprocessing", C.c_double),
    ]


class Result(C.Structure):
    _fields_ = [
        ("T", C.c_double * 16),
        ("num_iterations", C.c_int32),
        ("num_pure_se3_iterations", C.c_int32),
        ("status", C.c_int32),
        ("num_rechecked", C.c_int32),
        ("scaling_factor", C.c_double),
        ("time_setup_ms", C.c_double),
        ("time_loop_ms", C.c_double),
        ("time_se3_correspondence_search_ms", C.c_double),
        ("time_before_pure_icp_ms", C.c_double),
    ]


STOP_CONVERGED = 0
STOP_MAX_ITERATIONS = 1
STOP_MAX_SE3_ITERATIONS = 2
STOP_RUNAWAY = 3
STOP_REASONS = ["converged", "max_iterations", "max_se3_iterations", "runaway"]


class ReportOptions(C.Structure):
    """se3icp_report_options; the per-point buffers are addresses (host or device)."""
    _fields_ = [
        ("max_correspondence_distance", C.c_double),
        ("corr_idx", C.c_void_p),
        ("corr_dist", C.c_void_p),
        ("outputs_on_device", C.c_int32),
        ("_reserved", C.c_int32),
    ]


class Report(C.Structure):
    """se3icp_report."""
    _fields_ = [
        ("fitness", C.c_double),
        ("inlier_rmse", C.c_double),
        ("information", C.c_double * 36),
        ("final_mse", C.c_double),
        ("final_mse_change", C.c_double),
        ("n_inliers", C.c_int64),
        ("switched", C.c_int32),
        ("stop_reason", C.c_int32),
    ]


class Trace(C.Structure):
    _fields_ = [
        ("pair", C.c_int32),
        ("max_iters", C.c_int32),
        ("corr_idx", C.POINTER(C.c_int32)),
        ("corr_dist", C.POINTER(C.c_float)),
        ("trim_key", C.POINTER(C.c_uint64)),
        ("T", C.POINTER(C.c_double)),
        ("mse", C.POINTER(C.c_double)),
        ("phase", C.POINTER(C.c_int32)),
        ("iters_recorded", C.c_int32),
        ("_reserved", C.c_int32),
    ]


SETUP_XYZ, SETUP_ROWS, SETUP_NORMALS, SETUP_CONF = 1, 2, 4, 8


class SetupSide(C.Structure):
    """se3icp_setup_side."""
    _fields_ = [
        ("xyz", C.POINTER(C.c_double)),
        ("rows", C.POINTER(C.c_double)),
        ("normals", C.POINTER(C.c_double)),
        ("conf", C.POINTER(C.c_double)),
        ("cap", C.c_int64),
        ("n", C.c_int64),
        ("norm_center", C.c_double * 3),
        ("norm_scale", C.c_double),
        ("f32_center", C.c_double * 3),
        ("alpha", C.c_double),
        ("beta", C.c_double),
        ("written", C.c_int32),
        ("_reserved", C.c_int32),
    ]


class SetupRecord(C.Structure):
    """se3icp_setup_record."""
    _fields_ = [
        ("pair", C.c_int32),
        ("recorded", C.c_int32),
        ("src", SetupSide),
        ("tgt", SetupSide),
    ]


TREE_PERM, TREE_POS, TREE_VEC, TREE_TVEC, TREE_TVEC64, TREE_TPT64, TREE_BOXES = 1, 2, 4, 8, 16, 32, 64
TREE_BUILT = -1


class TreeSide(C.Structure):
    """se3icp_tree_side."""
    _fields_ = [
        ("perm", C.POINTER(C.c_int32)),
        ("pos", C.POINTER(C.c_int32)),
        ("vec", C.POINTER(C.c_float)),
        ("tvec", C.POINTER(C.c_float)),
        ("tvec64", C.POINTER(C.c_double)),
        ("tpt64", C.POINTER(C.c_double)),
        ("lo", C.POINTER(C.c_float)),
        ("hi", C.POINTER(C.c_float)),
        ("cap", C.c_int64),
        ("node_cap", C.c_int64),
        ("n", C.c_int64),
        ("exists", C.c_int32),
        ("D", C.c_int32),
        ("L", C.c_int32),
        ("nnodes", C.c_int32),
        ("G", C.c_int32),
        ("H", C.c_int32),
        ("role", C.c_int32),
        ("written", C.c_int32),
    ]


class TreeRecord(C.Structure):
    """se3icp_tree_record."""
    _fields_ = [
        ("pair", C.c_int32),
        ("recorded", C.c_int32),
        ("src3", TreeSide),
        ("tgt3", TreeSide),
        ("src12", TreeSide),
        ("tgt12", TreeSide),
    ]


# se3icp_last_graph_stats
GRAPH_STATS = ["clouds", "uses", "classes", "classes_full", "adopted", "rejected_order", "rejected_gap", "no_list",
               "bytes_uploaded"]
# se3icp_last_seed_stats
SEED_STATS = ["classes_seeded", "queries_seeded", "queries_unseeded", "queries_failed"]
# se3icp_last_take_stats
TAKE_STATS = ["classes_taking", "queries_taken", "queries_redone", "queries_failed"]
# se3icp_last_init_stats
INIT_STATS = ["posed_edges", "posed_variants", "classes_seeded_across"]
# se3icp_last_tree_stats
TREE_STATS = ["built_3d", "adopted_3d", "built_12d", "adopted_12d"]


class Se3IcpError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        msg = status_string(code) if _lib is not None else str(code)
        super().__init__(f"se3icp error {code} ({msg}){': ' + what if what else ''}")


_lib = None


def load():
    """Load libse3icp.so (build it with `make -C se3-icp_amd` or __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"HIP engine library not built: {LIB_PATH} is missing "
                          "(run __graft_entry__.build() or `make -C se3-icp_amd`)")
    L = C.CDLL(LIB_PATH)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    vp = C.c_void_p
    L.se3icp_abi_version.restype = C.c_int
    L.se3icp_status_string.restype = C.c_char_p
    L.se3icp_status_string.argtypes = [C.c_int]
    L.se3icp_method_from_name.argtypes = [C.c_char_p]
    L.se3icp_method_name.restype = C.c_char_p
    L.se3icp_method_name.argtypes = [C.c_int]
    L.se3icp_default_params.argtypes = [C.POINTER(Params)]
    L.se3icp_device_count.restype = C.c_int
    L.se3icp_registration_new.restype = vp
    L.se3icp_registration_free.argtypes = [vp]
    L.se3icp_set_source_cloud.argtypes = [vp, dp, C.c_int64]
    L.se3icp_set_target_cloud.argtypes = [vp, dp, C.c_int64]
    L.se3icp_params_of.restype = C.POINTER(Params)
    L.se3icp_params_of.argtypes = [vp]
    L.se3icp_run_icp.argtypes = [vp, C.c_char_p]
    L.se3icp_run_se3_icp.argtypes = [vp, C.c_char_p]
    L.se3icp_run_se3_icp_with_cf.argtypes = [vp]
    L.se3icp_run_se3_pure.argtypes = [vp, C.c_char_p]
    L.se3icp_get_result.argtypes = [vp, C.POINTER(Result)]
    L.se3icp_register_batch.argtypes = [C.c_int, C.c_int32, C.POINTER(dp), C.POINTER(C.c_int64), C.POINTER(dp),
                                        C.POINTER(C.c_int64), C.c_int, C.POINTER(Params), C.POINTER(Result)]
    L.se3icp_register_batch_device.argtypes = [C.c_int, C.c_int32, vp, C.POINTER(C.c_int64), vp,
                                               C.POINTER(C.c_int64), C.c_int, C.POINTER(Params), C.POINTER(Result), vp]
    L.se3icp_register_sweep.argtypes = [C.c_int, C.c_int32, C.POINTER(dp), C.POINTER(C.c_int64), C.POINTER(dp),
                                        C.POINTER(C.c_int64), C.c_int, C.c_int32, C.POINTER(Params), C.c_int32,
                                        C.POINTER(Result)]
    L.se3icp_register_sweep_device.argtypes = [C.c_int, C.c_int32, vp, C.POINTER(C.c_int64), vp,
                                               C.POINTER(C.c_int64), C.c_int, C.c_int32, C.POINTER(Params), C.c_int32,
                                               C.POINTER(Result), vp]
    rop, rep = C.POINTER(ReportOptions), C.POINTER(Report)
    L.se3icp_report_version.restype = C.c_int
    L.se3icp_register_batch_report.argtypes = L.se3icp_register_batch.argtypes + [rop, rep]
    L.se3icp_register_batch_report_device.argtypes = L.se3icp_register_batch_device.argtypes + [rop, rep]
    L.se3icp_register_sweep_report.argtypes = L.se3icp_register_sweep.argtypes + [rop, rep]
    L.se3icp_register_sweep_report_device.argtypes = L.se3icp_register_sweep_device.argtypes + [rop, rep]
    L.se3icp_register_graph.argtypes = [C.c_int, C.c_int32, C.POINTER(dp), C.POINTER(C.c_int64), C.c_int32, ip, ip,
                                        C.c_int, C.POINTER(Params), C.c_int32, C.POINTER(Result)]
    L.se3icp_register_graph_device.argtypes = [C.c_int, C.c_int32, vp, C.POINTER(C.c_int64), C.c_int32, ip, ip,
                                               C.c_int, C.POINTER(Params), C.c_int32, C.POINTER(Result), vp]
    L.se3icp_register_graph_report.argtypes = L.se3icp_register_graph.argtypes + [rop, rep]
    L.se3icp_register_graph_report_device.argtypes = L.se3icp_register_graph_device.argtypes + [rop, rep]
    L.se3icp_last_graph_stats.argtypes = [C.c_int, C.POINTER(C.c_int64), C.c_int]
    if hasattr(L, "se3icp_init_version"):  # (SE3ICP_LIB may name an older build for an A/B run)
        L.se3icp_init_version.restype = C.c_int
        L.se3icp_register_graph_init.argtypes = [C.c_int, C.c_int32, C.POINTER(dp), C.POINTER(C.c_int64), C.c_int32,
                                                 ip, ip, dp, C.c_int, C.POINTER(Params), C.c_int32, C.POINTER(Result),
                                                 rop, rep]
        L.se3icp_register_graph_init_device.argtypes = [C.c_int, C.c_int32, vp, C.POINTER(C.c_int64), C.c_int32, ip, ip,
                                                        dp, C.c_int, C.POINTER(Params), C.c_int32, C.POINTER(Result),
                                                        vp, rop, rep]
        L.se3icp_set_initial_transform.argtypes = [vp, dp]
        L.se3icp_set_pose_seeding.argtypes = [C.c_int, C.c_int]
        L.se3icp_last_init_stats.argtypes = [C.c_int, C.POINTER(C.c_int64), C.c_int]
        L.se3icp_transform_points.argtypes = [dp, dp, C.c_int64, dp]
        L.se3icp_transform_device.argtypes = [C.c_int, C.c_int32, vp, C.POINTER(C.c_int64), dp, vp, vp]
    L.se3icp_request_report.argtypes = [vp, rop]
    L.se3icp_get_report.argtypes = [vp, rep]
    L.se3icp_register.argtypes = [C.c_int, dp, C.c_int64, dp, C.c_int64, C.c_int, C.POINTER(Params),
                                  C.POINTER(Result)]
    L.se3icp_toldi_frames.argtypes = [C.c_int, dp, C.c_int64, C.c_int, dp]
    L.se3icp_knn_self.argtypes = [C.c_int, dp, C.c_int64, C.c_int, ip]
    L.se3icp_estimate_normals.argtypes = [C.c_int, dp, C.c_int64, C.c_int, dp]
    L.se3icp_nn.argtypes = [C.c_int, dp, C.c_int64, dp, C.c_int64, C.c_int, ip, dp, ip]
    if hasattr(L, "se3icp_nn_sequence"):  # (SE3ICP_LIB may name an older build for an A/B run)
        fp = C.POINTER(C.c_float)
        L.se3icp_nn_sequence_version.restype = C.c_int
        L.se3icp_nn_sequence.argtypes = [C.c_int, dp, C.c_int64, dp, C.c_int64, C.c_int, C.c_double, C.c_int32, dp,
                                         C.c_int32, ip, fp, fp, fp, ip, ip, ip, ip, ip]
    L.se3icp_synthetic_pairs.restype = C.c_int64
    L.se3icp_synthetic_pairs.argtypes = [C.c_int, dp, C.c_int64, C.c_int32, dp, C.c_double, C.c_double, C.c_uint64,
                                         vp, vp, C.c_int]
    L.se3icp_synthetic_reference.restype = C.c_int64
    L.se3icp_synthetic_reference.argtypes = [dp, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                                             C.c_int32, dp, dp, dp]
    L.se3icp_synthetic_reference_device.restype = C.c_int64
    L.se3icp_synthetic_reference_device.argtypes = [C.c_int, dp, C.c_int64, C.c_int32, C.c_double, C.c_double,
                                                    C.c_double, C.c_double, C.c_int32, vp, vp, dp, C.c_int]
    L.se3icp_random_downsample.restype = C.c_int64
    L.se3icp_random_downsample.argtypes = [dp, C.c_int64, C.c_double, C.c_uint32, dp]
    L.se3icp_voxel_version.restype = C.c_int
    L.se3icp_voxel_downsample_device.argtypes = [C.c_int, C.c_int32, vp, C.POINTER(C.c_int64), dp, vp,
                                                 C.POINTER(C.c_int64), vp, vp, vp]
    L.se3icp_voxel_downsample.restype = C.c_int64
    L.se3icp_voxel_downsample.argtypes = [C.c_int, dp, C.c_int64, C.c_double, dp, ip, ip]
    L.se3icp_set_profiling.argtypes = [C.c_int, C.c_int]
    L.se3icp_last_kernel_times.argtypes = [C.c_int, dp]
    L.se3icp_last_kernel_times_n.argtypes = [C.c_int, dp, C.c_int]
    L.se3icp_set_trace.argtypes = [C.c_int, C.POINTER(Trace)]
    if hasattr(L, "se3icp_setup_record_version"):  # (SE3ICP_LIB may name an older build for an A/B run)
        L.se3icp_setup_record_version.restype = C.c_int
        L.se3icp_set_setup_record.argtypes = [C.c_int, C.POINTER(SetupRecord)]
    if hasattr(L, "se3icp_tree_record_version"):  # (likewise)
        L.se3icp_tree_record_version.restype = C.c_int
        L.se3icp_set_tree_record.argtypes = [C.c_int, C.POINTER(TreeRecord)]
    L.se3icp_set_lrf_exact.argtypes = [C.c_int, C.c_int]
    L.se3icp_set_nn_events.argtypes = [C.c_int, C.c_int]
    # (se3icp_set_batch_sharing(int, int), se3icp_set_lrf_seeding(int, int),
    # se3icp_last_seed_stats(int, int64_t*, int), se3icp_set_tree_sharing(int, int),
    # se3icp_last_tree_stats(int, int64_t*, int), se3icp_set_lrf_taking(int, int) and
    # se3icp_last_take_stats(int, int64_t*, int) are called with ctypes' default conversions and
    # resolved at their first call: SE3ICP_LIB may name an older build for an A/B run)
    _lib = L
    return L


def status_string(code: int) -> str:
    return load().se3icp_status_string(int(code)).decode()


def check(code: int, what: str = "") -> int:
    if code != OK:
        raise Se3IcpError(code, what)
    return code


def default_params(**overrides) -> Params:
    p = Params()
    load().se3icp_default_params(C.byref(p))
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def device_count() -> int:
    return load().se3icp_device_count()


def method_id(name: str) -> int:
    m = load().se3icp_method_from_name(name.encode())
    if m < 0:
        raise ValueError(f"unknown method {name!r}; valid: {', '.join(METHODS)}")
    return m
