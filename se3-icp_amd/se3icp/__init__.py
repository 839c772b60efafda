"""se3icp — MI355X-native SE(3)-ICP registration (host side of libse3icp.so).

Drop-in for kenahm/se3-icp's ``IterativeSE3Registration`` (see registration.py);
the registration itself runs in hand-written HIP kernels for gfx950 (csrc/).
"""
from ._lib import (METHODS, Params, Result, Se3IcpError, default_params, device_count, load,  # noqa: F401
                   method_id, status_string)
from .io import read_ply_xyz, write_ply_xyz  # noqa: F401
from .registration import (DeviceBatchRunner, IterativeSE3Registration, PairResult, PipelinedBatchRunner,  # noqa: F401
                           cli_params,
                           estimate_normals,
                           kitti_params, knn_self, last_kernel_times, set_nn_events, set_profiling, lounge_params,
                           nearest_neighbors, nearest_neighbors_sequence,
                           register_batch, register_batch_device, register_batch_traced, setup_record, toldi_frames,
                           tree_record,
                           alpha_grid, register_sweep, register_sweep_device, register_sweep_traced, sweep_params,
                           PairReport, register_batch_report, register_batch_report_device, register_sweep_report,
                           register_sweep_report_device,
                           expand_edges, last_graph_stats, register_graph, register_graph_device,
                           register_graph_report, register_graph_traced, register_sequence, sequence_edges,
                           set_batch_sharing, set_lrf_seeding, last_seed_stats,
                           set_tree_sharing, last_tree_stats, set_lrf_taking, last_take_stats,
                           voxel_downsample, voxel_downsample_device,
                           edge_inits, last_init_stats, set_pose_seeding, transform_device, transform_points)
from ._lib import Report, ReportOptions  # noqa: F401

__all__ = [
    "IterativeSE3Registration", "register_batch", "register_batch_device", "DeviceBatchRunner", "PipelinedBatchRunner", "register_batch_traced", "toldi_frames", "knn_self",
    "estimate_normals", "nearest_neighbors", "nearest_neighbors_sequence", "default_params", "cli_params", "kitti_params", "lounge_params",
    "read_ply_xyz", "write_ply_xyz", "METHODS", "Se3IcpError",
    "register_sweep", "register_sweep_device", "register_sweep_traced", "alpha_grid", "sweep_params",
    "PairReport", "Report", "ReportOptions", "register_batch_report", "register_batch_report_device",
    "register_sweep_report", "register_sweep_report_device",
    "register_graph", "register_sequence", "sequence_edges", "expand_edges", "register_graph_device",
    "register_graph_report", "register_graph_traced", "last_graph_stats",
    "set_batch_sharing", "set_lrf_seeding", "last_seed_stats", "set_tree_sharing", "last_tree_stats",
    "set_lrf_taking", "last_take_stats", "setup_record", "tree_record",
    "voxel_downsample", "voxel_downsample_device",
    "edge_inits", "transform_points", "transform_device", "set_pose_seeding", "last_init_stats",
]
