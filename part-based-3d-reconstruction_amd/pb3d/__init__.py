"""pb3d -- MI355X-native semantic voxel carving & re-projection (host side).

Mirrors the reference's L2 function surface (utils.voxel_carving_utils, utils.voxel_utils,
utils.projection_utils, utils.camera_geometry, utils.camera_estimation.compute_partwise_iou and the
minaret extraction, the notebook-4 and inter-method evaluations, utils.config) on top of libpb3d.so.  `install()` rebinds those names inside an imported
reference `utils` package so notebooks 1-3 run unchanged.
"""
from . import _hostmem, _lib, device, dist, formats, labels, perspective, selection  # noqa: F401
from .formats import load_camera_params, load_voxel_grid, save_camera_params, save_voxel_grid  # noqa: F401
from .labels import (Palette, extrude_from_surface_labels, get_voxel_points_by_parts_labels, global_carve_labels, label_to_rgb,  # noqa: F401
                     left_right_guided_carve_labels, part_carve_labels, partwise_carve_labels, recolor_backward_components_labels, rgb_to_label,
                     voxel_grid_to_points_labels)
from ._hostmem import set_result_pool  # noqa: F401
from .camera_estimation import (CameraObjective, compute_partwise_iou, coordinate_descent, powell_search, projection_iou_by_part,  # noqa: F401
                                random_search)
from .camera_estimation import (auto_compute_initial_params_matching_bbox, bbox_init_from_bounds, optimize_camera_with_keypoints,  # noqa: F401
                                projection_overlays, visualize_voxel_projection_iou)
from .eval_helpers import (chamfer_distance, compute_f1_curve, compute_nn_distances, compute_nn_stats, f1_curve_from_distances,  # noqa: F401
                           filter_mesh, fscore_with_threshold, nn_distances, pca_shape_similarity, voxel_iou)
from .eval_helpers import (compute_surface_metrics, compute_triangle_normals, compute_vertex_normals, knn,  # noqa: F401
                           surface_metrics_per_vertex)
from .eval_helpers import density_grid_resident, pointcloud_to_voxel_grid  # noqa: F401
from .eval_helpers import get_marching_cubes_mesh, isosurface, marching_cubes_mesh_resident  # noqa: F401
from .eval_helpers import cloud_to_mesh_metrics, point_to_mesh_distances, sample_mesh_points  # noqa: F401
from .preprocess_helpers import (best_fit_transform_from_sums, flip_y_axis, icp_align, icp_align_resident, normalize_preserve_aspect,  # noqa: F401
                                 transform_points, transform_points_resident)
from .preprocess_helpers import best_fit_similarity_from_sums, icp_step_trimmed_resident  # noqa: F401
from .preprocess_helpers import (estimate_normals, estimate_normals_resident, icp_step_plane_resident,  # noqa: F401
                                 plane_step_from_sums)
from .selection import kth_smallest, kth_smallest_resident  # noqa: F401
from .preprocess_helpers import (crop_to_box, crop_to_box_resident, fit_plane_ransac, fit_plane_ransac_resident,  # noqa: F401
                                 plane_alignment_transform, plane_from_moments, plane_hypotheses_resident, plane_moments_resident,
                                 plane_score_resident, symmetric_completion, symmetric_completion_resident)
from .cluster import (cluster_points, cluster_points_resident, keep_largest_clusters, keep_largest_clusters_resident,  # noqa: F401
                      radius_neighbor_counts, radius_neighbor_counts_resident, select_points, select_points_resident)
from .downsample import voxel_downsample, voxel_downsample_resident  # noqa: F401
from .smooth import mesh_vertex_adjacency, mesh_vertex_adjacency_resident, smooth_mesh, smooth_mesh_resident  # noqa: F401
from .simplify import compact_mesh, compact_mesh_resident, simplify_mesh, simplify_mesh_resident  # noqa: F401
from .meshcomp import (keep_mesh_components, keep_mesh_components_resident, mesh_components, mesh_components_resident,  # noqa: F401
                       mesh_topology, mesh_topology_resident, select_faces, select_faces_resident)
from .voxelize import grid_overlap_counts, grid_overlap_counts_resident, mesh_grid_iou, voxelize_mesh, voxelize_mesh_resident  # noqa: F401
from .inside import (points_in_mesh, points_in_mesh_last, points_in_mesh_resident, select_points_in_mesh,  # noqa: F401
                     select_points_in_mesh_resident, signed_point_to_mesh_distances, signed_point_to_mesh_distances_resident)
from .distance import (close_grid, close_grid_resident, dilate_grid, dilate_grid_resident, distance_transform,  # noqa: F401
                       distance_transform_resident, erode_grid, erode_grid_resident, grid_surface_metrics, grid_surface_metrics_resident,
                       open_grid, open_grid_resident)
from .render import mesh_projection_iou, render_mesh, render_mesh_resident, render_shade_resident  # noqa: F401
from .orient import mesh_orientation, mesh_orientation_resident, orient_mesh, orient_mesh_resident  # noqa: F401
from .weld import weld_vertices, weld_vertices_resident  # noqa: F401
from .raycast import (camera_rays, cast_rays, cast_rays_last, cast_rays_resident, points_visible_from, rays_occluded,  # noqa: F401
                      rays_occluded_resident)
from .eval_helpers_intra import (color_presence, compute_binary_gt, compute_global_depth_buffer, grid_depth_buffer, grid_visible_bits,  # noqa: F401
                                 points_visible_bits, project_part_visible, run_minaret_iou_evaluation, run_minaret_kp_evaluation,
                                 run_part_minaret_binary_iou)
from .minarets import (extract_minaret_kps_for_view, extract_minaret_masks_by_label, extract_minaret_voxels_by_label,  # noqa: F401
                       extract_top_bottom_image_points, extract_top_bottom_voxel_points)
from .mask_utils import load_and_prepare_masks, load_mask, mask_parts_from_image  # noqa: F401
from .camera_geometry import look_at_rotation, project  # noqa: F401
from .deformation_estimation import (build_deformed_grid, deform_coords, deform_part, evaluate_part_deform,  # noqa: F401
                                     evaluate_part_deform_batch)
from .config import INTERIOR_PARTS, MAX_DIM, PART_COLORS, PART_COLORS_NP  # noqa: F401
from .projection_utils import project_colored_voxels  # noqa: F401
from .perspective import (pack_mask_bits, perspective_carve, perspective_carve_resident, perspective_paint,  # noqa: F401
                          perspective_paint_resident)
from .voxel_carving_utils import (apply_colored_mask_to_voxel_grid, carve_voxel_grid_with_masks, extrude_from_surface,  # noqa: F401
                                  global_carve, left_right_guided_carve, part_carve, partwise_carve, process_voxel_grid,
                                  recolor_backward_components)
from .voxel_utils import extract_top_k_components, get_voxel_points_by_parts, meshify_colored_voxel_grid, voxel_grid_to_points  # noqa: F401

_PATCH = {
    "voxel_carving_utils": ["carve_voxel_grid_with_masks", "process_voxel_grid", "apply_colored_mask_to_voxel_grid",
                            "part_carve", "global_carve", "_occupancy", "left_right_guided_carve", "extrude_from_surface",
                            "recolor_backward_components", "partwise_carve"],
    "voxel_utils": ["get_voxel_points_by_parts", "extract_top_k_components", "voxel_grid_to_points", "meshify_colored_voxel_grid"],
    "projection_utils": ["project_colored_voxels"],
    "camera_estimation": ["compute_partwise_iou", "extract_minaret_voxels_by_label", "extract_minaret_masks_by_label",
                          "extract_top_bottom_voxel_points", "extract_top_bottom_image_points", "extract_minaret_kps_for_view",
                          "auto_compute_initial_params_matching_bbox", "optimize_camera_with_keypoints", "visualize_voxel_projection_iou"],
    # load_mask is left out: utils.mask_utils has a load_mask of its own (another signature) and install() rebinds by name
    "eval_helpers_intra": ["compute_global_depth_buffer", "project_part_visible", "load_voxel_grid", "resize_mask_to_voxel_grid",
                           "load_camera_json", "project_keypoints", "compute_binary_gt", "_iou_bool", "run_minaret_kp_evaluation",
                           "run_minaret_iou_evaluation", "run_part_minaret_binary_iou"],
    "eval_helpers": ["filter_mesh", "_downsample", "chamfer_distance", "fscore_with_threshold", "pca_shape_similarity", "voxel_iou",
                     "compute_nn_stats", "compute_nn_distances", "f1_curve_from_distances", "compute_f1_curve", "compute_triangle_normals",
                     "compute_vertex_normals", "compute_surface_metrics", "pointcloud_to_voxel_grid", "get_marching_cubes_mesh"],
}


def install(utils_pkg=None):
    """Rebind the hot-path functions of an imported reference `utils` package to pb3d.

    Every module of the package that holds one of the names (the reference star-imports
    them across modules) is patched, so internal callers such as left_right_guided_carve or
    the camera aligner pick up the GPU path too.  Returns the list of (module, name) patched.
    """
    import importlib
    import sys
    import types

    if utils_pkg is None:
        utils_pkg = sys.modules.get("utils") or importlib.import_module("utils")
    here = sys.modules[__name__]
    patched = []
    names = {n: getattr(importlib.import_module(f"{__name__}.{mod}"), n) for mod, ns in _PATCH.items() for n in ns}
    for modname, mod in list(sys.modules.items()):
        if not isinstance(mod, types.ModuleType) or not (modname == utils_pkg.__name__ or modname.startswith(utils_pkg.__name__ + ".")):
            continue
        for n, fn in names.items():
            if n in mod.__dict__ and mod.__dict__[n] is not fn:
                mod.__dict__[n] = fn
                patched.append((modname, n))
    ev = sys.modules.get(utils_pkg.__name__ + ".eval_helpers_intra")
    if ev is not None:      # visualize=True of the notebook-4 evaluations calls the reference's own plotting functions
        here.eval_helpers_intra._REF["module"] = ev
    ce = sys.modules.get(utils_pkg.__name__ + ".camera_estimation")
    if ce is not None and hasattr(ce, "minimize"):      # the keypoint fit runs the reference's own minimiser
        here.camera_estimation._REF["minimize"] = ce.minimize
    vis = sys.modules.get(utils_pkg.__name__ + ".visualization")
    if vis is not None and hasattr(vis, "plot_voxel"):
        here.voxel_carving_utils.plot_voxel = vis.plot_voxel
    return patched
