"""ctypes loader of libbuildingsegment_hip.so (the C ABI of include/bs_api.h).

Fails loudly when the HIP library is missing or cannot be loaded: there is no
CPU fallback on the product path.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# BS_LIB_PATH: developer override (A/B runs of two builds of the same HIP library on one box)
LIB_PATH = os.environ.get("BS_LIB_PATH") or os.path.join(HERE, "libbuildingsegment_hip.so")

BS_OK = 0
STATUS = {0: "BS_OK", -1: "BS_ERR_INVALID", -2: "BS_ERR_RANGE", -3: "BS_ERR_NOMEM", -4: "BS_ERR_HIP",
          -5: "BS_ERR_NO_DEVICE", -6: "BS_ERR_INTERNAL", -7: "BS_ERR_UNCERTIFIED"}

# every symbol include/bs_api.h declares
EXPORTS = ["bs_api_version", "bs_sizeof_timings", "bs_strerror", "bs_params_default", "bs_create", "bs_destroy", "bs_last_error",
           "bs_set_stream", "bs_get_timings", "bs_knn_normals", "bs_knn_normals_halo", "bs_region_grow", "bs_segment",
           "bs_planes_free", "bs_plane_colors", "bs_knn_normals_dev", "bs_region_grow_dev",
           "bs_segment_dev", "bs_planes_fetch", "bs_shift_to_origin_dev", "bs_plane_colors_dev",
           "bs_selftest_center_div", "bs_selftest_forge_next", "bs_set_audit", "bs_selftest_grow_limits",
           "bs_get_grow_counters", "bs_ingest_dev", "bs_grid_dims", "bs_grid_picture", "bs_grid_picture_dev",
           "bs_cc_hook_dev", "bs_owner_fetch_dev", "bs_labels_from_owner_dev", "bs_remap_rows_dev",
           "bs_plane_seeds_dev", "bs_stream_sync", "bs_comm_rccl", "bs_comm_rccl_unique_id", "bs_comm_rccl_init",
           "bs_comm_rccl_destroy", "bs_comm_local_create", "bs_comm_local_destroy", "bs_segment_sharded",
           "bs_sharded_planes_fetch", "bs_footprints_dev", "bs_footprints", "bs_contours_free",
           "bs_contours_write_obj", "bs_segment_batch", "bs_segment_batch_dev", "bs_batch_planes_fetch",
           "bs_shift_tiles_to_origin_dev", "bs_tile_boxes_dev", "bs_grid_dims_batch", "bs_grid_picture_batch_dev",
           "bs_grid_picture_batch", "bs_footprints_batch_dev", "bs_footprints_batch", "bs_building_map_dev",
           "bs_building_map", "bs_buildings_free", "bs_assign_buildings_dev", "bs_assign_buildings",
           "bs_plane_buildings_dev", "bs_plane_buildings", "bs_buildings_write_obj", "bs_roof_homes", "bs_roofs_dev",
           "bs_roofs", "bs_roofs_free", "bs_roofs_write_obj", "bs_plane_fit_dev", "bs_plane_fit", "bs_plane_fits_free",
           "bs_plane_fit_apply", "bs_solids_count_dev", "bs_solids_emit_dev", "bs_solids", "bs_solids_free",
           "bs_solids_write_obj", "bs_roof_facets_dev", "bs_roof_facets", "bs_roof_facets_free", "bs_roof_edge_kinds",
           "bs_roof_edges_write_obj", "bs_roof_generalise_dev", "bs_roof_generalise", "bs_roof_generalise_free",
           "bs_facet_outlines_count_dev", "bs_facet_outlines_emit_dev", "bs_facet_outlines",
           "bs_outlines_free", "bs_outlines_write_obj", "bs_simple_outlines_count_dev", "bs_simple_outlines_emit_dev",
           "bs_simple_outlines", "bs_simple_outlines_free", "bs_simple_outlines_write_obj", "bs_clean_outlines_count_dev",
           "bs_clean_outlines_emit_dev", "bs_clean_outlines", "bs_clean_outlines_free", "bs_clean_outlines_write_obj",
           "bs_set_outline_sweeps", "bs_get_outline_sweeps",
           "bs_outline_triangles_count_dev", "bs_outline_triangles_emit_dev", "bs_outline_triangles",
           "bs_outline_triangles_free", "bs_outline_triangles_write_obj", "bs_poly_solids_count_dev",
           "bs_poly_solids_emit_dev", "bs_poly_solids", "bs_poly_solids_free", "bs_model_raster_dev", "bs_model_raster",
           "bs_model_raster_free", "bs_point_residuals_dev", "bs_point_residuals", "bs_point_residuals_free",
           "bs_terrain_dev", "bs_terrain", "bs_terrain_free", "bs_set_building_bases", "bs_get_building_bases",
           "bs_ground_dev", "bs_ground", "bs_ground_free", "bs_set_ground_model", "bs_set_ground_model_dev",
           "bs_get_ground_model", "bs_plane_quality", "bs_roof_evidence_dev", "bs_roof_evidence", "bs_set_footprint_screen",
           "bs_set_footprint_screen_dev", "bs_get_footprint_screen", "bs_selftest_scratch_guard",
           "bs_selftest_scratch_check", "bs_selftest_scratch_list", "bs_label_hulls_count_dev", "bs_label_hulls_emit_dev",
           "bs_label_hulls", "bs_label_hulls_free", "bs_hull_box_corners", "bs_hull_boxes_write_obj"]


class Params(C.Structure):
    _fields_ = [("k", C.c_int32), ("max_nn", C.c_int32), ("radius", C.c_double),
                ("th_thickness", C.c_int32), ("th_point_count", C.c_int32), ("cos_th", C.c_double),
                ("cell_size", C.c_int32), ("rg_mode", C.c_int32)]


class Planes(C.Structure):
    _fields_ = [("n_planes", C.c_int32), ("id", C.POINTER(C.c_int32)), ("normal", C.POINTER(C.c_double)),
                ("center", C.POINTER(C.c_int32)), ("offset", C.POINTER(C.c_int64)),
                ("point_idx", C.POINTER(C.c_int32))]


class Timings(C.Structure):
    _fields_ = [("grid_ms", C.c_double), ("knn_ms", C.c_double), ("grow_ms", C.c_double),
                ("total_ms", C.c_double), ("largest_plane", C.c_int64), ("n_seed_attempts", C.c_int64),
                ("n_fallback_queries", C.c_int64), ("rg_rounds", C.c_int64), ("grow_kernel_ms", C.c_double),
                ("grow_kernel_launches", C.c_int64), ("grow_setup_ms", C.c_double),
                ("validation_rejects", C.c_int64), ("forged_seed", C.c_int64), ("forged_refused", C.c_int64),
                ("audit_attempts", C.c_int64), ("audit_mismatches", C.c_int64), ("audit_ms", C.c_double),
                ("tie_rows", C.c_int64), ("rej_v1_robbed", C.c_int64), ("rej_v1_tag", C.c_int64), ("rej_v1_dup", C.c_int64),
                ("rej_v3_state", C.c_int64), ("incons_seed", C.c_int64), ("incons_list", C.c_int64),
                ("incons_log", C.c_int64)]


class GrowLimits(C.Structure):
    """bs_grow_limits (include/bs_api.h): capacities 0 = default, policies < 0 = default."""
    _fields_ = [("max_waves", C.c_int64), ("pool_cap", C.c_int64), ("max_pending", C.c_int64), ("pstore_cap", C.c_int64),
                ("retry_max_list", C.c_int32), ("retry_big_round", C.c_int32), ("full_refresh", C.c_int32),
                ("reserved", C.c_int32)]


class GrowCounters(C.Structure):
    _fields_ = [(k, C.c_int64) for k in
                ("rounds", "rounds_capped", "rounds_big", "attempts_nomem", "waves_cut", "max_waves_end", "attempts_stolen",
                 "dropped_pend_count", "dropped_pend_store", "dropped_other", "full_refreshes", "pool_cap")]


class ScratchSlot(C.Structure):
    """bs_scratch_slot (include/bs_api.h): one buffer of a context allocated under the scratch guard."""
    _fields_ = [("name", C.c_char * 24), ("address", C.c_uint64), ("requested", C.c_int64), ("guard", C.c_int64),
                ("first_bad", C.c_int64), ("last_bad", C.c_int64), ("host", C.c_int32), ("reserved", C.c_int32)]


class ScratchReport(C.Structure):
    _fields_ = [("n_guarded", C.c_int64), ("bytes_requested", C.c_int64), ("n_damaged", C.c_int64),
                ("n_listed", C.c_int64), ("damaged", ScratchSlot * 8)]


API_VERSION = 5  # BS_API_VERSION of include/bs_api.h this loader mirrors


class CommOps(C.Structure):
    """bs_comm_ops (include/bs_api.h): the three collectives bs_segment_sharded is built on."""
    _fields_ = [("handle", C.c_void_p), ("rank", C.c_int32), ("world", C.c_int32),
                ("all_reduce", C.c_void_p), ("all_gather", C.c_void_p), ("all_to_all_v", C.c_void_p)]


class ShardInfo(C.Structure):
    _fields_ = [("n_own", C.c_int64), ("n_local", C.c_int64), ("n_grow", C.c_int64), ("components", C.c_int64),
                ("planes_total", C.c_int64), ("cc_iterations", C.c_int32), ("halo_retries", C.c_int32),
                ("halo_mm", C.c_double), ("ms_partition", C.c_double), ("ms_halo", C.c_double), ("ms_knn", C.c_double),
                ("ms_components", C.c_double), ("ms_redistribute", C.c_double), ("ms_grow", C.c_double),
                ("ms_labels", C.c_double)]


class Contours(C.Structure):
    """bs_contours (include/bs_api.h): CSR point lists of the footprint contours, host memory owned by the library."""
    _fields_ = [("n_contours", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("offset", C.POINTER(C.c_int64)), ("xy", C.POINTER(C.c_int32)), ("area", C.POINTER(C.c_double)),
                ("perimeter", C.POINTER(C.c_double))]


class FootprintInfo(C.Structure):
    _fields_ = [("ms_mask", C.c_double), ("ms_close", C.c_double), ("ms_label", C.c_double), ("ms_trace", C.c_double),
                ("ms_total", C.c_double), ("fg_pixels", C.c_int64), ("border_states", C.c_int64),
                ("components", C.c_int64), ("jump_rounds", C.c_int64)]


class Buildings(C.Structure):
    """bs_buildings (include/bs_api.h): per-building figures, host memory owned by the library."""
    _fields_ = [("n_buildings", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("start_xy", C.POINTER(C.c_int32)), ("bbox", C.POINTER(C.c_int32)), ("pixels", C.POINTER(C.c_int64)),
                ("fg_pixels", C.POINTER(C.c_int64)), ("n_points", C.POINTER(C.c_int64)),
                ("n_above", C.POINTER(C.c_int64)), ("z_min", C.POINTER(C.c_int32)), ("z_max", C.POINTER(C.c_int32)),
                ("z_sum", C.POINTER(C.c_int64)), ("ms_label_mask", C.c_double), ("ms_label_fill", C.c_double),
                ("ms_number", C.c_double), ("ms_map", C.c_double), ("ms_assign", C.c_double)]


class Roofs(C.Structure):
    """bs_roofs (include/bs_api.h): per-plane roof figures, host memory owned by the library."""
    _fields_ = [("n_planes", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("fill_rounds", C.c_int32),
                ("seeded_pixels", C.c_int64), ("filled_pixels", C.c_int64), ("unroofed_pixels", C.c_int64),
                ("pixels", C.POINTER(C.c_int64)), ("seed_pixels", C.POINTER(C.c_int64)), ("bbox", C.POINTER(C.c_int32)),
                ("n_support", C.POINTER(C.c_int64)), ("z_min", C.POINTER(C.c_int32)), ("z_max", C.POINTER(C.c_int32)),
                ("z_sum", C.POINTER(C.c_int64)), ("ms_vote", C.c_double), ("ms_fill", C.c_double),
                ("ms_figures", C.c_double), ("ms_height", C.c_double)]


class PlaneFits(C.Structure):
    """bs_plane_fits (include/bs_api.h): per-plane fit, host memory owned by the library."""
    _fields_ = [("n_planes", C.c_int32), ("status", C.POINTER(C.c_int32)), ("n_points", C.POINTER(C.c_int64)),
                ("center", C.POINTER(C.c_int32)), ("normal", C.POINTER(C.c_double)), ("bbox", C.POINTER(C.c_int32)),
                ("dev_sum", C.POINTER(C.c_int64)), ("moment", C.POINTER(C.c_int64)), ("r_abs_max", C.POINTER(C.c_int32)),
                ("r_abs_sum", C.POINTER(C.c_int64)), ("r_sq_sum", C.POINTER(C.c_int64)), ("ms_sums", C.c_double),
                ("ms_moments", C.c_double), ("ms_solve", C.c_double), ("ms_residuals", C.c_double)]


class Solids(C.Structure):
    """bs_solids (include/bs_api.h): totals, per-building figures and (host-memory entry point) the mesh, host memory owned
    by the library."""
    _fields_ = [("n_buildings", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("bin", C.c_int32),
                ("base_z", C.c_int32), ("n_pixels", C.c_int64), ("n_vertices", C.c_int64), ("n_faces", C.c_int64),
                ("n_indices", C.c_int64), ("n_wall_faces", C.c_int64), ("n_crossing_walls", C.c_int64),
                ("total_volume6", C.c_int64), ("pixels", C.POINTER(C.c_int64)), ("vertices", C.POINTER(C.c_int64)),
                ("faces", C.POINTER(C.c_int64)), ("wall_faces", C.POINTER(C.c_int64)),
                ("crossing_walls", C.POINTER(C.c_int64)), ("top_min", C.POINTER(C.c_int32)),
                ("top_max", C.POINTER(C.c_int32)), ("volume6", C.POINTER(C.c_int64)), ("vertex", C.POINTER(C.c_int32)),
                ("face_offset", C.POINTER(C.c_int32)), ("face_index", C.POINTER(C.c_int32)),
                ("face_building", C.POINTER(C.c_int32)), ("face_kind", C.POINTER(C.c_uint8)), ("ms_tops", C.c_double),
                ("ms_vertices", C.c_double), ("ms_faces", C.c_double), ("ms_figures", C.c_double), ("ms_scans", C.c_double),
                ("ms_emit_vertices", C.c_double), ("ms_emit_faces", C.c_double)]


class RoofFacets(C.Structure):
    """bs_roof_facets (include/bs_api.h): totals, per-facet and per-edge figures, host memory owned by the library."""
    _fields_ = ([("width", C.c_int32), ("height", C.c_int32), ("n_facets", C.c_int64), ("n_edges", C.c_int64),
                 ("n_pixels", C.c_int64), ("n_border", C.c_int64)] +
                [("facet_" + k, C.POINTER(t)) for k, t in
                 (("building", C.c_int32), ("plane", C.c_int32), ("start_xy", C.c_int32), ("pixels", C.c_int64),
                  ("bbox", C.c_int32), ("inner_edges", C.c_int64), ("outer_edges", C.c_int64), ("top_min", C.c_int32),
                  ("top_max", C.c_int32), ("top_sum", C.c_int64))] +
                [("edge_" + k, C.POINTER(t)) for k, t in
                 (("facet", C.c_int32), ("building", C.c_int32), ("length", C.c_int64), ("n_dir0", C.c_int64),
                  ("n_step", C.c_int64), ("step_abs_sum", C.c_int64), ("step_abs_max", C.c_int64), ("rise_sum", C.c_int64),
                  ("bend_sum", C.c_int64), ("z_min", C.c_int32), ("z_max", C.c_int32), ("bbox", C.c_int32))] +
                [("ms_label", C.c_double), ("ms_number", C.c_double), ("ms_figures", C.c_double), ("ms_edges", C.c_double)])


GEN_FIG_CAP, GEN_PLANE_CAP = 1024, 1024  # BS_GEN_FIG_CAP, BS_GEN_PLANE_CAP of include/bs_api.h
GEN_SCALARS = ("n_facets_in", "n_facets_out", "n_edges_in", "n_edges_out", "n_flat_in", "n_flat_out", "n_small_in",
               "n_small_out", "pixels_changed", "pixels_roofed")
GEN_EVAL = ("eval_facets", "eval_movers", "eval_movers_small", "eval_movers_flat", "eval_longest_chain")
GEN_PLANE = ("plane_pixels_in", "plane_pixels_out")
GEN_BUILDING = ("building_facets_in", "building_facets_out", "building_pixels_changed", "building_sum_abs_dtop",
                "building_max_abs_dtop")
GEN_MS = ("ms_tops", "ms_facets", "ms_decide", "ms_apply", "ms_figures")


class RoofGeneraliseParams(C.Structure):
    """bs_roof_generalise_params (include/bs_api.h)"""
    _fields_ = [("min_pixels", C.c_int64), ("merge_flat", C.c_int32), ("step_tol", C.c_int32), ("bend_tol", C.c_int32),
                ("max_rounds", C.c_int32)]


class RoofGeneralise(C.Structure):
    """bs_roof_generalise (include/bs_api.h): totals, per-evaluation, per-plane and per-building figures, host memory owned
    by the library."""
    _fields_ = ([(k, C.c_int32) for k in ("width", "height", "n_buildings", "n_planes", "rounds", "converged")] +
                [(k, C.c_int64) for k in GEN_SCALARS] +
                [(k, C.POINTER(C.c_int64)) for k in GEN_EVAL + GEN_PLANE + GEN_BUILDING] + [(k, C.c_double) for k in GEN_MS])


class Outlines(C.Structure):
    """bs_outlines (include/bs_api.h): totals, per-ring and per-label arrays and (host-memory entry point) the vertices,
    host memory owned by the library."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_labels", C.c_int32), ("has_z", C.c_int32),
                ("n_half", C.c_int64), ("n_rings", C.c_int64), ("n_vertices", C.c_int64),
                ("ring_label", C.POINTER(C.c_int32)), ("ring_start", C.POINTER(C.c_int32)),
                ("ring_length", C.POINTER(C.c_int64)), ("ring_vertices", C.POINTER(C.c_int64)),
                ("ring_area2", C.POINTER(C.c_int64)), ("ring_bbox", C.POINTER(C.c_int32)),
                ("ring_offset", C.POINTER(C.c_int64)), ("label_ring_offset", C.POINTER(C.c_int64)),
                ("xy", C.POINTER(C.c_int32)), ("z", C.POINTER(C.c_int32)), ("ms_halfedges", C.c_double),
                ("ms_leaders", C.c_double), ("ms_rank", C.c_double), ("ms_rings", C.c_double), ("ms_emit", C.c_double)]


class SimpleOutlines(C.Structure):
    """bs_simple_outlines (include/bs_api.h): totals, per-ring arrays and (host-memory entry point) the kept vertices, host
    memory owned by the library."""
    _fields_ = ([("width", C.c_int32), ("height", C.c_int32), ("n_labels", C.c_int32), ("has_z", C.c_int32),
                 ("tol_num", C.c_int32), ("tol_den", C.c_int32)] +
                [(k, C.c_int64) for k in ("n_rings", "n_nodes", "n_junction_nodes", "n_arcs", "n_svertices", "rounds",
                                          "max_arc_nodes")] +
                [("ring_label", C.POINTER(C.c_int32)), ("ring_area2", C.POINTER(C.c_int64)),
                 ("s_ring_vertices", C.POINTER(C.c_int64)), ("s_ring_area2", C.POINTER(C.c_int64)),
                 ("s_ring_arcs", C.POINTER(C.c_int64)), ("s_ring_offset", C.POINTER(C.c_int64)),
                 ("label_ring_offset", C.POINTER(C.c_int64)), ("sxy", C.POINTER(C.c_int32)), ("sz", C.POINTER(C.c_int32)),
                 ("s_right", C.POINTER(C.c_int32)), ("s_flag", C.POINTER(C.c_uint8))] +
                [(k, C.c_double) for k in ("ms_outlines", "ms_nodes", "ms_placing", "ms_arcs", "ms_rounds", "ms_rings",
                                           "ms_emit")])


class CleanOutlines(C.Structure):
    """bs_clean_outlines (include/bs_api.h): the simplified outlines' totals and arrays over the repaired kept set, and the
    figures of the conflict check and repair."""
    _fields_ = ([("width", C.c_int32), ("height", C.c_int32), ("n_labels", C.c_int32), ("has_z", C.c_int32),
                 ("tol_num", C.c_int32), ("tol_den", C.c_int32), ("max_rounds", C.c_int32), ("cell_log2", C.c_int32)] +
                [(k, C.c_int64) for k in ("n_rings", "n_nodes", "n_junction_nodes", "n_arcs", "n_svertices", "rounds",
                                          "max_arc_nodes", "n_svertices_before", "n_marked_first", "n_marked_left", "n_forced",
                                          "repair_rounds", "n_entries", "max_cell_entries")] +
                [("ring_label", C.POINTER(C.c_int32)), ("ring_area2", C.POINTER(C.c_int64)),
                 ("s_ring_vertices", C.POINTER(C.c_int64)), ("s_ring_area2", C.POINTER(C.c_int64)),
                 ("s_ring_arcs", C.POINTER(C.c_int64)), ("s_ring_offset", C.POINTER(C.c_int64)),
                 ("label_ring_offset", C.POINTER(C.c_int64)), ("sxy", C.POINTER(C.c_int32)), ("sz", C.POINTER(C.c_int32)),
                 ("s_right", C.POINTER(C.c_int32)), ("s_flag", C.POINTER(C.c_uint8))] +
                [(k, C.c_double) for k in ("ms_simplify", "ms_detect", "ms_repair", "ms_rings", "ms_emit")])


SWEEP_WAVE_CAP = 64  # BS_SWEEP_WAVE_CAP of include/bs_api.h
SWEEP_FIGURES = ("n_lens_segments_first", "n_sweeping_first", "n_sweeping_only_first", "n_swept_pairs_first", "max_abs_winding",
                 "sweep_rounds", "n_sweeping_left", "n_items_first", "n_items_swapped_first", "n_candidates_first",
                 "n_exact_first", "n_exact_wave_first", "n_rejected_first")


class OutlineSweeps(C.Structure):
    """bs_outline_sweeps (include/bs_api.h): the figures of the sweep detection of the last clean count."""
    _fields_ = ([("mode", C.c_int32), ("wave_cap", C.c_int32)] + [(k, C.c_int64) for k in SWEEP_FIGURES] +
                [("ms_sweep", C.c_double)])


TRI_STATUS = {0: "BS_TRI_OK", 1: "BS_TRI_NO_BRIDGE", 2: "BS_TRI_STALLED", 3: "BS_TRI_EMPTY"}
TRI_WAVE_CAP, TRI_LDS_CAP = 64, 1024  # BS_TRI_WAVE_CAP, BS_TRI_LDS_CAP of include/bs_api.h


class OutlineTriangles(C.Structure):
    """bs_outline_triangles (include/bs_api.h): totals, per-label and per-ring arrays and (host-memory entry point) the
    triangles, host memory owned by the library."""
    _fields_ = ([("n_labels", C.c_int32), ("wave_cap", C.c_int32), ("lds_cap", C.c_int32), ("reserved", C.c_int32)] +
                [(k, C.c_int64) for k in ("n_rings", "n_svertices", "n_triangles", "n_failed_labels", "n_bridges", "n_tests",
                                          "max_label_occurrences", "n_labels_wave", "n_labels_lds", "n_labels_global")] +
                [("tri_offset", C.POINTER(C.c_int64)), ("label_status", C.POINTER(C.c_int32)),
                 ("label_area2", C.POINTER(C.c_int64)), ("label_tests", C.POINTER(C.c_int64)),
                 ("bridge", C.POINTER(C.c_int32)), ("tri", C.POINTER(C.c_int32))] +
                [(k, C.c_double) for k in ("ms_clean", "ms_prologue", "ms_wave", "ms_lds", "ms_global", "ms_emit")])


POLY_FIG_CAP = 1024  # BS_POLY_FIG_CAP of include/bs_api.h
POLY_FIGURES = (("status", C.c_int32), ("labels", C.c_int64), ("vertices", C.c_int64), ("faces", C.c_int64),
                ("roof_faces", C.c_int64), ("wall_faces", C.c_int64), ("crossing_walls", C.c_int64),
                ("max_wall_vertices", C.c_int64), ("z_min", C.c_int32), ("z_max", C.c_int32), ("area2", C.c_int64),
                ("volume6", C.c_int64))
POLY_TOTALS = ("n_open_buildings", "n_vertices", "n_faces", "n_indices", "n_roof_faces", "n_wall_faces", "n_crossing_walls",
               "max_wall_vertices_all", "total_area2", "total_volume6")
POLY_MS = ("ms_triangles", "ms_twins", "ms_vertices", "ms_count", "ms_emit_vertices", "ms_emit_faces")


class PolySolids(C.Structure):
    """bs_poly_solids (include/bs_api.h): totals, per-building figures and (host-memory entry point) the mesh, host memory
    owned by the library."""
    _fields_ = ([(k, C.c_int32) for k in ("n_buildings", "n_labels", "bin", "base_z", "fig_cap", "reserved")] +
                [(k, C.c_int64) for k in POLY_TOTALS] + [(k, C.POINTER(t)) for k, t in POLY_FIGURES] +
                [("vertex", C.POINTER(C.c_int32)), ("face_offset", C.POINTER(C.c_int32)), ("face_index", C.POINTER(C.c_int32)),
                 ("face_building", C.POINTER(C.c_int32)), ("face_kind", C.POINTER(C.c_uint8))] +
                [(k, C.c_double) for k in POLY_MS])


MRASTER_FIG_CAP = 512  # BS_MRASTER_FIG_CAP of include/bs_api.h
MRASTER_CHUNK = 256    # BS_MRASTER_CHUNK
MRASTER_FIG_GRID = 2048  # BS_MRASTER_FIG_GRID
MRASTER_FIGURES = ("pixels", "model_pixels", "kept", "multi", "err_pixels", "sum_abs_e2", "max_abs_e2", "sq_lo", "sq_hi")
MRASTER_TOTALS = ("n_triangles", "total_pixels", "total_model_pixels", "total_kept", "total_err_pixels", "total_sum_abs_e2",
                  "max_abs_e2_all", "total_sq_lo", "total_sq_hi", "n_uncovered", "n_spill", "n_moved", "n_multi", "sum_cover",
                  "n_rows", "n_items", "n_empty_spans", "max_span")
MRASTER_MS = ("ms_rows", "ms_spans", "ms_pixels", "ms_figures")


class ModelRaster(C.Structure):
    """bs_model_raster (include/bs_api.h): totals and per-label figures, host memory owned by the library."""
    _fields_ = ([(k, C.c_int32) for k in ("width", "height", "n_labels", "fig_cap", "chunk", "reserved")] +
                [(k, C.c_int64) for k in MRASTER_TOTALS] + [(k, C.POINTER(C.c_int64)) for k in MRASTER_FIGURES] +
                [(k, C.c_double) for k in MRASTER_MS])


PRESID_FIG_CAP = 256  # BS_PRESID_FIG_CAP of include/bs_api.h
PRESID_CHUNK = 256    # BS_PRESID_CHUNK
PRESID_GRID = 2048    # BS_PRESID_GRID
PRESID_HEAD = ("width", "height", "n_labels", "bin", "clip2", "fig_cap", "chunk", "grid")
PRESID_FIGURES = ("points", "multi", "above", "below", "in_points", "sum_r2", "sum_abs_r2", "max_abs_r2", "sq_lo", "sq_hi",
                  "plane_points", "plane_in")
PRESID_TOTALS = ("n_points", "n_triangles", "total_points", "total_above", "total_below", "total_in_points", "total_sum_r2",
                 "total_sum_abs_r2", "max_abs_r2_all", "total_sq_lo", "total_sq_hi", "total_plane_points", "total_plane_in",
                 "n_uncovered", "n_multi", "n_rows", "n_items", "max_list", "n_empty_pixel", "n_height_wide")
PRESID_MS = ("ms_rows", "ms_spans", "ms_lists", "ms_points")


class PointResiduals(C.Structure):
    """bs_point_residuals (include/bs_api.h): totals and per-label figures, host memory owned by the library."""
    _fields_ = ([(k, C.c_int32) for k in PRESID_HEAD] + [(k, C.c_int64) for k in PRESID_TOTALS] +
                [(k, C.POINTER(C.c_int64)) for k in PRESID_FIGURES] + [(k, C.c_double) for k in PRESID_MS])


TERRAIN_MAX_RING = 255  # BS_TERRAIN_MAX_RING of include/bs_api.h
TERRAIN_FIG_CAP = 1024  # BS_TERRAIN_FIG_CAP
TERRAIN_GRID = 2048     # BS_TERRAIN_GRID
TERRAIN_HEAD = ("width", "height", "n_buildings", "bin", "ring", "q_num", "q_den", "min_ground", "fallback_z", "fig_cap", "grid",
                "rounds_used", "n_fallback", "reserved")
TERRAIN_TOTALS = ("n_points", "n_ring_pixels", "n_ground_pixels", "n_ring_points")
TERRAIN_WIDE = ("ring_pixels", "ground_pixels", "ring_points", "ground_sum")
TERRAIN_NARROW = ("ground_min", "ground_max", "ground", "status")
TERRAIN_MS = ("ms_ring", "ms_points", "ms_pixels", "ms_pick")


class Terrain(C.Structure):
    """bs_terrain (include/bs_api.h): totals and per-building figures, host memory owned by the library."""
    _fields_ = ([(k, C.c_int32) for k in TERRAIN_HEAD] + [(k, C.c_int64) for k in TERRAIN_TOTALS] +
                [(k, C.POINTER(C.c_int64)) for k in TERRAIN_WIDE] + [(k, C.POINTER(C.c_int32)) for k in TERRAIN_NARROW] +
                [(k, C.c_double) for k in TERRAIN_MS])


GROUND_MAX_STEPS = 16    # BS_GROUND_MAX_STEPS of include/bs_api.h
GROUND_MAX_RADIUS = 255  # BS_GROUND_MAX_RADIUS
GROUND_GRID = 2048       # BS_GROUND_GRID
GROUND_ROW_LDS = 2048    # BS_GROUND_ROW_LDS
GROUND_EMPTY = 2 ** 31 - 1
GROUND_HEAD = ("width", "height", "cell", "n_steps")
GROUND_TABLES = ("radius", "threshold")
GROUND_NARROW = ("grid", "row_lds", "dtm_min", "dtm_max", "hag_min", "hag_max")
GROUND_WIDE = ("n_ground_pixels", "n_object_pixels", "n_empty_pixels", "n_filled_pixels", "n_ground_points", "n_low_points",
               "n_object_points", "sum_hag_ground")
GROUND_MS = ("ms_low", "ms_open", "ms_points")


class GroundParams(C.Structure):
    """bs_ground_params (include/bs_api.h)"""
    _fields_ = ([("cell", C.c_int32), ("n_steps", C.c_int32), ("radius", C.c_int32 * GROUND_MAX_STEPS)] +
                [(k, C.c_int32) for k in ("s_num", "s_den", "dh0", "dh_max", "tol", "min_height")])


class Ground(C.Structure):
    """bs_ground (include/bs_api.h): the lattice, the steps and the figures; it owns no memory."""
    _fields_ = ([(k, C.c_int32) for k in GROUND_HEAD] + [(k, C.c_int32 * GROUND_MAX_STEPS) for k in GROUND_TABLES] +
                [(k, C.c_int32) for k in GROUND_NARROW] + [("n_points", C.c_int64), ("step_pixels", C.c_int64 * GROUND_MAX_STEPS)] +
                [(k, C.c_int64) for k in GROUND_WIDE] + [(k, C.c_double) for k in GROUND_MS] +
                [("ms_step", C.c_double * GROUND_MAX_STEPS)])


EVIDENCE_RMAX = 15   # BS_EVIDENCE_RMAX
EVIDENCE_TILE = 32   # BS_EVIDENCE_TILE
EVIDENCE_GRID = 256  # BS_EVIDENCE_GRID
EVIDENCE_NARROW = ("width", "height", "r", "min_points", "num", "den", "grid", "tile", "max_window", "pad_")
EVIDENCE_WIDE = ("n_points", "n_counted", "n_planar", "n_pixels", "pixels_kept", "pixels_rejected", "pixels_thin")
EVIDENCE_MS = ("ms_counts", "ms_window")


class RoofEvidence(C.Structure):
    """bs_roof_evidence (include/bs_api.h): the lattice, the parameters and the figures; it owns no memory."""
    _fields_ = ([(k, C.c_int32) for k in EVIDENCE_NARROW] + [(k, C.c_int64) for k in EVIDENCE_WIDE] +
                [(k, C.c_double) for k in EVIDENCE_MS])


HULL_MAX_SIDE = 16383   # BS_HULL_MAX_SIDE of include/bs_api.h
HULL_ROUND_BATCH = 4    # BS_HULL_ROUND_BATCH
HULL_STATUS = {0: "BS_HULL_OK", 1: "BS_HULL_EMPTY", 2: "BS_HULL_TOO_LARGE"}
HULL_TOTALS = ("n_hull_vertices", "n_ok", "n_empty", "n_too_large")
HULL_LAYOUT = ("n_candidates", "rounds", "max_live")
# (name, type, columns) of the per-label arrays of bs_label_hulls
HULL_ARRAYS = (("status", C.c_int32, 1), ("box", C.c_int32, 4), ("pixels2", C.c_int64, 1), ("n_hull", C.c_int64, 1),
               ("hull_offset", C.c_int64, 1), ("hull_area2", C.c_int64, 1), ("best_edge", C.c_int32, 1), ("dir", C.c_int32, 2),
               ("len2", C.c_int64, 1), ("a_min", C.c_int64, 1), ("a_max", C.c_int64, 1), ("c_max", C.c_int64, 1),
               ("area_num", C.c_int64, 1))
HULL_MS = ("ms_outlines", "ms_candidates", "ms_rounds", "ms_order", "ms_boxes", "ms_emit")


class LabelHulls(C.Structure):
    """bs_label_hulls (include/bs_api.h): totals, layout figures, per-label arrays and (host-memory entry point) the hull
    vertices, host memory owned by the library."""
    _fields_ = ([(k, C.c_int32) for k in ("width", "height", "n_labels", "reserved")] +
                [(k, C.c_int64) for k in HULL_TOTALS + HULL_LAYOUT] + [(k, C.POINTER(t)) for k, t, _ in HULL_ARRAYS] +
                [("hull_xy", C.POINTER(C.c_int32))] + [(k, C.c_double) for k in HULL_MS])


class BsError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        super().__init__(f"{STATUS.get(status, status)}: {detail}")


_LIB = None


def load():
    """dlopen the HIP library; raise if it is absent (no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -m buildingsegment_amd.build` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    L.bs_api_version.restype = C.c_int
    L.bs_sizeof_timings.restype = C.c_int64
    if L.bs_api_version() != API_VERSION or L.bs_sizeof_timings() != C.sizeof(Timings):
        raise ImportError(f"{LIB_PATH} is API version {L.bs_api_version()} (bs_timings: {L.bs_sizeof_timings()} bytes), this "
                          f"loader mirrors version {API_VERSION} ({C.sizeof(Timings)} bytes): rebuild the library")
    vp, ip, dp, lp = C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)
    pp = C.POINTER(Params)
    L.bs_api_version.restype = C.c_int
    L.bs_strerror.restype = C.c_char_p
    L.bs_strerror.argtypes = [C.c_int]
    L.bs_params_default.argtypes = [pp]
    L.bs_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.bs_destroy.argtypes = [vp]
    L.bs_destroy.restype = None
    L.bs_last_error.argtypes = [vp]
    L.bs_last_error.restype = C.c_char_p
    L.bs_set_stream.argtypes = [vp, vp]
    L.bs_get_timings.argtypes = [vp, C.POINTER(Timings)]
    L.bs_knn_normals.argtypes = [vp, ip, C.c_int64, pp, ip, dp]
    L.bs_knn_normals_halo.argtypes = [vp, ip, ip, C.c_int64, C.c_int64, pp, ip, dp, C.c_double, lp]
    L.bs_region_grow.argtypes = [vp, ip, dp, ip, C.c_int64, pp, ip, C.POINTER(Planes)]
    L.bs_segment.argtypes = [vp, ip, C.c_int64, pp, ip, dp, ip, C.POINTER(Planes)]
    L.bs_planes_free.argtypes = [C.POINTER(Planes)]
    L.bs_planes_free.restype = None
    L.bs_plane_colors.argtypes = [C.POINTER(Planes), ip, C.c_int64, vp]
    L.bs_knn_normals_dev.argtypes = [vp, ip, ip, C.c_int64, C.c_int64, C.c_int64, pp, ip, dp, C.c_double, lp]
    L.bs_region_grow_dev.argtypes = [vp, ip, dp, ip, C.c_int64, pp, ip]
    L.bs_segment_dev.argtypes = [vp, ip, C.c_int64, pp, ip, dp, ip]
    L.bs_planes_fetch.argtypes = [vp, C.POINTER(Planes)]
    L.bs_shift_to_origin_dev.argtypes = [vp, ip, C.c_int64, ip]
    L.bs_ingest_dev.argtypes = [vp, vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                C.c_int32, ip, ip]
    L.bs_plane_colors_dev.argtypes = [vp, ip, C.c_int32, C.c_int64, vp]
    L.bs_selftest_forge_next.argtypes = [vp, C.c_int]
    L.bs_set_audit.argtypes = [vp, C.c_int]
    L.bs_selftest_grow_limits.argtypes = [vp, C.POINTER(GrowLimits)]
    L.bs_get_grow_counters.argtypes = [vp, C.POINTER(GrowCounters)]
    L.bs_selftest_scratch_guard.argtypes = [vp, C.c_int, C.c_int]
    L.bs_selftest_scratch_check.argtypes = [vp, C.POINTER(ScratchReport)]
    L.bs_selftest_scratch_list.argtypes = [vp, C.POINTER(ScratchSlot), C.c_int64, C.POINTER(C.c_int64)]
    L.bs_selftest_center_div.argtypes = [vp, ip, vp, ip, C.c_int64]
    L.bs_grid_dims.argtypes = [ip, C.c_int32, ip, ip]
    L.bs_grid_picture.argtypes = [vp, ip, C.c_int64, ip, C.c_int32, C.c_int32, dp, dp]
    L.bs_grid_picture_dev.argtypes = [vp, ip, C.c_int64, ip, C.c_int32, C.c_int32, dp, dp]
    L.bs_cc_hook_dev.argtypes = [vp, ip, ip, C.c_int64, C.c_int32, ip, C.c_int64, lp]
    L.bs_owner_fetch_dev.argtypes = [vp, ip]
    L.bs_plane_seeds_dev.argtypes = [vp, ip, C.c_int64, C.POINTER(C.c_int32)]
    L.bs_stream_sync.argtypes = [vp]
    L.bs_labels_from_owner_dev.argtypes = [vp, ip, C.c_int64, ip, C.c_int32, ip]
    L.bs_remap_rows_dev.argtypes = [vp, ip, C.c_int64, C.c_int32, ip, C.c_int64, ip, C.POINTER(C.c_int32)]
    L.bs_comm_rccl.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(CommOps)]
    L.bs_comm_rccl_unique_id.argtypes = [C.c_char_p]
    L.bs_comm_rccl_init.argtypes = [vp, C.c_char_p, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.bs_comm_rccl_destroy.argtypes = [vp]
    L.bs_comm_local_create.argtypes = [C.c_int32, C.POINTER(CommOps)]
    L.bs_comm_local_destroy.argtypes = [C.POINTER(CommOps)]
    L.bs_comm_local_destroy.restype = None
    L.bs_segment_sharded.argtypes = [vp, C.POINTER(CommOps), ip, ip, C.c_int64, C.c_int64, pp, C.c_double, ip,
                                     C.POINTER(ShardInfo)]
    L.bs_sharded_planes_fetch.argtypes = [vp, C.POINTER(Planes)]
    cp = C.POINTER(Contours)
    L.bs_footprints_dev.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, cp,
                                    C.POINTER(FootprintInfo)]
    L.bs_footprints.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, cp,
                                C.POINTER(FootprintInfo)]
    L.bs_contours_free.argtypes = [cp]
    L.bs_contours_free.restype = None
    L.bs_contours_write_obj.argtypes = [cp, C.c_char_p]
    L.bs_segment_batch.argtypes = [vp, ip, vp, C.c_int32, pp, ip, dp, ip, C.POINTER(Planes), ip]
    L.bs_segment_batch_dev.argtypes = [vp, ip, vp, C.c_int32, pp, ip, dp, ip]
    L.bs_batch_planes_fetch.argtypes = [vp, C.POINTER(Planes), ip]
    L.bs_shift_tiles_to_origin_dev.argtypes = [vp, ip, vp, C.c_int32, ip]
    L.bs_tile_boxes_dev.argtypes = [vp, ip, vp, C.c_int32, ip]
    L.bs_grid_dims_batch.argtypes = [ip, C.c_int32, C.c_int32, ip, ip, vp]
    L.bs_grid_picture_batch_dev.argtypes = [vp, ip, vp, C.c_int32, ip, C.c_int32, C.c_int32, dp, dp]
    L.bs_grid_picture_batch.argtypes = [vp, ip, vp, C.c_int32, ip, C.c_int32, C.c_int32, dp, dp]
    L.bs_footprints_batch_dev.argtypes = [vp, vp, ip, ip, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, cp, ip,
                                          C.POINTER(FootprintInfo)]
    L.bs_footprints_batch.argtypes = [vp, vp, ip, ip, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, cp, ip,
                                      C.POINTER(FootprintInfo)]
    bp = C.POINTER(Buildings)
    L.bs_building_map_dev.argtypes = [vp, vp, C.c_int32, C.c_int32, ip, bp]
    L.bs_building_map.argtypes = [vp, vp, C.c_int32, C.c_int32, ip, bp]
    L.bs_buildings_free.argtypes = [bp]
    L.bs_buildings_free.restype = None
    L.bs_assign_buildings_dev.argtypes = [vp, ip, C.c_int64, C.c_int32, C.c_double, ip, C.c_int32, C.c_int32, ip, bp]
    L.bs_assign_buildings.argtypes = [vp, ip, C.c_int64, C.c_int32, C.c_double, ip, C.c_int32, C.c_int32, ip, bp]
    L.bs_plane_buildings_dev.argtypes = [vp, ip, ip, C.c_int64, C.c_int32, C.c_int32, ip, vp, vp, vp]
    L.bs_plane_buildings.argtypes = [vp, ip, ip, C.c_int64, C.c_int32, C.c_int32, ip, vp, vp, vp]
    L.bs_buildings_write_obj.argtypes = [cp, bp, C.c_int32, ip, C.c_double, C.c_double, C.c_double, C.c_char_p]
    rp = C.POINTER(Roofs)
    L.bs_roof_homes.argtypes = [dp, ip, vp, vp, C.c_int32, C.c_double, ip]
    roofs_args = [vp, ip, C.c_int64, C.c_int32, C.c_double, ip, C.c_int32, C.c_int32, ip, C.c_int32, ip, dp, ip, C.c_int32,
                  ip, ip, ip, rp]
    L.bs_roofs_dev.argtypes = roofs_args
    L.bs_roofs.argtypes = roofs_args
    L.bs_roofs_free.argtypes = [rp]
    L.bs_roofs_free.restype = None
    L.bs_roofs_write_obj.argtypes = [ip, ip, C.c_int32, C.c_int32, rp, dp, ip, C.c_int32, ip, C.c_char_p]
    fitp = C.POINTER(PlaneFits)
    L.bs_plane_fit_dev.argtypes = [vp, ip, C.c_int64, ip, C.c_int32, ip, fitp]
    L.bs_plane_fit.argtypes = [vp, ip, C.c_int64, ip, C.c_int32, ip, fitp]
    L.bs_plane_fits_free.argtypes = [fitp]
    L.bs_plane_fits_free.restype = None
    L.bs_plane_fit_apply.argtypes = [fitp, dp, ip]
    sp = C.POINTER(Solids)
    solids_args = [vp, ip, ip, C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp, ip, ip, ip, C.c_int32, C.c_int32, ip, ip, sp]
    L.bs_solids_count_dev.argtypes = solids_args
    L.bs_solids.argtypes = solids_args
    L.bs_solids_emit_dev.argtypes = [vp, ip, ip, ip, ip, vp]
    L.bs_solids_free.argtypes = [sp]
    L.bs_solids_free.restype = None
    L.bs_solids_write_obj.argtypes = [ip, C.c_int64, ip, ip, ip, C.c_int64, C.c_int32, ip, C.c_char_p]
    fcp = C.POINTER(RoofFacets)
    facets_args = [vp, ip, ip, ip, C.c_int32, C.c_int32, C.c_int32, C.c_int32, ip, fcp]
    L.bs_roof_facets_dev.argtypes = facets_args
    L.bs_roof_facets.argtypes = facets_args
    L.bs_roof_facets_free.argtypes = [fcp]
    L.bs_roof_facets_free.restype = None
    L.bs_roof_edge_kinds.argtypes = [fcp, C.c_int32, C.c_int32, vp]
    L.bs_roof_edges_write_obj.argtypes = [ip, ip, ip, C.c_int32, C.c_int32, C.c_int32, fcp, vp, ip, C.c_char_p]
    gnp = C.POINTER(RoofGeneralise)
    gen_args = [vp, ip, ip, C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp, ip, ip, ip, C.c_int32, C.c_int32, ip,
                C.POINTER(RoofGeneraliseParams), ip, gnp]
    L.bs_roof_generalise_dev.argtypes = gen_args
    L.bs_roof_generalise.argtypes = gen_args
    L.bs_roof_generalise_free.argtypes = [gnp]
    L.bs_roof_generalise_free.restype = None
    olp = C.POINTER(Outlines)
    L.bs_facet_outlines_count_dev.argtypes = [vp, ip, ip, C.c_int32, C.c_int32, C.c_int32, olp]
    L.bs_facet_outlines.argtypes = [vp, ip, ip, C.c_int32, C.c_int32, C.c_int32, olp]
    L.bs_facet_outlines_emit_dev.argtypes = [vp, ip, ip]
    L.bs_outlines_free.argtypes = [olp]
    L.bs_outlines_free.restype = None
    L.bs_outlines_write_obj.argtypes = [olp, C.c_int32, ip, C.c_char_p]
    sop = C.POINTER(SimpleOutlines)
    simple_args = [vp, ip, ip, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, sop, olp]
    L.bs_simple_outlines_count_dev.argtypes = simple_args
    L.bs_simple_outlines.argtypes = simple_args
    L.bs_simple_outlines_emit_dev.argtypes = [vp, ip, ip, ip, vp]
    L.bs_simple_outlines_free.argtypes = [sop]
    L.bs_simple_outlines_free.restype = None
    L.bs_simple_outlines_write_obj.argtypes = [sop, C.c_int32, ip, C.c_char_p]
    cop = C.POINTER(CleanOutlines)
    clean_args = [vp, ip, ip, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, cop, sop, olp]
    L.bs_clean_outlines_count_dev.argtypes = clean_args
    L.bs_clean_outlines.argtypes = clean_args
    L.bs_clean_outlines_emit_dev.argtypes = [vp, ip, ip, ip, vp]
    L.bs_clean_outlines_free.argtypes = [cop]
    L.bs_clean_outlines_free.restype = None
    L.bs_clean_outlines_write_obj.argtypes = [cop, C.c_int32, ip, C.c_char_p]
    L.bs_set_outline_sweeps.argtypes = [vp, C.c_int32]
    L.bs_get_outline_sweeps.argtypes = [vp, C.POINTER(OutlineSweeps)]
    otp = C.POINTER(OutlineTriangles)
    tri_args = [vp, ip, ip, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, otp, cop, sop, olp]
    L.bs_outline_triangles_count_dev.argtypes = tri_args
    L.bs_outline_triangles.argtypes = tri_args
    L.bs_outline_triangles_emit_dev.argtypes = [vp, ip]
    L.bs_outline_triangles_free.argtypes = [otp]
    L.bs_outline_triangles_free.restype = None
    L.bs_outline_triangles_write_obj.argtypes = [otp, cop, C.c_int32, ip, C.c_char_p]
    psp = C.POINTER(PolySolids)
    poly_args = [vp, ip, ip, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, ip, C.c_int32, C.c_int32, C.c_int32,
                 psp, otp, cop, sop, olp]
    L.bs_poly_solids_count_dev.argtypes = poly_args
    L.bs_poly_solids.argtypes = poly_args
    L.bs_poly_solids_emit_dev.argtypes = [vp, ip, ip, ip, ip, vp]
    L.bs_poly_solids_free.argtypes = [psp]
    L.bs_poly_solids_free.restype = None
    mrp = C.POINTER(ModelRaster)
    L.bs_model_raster_dev.argtypes = [vp, ip, ip, C.c_int32, C.c_int32, ip, ip, ip, mrp]
    L.bs_model_raster.argtypes = [vp, ip, ip, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, ip, ip, ip, mrp,
                                  otp, cop, sop, olp]
    L.bs_model_raster_free.argtypes = [mrp]
    L.bs_model_raster_free.restype = None
    prp = C.POINTER(PointResiduals)
    L.bs_point_residuals_dev.argtypes = [vp, ip, C.c_int64, C.c_int32, ip, ip, C.c_int32, ip, ip, ip, prp]
    L.bs_point_residuals.argtypes = [vp, ip, ip, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, ip, C.c_int64,
                                     C.c_int32, ip, ip, C.c_int32, ip, ip, ip, prp, otp, cop, sop, olp]
    L.bs_point_residuals_free.argtypes = [prp]
    L.bs_point_residuals_free.restype = None
    tnp = C.POINTER(Terrain)
    for fn in (L.bs_terrain_dev, L.bs_terrain):
        fn.argtypes = [vp, ip, C.c_int64, C.c_int32, ip, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                       C.c_int32, ip, vp, ip, tnp]
    L.bs_terrain_free.argtypes = [tnp]
    L.bs_terrain_free.restype = None
    L.bs_set_building_bases.argtypes = [vp, ip, C.c_int32]
    L.bs_get_building_bases.argtypes = [vp, ip, C.c_int32, C.POINTER(C.c_int32)]
    gdp, i32p = C.POINTER(Ground), C.POINTER(C.c_int32)
    for fn in (L.bs_ground_dev, L.bs_ground):
        fn.argtypes = [vp, ip, C.c_int64, ip, C.POINTER(GroundParams), ip, ip, vp, ip, vp, gdp]
    L.bs_ground_free.argtypes = [gdp]
    L.bs_ground_free.restype = None
    for fn in (L.bs_set_ground_model, L.bs_set_ground_model_dev):
        fn.argtypes = [vp, ip, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.bs_get_ground_model.argtypes = [vp, ip, C.c_int64, i32p, i32p, i32p, i32p]
    L.bs_plane_quality.argtypes = [fitp, C.c_int64, C.c_int32, vp]
    for fn in (L.bs_roof_evidence_dev, L.bs_roof_evidence):
        fn.argtypes = [vp, ip, C.c_int64, ip, C.c_int32, vp, ip, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                       vp, ip, ip, ip, ip, C.POINTER(RoofEvidence)]
    for fn in (L.bs_set_footprint_screen, L.bs_set_footprint_screen_dev):
        fn.argtypes = [vp, vp, C.c_int32, C.c_int32]
    L.bs_get_footprint_screen.argtypes = [vp, vp, C.c_int64, i32p, i32p]
    hlp = C.POINTER(LabelHulls)
    L.bs_label_hulls_count_dev.argtypes = [vp, ip, C.c_int32, C.c_int32, C.c_int32, hlp]
    L.bs_label_hulls.argtypes = [vp, ip, C.c_int32, C.c_int32, C.c_int32, hlp]
    L.bs_label_hulls_emit_dev.argtypes = [vp, ip]
    L.bs_label_hulls_free.argtypes = [hlp]
    L.bs_label_hulls_free.restype = None
    L.bs_hull_box_corners.argtypes = [hlp, C.c_int32, C.c_int32, ip, vp]
    L.bs_hull_boxes_write_obj.argtypes = [hlp, C.c_int32, ip, C.c_char_p]
    _LIB = L
    return L
