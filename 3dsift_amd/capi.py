"""ctypes binding of the C-ABI in include/sift3d_hip.h (lib: 3dsift_amd/libsift3d_hip.so).

This is plumbing for tests/ and bench.py: the product is the HIP library itself and the C++ shell
in 3dsift_amd/host/ (namespace CPUSIFT).  There is NO CPU fallback anywhere in this module: if the
library is missing or no GPU is visible, calls raise.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("S3D_LIB") or os.path.join(HERE, "libsift3d_hip.so")  # S3D_LIB: kernel-variant A/B builds (scripts/ab_pyramid.py)
DESC = 768

KP_DTYPE = np.dtype(
    [
        ("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
        ("scale", "<f4"),
        ("octave", "<i4"), ("level", "<i4"),
        ("rx", "<f4"), ("ry", "<f4"), ("rz", "<f4"),
        ("win", "<f4", (3,)),
        ("eigvalue", "<f4", (3,)),
        ("eigvector", "<f4", (9,)),
        ("Rotation", "<f4", (9,)),
        ("str_tensor", "<f4", (9,)),
    ]
)
assert KP_DTYPE.itemsize == 168

# every symbol include/sift3d_hip.h and include/sift3d_hip_test.h declare (tests check that the library exports all of them)
SYMBOLS = [
    "sift3d_default_params", "sift3d_create", "sift3d_destroy", "sift3d_run", "sift3d_run_async", "sift3d_run_async_after", "sift3d_wait", "sift3d_run_stages",
    "sift3d_stage_times", "sift3d_num_keypoints", "sift3d_get_keypoints", "sift3d_device_results",
    "sift3d_num_octaves", "sift3d_level_info", "sift3d_copy_level", "sift3d_copy_input", "sift3d_num_extrema",
    "sift3d_get_extrema", "sift3d_get_orientation_codes", "sift3d_gaussian_smooth", "sift3d_downsample", "sift3d_dog_sub", "sift3d_conv_axis",
    "sift3d_orient_keypoint", "sift3d_describe_keypoint", "sift3d_match",
    "sift3d_match_handles",
    # detection options: the 80-neighbour rule and the sub-voxel refinement
    "sift3d_default_detect_options", "sift3d_set_detect_options", "sift3d_get_detect_options", "sift3d_get_refined",
    # RANSAC affine fits of matched pairs, global and per point
    "sift3d_default_ransac_options", "sift3d_fit_affine", "sift3d_fit_affine_local",
    # RANSAC rigid / similarity fits of the same pairs, and the rotation a fit holds
    "sift3d_fit_rigid", "sift3d_fit_rigid_local", "sift3d_fit_rotation",
    # one rigid / similarity fit per body of a labelled specimen, and IC-GN with every POI limited to its own body
    "sift3d_fit_rigid_bodies", "sift3d_labels_at_positions", "sift3d_icgn_init_from_body_fits", "sift3d_icgn_labelled",
    # guided matching: best and second best within a spatial gate around the position a fit predicts
    "sift3d_predict_positions", "sift3d_match_guided",
    # IC-GN displacement refinement (digital volume correlation)
    "sift3d_default_icgn_options", "sift3d_icgn_init_from_fits", "sift3d_icgn",
    # cubic B-spline interpolation of the target: the prefilter and the IC-GN mode on its coefficients
    "sift3d_bspline_prefilter", "sift3d_icgn_bspline",
    # second-order (30-parameter) IC-GN
    "sift3d_icgn2_init_from_icgn", "sift3d_icgn2", "sift3d_strain_input_from_icgn2",
    # ZNCC integer search: the initial guess of IC-GN where no local fit exists
    "sift3d_default_search_options", "sift3d_zncc_search", "sift3d_icgn_init_from_search",
    # strain fields from the refined displacements
    "sift3d_default_strain_options", "sift3d_strain_input_from_icgn", "sift3d_strain",
    # outlier validation of the displacement field (normalised median test)
    "sift3d_default_validate_options", "sift3d_validate_input_from_icgn", "sift3d_validate_input_from_icgn2", "sift3d_validate_displacements",
    "sift3d_validate_keep", "sift3d_icgn_init_from_validation", "sift3d_validate_stage_capacity",
    # the displacement field at real-valued positions (moving least squares) and the chaining of load steps
    "sift3d_default_field_options", "sift3d_field_eval", "sift3d_field_queries_from_displacements", "sift3d_field_unpack",
    "sift3d_compose_displacements", "sift3d_icgn_init_from_field",
    # subset screening: texture sums and a per-POI subset radius, the step in front of IC-GN
    "sift3d_default_subset_options", "sift3d_subset_quality", "sift3d_subset_group_by_radius",
    # masked IC-GN: subsets limited to a voxel mask of the reference, and the mask of a grey level
    "sift3d_icgn_masked", "sift3d_mask_from_level",
    # several bodies: connected-component labels of a mask, and the three window calls limited to a POI's own body
    "sift3d_mask_label", "sift3d_labels_at_points", "sift3d_test_label_tile", "sift3d_strain_labelled",
    "sift3d_validate_displacements_labelled", "sift3d_field_eval_labelled",
    # bodies that touch: the distance transform of a mask, exact erosion, and labels grown from the transform's cores
    "sift3d_mask_distance", "sift3d_mask_from_distance", "sift3d_distance_at_points", "sift3d_default_split_options", "sift3d_mask_split",
    "sift3d_device_count", "sift3d_error_string", "sift3d_last_error",
    # typed input: 8 / 16-bit integer voxels uploaded at their own width and widened on the GPU
    "sift3d_dtype_bytes", "sift3d_create_typed", "sift3d_volume_to_device", "sift3d_test_ingest_launch",
    # multi-GPU sharding (z-slabs of octave 0 + seeded replicated tail)
    "sift3d_slab_min_halo", "sift3d_slab_arena_floats", "sift3d_slab_create", "sift3d_slab_buffer", "sift3d_slab_upload",
    "sift3d_slab_input_absmax", "sift3d_slab_input_scale", "sift3d_slab_level", "sift3d_slab_level_hw", "sift3d_slab_halo_planes",
    "sift3d_slab_sync", "sift3d_slab_get_dogmax", "sift3d_slab_set_dogmax", "sift3d_slab_detect", "sift3d_slab_describe",
    "sift3d_slab_decimate", "sift3d_slab_admits", "sift3d_slab_set_ghost", "sift3d_slab_min_halo_ghost", "sift3d_create_seeded", "sift3d_seed_upload", "sift3d_set_describe_partition",
    "sift3d_export_device", "sift3d_import_descriptors_device", "sift3d_run_partial_orientation",
    "sift3d_export_orientation_device", "sift3d_import_orientation_device", "sift3d_run_describe",
    "sift3d_set_stream", "sift3d_slab_export_dogmax_device", "sift3d_slab_import_dogmax_device", "sift3d_slab_decimate_async",
    # r05: descriptor windows split along z over the ranks (partial integer histograms)
    "sift3d_slab_set_desc_partial", "sift3d_slab_min_halo_partial", "sift3d_slab_record_bytes", "sift3d_slab_desc_reach", "sift3d_slab_orient",
    "sift3d_slab_export_records", "sift3d_slab_describe_partial", "sift3d_slab_describe_finish", "sift3d_slab_orient_launch",
    "sift3d_slab_orient_count",
    # r06: the same stages without host read-backs, the tail's seed level in place, the native driver's plan
    "sift3d_slab_keypoints_launch", "sift3d_slab_keypoints_count", "sift3d_slab_describe_finish_launch", "sift3d_slab_describe_finish_count",
    "sift3d_seed_buffer", "sift3d_sharded_plan", "sift3d_slab_describe_launch", "sift3d_sharded_traffic",
    # test hooks / debug accessors / matcher timing
    # native driver of the z-slab sharding
    "sift3d_sharded_create", "sift3d_sharded_create_ex", "sift3d_sharded_run", "sift3d_sharded_num_keypoints", "sift3d_sharded_get_keypoints", "sift3d_sharded_info",
    "sift3d_sharded_error", "sift3d_sharded_destroy",
    "sift3d_test_hook", "sift3d_debug_counters", "sift3d_test_run_plan", "sift3d_debug_face_lookup", "sift3d_match_times", "sift3d_debug_copy_bandwidth",
    "sift3d_match_warmup", "sift3d_test_staging_slice", "sift3d_test_slab_plan", "sift3d_test_sharded_time_rank",
]
HOOKS = {"dog_eager": 0, "glast_eager": 1, "det_serial": 2, "separable": 3, "desc_nocache": 4, "match_nodma": 5, "one_stream": 6,
         "desc_mass_shift": 7, "list_cap": 8, "peer_copy": 9, "desc_nosplit": 10, "march_tiles": 11, "desc_exact_cells": 12, "lazy_generic": 13, "sharded_fail_rank": 14,
         "ori_grid": 15}
ORIENT_WORDS = 34
# SIFT3D_DT_ codes of include/sift3d_hip.h by numpy dtype name
DTYPES = {"float32": 0, "uint8": 1, "int8": 2, "uint16": 3, "int16": 4}
SHARDED_PARTIAL_WINDOWS = 1   # sift3d_sharded_create_ex flags
SHARDED_WHOLE_WINDOWS = 2
SHARDED_COPY_TRANSPORT = 4
SHARDED_GHOST_OCTAVE0 = 8


class Params(C.Structure):
    _fields_ = [("num_kp_levels", C.c_int), ("sigma_default", C.c_float), ("sigma_n_default", C.c_float),
                ("peak_thresh", C.c_float), ("max_eig_thres", C.c_float), ("corner_thresh", C.c_float)]


class DetectOptions(C.Structure):
    """sift3d_detect_options (include/sift3d_hip.h)"""
    _fields_ = [("neighbours", C.c_int), ("refine", C.c_int), ("max_offset", C.c_float), ("contrast_thresh", C.c_float),
                ("edge_ratio", C.c_float), ("reserved", C.c_int * 3)]


assert C.sizeof(DetectOptions) == 32

# sift3d_refined: refined coordinates / scale, the fit's offset (dx, dy, dz, ds) and D(x^)
REFINED_DTYPE = np.dtype([("rx", "<f4"), ("ry", "<f4"), ("rz", "<f4"), ("scale", "<f4"), ("offset", "<f4", (4,)), ("contrast", "<f4")])
assert REFINED_DTYPE.itemsize == 36


class RansacOptions(C.Structure):
    """sift3d_ransac_options (include/sift3d_hip.h)"""
    _fields_ = [("iterations", C.c_int), ("inlier_thresh", C.c_float), ("seed", C.c_uint), ("refine", C.c_int), ("min_det", C.c_float),
                ("reserved", C.c_int * 3)]


assert C.sizeof(RansacOptions) == 32

# sift3d_affine_fit: final transform, the best hypothesis's minimal-sample transform, status and counts
FIT_DTYPE = np.dtype([("A", "<f8", (12,)), ("hyp", "<f8", (12,)), ("status", "<i4"), ("candidates", "<i4"), ("best_hypothesis", "<i4"),
                      ("best_count", "<i4"), ("inliers", "<i4"), ("rms", "<f4"), ("reserved", "<i4", (2,))])
assert FIT_DTYPE.itemsize == 224


class IcgnOptions(C.Structure):
    """sift3d_icgn_options (include/sift3d_hip.h)"""
    _fields_ = [("subset_radius", C.c_int), ("max_iterations", C.c_int), ("tolerance", C.c_float), ("interpolation", C.c_int),
                ("reserved", C.c_int * 4)]


assert C.sizeof(IcgnOptions) == 32

# sift3d_icgn_result: p = (u, ux, uy, uz, v, vx, vy, vz, w, wx, wy, wz), zncc, last step, iterations, status
ICGN_DTYPE = np.dtype([("p", "<f8", (12,)), ("zncc", "<f8"), ("last_step", "<f8"), ("iterations", "<i4"), ("status", "<i4"),
                       ("reserved", "<i4", (2,))])
assert ICGN_DTYPE.itemsize == 128
# sift3d_icgn2_result: p = (c, cx, cy, cz, cxx, cyy, czz, cxy, cxz, cyz) of u, then v, then w
ICGN2_DTYPE = np.dtype([("p", "<f8", (30,)), ("zncc", "<f8"), ("last_step", "<f8"), ("iterations", "<i4"), ("status", "<i4"),
                        ("reserved", "<i4", (2,))])
assert ICGN2_DTYPE.itemsize == 272


class SearchOptions(C.Structure):
    """sift3d_search_options (include/sift3d_hip.h)"""
    _fields_ = [("subset_radius", C.c_int), ("search_radius", C.c_int), ("reserved", C.c_int * 6)]


assert C.sizeof(SearchOptions) == 32

# sift3d_search_result: d = (du, dv, dw), status, zncc at d, the best score away from d, candidates scored
SEARCH_DTYPE = np.dtype([("d", "<i4", (3,)), ("status", "<i4"), ("zncc", "<f8"), ("zncc_second", "<f8"), ("candidates", "<i4"),
                         ("reserved", "<i4", (3,))])
assert SEARCH_DTYPE.itemsize == 48


class StrainOptions(C.Structure):
    """sift3d_strain_options (include/sift3d_hip.h)"""
    _fields_ = [("radius", C.c_int), ("min_neighbours", C.c_int), ("measure", C.c_int), ("reserved", C.c_int * 5)]


assert C.sizeof(StrainOptions) == 32

# sift3d_strain_result: the fitted displacement, gradient (rows u v w, columns x y z), E (xx yy zz xy yz zx), its eigenvalues
# (descending), the equivalent strain, the fit's residual, the neighbour count and the status
STRAIN_DTYPE = np.dtype([("disp", "<f8", (3,)), ("G", "<f8", (9,)), ("E", "<f8", (6,)), ("principal", "<f8", (3,)), ("equivalent", "<f8"),
                         ("rms", "<f8"), ("neighbours", "<i4"), ("status", "<i4")])
assert STRAIN_DTYPE.itemsize == 192


class ValidateOptions(C.Structure):
    """sift3d_validate_options (include/sift3d_hip.h)"""
    _fields_ = [("radius", C.c_int), ("min_neighbours", C.c_int), ("passes", C.c_int), ("reserved0", C.c_int), ("threshold", C.c_double),
                ("eps", C.c_double), ("reserved", C.c_int * 4)]


assert C.sizeof(ValidateOptions) == 48

# sift3d_validate_result: the median and the MAD of the neighbours' estimates, the score against the final set, the neighbour count,
# the status, the flag and the pass that set it
VALIDATE_DTYPE = np.dtype([("median", "<f8", (3,)), ("mad", "<f8", (3,)), ("score", "<f8"), ("neighbours", "<i4"), ("status", "<i4"),
                           ("flagged", "<i4"), ("pass", "<i4")])
assert VALIDATE_DTYPE.itemsize == 72


class FieldOptions(C.Structure):
    """sift3d_field_options (include/sift3d_hip.h)"""
    _fields_ = [("radius", C.c_int), ("min_neighbours", C.c_int), ("weighting", C.c_int), ("require_enclosed", C.c_int),
                ("reserved", C.c_int * 4)]


assert C.sizeof(FieldOptions) == 32

# sift3d_field_result: the field at the query, its gradient (rows u v w, columns x y z), the weighted residual, the sum of the weights,
# the counted members, the sides they lie on and the status
FIELD_DTYPE = np.dtype([("disp", "<f8", (3,)), ("G", "<f8", (9,)), ("rms", "<f8"), ("wsum", "<f8"), ("neighbours", "<i4"), ("sides", "<i4"),
                        ("status", "<i4"), ("reserved", "<i4")])
assert FIELD_DTYPE.itemsize == 128


class SubsetOptions(C.Structure):
    """sift3d_subset_options (include/sift3d_hip.h)"""
    _fields_ = [("r_min", C.c_int), ("r_max", C.c_int), ("criterion", C.c_int), ("reserved0", C.c_int), ("threshold", C.c_double),
                ("level", C.c_double), ("fraction_min", C.c_double), ("reserved", C.c_int * 2)]


assert C.sizeof(SubsetOptions) == 48

# sift3d_subset_result: mean and dR of the reported cube, G (xx yy zz xy xz yz), its eigenvalues (descending), the reported radius,
# the status, the largest feasible radius and the material count
SUBSET_DTYPE = np.dtype([("mean", "<f8"), ("dR", "<f8"), ("G", "<f8", (6,)), ("eig", "<f8", (3,)), ("radius", "<i4"), ("status", "<i4"),
                         ("feasible", "<i4"), ("material", "<i4")])
assert SUBSET_DTYPE.itemsize == 104


class SplitOptions(C.Structure):
    """sift3d_split_options (include/sift3d_hip.h)"""
    _fields_ = [("connectivity", C.c_int), ("core_dist2", C.c_int), ("min_core_voxels", C.c_int), ("border", C.c_int), ("max_rounds", C.c_int),
                ("keep_unreached", C.c_int), ("min_voxels", C.c_int)]


class SplitInfo(C.Structure):
    """sift3d_split_info (include/sift3d_hip.h)"""
    _fields_ = [("cores", C.c_int), ("unreached_bodies", C.c_int), ("rounds", C.c_int), ("unlabelled", C.c_int)]


assert C.sizeof(SplitOptions) == 28 and C.sizeof(SplitInfo) == 16
DIST2_NONE = 2 ** 31 - 1  # SIFT3D_DIST2_NONE


class SlabDesc(C.Structure):
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("z0", C.c_int), ("z1", C.c_int), ("halo", C.c_int),
                ("noct_total", C.c_int), ("octave", C.c_int)]


class Sift3dError(RuntimeError):
    pass


_lib = None
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int)


def lib():
    """Load the HIP library; fails loudly when it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Sift3dError(f"{LIB_PATH} is missing: build it with `make -C 3dsift_amd/csrc` "
                              f"(or __graft_entry__.build()); there is no CPU fallback")
        # PyTorch-ROCm wheels bundle their own libamdhip64.so.7; a process must not end up with two HIP runtimes (the
        # second one finds no GPU).  Loading torch's first makes this library bind to the same runtime by soname, so
        # torch-allocated device memory (halo arenas, synthetic volumes) and this library share one HIP context.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.sift3d_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.c_int, C.c_int]
        L.sift3d_create_typed.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.c_int, C.c_int]
        L.sift3d_dtype_bytes.argtypes = [C.c_int, _ip]
        L.sift3d_volume_to_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_test_ingest_launch.argtypes = [C.c_int, _ip, _ip, _ip, _ip]
        L.sift3d_destroy.argtypes = [C.c_void_p]
        L.sift3d_run.argtypes = [C.c_void_p]
        L.sift3d_run_async.argtypes = [C.c_void_p]
        L.sift3d_wait.argtypes = [C.c_void_p]
        L.sift3d_run_stages.argtypes = [C.c_void_p, C.c_int]
        L.sift3d_stage_times.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_num_keypoints.argtypes = [C.c_void_p, _ip]
        L.sift3d_get_keypoints.argtypes = [C.c_void_p, C.c_void_p, _fp]
        L.sift3d_device_results.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _ip]
        L.sift3d_num_octaves.argtypes = [C.c_void_p, _ip]
        L.sift3d_level_info.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, _fp, _fp]
        L.sift3d_copy_level.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp]
        L.sift3d_copy_input.argtypes = [C.c_void_p, _fp]
        L.sift3d_num_extrema.argtypes = [C.c_void_p, _ip]
        L.sift3d_get_extrema.argtypes = [C.c_void_p, C.c_void_p]
        L.sift3d_get_orientation_codes.argtypes = [C.c_void_p, _ip]
        L.sift3d_gaussian_smooth.argtypes = [_fp, C.c_int, C.c_int, C.c_int, C.c_float, _fp, C.c_int]
        L.sift3d_downsample.argtypes = [_fp, C.c_int, C.c_int, C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int]
        L.sift3d_dog_sub.argtypes = [_fp, _fp, C.c_size_t, _fp, C.c_int]
        L.sift3d_conv_axis.argtypes = [_fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, C.c_int, _fp, C.c_int]
        L.sift3d_orient_keypoint.argtypes = [_fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int, _ip]
        L.sift3d_describe_keypoint.argtypes = [_fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, _fp, C.c_int]
        L.sift3d_match.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int,
                                   C.c_int, C.c_int, _ip, _ip, _fp, _fp, _fp, _ip, C.POINTER(C.c_double)]
        L.sift3d_match_handles.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, _ip, _ip, _fp, _fp, _fp, _ip, C.POINTER(C.c_double)]
        L.sift3d_device_count.argtypes = [_ip]
        L.sift3d_default_detect_options.argtypes = [C.POINTER(DetectOptions)]
        L.sift3d_default_detect_options.restype = None
        L.sift3d_set_detect_options.argtypes = [C.c_void_p, C.POINTER(DetectOptions)]
        L.sift3d_get_detect_options.argtypes = [C.c_void_p, C.POINTER(DetectOptions)]
        L.sift3d_get_refined.argtypes = [C.c_void_p, C.c_void_p]
        L.sift3d_default_ransac_options.argtypes = [C.POINTER(RansacOptions)]
        L.sift3d_default_ransac_options.restype = None
        L.sift3d_fit_affine.argtypes = [C.c_void_p, C.c_int, C.POINTER(RansacOptions), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_double)]
        L.sift3d_fit_affine_local.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.POINTER(RansacOptions), C.c_int,
                                              C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_fit_rigid.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(RansacOptions), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.POINTER(C.c_double)]
        L.sift3d_fit_rigid_local.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.POINTER(RansacOptions),
                                             C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_fit_rotation.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sift3d_fit_rigid_bodies.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(RansacOptions), C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_labels_at_positions.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                 C.c_int]
        L.sift3d_icgn_init_from_body_fits.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.sift3d_icgn_labelled.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_int, C.c_void_p, C.POINTER(IcgnOptions), C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_predict_positions.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.sift3d_match_guided.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_double,
                                          C.c_int, C.c_int, C.c_int, _ip, _ip, _fp, _fp, _ip, _fp, _ip, C.POINTER(C.c_double)]
        L.sift3d_default_icgn_options.argtypes = [C.POINTER(IcgnOptions)]
        L.sift3d_default_icgn_options.restype = None
        L.sift3d_icgn_init_from_fits.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.sift3d_icgn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                  C.POINTER(IcgnOptions), C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_bspline_prefilter.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.sift3d_icgn_bspline.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                          C.c_void_p, C.POINTER(IcgnOptions), C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_default_search_options.argtypes = [C.POINTER(SearchOptions)]
        L.sift3d_default_search_options.restype = None
        L.sift3d_zncc_search.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                         C.c_void_p, C.POINTER(SearchOptions), C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_icgn2_init_from_icgn.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.sift3d_icgn2.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                   C.POINTER(IcgnOptions), C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_strain_input_from_icgn2.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
        L.sift3d_icgn_init_from_search.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.sift3d_default_strain_options.argtypes = [C.POINTER(StrainOptions)]
        L.sift3d_default_strain_options.restype = None
        L.sift3d_strain_input_from_icgn.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
        L.sift3d_strain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(StrainOptions), C.c_int, C.c_int, C.c_void_p,
                                    C.POINTER(C.c_double)]
        L.sift3d_default_validate_options.argtypes = [C.POINTER(ValidateOptions)]
        L.sift3d_default_validate_options.restype = None
        L.sift3d_validate_input_from_icgn.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sift3d_validate_input_from_icgn2.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sift3d_validate_displacements.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(ValidateOptions), C.c_int,
                                                    C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_validate_keep.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.sift3d_default_subset_options.argtypes = [C.POINTER(SubsetOptions)]
        L.sift3d_default_subset_options.restype = None
        L.sift3d_subset_quality.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(SubsetOptions), C.c_int,
                                            C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_subset_group_by_radius.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.sift3d_icgn_init_from_validation.argtypes = [C.c_void_p, C.c_int, C.c_void_p, _ip]
        L.sift3d_icgn_masked.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_void_p, C.POINTER(IcgnOptions), C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_mask_from_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_int,
                                             C.POINTER(C.c_double)]
        L.sift3d_mask_label.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, _ip, C.c_int, C.c_int,
                                        C.POINTER(C.c_double)]
        L.sift3d_labels_at_points.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.sift3d_test_label_tile.argtypes = [_ip]
        L.sift3d_default_split_options.argtypes = [C.POINTER(SplitOptions)]
        L.sift3d_default_split_options.restype = None
        L.sift3d_mask_distance.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.sift3d_mask_from_distance.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                C.POINTER(C.c_double)]
        L.sift3d_distance_at_points.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.sift3d_mask_split.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(SplitOptions), C.c_void_p, _ip, C.c_void_p,
                                        C.POINTER(SplitInfo), C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.sift3d_strain_labelled.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(StrainOptions), C.c_int, C.c_int,
                                             C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_validate_displacements_labelled.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                             C.POINTER(ValidateOptions), C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_field_eval_labelled.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.POINTER(FieldOptions), C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_validate_stage_capacity.argtypes = [_ip]
        L.sift3d_default_field_options.argtypes = [C.POINTER(FieldOptions)]
        L.sift3d_default_field_options.restype = None
        L.sift3d_field_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(FieldOptions), C.c_int,
                                        C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        L.sift3d_field_queries_from_displacements.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.sift3d_field_unpack.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sift3d_compose_displacements.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sift3d_icgn_init_from_field.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, _ip]
        _sz = C.POINTER(C.c_size_t)
        L.sift3d_slab_min_halo.argtypes = [C.POINTER(Params), _ip]
        L.sift3d_slab_arena_floats.argtypes = [C.POINTER(SlabDesc), C.POINTER(Params), _sz]
        L.sift3d_slab_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(SlabDesc), C.POINTER(Params), C.c_int, C.c_void_p, C.c_size_t]
        L.sift3d_slab_buffer.argtypes = [C.c_void_p, C.c_int, C.c_int, _sz, _ip, _ip]
        L.sift3d_slab_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.sift3d_slab_input_absmax.argtypes = [C.c_void_p, _fp]
        L.sift3d_slab_input_scale.argtypes = [C.c_void_p, C.c_float]
        L.sift3d_slab_level.argtypes = [C.c_void_p, C.c_int]
        L.sift3d_slab_halo_planes.argtypes = [C.c_void_p, C.c_int, _ip]
        L.sift3d_slab_level_hw.argtypes = [C.c_void_p, C.c_int, _ip]
        L.sift3d_slab_sync.argtypes = [C.c_void_p]
        L.sift3d_slab_get_dogmax.argtypes = [C.c_void_p, _fp]
        L.sift3d_slab_set_dogmax.argtypes = [C.c_void_p, _fp]
        L.sift3d_slab_detect.argtypes = [C.c_void_p]
        L.sift3d_slab_describe.argtypes = [C.c_void_p]
        L.sift3d_slab_set_desc_partial.argtypes = [C.c_void_p, C.c_int]
        L.sift3d_slab_min_halo_partial.argtypes = [C.POINTER(Params), _ip]
        L.sift3d_slab_record_bytes.argtypes = [_ip]
        L.sift3d_slab_desc_reach.argtypes = [C.c_void_p, _ip]
        L.sift3d_slab_orient.argtypes = [C.c_void_p]
        L.sift3d_slab_export_records.argtypes = [C.c_void_p, C.c_void_p]
        L.sift3d_slab_describe_partial.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), _ip, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                   C.POINTER(C.c_void_p), _ip, _ip]
        L.sift3d_slab_describe_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p,
                                                  C.c_int, C.c_void_p, C.c_void_p, _ip]
        L.sift3d_slab_orient_launch.argtypes = [C.c_void_p]
        L.sift3d_slab_orient_count.argtypes = [C.c_void_p, _ip]
        L.sift3d_slab_decimate.argtypes = [C.c_void_p, C.c_void_p]
        L.sift3d_slab_decimate_async.argtypes = [C.c_void_p, C.c_void_p]
        L.sift3d_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.sift3d_slab_export_dogmax_device.argtypes = [C.c_void_p, C.c_void_p]
        L.sift3d_slab_import_dogmax_device.argtypes = [C.c_void_p, C.c_void_p]
        L.sift3d_create_seeded.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.c_int]
        L.sift3d_seed_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.sift3d_set_describe_partition.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.sift3d_export_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.sift3d_run_partial_orientation.argtypes = [C.c_void_p]
        L.sift3d_export_orientation_device.argtypes = [C.c_void_p, C.c_void_p]
        L.sift3d_import_orientation_device.argtypes = [C.c_void_p, C.c_void_p]
        L.sift3d_run_describe.argtypes = [C.c_void_p]
        L.sift3d_import_descriptors_device.argtypes = [C.c_void_p, C.c_void_p]
        L.sift3d_sharded_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Params), _ip, C.c_int, C.c_int, C.c_int]
        L.sift3d_sharded_create_ex.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Params), _ip, C.c_int, C.c_int, C.c_int, C.c_uint]
        L.sift3d_sharded_run.argtypes = [C.c_void_p]
        L.sift3d_sharded_num_keypoints.argtypes = [C.c_void_p, _ip]
        L.sift3d_sharded_get_keypoints.argtypes = [C.c_void_p, C.c_void_p, _fp]
        L.sift3d_sharded_info.argtypes = [C.c_void_p, _ip, _ip, _ip, C.POINTER(C.c_double)]
        L.sift3d_sharded_error.argtypes = [C.c_void_p]
        L.sift3d_sharded_error.restype = C.c_char_p
        L.sift3d_sharded_destroy.argtypes = [C.c_void_p]
        L.sift3d_sharded_plan.argtypes = [C.c_void_p, _ip, _ip, _ip, _ip]
        L.sift3d_test_hook.argtypes = [C.c_int, C.c_int]
        L.sift3d_debug_counters.argtypes = [C.c_void_p, _ip]
        L.sift3d_test_run_plan.argtypes = [C.c_void_p, _ip, C.c_int, _ip]
        L.sift3d_debug_face_lookup.argtypes = [_fp, C.c_int, C.c_int, _ip, _fp, C.c_int]
        L.sift3d_debug_copy_bandwidth.argtypes = [C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.sift3d_match_times.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.sift3d_error_string.argtypes = [C.c_int]
        L.sift3d_error_string.restype = C.c_char_p
        L.sift3d_last_error.restype = C.c_char_p
        _lib = L
        # measurement scripts: S3D_HOOKS="one_stream=1,det_serial=1" sets test hooks of the library from the environment of the
        # PYTHON driver (the library itself never reads the environment)
        for item in filter(None, os.environ.get("S3D_HOOKS", "").split(",")):
            k, _, v = item.partition("=")
            L.sift3d_test_hook(HOOKS[k.strip()], int(v or 1))
    return _lib


def _check(rc):
    if rc != 0:
        L = lib()
        raise Sift3dError(f"{L.sift3d_error_string(rc).decode()}: {L.sift3d_last_error().decode()}")


def _f(a):
    return a.ctypes.data_as(_fp)


def kernel_source_sha():
    """sha256 over the kernel sources (3dsift_amd/csrc/*.hip, *.h, include/*.h): stamps measurements that are taken offline
    (profiles/pyramid_traffic_*.json) with the build they belong to"""
    import glob
    import hashlib
    h = hashlib.sha256()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(glob.glob(os.path.join(root, "3dsift_amd", "csrc", "*.hip")) + glob.glob(os.path.join(root, "3dsift_amd", "csrc", "*.h")) +
                   glob.glob(os.path.join(root, "include", "*.h")))
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


class hook:
    """with capi.hook("list_cap", 64): ...  -- sets a test hook of the library (include/sift3d_hip.h) and restores it"""

    def __init__(self, name, value):
        self.which, self.value = HOOKS[name], int(value)

    def __enter__(self):
        self.prev = lib().sift3d_test_hook(self.which, self.value)
        return self

    def __exit__(self, *exc):
        lib().sift3d_test_hook(self.which, self.prev)
        return False


def copy_bandwidth(nbytes=1 << 30, iters=5, device=0):
    """GB/s of the library's float4 device copy kernel (read + write)"""
    g = C.c_double(0)
    _check(lib().sift3d_debug_copy_bandwidth(nbytes, iters, device, C.byref(g)))
    return g.value


def face_lookup(grad3, route=0, device=0):
    """Check_intersect_faces of k_describe on [n, 3] gradients: (face [n] int32, bary [n, 3]); route 0 predicted+verified, 1 literal scan"""
    g = np.ascontiguousarray(grad3, np.float32).reshape(-1, 3)
    face = np.zeros(len(g), np.int32); bary = np.zeros((len(g), 3), np.float32)
    _check(lib().sift3d_debug_face_lookup(_f(g), len(g), int(route), face.ctypes.data_as(_ip), _f(bary), device))
    return face, bary


def default_detect_options():
    """sift3d_default_detect_options as a dict (needs no GPU)"""
    o = DetectOptions()
    lib().sift3d_default_detect_options(C.byref(o))
    return _options_dict(o)


def _options_dict(o):
    return {"neighbours": o.neighbours, "refine": bool(o.refine), "max_offset": o.max_offset, "contrast_thresh": o.contrast_thresh,
            "edge_ratio": o.edge_ratio}


def _options(cls, default_fn_name, names, what, opts):
    """the options struct `cls` filled with the library's defaults (needs no GPU) and then with opts, whose keys must be in names"""
    o = cls()
    getattr(lib(), default_fn_name)(C.byref(o))
    for k, v in opts.items():
        if k not in names:
            raise TypeError(f"unknown {what} option {k!r}")
        setattr(o, k, v)
    return o


RANSAC_OPTIONS = ("iterations", "inlier_thresh", "seed", "refine", "min_det")


def default_ransac_options():
    """sift3d_default_ransac_options as a dict (needs no GPU)"""
    o = _ransac_options({})
    return {k: getattr(o, k) for k in RANSAC_OPTIONS}


def _ransac_options(opts):
    return _options(RansacOptions, "sift3d_default_ransac_options", RANSAC_OPTIONS, "RANSAC", opts)


def _is_dev(a):
    """a device tensor (the entry points take it as it lies: it must be contiguous)"""
    return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)


def _p(a):
    """the pointer to a host array, which the caller keeps alive"""
    return C.c_void_p(a.ctypes.data)


def _table(a, dtype, width, like):
    """(pointer or None, rows, keep-alive) of an optional (m, width) table (width 0: (m,)) as contiguous `dtype` (a numpy type): a numpy
    array when `like` is a host array, a tensor on like.device otherwise"""
    if a is None:
        return None, 0, None
    shape = (-1, width) if width else (-1,)
    if _is_dev(like):
        import torch

        t = torch.as_tensor(a, dtype=getattr(torch, np.dtype(dtype).name), device=like.device).reshape(shape).contiguous()
        return C.c_void_p(t.data_ptr()), t.shape[0], t
    h = np.ascontiguousarray(a, dtype).reshape(shape)
    return _p(h), len(h), h


def _rows(a, width, name):
    """(pointer, rows, keep-alive, on_device) of an (n, width) float32 numpy array or a contiguous float32 device tensor"""
    if _is_dev(a):
        if str(a.dtype) != "torch.float32" or not a.is_contiguous() or (a.numel() and a.shape[-1] != width):
            raise ValueError(f"{name}: a contiguous float32 (n, {width}) device tensor is needed")
        return C.c_void_p(a.data_ptr()), a.numel() // width, a, 1
    h = np.ascontiguousarray(a, np.float32).reshape(-1, width)
    return _p(h), len(h), h, 0


def _volume(a, name, on_dev):
    if on_dev:
        if str(a.dtype) != "torch.float32" or not a.is_contiguous() or a.dim() != 3:
            raise ValueError(f"{name}: a contiguous float32 (nz, ny, nx) device tensor is needed")
        return C.c_void_p(a.data_ptr()), a
    h = np.ascontiguousarray(a, np.float32)
    if h.ndim != 3:
        raise ValueError(f"{name}: a (nz, ny, nx) volume is needed")
    return _p(h), h


def _dtype_code(dtype):
    """the SIFT3D_DT_ code of a numpy / torch dtype or of its name; an int passes through (the library checks it)"""
    if isinstance(dtype, (int, np.integer)):
        return int(dtype)
    name = str(dtype).replace("torch.", "")
    try:
        name = np.dtype(name).name
    except TypeError:
        pass
    if name not in DTYPES:
        raise ValueError(f"dtype {dtype}: one of {sorted(DTYPES)} is needed")
    return DTYPES[name]


def ingest_launch(dtype):
    """sift3d_test_ingest_launch: (lanes per workgroup, elements per 16-byte piece, most workgroups of k_ingest (0: one piece per lane,
    no cap), most workgroups of k_absmax_t) for an integer dtype.  Host only."""
    v = [C.c_int(0) for _ in range(4)]
    _check(lib().sift3d_test_ingest_launch(_dtype_code(dtype), *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def to_device(vol, device=0, with_seconds=False, dtype=None):
    """sift3d_volume_to_device: vol as a new float32 (nz, ny, nx) torch tensor on the device, ready for icgn, zncc_search,
    bspline_prefilter and CSIFT3D(device_ptr=...): uploaded once, used often.  vol: a C-contiguous (nz, ny, nx) numpy array of float32,
    uint8, int8, uint16 or int16 (uploaded at its own width through the pinned staging pool, integers widened on the GPU), or a
    contiguous device tensor of one of those dtypes torch has.  dtype: how the voxels are to be read when that is not vol's own dtype of
    the same width (uint16 data held in an int16 tensor: dtype="uint16").  with_seconds: also the device seconds of the widening."""
    import torch

    on_dev = _is_dev(vol)
    if on_dev:
        if not vol.is_contiguous() or vol.dim() != 3:
            raise ValueError("vol: a contiguous (nz, ny, nx) device tensor is needed")
        device = vol.device.index if vol.device.index is not None else device
        ptr, width = C.c_void_p(vol.data_ptr()), vol.element_size()
    else:
        if not isinstance(vol, np.ndarray) or vol.ndim != 3 or not vol.flags.c_contiguous:
            raise ValueError("vol: a C-contiguous (nz, ny, nx) numpy array is needed")
        ptr, width = _p(vol), vol.dtype.itemsize
    code = _dtype_code(vol.dtype if dtype is None else dtype)
    if not isinstance(dtype, (int, np.integer)) and {0: 4, 1: 1, 2: 1, 3: 2, 4: 2}[code] != width:
        raise ValueError(f"dtype {dtype} does not have the width of vol's {vol.dtype}")
    nz, ny, nx = vol.shape
    out = torch.empty((nz, ny, nx), dtype=torch.float32, device=f"cuda:{int(device)}")
    sec = C.c_double(0)
    _check(lib().sift3d_volume_to_device(ptr, code, nx, ny, nz, int(on_dev), int(device), C.c_void_p(out.data_ptr()), C.byref(sec)))
    return (out, sec.value) if with_seconds else out


def _volume_pair(ref, tar):
    """((ref pointer, tar pointer), ((nx, ny, nz) of ref, of tar), on_device, keep-alives) of two (nz, ny, nx) float32 volumes"""
    on_dev = _is_dev(ref)
    if on_dev != _is_dev(tar):
        raise ValueError("ref and tar must both be numpy arrays or both device tensors")
    (rp, r), (tp, t) = _volume(ref, "ref", on_dev), _volume(tar, "tar", on_dev)
    return (rp, tp), (r.shape[::-1], t.shape[::-1]), int(on_dev), (r, t)


def _fields(rec, m, names):
    """copies of the named fields of the first m records (m None: of the one record of a 0-d array)"""
    if m is not None:
        rec = rec[:m]
    return {k: rec[k].copy() for k in names}


FIT_FIELDS = ("A", "hyp", "status", "candidates", "best_hypothesis", "best_count", "inliers", "rms")


def _fit_dict(f, m):
    d = _fields(f, m, FIT_FIELDS)
    for k in ("A", "hyp"):
        d[k] = d[k].reshape(d[k].shape[:-1] + (3, 4))
    return d


FIT_MODELS = {"rigid": 0, "similarity": 1}


def _model_code(model):
    """the model argument of sift3d_fit_rigid[_local] of a name; an int passes through (the library checks it)"""
    if isinstance(model, (int, np.integer)):
        return int(model)
    if model not in FIT_MODELS:
        raise ValueError(f"model {model!r}: one of {sorted(FIT_MODELS)} is needed")
    return FIT_MODELS[model]


def _fit_global(pairs, model, device, opts):
    """the global fit of one model (None: affine)"""
    o = _ransac_options(opts)
    pp, n, keep, on_dev = _rows(pairs, 6, "pairs")
    out = np.zeros((), FIT_DTYPE)
    mask = np.zeros(max(n, 1), np.uint8)
    sec = C.c_double(0)
    tail = (C.byref(o), on_dev, int(device), _p(out), _p(mask), C.byref(sec))
    _check(lib().sift3d_fit_affine(pp, n, *tail) if model is None else lib().sift3d_fit_rigid(pp, n, _model_code(model), *tail))
    d = {k: (v if k in ("A", "hyp") else v.item()) for k, v in _fit_dict(out, None).items()}
    d["mask"] = mask[:n].astype(bool)
    d["seconds"] = sec.value
    return d


def fit_affine(pairs, device=0, **opts):
    """sift3d_fit_affine: RANSAC affine t = L r + b over all rows of pairs ((n, 6) float32: ref rx ry rz, tar rx ry rz; numpy or a
    device tensor).  Returns the fit's fields (A and hyp as (3, 4) float64, scalars as Python numbers), the inlier mask (bool [n])
    and the device seconds."""
    return _fit_global(pairs, None, device, opts)


def fit_rigid(pairs, model="rigid", device=0, **opts):
    """sift3d_fit_rigid: RANSAC rigid (t = R r + b) or similarity (t = s R r + b) fit over all rows of pairs; what fit_affine takes
    and returns, with A = hyp = [s R | b].  Three pairs that are not collinear fix the fit, so coplanar pairs are fitted."""
    return _fit_global(pairs, model, device, opts)


def _fit_local(pairs, points, k, radius, model, device, opts):
    """the local fits of one model (None: affine)"""
    o = _ransac_options(opts)
    pp, n, keep_p, dev_p = _rows(pairs, 6, "pairs")
    qp, m, keep_q, dev_q = _rows(points, 3, "points")
    if dev_p != dev_q:
        raise ValueError("pairs and points must both be host arrays or both device tensors")
    out = np.zeros(max(m, 1), FIT_DTYPE)
    nb = np.zeros((max(m, 1), max(int(k), 1)), np.int32)
    sec = C.c_double(0)
    head, tail = (pp, n, qp, m, int(k), float(radius)), (C.byref(o), dev_p, int(device), _p(out), _p(nb), C.byref(sec))
    _check(lib().sift3d_fit_affine_local(*head, *tail) if model is None else lib().sift3d_fit_rigid_local(*head, _model_code(model), *tail))
    d = _fit_dict(out, m)
    d["neighbours"] = nb[:m].copy()
    d["seconds"] = sec.value
    return d


def fit_affine_local(pairs, points, k=32, radius=0.0, device=0, **opts):
    """sift3d_fit_affine_local: one RANSAC affine per query point ((m, 3) reference coordinates) on its k nearest pairs (within radius
    when radius > 0).  Returns per-point arrays (A, hyp: (m, 3, 4); status, counts, rms: (m,)), neighbours (m, k) int32 (-1 padded)
    and the device seconds."""
    return _fit_local(pairs, points, k, radius, None, device, opts)


def fit_rigid_local(pairs, points, k=16, radius=0.0, model="rigid", device=0, **opts):
    """sift3d_fit_rigid_local: one RANSAC rigid or similarity fit per query point on its k nearest pairs, k in 3..64; what
    fit_affine_local takes and returns.  icgn_init_from_fits takes the result as it takes an affine one."""
    return _fit_local(pairs, points, k, radius, model, device, opts)


def fit_rigid_bodies(pairs, pair_label, count, model="rigid", device=0, **opts):
    """sift3d_fit_rigid_bodies: one RANSAC rigid or similarity fit per body.  pairs: (n, 6) float32 as for fit_rigid; pair_label: (n,)
    int32, the body 1..count of each pair (labels_at_positions on pairs gives it; any other value: no body), a numpy array or, where
    pairs is a device tensor, an int32 device tensor.  iterations 0 means 256.  Returns fit_rigid_local's fields with a leading body
    axis (A, hyp: (count, 3, 4); status, counts, rms: (count,); row L - 1 is body L), mask (bool [n]: pair i is an inlier of its own
    body's fit) and the device seconds."""
    o = _ransac_options(opts)
    pp, n, keep, on_dev = _rows(pairs, 6, "pairs")
    lp, nl, lab = _table(pair_label, np.int32, 0, pairs)
    if lab is None or nl != n:
        raise ValueError("pair_label: one label per pair")
    count = int(count)
    out = np.zeros(max(count, 1), FIT_DTYPE)
    mask = np.zeros(max(n, 1), np.uint8)
    sec = C.c_double(0)
    _check(lib().sift3d_fit_rigid_bodies(pp, n, lp, count, _model_code(model), C.byref(o), on_dev, int(device), _p(out), _p(mask),
                                         C.byref(sec)))
    d = _fit_dict(out, max(count, 0))
    d["mask"] = mask[:n].astype(bool)
    d["seconds"] = sec.value
    return d


def fit_rotation(fits):
    """sift3d_fit_rotation (needs no GPU): the rotation each fit holds, from the dict fit_rigid / fit_rigid_local returns (A (3, 4) or
    (m, 3, 4), status).  Returns quat ((m, 4): w, x, y, z with w >= 0), scale (m,) and angle_deg (m,) -- without the leading axis for
    one fit; a failed fit gives NaN."""
    A = np.asarray(fits["A"], np.float64)
    single = A.ndim == 2
    A = A.reshape(-1, 12)
    m = len(A)
    f = np.zeros(max(m, 1), FIT_DTYPE)
    f["A"][:m] = A
    f["status"][:m] = np.asarray(fits["status"]).reshape(-1)
    quat, scale, angle = np.zeros((max(m, 1), 4)), np.zeros(max(m, 1)), np.zeros(max(m, 1))
    _check(lib().sift3d_fit_rotation(_p(f), m, _p(quat), _p(scale), _p(angle)))
    if single:
        return {"quat": quat[0].copy(), "scale": float(scale[0]), "angle_deg": float(angle[0])}
    return {"quat": quat[:m].copy(), "scale": scale[:m].copy(), "angle_deg": angle[:m].copy()}


def predict_positions(fit, xyz):
    """sift3d_predict_positions (needs no GPU): where a fit sends the reference positions xyz ((n, 3) float32 rx, ry, rz), as (n, 3)
    float32 -- the `pred` of match_guided.  fit: the dict fit_affine / fit_rigid returns (A (3, 4): one fit for all rows) or the one
    fit_affine_local / fit_rigid_local returns when queried at xyz itself (A (n, 3, 4)); a failed fit (status != 0) gives a NaN row,
    whose gate is empty."""
    A = np.asarray(fit["A"], np.float64)
    A = A.reshape(-1, 12)
    r = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    f = np.zeros(max(len(A), 1), FIT_DTYPE)
    f["A"][:len(A)] = A
    f["status"][:len(A)] = np.asarray(fit["status"]).reshape(-1)
    out = np.zeros((max(len(r), 1), 3), np.float32)
    _check(lib().sift3d_predict_positions(_p(f), len(A), _p(r), len(r), _p(out)))
    return out[:len(r)].copy()


MATCH_MODES = {"inject": 1, "biject": 2, "enhanced": 3}


def match_guided(ref_desc, ref_xyz, tar_desc, tar_xyz, pred, radius, thresHold=0.85, mode="enhanced", device=0):
    """sift3d_match_guided: muBruteMatcher's match with every row's targets limited to its gate -- the targets within `radius` of
    pred[i] on each axis (fp32).  The five tables are numpy arrays or contiguous float32 device tensors, all of one kind (desc (n, 768)
    / (m, 768), xyz and pred (n, 3) / (m, 3)); mode: "inject" | "biject" | "enhanced" or 1..3.  Returns gIdx, sIdx, gDist, sDist,
    candidates (n,), pairs (k, 6) and the device seconds."""
    tabs = [_rows(ref_desc, DESC, "ref_desc"), _rows(ref_xyz, 3, "ref_xyz"), _rows(tar_desc, DESC, "tar_desc"), _rows(tar_xyz, 3, "tar_xyz"),
            _rows(pred, 3, "pred")]
    if len({t[3] for t in tabs}) != 1:
        raise ValueError("the five tables must all be host arrays or all device tensors")
    n, m = tabs[0][1], tabs[2][1]
    if tabs[1][1] != n or tabs[4][1] != n or tabs[3][1] != m:
        raise ValueError("ref_xyz and pred need one row per reference descriptor, tar_xyz one per target descriptor")
    if not isinstance(mode, (int, np.integer)):
        if mode not in MATCH_MODES:
            raise ValueError(f"mode {mode!r}: one of {sorted(MATCH_MODES)} is needed")
        mode = MATCH_MODES[mode]
    nn = max(n, 1)
    gi = np.zeros(nn, np.int32); si = np.zeros(nn, np.int32); cand = np.zeros(nn, np.int32)
    gd = np.zeros(nn, np.float32); sd = np.zeros(nn, np.float32)
    pairs = np.zeros((nn, 6), np.float32)
    k = C.c_int(0); sec = C.c_double(0)
    _check(lib().sift3d_match_guided(tabs[0][0], tabs[1][0], n, tabs[2][0], tabs[3][0], m, tabs[4][0], float(radius), float(thresHold),
                                     int(mode), tabs[0][3], int(device), gi.ctypes.data_as(_ip), si.ctypes.data_as(_ip),
                                     _f(gd), _f(sd), cand.ctypes.data_as(_ip), _f(pairs), C.byref(k), C.byref(sec)))
    return dict(gIdx=gi[:n], sIdx=si[:n], gDist=gd[:n], sDist=sd[:n], candidates=cand[:n], pairs=pairs[:k.value].copy(), seconds=sec.value)


ICGN_OPTIONS = ("subset_radius", "max_iterations", "tolerance", "interpolation")


def default_icgn_options():
    """sift3d_default_icgn_options as a dict (needs no GPU)"""
    o = _icgn_options({})
    return {k: getattr(o, k) for k in ICGN_OPTIONS}


def _icgn_options(opts):
    return _options(IcgnOptions, "sift3d_default_icgn_options", ICGN_OPTIONS, "IC-GN", opts)


def icgn_init_from_fits(fits, points):
    """sift3d_icgn_init_from_fits: (m, 12) float64 initial parameters from the dict fit_affine_local returns (A (m, 3, 4), status) at
    the integer points ((m, 3) x, y, z); a failed fit gives a NaN row"""
    A = np.asarray(fits["A"], np.float64).reshape(-1, 12)
    f = np.zeros(max(len(A), 1), FIT_DTYPE)
    f["A"][:len(A)] = A
    f["status"][:len(A)] = np.asarray(fits["status"])
    q = np.ascontiguousarray(points, np.int32).reshape(-1, 3)
    if len(q) != len(A):
        raise ValueError("one point per fit")
    out = np.zeros((max(len(A), 1), 12), np.float64)
    _check(lib().sift3d_icgn_init_from_fits(_p(f), _p(q), len(A), _p(out)))
    return out[:len(A)].copy()


def icgn_init_from_body_fits(fits, poi_label, points):
    """sift3d_icgn_init_from_body_fits (needs no GPU): (m, 12) float64 initial parameters from the dict fit_rigid_bodies returns (A
    (count, 3, 4), status), the body of each point (poi_label (m,) int32: labels_at's output) and the integer points ((m, 3) x, y, z):
    row i is icgn_init_from_fits' for the fit of body poi_label[i]; a point of no body and a failed fit give a NaN row"""
    A = np.asarray(fits["A"], np.float64).reshape(-1, 12)
    f = np.zeros(max(len(A), 1), FIT_DTYPE)
    f["A"][:len(A)] = A
    f["status"][:len(A)] = np.asarray(fits["status"])
    q = np.ascontiguousarray(points, np.int32).reshape(-1, 3)
    lab = np.ascontiguousarray(poi_label, np.int32).reshape(-1)
    if len(q) != len(lab):
        raise ValueError("one label per point")
    out = np.zeros((max(len(q), 1), 12), np.float64)
    _check(lib().sift3d_icgn_init_from_body_fits(_p(f), len(A), _p(lab), _p(q), len(q), _p(out)))
    return out[:len(q)].copy()


def icgn(ref, tar, points, init=None, device=0, **opts):
    """sift3d_icgn: IC-GN refinement of the displacement at each point ((m, 3) int32 x, y, z of ref) from ref to tar.  ref / tar:
    (nz, ny, nx) float32 numpy arrays or contiguous float32 device tensors, both of the same kind; init: (m, 12) float64 or None (zero).
    Options: subset_radius, max_iterations, tolerance, interpolation (0 tricubic, 1 trilinear).  Returns p (m, 12), displacement
    (m, 3) = (u, v, w), gradient (m, 3, 3) (rows u, v, w; columns x, y, z), zncc, last_step, iterations, status (m,) and the device
    seconds."""
    return _icgn(1, "sift3d_icgn", ref, tar, points, init, device, opts, None)


def _icgn(order, entry, ref, tar, points, init, device, opts, coefficients, mask=None, min_fraction=0.0, labels=None):
    """the call behind icgn, icgn_bspline, icgn_masked, icgn_labelled (order 1) and icgn2 (order 2); entry: the exported function's
    name; coefficients None: the entry has no tar_is_coefficients argument; mask: icgn_masked's, with its min_fraction (the entry then
    takes the mask behind the volumes, min_fraction behind the options and the active counts behind the records); labels:
    icgn_labelled's, in the mask's place (the entry also takes the POI labels behind the active counts)"""
    width, dtype = {1: (12, ICGN_DTYPE), 2: (30, ICGN2_DTYPE)}[order]
    o = _icgn_options(opts)
    (rp, tp), (rdim, tdim), on_dev, keep = _volume_pair(ref, tar)
    qp, m, q = _table(points, np.int32, 3, ref)
    ip, mi, ini = _table(init, np.float64, width, ref)
    if ini is not None and mi != m:
        raise ValueError(f"init: one row of {width} per point")
    out = np.zeros(max(m, 1), dtype)
    sec = C.c_double(0)
    coef = () if coefficients is None else (int(bool(coefficients)),)
    mp = mf = ap = ()
    if mask is not None:
        active = np.zeros(max(m, 1), np.int32)
        mptr, mkeep = _mask(mask, keep[0].shape, on_dev)  # (mkeep: the array behind the pointer lives until the call returns)
        mp, mf, ap = (mptr,), (float(min_fraction),), (_p(active),)
    if labels is not None:
        active, poi_label = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.int32)
        mptr, mkeep = _label_volume(labels, keep[0].shape, on_dev)
        mp, mf, ap = (mptr,), (float(min_fraction),), (_p(active), _p(poi_label))
    _check(getattr(lib(), entry)(rp, *rdim, tp, *tdim, *mp, qp, m, ip, C.byref(o), *mf, *coef, on_dev, int(device), _p(out), *ap, C.byref(sec)))
    d = _fields(out, m, ("p", "zncc", "last_step", "iterations", "status"))
    if mask is not None or labels is not None:
        d["active"] = active[:m].copy()
    if labels is not None:
        d["label"] = poi_label[:m].copy()
    e = d["p"].reshape(-1, 3, width // 3)
    d["displacement"] = e[:, :, 0].copy()
    d["gradient"] = e[:, :, 1:4].copy()
    if order == 2:
        d["second"] = e[:, :, 4:].copy()
    d["seconds"] = sec.value
    return d


def bspline_prefilter(vol, device=0, with_seconds=False):
    """sift3d_bspline_prefilter: the cubic B-spline coefficients (mirror boundary) of vol, an (nz, ny, nx) float32 numpy array or a
    contiguous float32 device tensor; returns an array / a tensor of the same kind (with_seconds: and the device seconds)"""
    on_dev = _is_dev(vol)
    vp, v = _volume(vol, "vol", on_dev)
    if on_dev:
        import torch

        out = torch.empty_like(v)
        op = C.c_void_p(out.data_ptr())
    else:
        out = np.empty_like(v)
        op = _p(out)
    sec = C.c_double(0)
    _check(lib().sift3d_bspline_prefilter(vp, *v.shape[::-1], op, int(on_dev), int(device), C.byref(sec)))
    return (out, sec.value) if with_seconds else out


def icgn_bspline(ref, tar, points, init=None, coefficients=False, device=0, **opts):
    """sift3d_icgn_bspline: icgn with the target interpolated by cubic B-splines.  coefficients False: tar is the volume, prefiltered
    inside the call; True: tar is bspline_prefilter's output.  Options: subset_radius, max_iterations, tolerance (interpolation must
    stay 0).  Returns what icgn returns."""
    return _icgn(1, "sift3d_icgn_bspline", ref, tar, points, init, device, opts, bool(coefficients))


def icgn2_init_from_icgn(res):
    """sift3d_icgn2_init_from_icgn: (m, 30) float64 initial parameters for icgn2 from the dict icgn / icgn_bspline returns (p,
    status): a row with status 0 or 1 gives its 12 parameters and zero second derivatives, any other status a NaN row.  Needs no GPU."""
    p = np.asarray(res["p"], np.float64).reshape(-1, 12)
    m = len(p)
    rec = np.zeros(max(m, 1), ICGN_DTYPE)
    rec["p"][:m] = p
    rec["status"][:m] = np.asarray(res["status"])
    out = np.zeros((max(m, 1), 30), np.float64)
    _check(lib().sift3d_icgn2_init_from_icgn(_p(rec), m, _p(out)))
    return out[:m].copy()


def icgn2(ref, tar, points, init=None, coefficients=False, device=0, **opts):
    """sift3d_icgn2: second-order IC-GN at each point ((m, 3) int32 x, y, z of ref) from ref to tar.  ref / tar as for icgn; init:
    (m, 30) float64 (icgn2_init_from_icgn) or None (zero).  Options: subset_radius, max_iterations, tolerance, interpolation (0
    tricubic Keys, 1 trilinear, 2 cubic B-spline; coefficients True: tar is bspline_prefilter's output, interpolation 2 only).
    Returns p (m, 30), displacement (m, 3), gradient (m, 3, 3) (rows u, v, w; columns x, y, z), second (m, 3, 6) (columns xx, yy, zz,
    xy, xz, yz), zncc, last_step, iterations, status (m,) and the device seconds."""
    return _icgn(2, "sift3d_icgn2", ref, tar, points, init, device, opts, bool(coefficients))


def _mask(a, shape, on_dev):
    """(pointer, keep-alive) of a uint8 mask of `shape` that lies where the volumes lie"""
    if on_dev:
        if not _is_dev(a) or str(a.dtype) != "torch.uint8" or not a.is_contiguous() or tuple(a.shape) != tuple(shape):
            raise ValueError(f"mask: a contiguous uint8 device tensor of shape {tuple(shape)} is needed")
        return C.c_void_p(a.data_ptr()), a
    if _is_dev(a):
        raise ValueError("mask must lie where ref and tar lie")
    h = np.ascontiguousarray(a)
    if h.dtype == np.bool_:
        h = h.view(np.uint8)
    if h.dtype != np.uint8 or h.shape != tuple(shape):
        raise ValueError(f"mask: a uint8 or bool array of shape {tuple(shape)} is needed")
    return _p(h), h


def icgn_masked(ref, tar, mask, points, init=None, min_fraction=0.0, tar_is_coefficients=False, device=0, **opts):
    """sift3d_icgn_masked: icgn limited to the active voxels of each subset -- those that, with their six face neighbours, are in mask,
    an (nz, ny, nx) uint8 (or bool) numpy array, or a contiguous uint8 device tensor where ref and tar are device tensors; any non-zero
    byte is "in".  Options: icgn's, with interpolation 0 tricubic Keys, 1 trilinear, 2 cubic B-spline (tar_is_coefficients True: tar is
    bspline_prefilter's output, interpolation 2 only).  A point whose subset holds no active voxel, or fewer than min_fraction (0..1)
    of its (2r+1)^3, returns status 7.  Returns what icgn returns and active (m,) int32, the active voxels of each subset."""
    return _icgn(1, "sift3d_icgn_masked", ref, tar, points, init, device, opts, bool(tar_is_coefficients), mask, min_fraction)


def _label_volume(a, shape, on_dev):
    """(pointer, keep-alive) of an int32 label volume of `shape` that lies where the volumes lie"""
    if on_dev:
        if not _is_dev(a) or str(a.dtype) != "torch.int32" or not a.is_contiguous() or tuple(a.shape) != tuple(shape):
            raise ValueError(f"labels: a contiguous int32 device tensor of shape {tuple(shape)} is needed")
        return C.c_void_p(a.data_ptr()), a
    if _is_dev(a):
        raise ValueError("labels must lie where ref and tar lie")
    h = np.ascontiguousarray(a, np.int32)
    if h.shape != tuple(shape):
        raise ValueError(f"labels: an int32 array of shape {tuple(shape)} is needed")
    return _p(h), h


def icgn_labelled(ref, tar, labels, points, init=None, min_fraction=0.0, tar_is_coefficients=False, device=0, **opts):
    """sift3d_icgn_labelled: every point correlated over its own body, in one call: point i is treated as icgn_masked treats it under
    the mask labels == labels[point i].  labels: an (nz, ny, nx) int32 numpy array (what mask_label returns; any positive int is a
    label), or a contiguous int32 device tensor where ref and tar are device tensors.  A point on a voxel whose label is <= 0 returns
    status 7.  Options and the other arguments: icgn_masked's.  Returns what icgn_masked returns and label (m,) int32, the label under
    each point (0 outside ref)."""
    return _icgn(1, "sift3d_icgn_labelled", ref, tar, points, init, device, opts, bool(tar_is_coefficients), None, min_fraction, labels)


def mask_from_level(vol, level, device=0, with_seconds=False):
    """sift3d_mask_from_level: the uint8 mask icgn_masked takes, 1 where float64(vol) >= level (subset_quality's rule for `material`; a
    NaN voxel is 0), else 0.  vol: an (nz, ny, nx) float32 numpy array or a contiguous float32 device tensor; returns an array / a
    tensor of the same kind (with_seconds: and the device seconds)."""
    on_dev = _is_dev(vol)
    vp, v = _volume(vol, "vol", on_dev)
    if on_dev:
        import torch

        out = torch.empty(v.shape, dtype=torch.uint8, device=v.device)
        op = C.c_void_p(out.data_ptr())
        device = v.device.index if v.device.index is not None else device
    else:
        out = np.empty(v.shape, np.uint8)
        op = _p(out)
    sec = C.c_double(0)
    _check(lib().sift3d_mask_from_level(vp, *v.shape[::-1], float(level), op, int(on_dev), int(device), C.byref(sec)))
    return (out, sec.value) if with_seconds else out


def label_tile():
    """sift3d_test_label_tile (test hook): the extents (tx, ty, tz) of the tile whose union-find mask_label runs in LDS.  Needs no GPU."""
    t = (C.c_int * 3)()
    _check(lib().sift3d_test_label_tile(t))
    return tuple(t)


def mask_label(mask, connectivity=6, min_voxels=1, device=0, with_seconds=False):
    """sift3d_mask_label: the connected components of a mask, an (nz, ny, nx) uint8 (or bool) numpy array or a contiguous uint8 device
    tensor; any non-zero byte is "in".  connectivity: 6 (faces) or 26 (faces, edges and corners).  Returns labels, an int32 array / tensor
    of the same shape and kind -- 0 outside the mask and in components of fewer than min_voxels voxels, else 1..count in ascending
    order of a component's lowest voxel (scipy.ndimage.label's numbering) -- and count (with_seconds: and the device seconds)."""
    on_dev = _is_dev(mask)
    if on_dev:
        import torch

        if str(mask.dtype) not in ("torch.uint8", "torch.bool") or not mask.is_contiguous() or mask.dim() != 3:
            raise ValueError("mask: a contiguous uint8 (nz, ny, nx) device tensor is needed")
        v = mask
        vp = C.c_void_p(v.data_ptr())
        out = torch.empty(v.shape, dtype=torch.int32, device=v.device)
        op = C.c_void_p(out.data_ptr())
        device = v.device.index if v.device.index is not None else device
    else:
        v = np.asarray(mask)
        if v.ndim != 3 or v.dtype not in (np.uint8, np.bool_):
            raise ValueError("mask: a uint8 or bool (nz, ny, nx) array is needed")
        v = np.ascontiguousarray(v).view(np.uint8)
        vp = _p(v)
        out = np.empty(v.shape, np.int32)
        op = _p(out)
    sec, count = C.c_double(0), C.c_int(0)
    _check(lib().sift3d_mask_label(vp, *tuple(v.shape)[::-1], int(connectivity), int(min_voxels), op, C.byref(count), int(on_dev), int(device),
                                   C.byref(sec)))
    return (out, count.value, sec.value) if with_seconds else (out, count.value)


def labels_at(labels, points, device=0):
    """sift3d_labels_at_points: the label (m,) int32 at each point ((m, 3) int32 x, y, z) of labels, an (nz, ny, nx) int32 numpy array or
    contiguous int32 device tensor (what mask_label returns); 0 for a point outside the volume.  With a host array it needs no GPU."""
    on_dev = _is_dev(labels)
    if on_dev:
        if str(labels.dtype) != "torch.int32" or not labels.is_contiguous() or labels.dim() != 3:
            raise ValueError("labels: a contiguous int32 (nz, ny, nx) device tensor is needed")
        lab, lp = labels, C.c_void_p(labels.data_ptr())
        device = labels.device.index if labels.device.index is not None else device
    else:
        lab = np.ascontiguousarray(labels, np.int32)
        if lab.ndim != 3:
            raise ValueError("labels: an (nz, ny, nx) volume is needed")
        lp = _p(lab)
    qp, m, q = _table(points, np.int32, 3, labels)
    out = np.zeros(max(m, 1), np.int32)
    _check(lib().sift3d_labels_at_points(lp, *tuple(lab.shape)[::-1], qp, m, _p(out), int(on_dev), int(device)))
    return out[:m].copy()


def labels_at_positions(labels, xyz, device=0):
    """sift3d_labels_at_positions: the label (n,) int32 at the voxel nearest to each fp32 position of xyz -- (n, 3) x, y, z, or the
    (n, 6) pairs of the fits, whose reference positions are then used -- 0 for a position outside the volume (closer than half a
    voxel to the first or last voxel counts as inside).  labels: an (nz, ny, nx) int32 numpy array, or a contiguous int32 device tensor
    with xyz a float32 device tensor.  With host arrays it needs no GPU."""
    on_dev = _is_dev(labels)
    if on_dev != _is_dev(xyz):
        raise ValueError("labels and xyz must both be numpy arrays or both device tensors")
    if on_dev:
        if str(labels.dtype) != "torch.int32" or not labels.is_contiguous() or labels.dim() != 3:
            raise ValueError("labels: a contiguous int32 (nz, ny, nx) device tensor is needed")
        if str(xyz.dtype) != "torch.float32" or not xyz.is_contiguous() or xyz.dim() != 2 or xyz.shape[1] not in (3, 6):
            raise ValueError("xyz: a contiguous float32 (n, 3) or (n, 6) device tensor is needed")
        lab, lp, pos, xp = labels, C.c_void_p(labels.data_ptr()), xyz, C.c_void_p(xyz.data_ptr())
        device = labels.device.index if labels.device.index is not None else device
    else:
        lab = np.ascontiguousarray(labels, np.int32)
        if lab.ndim != 3:
            raise ValueError("labels: an (nz, ny, nx) volume is needed")
        pos = np.ascontiguousarray(xyz, np.float32)
        if pos.ndim != 2 or pos.shape[1] not in (3, 6):
            raise ValueError("xyz: an (n, 3) or (n, 6) array is needed")
        lp, xp = _p(lab), _p(pos)
    n, stride = int(pos.shape[0]), int(pos.shape[1])
    out = np.zeros(max(n, 1), np.int32)
    _check(lib().sift3d_labels_at_positions(lp, *tuple(lab.shape)[::-1], xp, stride, n, _p(out), int(on_dev), int(device)))
    return out[:n].copy()


def _mask_input(mask):
    """(pointer, the uint8 array / tensor, on_device) of an (nz, ny, nx) uint8 or bool mask"""
    on_dev = _is_dev(mask)
    if not on_dev:
        mask = np.asarray(mask)
    if len(mask.shape) != 3:
        raise ValueError("mask: an (nz, ny, nx) volume is needed")
    p, v = _mask(mask, mask.shape, on_dev)
    return p, v, on_dev


def _like(v, on_dev, dtype):
    """(pointer, an uninitialised array / tensor of v's shape and kind)"""
    if on_dev:
        import torch

        out = torch.empty(v.shape, dtype=getattr(torch, np.dtype(dtype).name), device=v.device)
        return C.c_void_p(out.data_ptr()), out
    out = np.empty(v.shape, dtype)
    return _p(out), out


def _device_of(v, on_dev, device):
    return v.device.index if on_dev and v.device.index is not None else device


def mask_distance(mask, border=1, device=0, with_seconds=False):
    """sift3d_mask_distance: the exact squared Euclidean distance of every in-voxel of mask -- an (nz, ny, nx) uint8 (or bool) numpy
    array or a contiguous uint8 device tensor; any non-zero byte is "in" -- to the nearest out-voxel, 0 for an out-voxel.  border 1: the
    layer of voxels around the volume counts as out; border 0: only the volume's own out-voxels, DIST2_NONE everywhere when there is
    none.  Returns an int32 array / tensor of the same shape and kind (with_seconds: and the device seconds)."""
    vp, v, on_dev = _mask_input(mask)
    op, out = _like(v, on_dev, np.int32)
    sec = C.c_double(0)
    _check(lib().sift3d_mask_distance(vp, *tuple(v.shape)[::-1], int(border), op, int(on_dev), int(_device_of(v, on_dev, device)), C.byref(sec)))
    return (out, sec.value) if with_seconds else out


def _dist_input(dist2):
    """(pointer, the int32 array / tensor, on_device) of an (nz, ny, nx) int32 volume"""
    on_dev = _is_dev(dist2)
    if not on_dev:
        dist2 = np.asarray(dist2)
    if len(dist2.shape) != 3:
        raise ValueError("dist2: an (nz, ny, nx) volume is needed")
    p, v = _label_volume(dist2, dist2.shape, on_dev)
    return p, v, on_dev


def mask_from_distance(dist2, level2, device=0, with_seconds=False):
    """sift3d_mask_from_distance: the uint8 mask dist2 >= level2 of mask_distance's output (an int32 numpy array or device tensor): with
    level2 >= 1 the exact erosion of the mask by the open ball of squared radius level2.  Returns an array / a tensor of the same kind
    (with_seconds: and the device seconds)."""
    vp, v, on_dev = _dist_input(dist2)
    op, out = _like(v, on_dev, np.uint8)
    sec = C.c_double(0)
    _check(lib().sift3d_mask_from_distance(vp, *tuple(v.shape)[::-1], int(level2), op, int(on_dev), int(_device_of(v, on_dev, device)),
                                           C.byref(sec)))
    return (out, sec.value) if with_seconds else out


def distance_at(dist2, points, device=0):
    """sift3d_distance_at_points: dist2 (m,) int32 at each point ((m, 3) int32 x, y, z) of mask_distance's output, an int32 numpy array or
    device tensor; 0 for a point outside the volume.  With a host array it needs no GPU."""
    vp, v, on_dev = _dist_input(dist2)
    qp, m, q = _table(points, np.int32, 3, dist2)
    out = np.zeros(max(m, 1), np.int32)
    _check(lib().sift3d_distance_at_points(vp, *tuple(v.shape)[::-1], qp, m, _p(out), int(on_dev), int(_device_of(v, on_dev, device))))
    return out[:m].copy()


SPLIT_OPTIONS = ("connectivity", "core_dist2", "min_core_voxels", "border", "max_rounds", "keep_unreached", "min_voxels")
SPLIT_INFO = ("cores", "unreached_bodies", "rounds", "unlabelled")


def default_split_options():
    """sift3d_default_split_options as a dict (needs no GPU)"""
    o = _options(SplitOptions, "sift3d_default_split_options", SPLIT_OPTIONS, "split", {})
    return {k: getattr(o, k) for k in SPLIT_OPTIONS}


def mask_split(mask, device=0, with_seconds=False, return_distance=False, **opts):
    """sift3d_mask_split: labels of bodies that may touch.  The cores -- the components of mask_distance(mask, border) >= core_dist2 --
    are numbered as mask_label numbers them and grown back over the mask in synchronous rounds, a voxel taking the label of its labelled
    neighbour with the largest distance (ties: the smallest label); with keep_unreached the components no core reaches are numbered
    behind the cores.  mask: as for mask_label.  Options: SPLIT_OPTIONS (default_split_options()).  Returns labels (int32, the mask's
    shape and kind), count and info, a dict of SPLIT_INFO (return_distance: then dist2, what mask_distance returns; with_seconds: then
    the device seconds)."""
    o = _options(SplitOptions, "sift3d_default_split_options", SPLIT_OPTIONS, "split", {k: int(v) for k, v in opts.items()})
    vp, v, on_dev = _mask_input(mask)
    op, out = _like(v, on_dev, np.int32)
    dp, dist = _like(v, on_dev, np.int32) if return_distance else (None, None)
    sec, count, info = C.c_double(0), C.c_int(0), SplitInfo()
    _check(lib().sift3d_mask_split(vp, *tuple(v.shape)[::-1], C.byref(o), op, C.byref(count), dp, C.byref(info), int(on_dev),
                                   int(_device_of(v, on_dev, device)), C.byref(sec)))
    res = (out, count.value, {k: getattr(info, k) for k in SPLIT_INFO})
    if return_distance:
        res += (dist,)
    return res + (sec.value,) if with_seconds else res


SEARCH_OPTIONS = ("subset_radius", "search_radius")


def default_search_options():
    """sift3d_default_search_options as a dict (needs no GPU)"""
    o = _options(SearchOptions, "sift3d_default_search_options", SEARCH_OPTIONS, "search", {})
    return {k: getattr(o, k) for k in SEARCH_OPTIONS}


def zncc_search(ref, tar, points, guess=None, device=0, **opts):
    """sift3d_zncc_search: the integer displacement of highest ZNCC at each point ((m, 3) int32 x, y, z of ref) within search_radius of
    guess ((m, 3) int32 or None: zero).  ref / tar: (nz, ny, nx) float32 numpy arrays or contiguous float32 device tensors, both of
    the same kind.  Options: subset_radius, search_radius.  Returns d (m, 3) int32, zncc, zncc_second, candidates, status (m,) and
    the device seconds."""
    o = _options(SearchOptions, "sift3d_default_search_options", SEARCH_OPTIONS, "search", opts)
    (rp, tp), (rdim, tdim), on_dev, keep = _volume_pair(ref, tar)
    qp, m, q = _table(points, np.int32, 3, ref)
    gp, mg, gs = _table(guess, np.int32, 3, ref)
    if gs is not None and mg != m:
        raise ValueError("guess: one (gx, gy, gz) per point")
    out = np.zeros(max(m, 1), SEARCH_DTYPE)
    sec = C.c_double(0)
    _check(lib().sift3d_zncc_search(rp, *rdim, tp, *tdim, qp, m, gp, C.byref(o), on_dev, int(device), _p(out), C.byref(sec)))
    d = _fields(out, m, ("d", "zncc", "zncc_second", "candidates", "status"))
    d["seconds"] = sec.value
    return d


def icgn_init_from_search(res, init=None, only_missing=True):
    """sift3d_icgn_init_from_search: (m, 12) float64 initial parameters for icgn from the dict zncc_search returns.  Rows of init
    (None: all NaN) whose search has status 0 become (du, 0, 0, 0, dv, 0, 0, 0, dw, 0, 0, 0) -- with only_missing only the rows that
    hold a non-finite value; every other row is returned as given."""
    d = np.ascontiguousarray(res["d"], np.int32).reshape(-1, 3)
    m = len(d)
    rec = np.zeros(max(m, 1), SEARCH_DTYPE)
    rec["d"][:m] = d
    rec["status"][:m] = np.asarray(res["status"])
    out = np.full((max(m, 1), 12), np.nan)
    if init is not None:
        ini = np.asarray(init, np.float64).reshape(-1, 12)
        if len(ini) != m:
            raise ValueError("init: one row of 12 per search result")
        out[:m] = ini
    _check(lib().sift3d_icgn_init_from_search(_p(rec), m, int(bool(only_missing)), _p(out)))
    return out[:m].copy()


STRAIN_OPTIONS = ("radius", "min_neighbours", "measure")


def default_strain_options():
    """sift3d_default_strain_options as a dict (needs no GPU)"""
    o = _options(StrainOptions, "sift3d_default_strain_options", STRAIN_OPTIONS, "strain", {})
    return {k: getattr(o, k) for k in STRAIN_OPTIONS}


def strain_input_from_icgn(res, zncc_min=0.0, accept_unconverged=False):
    """sift3d_strain_input_from_icgn: the displacements (m, 3) float64 and the validity bytes (m,) uint8 that strain takes, from the
    dict icgn returns (p, zncc, status): valid where IC-GN converged (or ran out of iterations, with accept_unconverged), zncc >=
    zncc_min and the displacement is finite.  Needs no GPU."""
    p = np.asarray(res["p"], np.float64).reshape(-1, 12)
    m = len(p)
    rec = np.zeros(max(m, 1), ICGN_DTYPE)
    rec["p"][:m] = p
    rec["zncc"][:m] = np.asarray(res["zncc"])
    rec["status"][:m] = np.asarray(res["status"])
    disp = np.zeros((max(m, 1), 3), np.float64)
    valid = np.zeros(max(m, 1), np.uint8)
    _check(lib().sift3d_strain_input_from_icgn(_p(rec), m, float(zncc_min), int(bool(accept_unconverged)), _p(disp), _p(valid)))
    return disp[:m].copy(), valid[:m].copy()


def strain_input_from_icgn2(res, zncc_min=0.0, accept_unconverged=False):
    """sift3d_strain_input_from_icgn2: strain_input_from_icgn for the dict icgn2 returns.  Needs no GPU."""
    p = np.asarray(res["p"], np.float64).reshape(-1, 30)
    m = len(p)
    rec = np.zeros(max(m, 1), ICGN2_DTYPE)
    rec["p"][:m] = p
    rec["zncc"][:m] = np.asarray(res["zncc"])
    rec["status"][:m] = np.asarray(res["status"])
    disp = np.zeros((max(m, 1), 3), np.float64)
    valid = np.zeros(max(m, 1), np.uint8)
    _check(lib().sift3d_strain_input_from_icgn2(_p(rec), m, float(zncc_min), int(bool(accept_unconverged)), _p(disp), _p(valid)))
    return disp[:m].copy(), valid[:m].copy()


def strain(points, disp, valid=None, device=0, label=None, **opts):
    """sift3d_strain: a plane fitted to the displacements ((m, 3) float64 u, v, w) of the POIs ((m, 3) int32 x, y, z) within `radius`
    voxels (Chebyshev) of each POI, and the strain of the fitted gradient.  valid: (m,) bytes or None (all valid).  points / disp /
    valid: numpy arrays or contiguous device tensors, all of the same kind.  Options: radius, min_neighbours, measure (0
    Green-Lagrange, 1 infinitesimal).  label: None, or (m,) int32 body labels (sift3d_strain_labelled: a POI's neighbours are those of
    its own label, which is > 0; what labels_at returns).  Returns disp (m, 3), G (m, 3, 3) (rows u, v, w; columns x, y, z), E (m, 6)
    (xx yy zz xy yz zx), principal (m, 3), equivalent, rms, neighbours, status (m,) and the device seconds."""
    o = _options(StrainOptions, "sift3d_default_strain_options", STRAIN_OPTIONS, "strain", opts)
    dev = [_is_dev(a) for a in (points, disp, valid) if a is not None]
    if any(dev) != all(dev):
        raise ValueError("points, disp and valid must all be numpy arrays or all device tensors")
    qp, m, q = _table(points, np.int32, 3, points)
    up, mu, u = _table(disp, np.float64, 3, points)
    ok = None if valid is None else (valid.ne(0) if dev[0] else np.asarray(valid) != 0)
    vp, mv, ok = _table(ok, np.uint8, 0, points)
    lp, ml, lab = _table(label, np.int32, 0, points)
    if mu != m or (ok is not None and mv != m) or (lab is not None and ml != m):
        raise ValueError("disp, valid, label: one row per point")
    out = np.zeros(max(m, 1), STRAIN_DTYPE)
    sec = C.c_double(0)
    if lab is None:
        _check(lib().sift3d_strain(qp, up, vp, m, C.byref(o), int(dev[0]), int(device), _p(out), C.byref(sec)))
    else:
        _check(lib().sift3d_strain_labelled(qp, up, vp, lp, m, C.byref(o), int(dev[0]), int(device), _p(out), C.byref(sec)))
    d = _fields(out, m, ("disp", "G", "E", "principal", "equivalent", "rms", "neighbours", "status"))
    d["G"] = d["G"].reshape(-1, 3, 3)
    d["seconds"] = sec.value
    return d


VALIDATE_OPTIONS = ("radius", "min_neighbours", "passes", "threshold", "eps")
VALIDATE_FIELDS = ("median", "mad", "score", "neighbours", "status", "flagged", "pass")


def default_validate_options():
    """sift3d_default_validate_options as a dict (needs no GPU)"""
    o = _options(ValidateOptions, "sift3d_default_validate_options", VALIDATE_OPTIONS, "validate", {})
    return {k: getattr(o, k) for k in VALIDATE_OPTIONS}


def validate_stage_capacity():
    """sift3d_validate_stage_capacity (test hook): the neighbour count up to which validate selects its medians in LDS.  Needs no GPU."""
    n = C.c_int(0)
    _check(lib().sift3d_validate_stage_capacity(C.byref(n)))
    return n.value


def validate_input_from_icgn(res, zncc_min=0.0, accept_unconverged=False):
    """sift3d_validate_input_from_icgn / _icgn2 (by the width of res["p"]: 12 or 30): the displacements (m, 3) float64, the gradients
    (m, 9) float64 and the validity bytes (m,) uint8 that validate takes, from the dict icgn or icgn2 returns.  Needs no GPU."""
    p = np.asarray(res["p"], np.float64)
    width = p.shape[-1] if p.ndim == 2 else 12
    if width not in (12, 30):
        raise ValueError("p: (m, 12) first-order or (m, 30) second-order parameters")
    p = p.reshape(-1, width)
    m = len(p)
    rec = np.zeros(max(m, 1), ICGN_DTYPE if width == 12 else ICGN2_DTYPE)
    rec["p"][:m] = p
    rec["zncc"][:m] = np.asarray(res["zncc"])
    rec["status"][:m] = np.asarray(res["status"])
    disp = np.zeros((max(m, 1), 3), np.float64)
    grad = np.zeros((max(m, 1), 9), np.float64)
    valid = np.zeros(max(m, 1), np.uint8)
    fn = lib().sift3d_validate_input_from_icgn if width == 12 else lib().sift3d_validate_input_from_icgn2
    _check(fn(_p(rec), m, float(zncc_min), int(bool(accept_unconverged)), _p(disp), _p(grad), _p(valid)))
    return disp[:m].copy(), grad[:m].copy(), valid[:m].copy()


def validate(points, disp, grad=None, valid=None, device=0, label=None, **opts):
    """sift3d_validate_displacements: the normalised median test of the displacements ((m, 3) float64 u, v, w) of the POIs ((m, 3) int32
    x, y, z) against the POIs within `radius` voxels (Chebyshev) of each.  grad: (m, 9) float64 gradients of the POIs (rows u, v, w;
    columns x, y, z) that carry a neighbour's value to the tested POI, or None; valid: (m,) bytes or None (all valid).  points / disp /
    grad / valid: numpy arrays or contiguous device tensors, all of the same kind.  Options: radius, min_neighbours, passes,
    threshold, eps.  label: None, or (m,) int32 body labels (sift3d_validate_displacements_labelled: a POI's neighbours are those of its
    own label, which is > 0).  Returns median (m, 3), mad (m, 3), score, neighbours, status, flagged, pass (m,), the records themselves as
    `records` (VALIDATE_DTYPE: what validate_keep and icgn_init_from_validation take) and the device seconds."""
    o = _options(ValidateOptions, "sift3d_default_validate_options", VALIDATE_OPTIONS, "validate", opts)
    dev = [_is_dev(a) for a in (points, disp, grad, valid) if a is not None]
    if any(dev) != all(dev):
        raise ValueError("points, disp, grad and valid must all be numpy arrays or all device tensors")
    qp, m, q = _table(points, np.int32, 3, points)
    up, mu, u = _table(disp, np.float64, 3, points)
    gp, mg, gr = _table(grad, np.float64, 9, points)
    ok = None if valid is None else (valid.ne(0) if dev[0] else np.asarray(valid) != 0)
    vp, mv, ok = _table(ok, np.uint8, 0, points)
    lp, ml, lab = _table(label, np.int32, 0, points)
    if mu != m or (gr is not None and mg != m) or (ok is not None and mv != m) or (lab is not None and ml != m):
        raise ValueError("disp, grad, valid, label: one row per point")
    out = np.zeros(max(m, 1), VALIDATE_DTYPE)
    sec = C.c_double(0)
    if lab is None:
        _check(lib().sift3d_validate_displacements(qp, up, gp, vp, m, C.byref(o), int(dev[0]), int(device), _p(out), C.byref(sec)))
    else:
        _check(lib().sift3d_validate_displacements_labelled(qp, up, gp, vp, lp, m, C.byref(o), int(dev[0]), int(device), _p(out),
                                                            C.byref(sec)))
    d = _fields(out, m, VALIDATE_FIELDS)
    d["records"] = out[:m].copy()
    d["seconds"] = sec.value
    return d


def _validate_records(val):
    rec = val["records"] if isinstance(val, dict) else val
    return np.ascontiguousarray(rec, VALIDATE_DTYPE).reshape(-1)


def validate_keep(val, valid=None):
    """sift3d_validate_keep: the bytes (m,) uint8 to hand to strain -- valid (None: all), tested (status 0) and not flagged -- from what
    validate returns (or its records).  Needs no GPU."""
    rec = _validate_records(val)
    m = len(rec)
    vin = None if valid is None else np.ascontiguousarray(np.asarray(valid) != 0, np.uint8).reshape(-1)
    if vin is not None and len(vin) != m:
        raise ValueError("valid: one byte per record")
    buf = np.zeros(max(m, 1), VALIDATE_DTYPE)
    buf[:m] = rec
    out = np.zeros(max(m, 1), np.uint8)
    _check(lib().sift3d_validate_keep(_p(buf), None if vin is None or m == 0 else _p(vin), m, _p(out)))
    return out[:m].copy()


def icgn_init_from_validation(val, init=None):
    """sift3d_icgn_init_from_validation: (m, 12) float64 initial parameters for a second icgn run and the number of rows written.  Rows
    of init (None: all NaN) whose record is flagged with status 0, or has status 3, become (median_u, 0, 0, 0, median_v, 0, 0, 0,
    median_w, 0, 0, 0); every other row is returned as given.  Needs no GPU."""
    rec = _validate_records(val)
    m = len(rec)
    buf = np.zeros(max(m, 1), VALIDATE_DTYPE)
    buf[:m] = rec
    out = np.full((max(m, 1), 12), np.nan)
    if init is not None:
        ini = np.asarray(init, np.float64).reshape(-1, 12)
        if len(ini) != m:
            raise ValueError("init: one row of 12 per record")
        out[:m] = ini
    count = C.c_int(0)
    _check(lib().sift3d_icgn_init_from_validation(_p(buf), m, _p(out), C.byref(count)))
    return out[:m].copy(), count.value


FIELD_OPTIONS = ("radius", "min_neighbours", "weighting", "require_enclosed")
FIELD_FIELDS = ("disp", "G", "rms", "wsum", "neighbours", "sides", "status")


def default_field_options():
    """sift3d_default_field_options as a dict (needs no GPU)"""
    o = _options(FieldOptions, "sift3d_default_field_options", FIELD_OPTIONS, "field", {})
    return {k: getattr(o, k) for k in FIELD_OPTIONS}


def field_eval(points, disp, valid, queries, device=0, label=None, query_label=None, **opts):
    """sift3d_field_eval: the displacement field of the POIs ((m, 3) int32 x, y, z with displacements (m, 3) float64 and validity bytes
    (m,) or None) at the real-valued positions queries ((nq, 3) float64): a plane fitted to the POIs within `radius` voxels (Chebyshev)
    of each query, weighted by the tensor biweight (weighting 1) or uniformly (0).  points / disp / valid / queries: numpy arrays or
    contiguous device tensors, all of the same kind.  Options: radius, min_neighbours, weighting, require_enclosed.  label and
    query_label: both None, or the (m,) and (nq,) int32 body labels of the POIs and of the queries (sift3d_field_eval_labelled: a query's
    members are the POIs of its label, which is > 0).  Returns disp
    (nq, 3), G (nq, 3, 3) (rows u, v, w; columns x, y, z), rms, wsum, neighbours, sides, status (nq,), the records themselves as
    `records` (FIELD_DTYPE: what field_unpack and compose_displacements take) and the device seconds."""
    o = _options(FieldOptions, "sift3d_default_field_options", FIELD_OPTIONS, "field", opts)
    dev = [_is_dev(a) for a in (points, disp, valid, queries) if a is not None]
    if any(dev) != all(dev):
        raise ValueError("points, disp, valid and queries must all be numpy arrays or all device tensors")
    qp, m, q = _table(points, np.int32, 3, points)
    up, mu, u = _table(disp, np.float64, 3, points)
    ok = None if valid is None else (valid.ne(0) if dev[0] else np.asarray(valid) != 0)
    vp, mv, ok = _table(ok, np.uint8, 0, points)
    xp, nq, x = _table(queries, np.float64, 3, points)
    if mu != m or (ok is not None and mv != m):
        raise ValueError("disp, valid: one row per point")
    if (label is None) != (query_label is None):
        raise ValueError("label and query_label: both or neither")
    lp, ml, lab = _table(label, np.int32, 0, points)
    kp, nk, qlab = _table(query_label, np.int32, 0, points)
    if lab is not None and (ml != m or nk != nq):
        raise ValueError("label: one per point; query_label: one per query")
    out = np.zeros(max(nq, 1), FIELD_DTYPE)
    sec = C.c_double(0)
    if lab is None:
        _check(lib().sift3d_field_eval(qp, up, vp, m, xp, nq, C.byref(o), int(dev[0]), int(device), _p(out), C.byref(sec)))
    else:
        _check(lib().sift3d_field_eval_labelled(qp, up, vp, lp, m, xp, kp, nq, C.byref(o), int(dev[0]), int(device), _p(out), C.byref(sec)))
    d = _fields(out, nq, FIELD_FIELDS)
    d["G"] = d["G"].reshape(-1, 3, 3)
    d["records"] = out[:nq].copy()
    d["seconds"] = sec.value
    return d


def _field_records(res):
    rec = res["records"] if isinstance(res, dict) else res
    return np.ascontiguousarray(rec, FIELD_DTYPE).reshape(-1)


def field_queries(points, disp):
    """sift3d_field_queries_from_displacements: the positions (m, 3) float64 the POIs ((m, 3) int32) moved to under disp ((m, 3)
    float64), x = p + u: the queries of the next load step.  Non-finite where disp is.  Needs no GPU."""
    q = np.ascontiguousarray(points, np.int32).reshape(-1, 3)
    u = np.ascontiguousarray(disp, np.float64).reshape(-1, 3)
    if len(u) != len(q):
        raise ValueError("disp: one row per point")
    m = len(q)
    out = np.zeros((max(m, 1), 3), np.float64)
    _check(lib().sift3d_field_queries_from_displacements(_p(q), _p(u), m, _p(out)))
    return out[:m].copy()


def field_unpack(res):
    """sift3d_field_unpack: disp (n, 3), grad (n, 9) float64 and valid (n,) uint8 (status 0) of what field_eval returns (or its
    records).  Needs no GPU."""
    rec = _field_records(res)
    n = len(rec)
    buf = np.zeros(max(n, 1), FIELD_DTYPE)
    buf[:n] = rec
    disp, grad, valid = np.zeros((max(n, 1), 3)), np.zeros((max(n, 1), 9)), np.zeros(max(n, 1), np.uint8)
    _check(lib().sift3d_field_unpack(_p(buf), n, _p(disp), _p(grad), _p(valid)))
    return disp[:n].copy(), grad[:n].copy(), valid[:n].copy()


def compose_displacements(disp_a, grad_a, valid_a, at_b):
    """sift3d_compose_displacements: step A's displacements (m, 3), gradients (m, 9) or None and validity bytes (m,) or None at its
    POIs, and step B's field evaluated where those POIs moved to (what field_eval returned at field_queries(points, disp_a), or its
    records) -> the total in step A's frame: disp (m, 3) = u_A + u_B, grad (m, 9) = G_A + G_B + G_B G_A (None without grad_a) and
    valid (m,) uint8.  Invalid rows are zero.  Needs no GPU."""
    rec = _field_records(at_b)
    m = len(rec)
    ua = np.ascontiguousarray(disp_a, np.float64).reshape(-1, 3)
    ga = None if grad_a is None else np.ascontiguousarray(grad_a, np.float64).reshape(-1, 9)
    va = None if valid_a is None else np.ascontiguousarray(np.asarray(valid_a) != 0, np.uint8).reshape(-1)
    if len(ua) != m or (ga is not None and len(ga) != m) or (va is not None and len(va) != m):
        raise ValueError("disp_a, grad_a, valid_a: one row per record")
    buf = np.zeros(max(m, 1), FIELD_DTYPE)
    buf[:m] = rec
    disp, valid = np.zeros((max(m, 1), 3)), np.zeros(max(m, 1), np.uint8)
    grad = None if ga is None else np.zeros((max(m, 1), 9))
    _check(lib().sift3d_compose_displacements(_p(ua) if m else None, None if ga is None or m == 0 else _p(ga),
                                              None if va is None or m == 0 else _p(va), _p(buf), m, _p(disp),
                                              None if grad is None else _p(grad), _p(valid)))
    return disp[:m].copy(), None if grad is None else grad[:m].copy(), valid[:m].copy()


def icgn_init_from_field(disp, grad=None, valid=None, only_valid=True, init=None):
    """sift3d_icgn_init_from_field: (m, 12) float64 initial parameters of icgn from a measured field and the number of rows written.
    Row i becomes (u, G00, G01, G02, v, G10, ..) of disp (m, 3) and grad ((m, 9), None: zero).  With only_valid only the rows whose
    valid byte is set are written and the others are returned as given in init (None: all NaN).  Needs no GPU."""
    u = np.ascontiguousarray(disp, np.float64).reshape(-1, 3)
    m = len(u)
    g = None if grad is None else np.ascontiguousarray(grad, np.float64).reshape(-1, 9)
    v = None if valid is None else np.ascontiguousarray(np.asarray(valid) != 0, np.uint8).reshape(-1)
    if (g is not None and len(g) != m) or (v is not None and len(v) != m):
        raise ValueError("grad, valid: one row per displacement")
    out = np.full((max(m, 1), 12), np.nan)
    if init is not None:
        ini = np.asarray(init, np.float64).reshape(-1, 12)
        if len(ini) != m:
            raise ValueError("init: one row of 12 per displacement")
        out[:m] = ini
    count = C.c_int(0)
    _check(lib().sift3d_icgn_init_from_field(_p(u) if m else None, None if g is None or m == 0 else _p(g),
                                             None if v is None or m == 0 else _p(v), m, int(bool(only_valid)), _p(out), C.byref(count)))
    return out[:m].copy(), count.value


SUBSET_OPTIONS = ("r_min", "r_max", "criterion", "threshold", "level", "fraction_min")
SUBSET_FIELDS = ("mean", "dR", "G", "eig", "radius", "status", "feasible", "material")


def default_subset_options():
    """sift3d_default_subset_options as a dict (needs no GPU)"""
    o = _options(SubsetOptions, "sift3d_default_subset_options", SUBSET_OPTIONS, "subset", {})
    return {k: getattr(o, k) for k in SUBSET_OPTIONS}


def subset_quality(ref, points, device=0, **opts):
    """sift3d_subset_quality: the texture sums of the subset around each point ((m, 3) int32 x, y, z of ref) and the smallest radius
    of r_min .. r_max whose criterion reaches the threshold.  ref: an (nz, ny, nx) float32 numpy array or a contiguous float32 device
    tensor.  Options: r_min, r_max, criterion (0 min(Gxx, Gyy, Gzz), 1 the smallest eigenvalue of G), threshold, level, fraction_min.
    Returns mean, dR (m,), G (m, 6: xx yy zz xy xz yz), eig (m, 3), radius, status, feasible, material (m,), the records themselves
    (SUBSET_DTYPE, for subset_groups) and the device seconds."""
    o = _options(SubsetOptions, "sift3d_default_subset_options", SUBSET_OPTIONS, "subset", opts)
    on_dev = int(_is_dev(ref))
    rp, r = _volume(ref, "ref", on_dev)
    qp, m, q = _table(points, np.int32, 3, ref)
    out = np.zeros(max(m, 1), SUBSET_DTYPE)
    sec = C.c_double(0)
    _check(lib().sift3d_subset_quality(rp, *r.shape[::-1], qp, m, C.byref(o), on_dev, int(device), _p(out), C.byref(sec)))
    d = _fields(out, m, SUBSET_FIELDS)
    d["records"] = out[:m].copy()
    d["seconds"] = sec.value
    return d


def subset_groups(res, r_min, r_max):
    """sift3d_subset_group_by_radius: the status-0 records of subset_quality's dict (or of a SUBSET_DTYPE array) grouped by radius:
    a list of (radius, indices) for the non-empty groups, radius ascending, indices (int32) ascending -- one icgn call per entry
    with subset_radius = radius on points[indices].  Needs no GPU."""
    if isinstance(res, dict):
        radius, status = np.asarray(res["radius"]), np.asarray(res["status"])
        rec = np.zeros(len(radius), SUBSET_DTYPE)
        rec["radius"], rec["status"] = radius, status
    else:
        rec = np.ascontiguousarray(res, SUBSET_DTYPE)
    m = len(rec)
    buf = np.zeros(max(m, 1), SUBSET_DTYPE)
    buf[:m] = rec
    order = np.zeros(max(m, 1), np.int32)
    offsets = np.zeros(max(int(r_max) - int(r_min) + 2, 2), np.int32)
    count = C.c_int(0)
    _check(lib().sift3d_subset_group_by_radius(_p(buf), m, int(r_min), int(r_max), _p(order), _p(offsets), C.byref(count)))
    return [(int(r_min) + g, order[offsets[g]:offsets[g + 1]].copy()) for g in range(int(r_max) - int(r_min) + 1)
            if offsets[g + 1] > offsets[g]]


def device_count():
    n = C.c_int(0)
    lib().sift3d_device_count(C.byref(n))
    return n.value


class CSIFT3D:
    """Python mirror of CPUSIFT::CSIFT3D over the C-ABI (same method names as the reference class,
    Include/cSIFT3D.h:118-181).  vol is [z, y, x] fp32 (x fastest).  keep_dtype=True: a numpy volume of uint8, int8, uint16 or int16
    goes to the library as it is (sift3d_create_typed: uploaded at its own width, widened on the GPU; the same extractor bit for bit);
    the default converts to float32 on the host.  device_ptr with dtype=: the device volume holds voxels of that dtype."""

    def __init__(self, volume, num_kp_levels=3, sigma_default=1.6, sigma_n_default=1.15, peak_thresh=0.1,
                 max_eig_thres=0.9, corner_thresh=0.4, device=0, device_ptr=None, shape=None, keep_dtype=False, dtype=None):
        L = lib()
        self._h = C.c_void_p()
        p = Params(num_kp_levels, sigma_default, sigma_n_default, peak_thresh, max_eig_thres, corner_thresh)
        self.levels = num_kp_levels
        if device_ptr is not None:
            nz, ny, nx = shape
            self.shape = tuple(shape)
            if dtype is not None:
                _check(L.sift3d_create_typed(C.byref(self._h), C.c_void_p(device_ptr), _dtype_code(dtype), nx, ny, nz, C.byref(p), device, 1))
            else:
                _check(L.sift3d_create(C.byref(self._h), C.c_void_p(device_ptr), nx, ny, nz, C.byref(p), device, 1))
        elif keep_dtype and isinstance(volume, np.ndarray) and volume.dtype.name in DTYPES:  # (float32: SIFT3D_DT_F32, which is sift3d_create)
            vol = np.ascontiguousarray(volume)
            nz, ny, nx = vol.shape
            self.shape = vol.shape
            _check(L.sift3d_create_typed(C.byref(self._h), vol.ctypes.data_as(C.c_void_p), DTYPES[vol.dtype.name], nx, ny, nz, C.byref(p), device, 0))
        else:
            vol = np.ascontiguousarray(volume, dtype=np.float32)
            nz, ny, nx = vol.shape
            self.shape = vol.shape
            _check(L.sift3d_create(C.byref(self._h), vol.ctypes.data_as(C.c_void_p), nx, ny, nz, C.byref(p), device, 0))

    def set_stream(self, stream_handle):
        """every later call enqueues on this hipStream_t (e.g. torch.cuda.Stream().cuda_stream); 0 / None = own stream"""
        _check(lib().sift3d_set_stream(self._h, C.c_void_p(int(stream_handle or 0))))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().sift3d_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- reference API names -------------------------------------------------------------------
    def KpSiftAlgorithm(self):
        _check(lib().sift3d_run(self._h))
        return self

    def KpSiftAlgorithmAsync(self, after=None):
        """enqueue the whole pipeline and return (sift3d_run_async); Wait() -- or any accessor -- completes it.  after = another extractor
        with a run in flight on the same GPU: this pipeline starts when that one's orientation stage has ended (sift3d_run_async_after)"""
        if after is not None:
            _check(lib().sift3d_run_async_after(self._h, after._h))
        else:
            _check(lib().sift3d_run_async(self._h))
        return self

    def Wait(self):
        _check(lib().sift3d_wait(self._h))
        return self

    def run_stages(self, upto):
        _check(lib().sift3d_run_stages(self._h, int(upto)))
        return self

    def GetKeypoints(self, with_desc=True, out=None):
        """out = (kp, desc): arrays of the result's size to fill instead of new ones (the C++ caller's vectors)"""
        n = C.c_int(0)
        _check(lib().sift3d_num_keypoints(self._h, C.byref(n)))
        if out is not None:
            kp, desc = out
            assert kp.dtype == KP_DTYPE and kp.shape == (n.value,) and desc.dtype == np.float32 and desc.shape == (n.value, DESC)
            assert kp.flags.c_contiguous and desc.flags.c_contiguous
        else:
            kp = np.zeros(n.value, KP_DTYPE)
            desc = np.zeros((n.value, DESC), np.float32)
        if n.value:
            _check(lib().sift3d_get_keypoints(self._h, kp.ctypes.data, _f(desc) if with_desc else None))
        return kp, desc

    @property
    def m_timer(self):
        t = (C.c_double * 8)()
        _check(lib().sift3d_stage_times(self._h, t))
        keys = ["d_TotalTime", "d_Allocation", "d_BuildGSS", "d_BuildDOG", "d_Detect", "d_AssignOrientation", "d_Extraction", "d_release"]
        return dict(zip(keys, list(t)))

    # --- checking accessors (GET_GSS / GET_DOG / GET_LEVEL) ---------------------------------------
    @property
    def num_octaves(self):
        n = C.c_int(0)
        _check(lib().sift3d_num_octaves(self._h, C.byref(n)))
        return n.value

    def level_info(self, is_dog, idx):
        d = np.zeros(3, np.int32); u = np.zeros(3, np.float32); s = np.zeros(1, np.float32)
        _check(lib().sift3d_level_info(self._h, int(is_dog), idx, d.ctypes.data_as(_ip), _f(u), _f(s)))
        return tuple(int(v) for v in d), tuple(float(v) for v in u), float(s[0])

    def level(self, is_dog, idx):
        (nx, ny, nz), _, _ = self.level_info(is_dog, idx)
        out = np.empty((nz, ny, nx), np.float32)
        _check(lib().sift3d_copy_level(self._h, int(is_dog), idx, _f(out)))
        return out

    def gss(self, octave, i):
        return self.level(0, octave * (self.levels + 3) + i)

    def dog(self, octave, i):
        return self.level(1, octave * (self.levels + 2) + i)

    def input(self):
        out = np.empty(self.shape, np.float32)
        _check(lib().sift3d_copy_input(self._h, _f(out)))
        return out

    def extrema(self):
        n = C.c_int(0)
        _check(lib().sift3d_num_extrema(self._h, C.byref(n)))
        out = np.zeros(n.value, KP_DTYPE)
        if n.value:
            _check(lib().sift3d_get_extrema(self._h, out.ctypes.data))
        return out

    def orientation_codes(self):
        n = C.c_int(0)
        _check(lib().sift3d_num_extrema(self._h, C.byref(n)))
        out = np.zeros(n.value, np.int32)
        if n.value:
            _check(lib().sift3d_get_orientation_codes(self._h, out.ctypes.data_as(_ip)))
        return out

    def device_results(self):
        d = C.c_void_p(); x = C.c_void_p(); n = C.c_int(0)
        _check(lib().sift3d_device_results(self._h, C.byref(d), C.byref(x), C.byref(n)))
        return d.value, x.value, n.value

    def export_device(self, desc_ptr, xyz_ptr=None):
        """D2D copy of the results into caller-owned device buffers (n*768, n*3 floats)"""
        _check(lib().sift3d_export_device(self._h, C.c_void_p(int(desc_ptr)), C.c_void_p(int(xyz_ptr)) if xyz_ptr else None))

    # --- detection options (no reference counterpart; include/sift3d_hip.h, sift3d_set_detect_options) -----------------------
    def set_detect_options(self, neighbours=8, refine=False, max_offset=0.5, contrast_thresh=0.0, edge_ratio=0.0):
        """the extremum rule of the next run: neighbours 8 (the reference's, default) or 80; refine: sub-voxel quadratic fit with its
        rejection tests.  Raises Sift3dError on a refusal (bad values, a run in flight, a slab / seeded handle)."""
        o = DetectOptions(int(neighbours), int(refine), float(max_offset), float(contrast_thresh), float(edge_ratio))
        _check(lib().sift3d_set_detect_options(self._h, C.byref(o)))
        return self

    def detect_options(self):
        o = DetectOptions()
        _check(lib().sift3d_get_detect_options(self._h, C.byref(o)))
        return _options_dict(o)

    def refined(self):
        """REFINED_DTYPE records of the last run's keypoints, GetKeypoints() order (the run must have had refine on)"""
        n = C.c_int(0)
        _check(lib().sift3d_num_keypoints(self._h, C.byref(n)))
        out = np.zeros(max(n.value, 1), REFINED_DTYPE)  # (the call checks its state even for zero keypoints)
        _check(lib().sift3d_get_refined(self._h, out.ctypes.data))
        return out[:n.value]

    def debug_counters(self):
        """{list_regrows, desc_second_passes, match_exact_rows}: how often the rare paths ran (sift3d_debug_counters)"""
        a = (C.c_int * 4)()
        _check(lib().sift3d_debug_counters(self._h, a))
        return {"list_regrows": a[0], "desc_second_passes": a[1], "match_exact_rows": a[2]}

    def run_plan(self):
        """the schedule of the last prepared run (sift3d_test_run_plan, layout: include/sift3d_hip_test.h): a dict of the run's values and
        "octaves", one (head stream, tail stream, tail_moved, prio, head_slots, tail_slots) per octave; stream -1 = the chain stream"""
        a = (C.c_int * 256)()
        n = C.c_int(0)
        _check(lib().sift3d_test_run_plan(self._h, a, 256, C.byref(n)))
        keys = ["noct", "small_first", "chain", "small_hwp", "small_build_mask", "small_dog_mask", "dog_elide", "g_last_elide", "run_full",
                "run_refine", "det_two", "det_early", "det_rest_stream", "det_rest_own", "emit"]
        out = dict(zip(keys, a[:15]))
        out["octaves"] = [tuple(a[15 + 6 * o:21 + 6 * o]) for o in range(out["noct"])]
        return out


def _params(kw):
    return Params(kw.get("num_kp_levels", 3), kw.get("sigma_default", 1.6), kw.get("sigma_n_default", 1.15),
                  kw.get("peak_thresh", 0.1), kw.get("max_eig_thres", 0.9), kw.get("corner_thresh", 0.4))


def slab_min_halo(**kw):
    p = _params(kw); h = C.c_int(0)
    _check(lib().sift3d_slab_min_halo(C.byref(p), C.byref(h)))
    return h.value


def slab_admits(nx, ny, nz, first_octave=True, **kw):
    """can slab contexts hold an octave of these GLOBAL dims with these parameters (sift3d_slab_admits)?"""
    p = _params(kw); ok = C.c_int(0)
    lib().sift3d_slab_admits.argtypes = [C.POINTER(Params), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    _check(lib().sift3d_slab_admits(C.byref(p), int(nx), int(ny), int(nz), int(bool(first_octave)), C.byref(ok)))
    return bool(ok.value)


def slab_min_halo_partial(**kw):
    """planes per side a slab's level buffers need when the descriptor windows are split along z over the ranks (r05)"""
    p = _params(kw); h = C.c_int(0)
    _check(lib().sift3d_slab_min_halo_partial(C.byref(p), C.byref(h)))
    return h.value


def slab_record_words():
    """int32 words of one keypoint record of the partial-window exchange (opaque to the driver)"""
    n = C.c_int(0)
    _check(lib().sift3d_slab_record_bytes(C.byref(n)))
    assert n.value % 4 == 0
    return n.value // 4


class SeededCSIFT3D(CSIFT3D):
    """Octaves octave_base.. of a volume whose G[octave_base][0] the caller provides (multi-GPU tail, see slab.py).
    shape = (nz, ny, nx) of that level."""

    def __init__(self, shape, octave_base, noct_total, device=0, **kw):
        self._h = C.c_void_p()
        p = _params(kw)
        self.levels = p.num_kp_levels
        self.shape = tuple(shape)
        nz, ny, nx = shape
        _check(lib().sift3d_create_seeded(C.byref(self._h), nx, ny, nz, octave_base, noct_total, C.byref(p), device))

    def seed(self, ptr, on_device=True):
        _check(lib().sift3d_seed_upload(self._h, C.c_void_p(int(ptr)), int(bool(on_device))))

    def seed_host(self, vol):
        vol = np.ascontiguousarray(vol, np.float32)
        _check(lib().sift3d_seed_upload(self._h, vol.ctypes.data_as(C.c_void_p), 0))

    def set_partition(self, rank, world):
        _check(lib().sift3d_set_describe_partition(self._h, rank, world))

    def run_partial_orientation(self):
        _check(lib().sift3d_run_partial_orientation(self._h))

    def export_orientation(self, ptr):
        _check(lib().sift3d_export_orientation_device(self._h, C.c_void_p(int(ptr))))

    def import_orientation(self, ptr):
        _check(lib().sift3d_import_orientation_device(self._h, C.c_void_p(int(ptr))))

    def run_describe(self):
        _check(lib().sift3d_run_describe(self._h))

    def num_extrema(self):
        n = C.c_int(0)
        _check(lib().sift3d_num_extrema(self._h, C.byref(n)))
        return n.value

    def import_descriptors(self, desc_ptr):
        _check(lib().sift3d_import_descriptors_device(self._h, C.c_void_p(int(desc_ptr))))


class SlabCSIFT3D(CSIFT3D):
    """One z-slab of octave 0 (include/sift3d_hip.h, multi-GPU section).  The level buffers live in `arena_ptr`
    (caller-owned device memory of arena_floats(...) floats) so the caller's communication layer can address halo planes."""

    @staticmethod
    def arena_floats(nx, ny, nz, z0, z1, halo, noct_total, octave=0, **kw):
        d = SlabDesc(nx, ny, nz, z0, z1, halo, noct_total, octave); p = _params(kw); n = C.c_size_t(0)
        _check(lib().sift3d_slab_arena_floats(C.byref(d), C.byref(p), C.byref(n)))
        return n.value

    def __init__(self, nx, ny, nz, z0, z1, halo, noct_total, arena_ptr, arena_floats, device=0, octave=0, **kw):
        self._h = C.c_void_p()
        p = _params(kw)
        self.levels = p.num_kp_levels
        self.dims = (nx, ny, nz)
        self.z0, self.z1, self.halo = z0, z1, halo
        self.shape = (z1 - z0 + 2 * halo, ny, nx)
        self.octave = octave
        d = SlabDesc(nx, ny, nz, z0, z1, halo, noct_total, octave)
        _check(lib().sift3d_slab_create(C.byref(self._h), C.byref(d), C.byref(p), device, C.c_void_p(int(arena_ptr)), arena_floats))

    def buffer(self, kind, idx=0):
        """(offset in floats inside the arena, planes held, global z of plane 0); kind 0 input, 1 GSS, 2 DoG"""
        off = C.c_size_t(0); pl = C.c_int(0); zo = C.c_int(0)
        _check(lib().sift3d_slab_buffer(self._h, kind, idx, C.byref(off), C.byref(pl), C.byref(zo)))
        return off.value, pl.value, zo.value

    def held_level(self, is_dog, idx):
        """all planes the buffer holds, [planes, ny, nx]; plane k is global plane (z0 - halo) + k"""
        out = np.empty(self.shape, np.float32)
        _check(lib().sift3d_copy_level(self._h, int(is_dog), idx, _f(out)))
        return out

    def upload(self, planes, zg0, zg1, device_ptr=None):
        if device_ptr is not None:
            _check(lib().sift3d_slab_upload(self._h, C.c_void_p(int(device_ptr)), zg0, zg1, 1))
        else:
            a = np.ascontiguousarray(planes, np.float32)
            assert a.shape == (zg1 - zg0, self.dims[1], self.dims[0])
            _check(lib().sift3d_slab_upload(self._h, a.ctypes.data_as(C.c_void_p), zg0, zg1, 0))

    def input_absmax(self):
        m = C.c_float(0)
        _check(lib().sift3d_slab_input_absmax(self._h, C.byref(m)))
        return m.value

    def input_scale(self, gmax):
        _check(lib().sift3d_slab_input_scale(self._h, C.c_float(gmax)))

    def level_async(self, i):
        _check(lib().sift3d_slab_level(self._h, i))

    def level_hw(self, i):
        n = C.c_int(0)
        _check(lib().sift3d_slab_level_hw(self._h, i, C.byref(n)))
        return n.value

    def halo_planes(self, i):
        n = C.c_int(0)
        _check(lib().sift3d_slab_halo_planes(self._h, i, C.byref(n)))
        return n.value

    def sync(self):
        _check(lib().sift3d_slab_sync(self._h))

    def get_dogmax(self):
        a = np.zeros(8, np.float32)
        _check(lib().sift3d_slab_get_dogmax(self._h, _f(a)))
        return a[: self.levels + 2].copy()

    def set_dogmax(self, a):
        b = np.zeros(8, np.float32); b[: self.levels + 2] = a
        _check(lib().sift3d_slab_set_dogmax(self._h, _f(b)))

    def detect(self):
        _check(lib().sift3d_slab_detect(self._h))

    def describe(self):
        _check(lib().sift3d_slab_describe(self._h))

    # ---- r05: descriptor windows split along z over the ranks (include/sift3d_hip.h) ----
    def set_desc_partial(self, on=True):
        _check(lib().sift3d_slab_set_desc_partial(self._h, int(bool(on))))

    def desc_reach(self):
        n = C.c_int(0)
        _check(lib().sift3d_slab_desc_reach(self._h, C.byref(n)))
        return n.value

    def orient(self):
        """orientation of the owned extrema -> number of accepted keypoints"""
        _check(lib().sift3d_slab_orient(self._h))
        n = C.c_int(0)
        _check(lib().sift3d_num_keypoints(self._h, C.byref(n)))
        return n.value

    def export_records(self, dst_ptr):
        _check(lib().sift3d_slab_export_records(self._h, C.c_void_p(int(dst_ptr))))

    def describe_partial(self, lists):
        """lists: [(records ptr, n, units ptr or None, hist ptr, mass ptr, owner z0, owner z1), ...] -- one launch (include/sift3d_hip.h)"""
        k = len(lists)
        if not k:
            return
        vp = C.c_void_p * k
        ia = C.c_int * k
        recs = vp(*[C.c_void_p(int(t[0])) if t[1] else None for t in lists])
        ns = ia(*[int(t[1]) for t in lists])
        units = vp(*[C.c_void_p(int(t[2])) if t[2] else None for t in lists])
        hist = vp(*[C.c_void_p(int(t[3])) if t[1] else None for t in lists])
        mass = vp(*[C.c_void_p(int(t[4])) if t[1] else None for t in lists])
        z0 = ia(*[int(t[5]) for t in lists]); z1 = ia(*[int(t[6]) for t in lists])
        _check(lib().sift3d_slab_describe_partial(self._h, k, recs, ns, units, hist, mass, z0, z1))

    def describe_finish(self, rec_ptr, n, parts, units_ptr=None, final_round=False, redo_ptr=None, units_next_ptr=None):
        """parts: [(hist ptr, mass ptr), ...] of the n records, ascending rank -> records flagged for the second round"""
        k = C.c_int(0)
        vp = C.c_void_p * max(1, len(parts))
        hs = vp(*[C.c_void_p(int(h)) for h, _ in parts]) if parts else vp()
        ms = vp(*[C.c_void_p(int(m)) for _, m in parts]) if parts else vp()
        _check(lib().sift3d_slab_describe_finish(self._h, C.c_void_p(int(rec_ptr)) if n else None, int(n), len(parts), hs, ms,
                                                 C.c_void_p(int(units_ptr)) if units_ptr else None, int(bool(final_round)),
                                                 C.c_void_p(int(redo_ptr)) if redo_ptr else None,
                                                 C.c_void_p(int(units_next_ptr)) if units_next_ptr else None, C.byref(k)))
        return k.value

    def orient_launch(self):
        _check(lib().sift3d_slab_orient_launch(self._h))

    def orient_count(self):
        n = C.c_int(0)
        _check(lib().sift3d_slab_orient_count(self._h, C.byref(n)))
        return n.value

    def decimate(self, dst_ptr, wait=True):
        fn = lib().sift3d_slab_decimate if wait else lib().sift3d_slab_decimate_async
        _check(fn(self._h, C.c_void_p(int(dst_ptr))))

    def export_dogmax(self, dst_ptr):
        _check(lib().sift3d_slab_export_dogmax_device(self._h, C.c_void_p(int(dst_ptr))))

    def import_dogmax(self, src_ptr):
        _check(lib().sift3d_slab_import_dogmax_device(self._h, C.c_void_p(int(src_ptr))))


class ShardedCSIFT3D:
    """One host volume [z, y, x] sharded as z-slabs by the library's native driver (csrc/sharded.hip): `devices` = one rank per GPU
    over RCCL, or sim_ranks = n ranks simulated on devices[0].  partial_windows: descriptor windows split along z over the ranks
    (sift3d_sharded_create_ex, SIFT3D_SHARDED_PARTIAL_WINDOWS) instead of whole windows on wide halos."""

    def __init__(self, volume, devices=(0,), sim_ranks=0, sharded_octaves=0, partial_windows=None, transport="rccl", ghost_octave0=False, **kw):
        """partial_windows: None = the driver's rule (descriptor windows split along z unless a slab is too thin for that), True = split or
        refuse, False = whole windows on the wide halos.  transport: "rccl" (one rank per device) or "copies" (SIFT3D_SHARDED_COPY_TRANSPORT:
        event + device / peer copies; `devices` may repeat a device -- rank threads sharing one GPU)"""
        vol = np.ascontiguousarray(volume, np.float32)
        assert vol.ndim == 3
        nz, ny, nx = vol.shape
        self._h = C.c_void_p()
        p = _params(kw)
        devs = (C.c_int * len(devices))(*devices)
        flags = 0 if partial_windows is None else (SHARDED_PARTIAL_WINDOWS if partial_windows else SHARDED_WHOLE_WINDOWS)
        assert transport in ("rccl", "copies")
        if transport == "copies":
            flags |= SHARDED_COPY_TRANSPORT
        if ghost_octave0:   # SIFT3D_SHARDED_GHOST_OCTAVE0: octave 0 recomputed on ghost planes instead of exchanged level by level
            flags |= SHARDED_GHOST_OCTAVE0
        _check(lib().sift3d_sharded_create_ex(C.byref(self._h), vol.ctypes.data_as(C.c_void_p), nx, ny, nz, C.byref(p), devs, len(devices),
                                              int(sim_ranks), int(sharded_octaves), flags))

    def KpSiftAlgorithm(self):
        rc = lib().sift3d_sharded_run(self._h)
        if rc:
            raise Sift3dError(f"{lib().sift3d_error_string(rc).decode()}: {lib().sift3d_sharded_error(self._h).decode()}")
        return self

    def GetKeypoints(self):
        n = C.c_int(0)
        _check(lib().sift3d_sharded_num_keypoints(self._h, C.byref(n)))
        kp = np.zeros(n.value, KP_DTYPE); desc = np.zeros((n.value, DESC), np.float32)
        if n.value:
            _check(lib().sift3d_sharded_get_keypoints(self._h, kp.ctypes.data, _f(desc)))
        return kp, desc

    def info(self):
        w = C.c_int(0); s = C.c_int(0); h = C.c_int(0); t = (C.c_double * 2)()
        _check(lib().sift3d_sharded_info(self._h, C.byref(w), C.byref(s), C.byref(h), t))
        pw = C.c_int(0); tr = C.c_int(0); pl = (C.c_int * max(1, w.value))(); sp = (C.c_int * max(1, s.value))()
        _check(lib().sift3d_sharded_plan(self._h, C.byref(pw), C.byref(tr), pl, sp))
        return {"world": w.value, "sharded_octaves": s.value, "halo": h.value, "seconds": t[0], "seconds_incl_merge": t[1],
                "partial_windows": bool(pw.value), "stage_partial": [bool(v) for v in sp][:s.value], "tail_rank": tr.value, "planes": [int(v) for v in pl][:w.value]}

    def traffic(self):
        """bytes every rank receives per step: (plane halos, records + partial histograms of the last run)"""
        w = self.info()["world"]
        a = (C.c_double * w)(); b = (C.c_double * w)()
        lib().sift3d_sharded_traffic.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _check(lib().sift3d_sharded_traffic(self._h, a, b))
        return [float(v) for v in a], [float(v) for v in b]

    def time_rank(self, rank):
        """simulated ranks, after a run: the GPU time (s) of one rank's whole step, re-run alone (sift3d_test_sharded_time_rank)"""
        t = C.c_double(0)
        lib().sift3d_test_sharded_time_rank.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        rc = lib().sift3d_test_sharded_time_rank(self._h, int(rank), C.byref(t))
        if rc:
            raise Sift3dError(f"{lib().sift3d_error_string(rc).decode()}: {lib().sift3d_last_error().decode()}")
        return t.value

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().sift3d_sharded_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def CreateCSIFT3D(volume, **kw):
    """CSIFT3DFactory::CreateCSIFT3D (Include/cSIFT3D.h:184-194)."""
    return CSIFT3D(volume, **kw)


def gaussian_smooth(vol, sigma, device=0):
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    nz, ny, nx = vol.shape
    out = np.empty_like(vol)
    _check(lib().sift3d_gaussian_smooth(_f(vol), nx, ny, nz, float(sigma), _f(out), device))
    return out


def downsample(vol, out_shape=None, device=0):
    """DownSample_3D (Include/cSIFT3D.h:210): out(k, m, n) = vol(2k, 2m, 2n); out_shape defaults to the halves (rounded down)."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    snz, sny, snx = vol.shape
    nz, ny, nx = out_shape if out_shape is not None else (snz // 2, sny // 2, snx // 2)
    out = np.empty((nz, ny, nx), np.float32)
    _check(lib().sift3d_downsample(_f(vol), snx, sny, snz, _f(out), nx, ny, nz, device))
    return out


def dog_sub(prev, cur, device=0):
    """Sub (Include/cSIFT3D.h:218): (cur - prev) * (-1)."""
    prev = np.ascontiguousarray(prev, dtype=np.float32); cur = np.ascontiguousarray(cur, dtype=np.float32)
    assert prev.shape == cur.shape
    out = np.empty_like(prev)
    _check(lib().sift3d_dog_sub(_f(prev), _f(cur), prev.size, _f(out), device))
    return out


def conv_axis(vol, dim, weight, device=0):
    """GaussianSmooth_3D_Imp (Include/cSIFT3D.h:214): one pass along dim (0 x, 1 y, 2 z) with the caller's taps."""
    vol = np.ascontiguousarray(vol, dtype=np.float32); w = np.ascontiguousarray(weight, dtype=np.float32)
    nz, ny, nx = vol.shape
    out = np.empty_like(vol)
    _check(lib().sift3d_conv_axis(_f(vol), nx, ny, nz, int(dim), _f(w), int(w.size), _f(out), device))
    return out


def orient_keypoint(level, unit, kp, sigma, max_eig_ratio=0.9, corner_thresh=0.4, device=0):
    """Assign_Orientation_Imp (Include/cSIFT3D.h:224) for ONE keypoint record (a KP_DTYPE scalar array of shape (1,), updated in place)
    on a host level [z, y, x]; returns the reference's code."""
    level = np.ascontiguousarray(level, dtype=np.float32)
    nz, ny, nx = level.shape
    assert kp.dtype == KP_DTYPE and kp.shape == (1,) and kp.flags.c_contiguous
    code = C.c_int(0)
    _check(lib().sift3d_orient_keypoint(_f(level), nx, ny, nz, float(unit), kp.ctypes.data_as(C.c_void_p), float(sigma), float(max_eig_ratio),
                                        float(corner_thresh), device, C.byref(code)))
    return code.value


def describe_keypoint(level, unit, kp, device=0):
    """Extract_Descriptor_Imp (Include/cSIFT3D.h:228) for ONE keypoint record (shape (1,), Rotation transposed in place); returns desc[768]."""
    level = np.ascontiguousarray(level, dtype=np.float32)
    nz, ny, nx = level.shape
    assert kp.dtype == KP_DTYPE and kp.shape == (1,) and kp.flags.c_contiguous
    desc = np.zeros(DESC, np.float32)
    _check(lib().sift3d_describe_keypoint(_f(level), nx, ny, nz, float(unit), kp.ctypes.data_as(C.c_void_p), _f(desc), device))
    return desc


def describe_keypoint_second_passes():
    """second passes (0 or 1) of this thread's last describe_keypoint: the first fixed-point unit failed and the window was repeated"""
    a = (C.c_int * 4)()
    _check(lib().sift3d_debug_counters(None, a))
    return a[3]


class muBruteMatcher:
    """Python mirror of CPUSIFT::muBruteMatcher (Include/cMatcher.h:12-88)."""

    MODES = {"inject": 1, "biject": 2, "enhanced": 3}

    def __init__(self, device=0):
        self.device = device
        self.totalTime = 0.0   # device time of the last call (HIP events on the matcher's stream)
        self.wallTime = 0.0    # host clock around the last call
        self.exact_rows = 0    # rows the near-tie guard re-scored exactly in the last call
        self._last = None
        if device_count() > 0:
            lib().sift3d_match_warmup(int(device))   # (like the C++ shell's constructor; failures surface in the first call)

    def _match(self, ref_desc, ref_xyz, tar_desc, tar_xyz, thresHold, mode, on_device=False, n=None, m=None):
        L = lib()
        if on_device:
            pa, px, pb, py = (C.c_void_p(int(v)) for v in (ref_desc, ref_xyz, tar_desc, tar_xyz))
        else:
            a = np.ascontiguousarray(ref_desc, np.float32); b = np.ascontiguousarray(tar_desc, np.float32)
            ax = np.ascontiguousarray(ref_xyz, np.float32); bx = np.ascontiguousarray(tar_xyz, np.float32)
            n, m = a.shape[0], b.shape[0]
            pa, px, pb, py = (v.ctypes.data_as(C.c_void_p) for v in (a, ax, b, bx))
        nn = max(n, 1)
        gi = np.zeros(nn, np.int32); si = np.zeros(nn, np.int32)
        gd = np.zeros(nn, np.float32); sd = np.zeros(nn, np.float32)
        pairs = np.zeros((nn, 6), np.float32)
        k = C.c_int(0); sec = C.c_double(0)
        _check(L.sift3d_match(pa, px, n, pb, py, m, float(thresHold), int(mode), int(bool(on_device)), self.device,
                              gi.ctypes.data_as(_ip), si.ctypes.data_as(_ip), _f(gd), _f(sd), _f(pairs), C.byref(k), C.byref(sec)))
        self.totalTime = sec.value
        dv = C.c_double(0); wl = C.c_double(0)
        L.sift3d_match_times(C.byref(dv), C.byref(wl))
        self.wallTime = wl.value
        a = (C.c_int * 4)()
        L.sift3d_debug_counters(None, a)
        self.exact_rows = a[2]
        self._last = dict(gIdx=gi[:n], sIdx=si[:n], gDist=gd[:n], sDist=sd[:n], pairs=pairs[:k.value].copy())
        return self._last

    def matchExtractors(self, ref, tar, thresHold=0.85, mode="enhanced"):
        """sift3d_match_handles: the device-resident results of two CSIFT3D objects, wherever they live (peer copy across GPUs)"""
        n = max(len(ref.GetKeypoints(with_desc=False)[0]), 1)
        gi = np.zeros(n, np.int32); si = np.zeros(n, np.int32); gd = np.zeros(n, np.float32); sd = np.zeros(n, np.float32)
        pairs = np.zeros((n, 6), np.float32); k = C.c_int(0); sec = C.c_double(0)
        _check(lib().sift3d_match_handles(ref._h, tar._h, float(thresHold), self.MODES[mode], gi.ctypes.data_as(_ip), si.ctypes.data_as(_ip),
                                          _f(gd), _f(sd), _f(pairs), C.byref(k), C.byref(sec)))
        self.totalTime = sec.value
        nk = len(ref.GetKeypoints(with_desc=False)[0])
        self._last = dict(gIdx=gi[:nk], sIdx=si[:nk], gDist=gd[:nk], sDist=sd[:nk], pairs=pairs[:k.value].copy())
        return self._last

    def injectMatch(self, ref_desc, ref_xyz, tar_desc, tar_xyz, thresHold=0.85, **kw):
        return self._match(ref_desc, ref_xyz, tar_desc, tar_xyz, thresHold, 1, **kw)

    def bijectMatch(self, ref_desc, ref_xyz, tar_desc, tar_xyz, thresHold=0.85, **kw):
        return self._match(ref_desc, ref_xyz, tar_desc, tar_xyz, thresHold, 2, **kw)

    def enhancedMatch(self, ref_desc, ref_xyz, tar_desc, tar_xyz, thresHold=0.85, **kw):
        return self._match(ref_desc, ref_xyz, tar_desc, tar_xyz, thresHold, 3, **kw)

    def getCalculationTime(self):
        return self.totalTime

    def getGlodenIdx(self):
        return self._last["gIdx"]

    def getSilverIdx(self):
        return self._last["sIdx"]

    def getGlodenDistSquare(self):
        return self._last["gDist"]

    def getSilverDistSquare(self):
        return self._last["sDist"]
