"""ctypes binding of include/uda_hip.h (csrc/libuda_hip.so).

The structures below mirror the header field for field; `tests/test_capi_symbols.py`
checks that every function the header declares is exported by the library and that the
structure sizes agree with the C side's.  The product path has no CPU fallback: when the
library (or a GPU) is missing, loading / creating fails loudly.
"""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.environ.get("UDA_LIB") or os.path.join(CSRC, "libuda_hip.so")   # UDA_LIB: an alternative build for A/B runs
HEADER = os.path.join(os.path.dirname(HERE), "include", "uda_hip.h")

UDA_ABI_VERSION = 5
MAX_LEVELS = 8
MAX_FUSE = 3

OP_STEM, OP_PW, OP_DW, OP_SE, OP_FUSE, OP_POOL, OP_MBX, OP_SEP = 1, 2, 3, 4, 5, 6, 7, 8
ACT_NONE, ACT_SWISH, ACT_RELU, ACT_RELU6, ACT_HSWISH, ACT_MISH = 0, 1, 2, 3, 4, 5
RS_NONE, RS_NEAREST_UP, RS_MAXPOOL = 0, 1, 2
DECODE_PLAIN, DECODE_LNORM, DECODE_FALSEDEC, DECODE_SAMPLE = 0, 1, 2, 3
POST_GLOBAL, POST_PER_CLASS = 0, 1
CALIB_TS_ALL, CALIB_TS_PERCOO, CALIB_ISO_ALL, CALIB_ISO_PERCOO, CALIB_ISO_PERCLSCOO = 0, 1, 2, 3, 4
CLS_TS, CLS_ISO_ALL, CLS_ISO_PERCLS = 0, 1, 2
ASSIGN_IOU, ASSIGN_MSE, ASSIGN_RANK = 0, 1, 2
ASSIGN_KEEP_VALIDATE, ASSIGN_KEEP_CALIBRATE = 0, 1
SCORE_ENTROPY, SCORE_DET_SCORE, SCORE_ALBOX, SCORE_MCBOX, SCORE_MCCLASS = 0, 1, 2, 3, 4
SCORE_SCALAR, SCORE_MEAN, SCORE_REL_MEAN = 0, 1, 2
SCORE_MAX_COMP = 3
PROF_AGGREGATE, PROF_NMS, PROF_PREPROCESS, PROF_SCORE, PROF_EVAL, PROF_PSEUDO = 16, 17, 18, 19, 20, 21
EVAL_MAX_GT, EVAL_MAX_THRS = 256, 32
THR_MAX_N, THR_MAX_U, THR_MAX_THRS, THR_MAX_P, THR_MAX_G = 262144, 4, 32, 65536, 8192
THR_REPORT_MAX_S, THR_REPORT_MAX_SEGS = 8, 16384
HEAT_TILE_H, HEAT_TILE_W, HEAT_CHUNK = 32, 64, 256
HEAT_MAX_MAPS, HEAT_MAX_RECTS, HEAT_MAX_VALUES, HEAT_MAX_SELS, HEAT_MAX_PIXELS = 16, 4, 16, 8, 4194304
PRUNE_ROWS, PRUNE_COLS, PRUNE_MAX_N, PRUNE_MAX_W = 256, 512, 1048576, 4
KNN_ROWS, KNN_COLS, KNN_MAX_D, KNN_MAX_N, KNN_MAX_B, KNN_MAX_PAIRS = 256, 512, 4, 1048576, 4096, 1 << 38
KDE_POINTS, KDE_RUN, KDE_MAX_D, KDE_MAX_N, KDE_MAX_B, KDE_MAX_PAIRS = 256, 256, 4, 1048576, 4096, 1 << 36
LC_MD, LC_MISTAKES, LC_NOISY = 1, 2, 4
LC_MD_EQ, LC_MD_LE = 0, 1
LC_GT_MISTAKE, LC_GT_NOISY, LC_GT_REPLACED = 1, 2, 4
LC_DET_KEPT, LC_DET_MISSING = 1, 2
LC_MAX_M, LC_MAX_G = 4096, 16384
AUDIT_DET_EXTRA, AUDIT_GT_NOMATCH = 1, 1
AUDIT_MAX_G, AUDIT_MAX_D, AUDIT_MAX_B = 1024, 1024, 1048576
REPORT_ROWS, REPORT_MAX_K, REPORT_MAX_L, REPORT_MAX_B, REPORT_MAX_ROWS = 256, 16, 128, 4096, 1 << 22
CLASSREP_ROWS, CLASSREP_MAX_B, CLASSREP_MAX_M, CLASSREP_MAX_C, CLASSREP_MAX_E, CLASSREP_MAX_ROWS = 256, 4096, 8, 128, 64, 1 << 22
RESAMPLE_TILE, RESAMPLE_MAX_SIDE, RESAMPLE_MAX_SCRATCH = 32, 65536, 1 << 34
FILTER_LANCZOS, FILTER_BICUBIC = 1, 3
PHASH_PRE_W, PHASH_PRE_H, PHASH_SIDE, PHASH_LOW, PHASH_MAX_BYTES = 512, 256, 32, 8, 1 << 32
AUGMENT_TILE, AUGMENT_ROWS, BLUR_MAX_RADIUS, BLUR_MAX_BOX = 32, 8, 16.0, 15


class BufDesc(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("per_sample", C.c_int32),
                ("offset", C.c_int64), ("kind", C.c_int32), ("level", C.c_int32)]


class Op(C.Structure):
    _fields_ = [("kind", C.c_int32), ("in_", C.c_int32 * MAX_FUSE), ("out", C.c_int32),
                ("se_scale", C.c_int32), ("se_partial", C.c_int32), ("residual", C.c_int32),
                ("k", C.c_int32), ("stride", C.c_int32), ("act", C.c_int32),
                ("w_off", C.c_int64), ("bias_off", C.c_int64), ("bn_scale_off", C.c_int64),
                ("bn_shift_off", C.c_int64), ("se_w1_off", C.c_int64), ("se_b1_off", C.c_int64),
                ("se_w2_off", C.c_int64), ("se_b2_off", C.c_int64), ("se_mid", C.c_int32),
                ("drop_site", C.c_int32), ("resample", C.c_int32 * MAX_FUSE),
                ("fuse_w", C.c_float * MAX_FUSE), ("n_in", C.c_int32), ("drop_site2", C.c_int32),
                ("w2_off", C.c_int64), ("bn2_scale_off", C.c_int64), ("bn2_shift_off", C.c_int64),
                ("launch_group", C.c_int32), ("fuse_in", C.c_int32), ("fuse_act", C.c_int32)]


class DropSite(C.Structure):
    _fields_ = [("channels", C.c_int32), ("rate", C.c_float)]


class Model(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("image_h", C.c_int32), ("image_w", C.c_int32),
                ("mean_rgb", C.c_float * 3), ("stddev_rgb", C.c_float * 3),
                ("num_levels", C.c_int32), ("level_h", C.c_int32 * MAX_LEVELS),
                ("level_w", C.c_int32 * MAX_LEVELS), ("anchors_per_loc", C.c_int32),
                ("num_classes", C.c_int32), ("loss_attenuation", C.c_int32),
                ("mc_samples", C.c_int32), ("cls_stacked", C.c_int32), ("box_stacked", C.c_int32),
                ("has_uncert", C.c_int32), ("decode_method", C.c_int32),
                ("enable_softmax", C.c_int32), ("nms_soft_sigma", C.c_float),
                ("nms_iou_thresh", C.c_float), ("nms_score_thresh", C.c_float),
                ("max_output_size", C.c_int32), ("max_nms_inputs", C.c_int32),
                ("post_mode", C.c_int32), ("chunk_images", C.c_int32), ("max_images", C.c_int32),
                ("arena_floats", C.c_int64), ("n_drop_sites", C.c_int32), ("decode_nsamples", C.c_int32),
                ("pw_scheme", C.c_int32)]


class ScoreTerm(C.Structure):
    _fields_ = [("source", C.c_int32), ("transform", C.c_int32), ("weight", C.c_double)]


class ScoreDesc(C.Structure):
    """uda_score_desc_t: per component one or two (source, transform, weight) terms; mean or max over the kept rows."""
    _fields_ = [("n_comp", C.c_int32), ("reduce_mean", C.c_int32), ("n_terms", C.c_int32 * SCORE_MAX_COMP),
                ("reserved", C.c_int32), ("term", (ScoreTerm * 2) * SCORE_MAX_COMP)]


_P = C.c_void_p
_SIGNATURES = {
    "uda_create": (C.c_int, [C.POINTER(Model), C.POINTER(BufDesc), C.c_int32, C.POINTER(Op), C.c_int32,
                             C.POINTER(DropSite), _P, C.c_int64, _P, C.c_int32, C.POINTER(_P)]),
    "uda_destroy": (None, [_P]),
    "uda_last_error": (C.c_char_p, [_P]),
    "uda_set_images_u8": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32]),
    "uda_set_images_u8_device": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32]),
    "uda_set_images_u8_ragged": (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    "uda_input_u8_device": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "uda_prefetch_images_u8": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32]),
    "uda_prefetch_images_u8_ragged": (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    "uda_swap_prefetched": (C.c_int, [_P]),
    "uda_set_images_f32": (C.c_int, [_P, _P, C.c_int32, _P]),
    "uda_set_dropout_seed": (C.c_int, [_P, C.c_uint64]),
    "uda_set_dropout_image_offset": (C.c_int, [_P, C.c_int64]),
    "uda_set_dropout_sample_shard": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32]),
    "uda_set_dropout_masks": (C.c_int, [_P, _P, C.c_int64]),
    "uda_get_dropout_masks": (C.c_int, [_P, _P, C.c_int64]),
    "uda_run": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "uda_synchronize": (C.c_int, [_P]),
    "uda_run_async": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32)]),
    "uda_run_consistency": (C.c_int, [_P, C.c_int32]),
    "uda_get_consistency": (C.c_int, [_P, _P, _P]),
    "uda_get_augmented_u8": (C.c_int, [_P, _P, C.c_int64]),
    "uda_collect": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P]),
    "uda_collect_device": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P), C.POINTER(C.c_int32)]),
    "uda_drain": (C.c_int, [_P]),
    "uda_range_demotions": (C.c_int64, [_P]),
    "uda_debug_op_scheme": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                      C.POINTER(C.c_int32)]),
    "uda_nms_prefix_fallbacks": (C.c_int64, [_P]),
    "uda_nms_coop_fallbacks": (C.c_int64, [_P]),
    "uda_nms_coop_not_launched": (C.c_int64, [_P]),
    "uda_get_detections": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "uda_detection_cols": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "uda_detections_device": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(_P), C.POINTER(C.c_int32)]),
    "uda_get_class_probs": (C.c_int, [_P, _P, _P]),
    "uda_set_ground_truth": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32]),
    "uda_assign_ground_truth": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "uda_get_assignment": (C.c_int, [_P, _P, _P, _P]),
    "uda_get_assigned_rows": (C.c_int, [_P, _P, C.c_int64]),
    "uda_assigned_row_cols": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "uda_assign_gt_np": (C.c_int, [C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "uda_score_images": (C.c_int, [_P, C.POINTER(ScoreDesc), C.c_float]),
    "uda_image_scores_shape": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "uda_get_image_scores": (C.c_int, [_P, _P, _P, _P]),
    "uda_score_images_np": (C.c_int, [C.c_int32, C.POINTER(ScoreDesc), C.c_double, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, _P, _P, _P]),
    "uda_score_images_np_f32": (C.c_int, [C.c_int32, C.POINTER(ScoreDesc), C.c_float, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_int32, _P, _P, _P]),
    "uda_pseudo_rows": (C.c_int, [_P, C.POINTER(ScoreDesc), C.c_int32, C.c_int32, C.c_float, C.c_double, C.c_int32]),
    "uda_pseudo_rows_shape": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "uda_get_pseudo_rows": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P]),
    "uda_pseudo_rows_np": (C.c_int, [C.c_int32, C.POINTER(ScoreDesc), C.c_double, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, _P, C.POINTER(C.c_int64),
                                     _P, _P, _P]),
    "uda_pseudo_rows_np_f32": (C.c_int, [C.c_int32, C.POINTER(ScoreDesc), C.c_float, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, _P, C.POINTER(C.c_int64),
                                         _P, _P, _P]),
    "uda_set_eval_ground_truth": (C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    "uda_eval_match": (C.c_int, [_P, _P, C.c_int32]),
    "uda_get_eval_records": (C.c_int, [_P, _P, _P, _P]),
    "uda_eval_match_np": (C.c_int, [C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    "uda_thr_objective_np": (C.c_int, [C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32,
                                       C.c_int32, C.c_double, _P, _P, _P]),
    "uda_thr_report_np": (C.c_int, [C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32,
                                    C.c_double, _P, _P, _P, _P]),
    "uda_heat_maps_np": (C.c_int, [C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32,
                                   C.c_int32, C.c_int32, _P, _P]),
    "uda_thr_post_np": (C.c_int, [C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "uda_hash_neighbors_np": (C.c_int, [C.c_int32, _P, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int64, C.POINTER(C.c_int32),
                                        _P, _P, C.POINTER(C.c_int64)]),
    "uda_nn_dist2_np": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "uda_kde_eval_np": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "uda_pseudo_audit_np": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_double, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "uda_uncert_report_np": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "uda_class_report_np": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                      _P, _P]),
    "uda_resample_np": (C.c_int, [C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "uda_resample_coeffs_np": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), _P, _P, C.c_int64]),
    "uda_resample_coeffs_filter_np": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), _P, _P, C.c_int64]),
    "uda_phash_np": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "uda_phash_table_np": (C.c_int, [_P]),
    "uda_collage_np": (C.c_int, [C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P,
                                 C.c_int64, _P, _P]),
    "uda_gauss_box_np": (C.c_int, [C.c_double, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "uda_label_check": (C.c_int, [_P, C.c_float, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_float, C.c_int32]),
    "uda_get_label_check": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "uda_label_check_np": (C.c_int, [C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double,
                                     C.c_int32, C.c_double, C.c_double, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "uda_label_check_np_f32": (C.c_int, [C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_double,
                                         C.c_double, C.c_int32, C.c_double, C.c_float, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "uda_calibrate_box": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    "uda_calibrate_class": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_uint64, _P, _P, _P]),
    "uda_serve": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    "uda_get_head_outputs": (C.c_int, [_P, C.c_int32, _P, _P]),
    "uda_set_head_outputs": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int64, _P, C.c_int64]),
    "uda_head_outputs_device": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(_P), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "uda_set_num_images": (C.c_int, [_P, C.c_int32]),
    "uda_postprocess_heads": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),
    "uda_copy_heads": (C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    "uda_predict": (C.c_int, [_P, _P, C.c_int32]),
    "uda_get_candidates": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "uda_num_candidates": (C.c_int32, [_P]),
    "uda_read_buffer": (C.c_int, [_P, C.c_int32, _P, C.c_int64]),
    "uda_get_preprocessed": (C.c_int, [_P, _P, _P]),
    "uda_nms": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float,
                          C.c_int32, _P, _P, _P]),
    "uda_debug_pw": (C.c_int, [C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                               C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(C.c_float)]),
    "uda_nms_np": (C.c_int, [C.c_int32, _P, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, _P, C.POINTER(C.c_int32)]),
    "uda_per_class_nms_np": (C.c_int, [C.c_int32, _P, _P, _P, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_float, C.c_float, C.c_float, _P]),
    "uda_crc32c": (C.c_uint32, [_P, C.c_uint64, C.c_uint32]),
    "uda_profile_enable": (C.c_int, [_P, C.c_uint32]),
    "uda_profile_read": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int32]),
}
EXPORTS = tuple(_SIGNATURES)

_lib = None


def build(force=False):
    """Compile csrc/*.hip for gfx950 into csrc/libuda_hip.so (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-j4"])
    return LIB_PATH


def load():
    """dlopen the library; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "HIP library %s is missing: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (or `make -C %s`). There is no CPU fallback." % (LIB_PATH, CSRC))
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class UdaError(RuntimeError):
    pass


def check(lib, ctx, rc, what):
    if rc != 0:
        msg = lib.uda_last_error(ctx)
        raise UdaError("%s failed: %s" % (what, msg.decode() if msg else "unknown error"))
