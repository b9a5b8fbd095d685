/* uda_hip.h — C ABI of the MI355X (gfx950) hot path of uncertainty-detection-autolabeling.
 *
 * One shared library (uncertainty-detection-autolabeling_amd/csrc/libuda_hip.so), plain
 * pointers and sizes, no torch / C++ types.  It replaces what the reference reaches
 * through `infer_lib.ServingDriver` (reference src/infer_lib.py:118-296):
 *
 *   uda_create            <- KerasDriver.__init__: build EfficientDetModel + restore weights
 *                            (infer_lib.py:416-440; efficientdet_keras.py:850-970)
 *   uda_set_images_u8     <- the uint8 [N,h,w,3] `image_arrays` argument of serve()  (infer_lib.py:337-343,442-448)
 *   uda_run               <- EfficientDetModel.call: _preprocessing -> EfficientDetNet.call (MC loop)
 *                            -> _postprocess                     (efficientdet_keras.py:1076-1146, 979-1050)
 *   uda_get_detections    <- the output tuple of postprocess_global / postprocess_per_class
 *                            (postprocess.py:472-621, 624-740)
 *   uda_serve             <- ServingDriver.serve                (set_images + run + get_detections)
 *   uda_predict           <- ServingDriver.predict with only_network=True: float images -> raw head outputs
 *                            (infer_lib.py:345-350,450-457)
 *   uda_postprocess_heads <- ServingDriver._postprocess = postprocess_global on given head outputs
 *                            (infer_lib.py:263-267)
 *   uda_assign_ground_truth <- the gt_box_assigner walk of the validate / calibrate modes over the ground-truth rows
 *                            (utils_extra.py:44-64; validate_model.py:314-470, calibrate_model.py:133-190)
 *   uda_score_images      <- ActiveLearning.score_image's per-detection numbers and per-image mean / max
 *                            (active_learning_loop.py:528-733)
 *   uda_pseudo_rows       <- STAC.score_image's per-detection value, candidate rows and min / max (pseudo-labelling)
 *                            (SSL_stac.py:302-642)
 *   uda_eval_match        <- COCOeval_all.evaluateImg for the detections and ground truth EvaluationMetric.update_state
 *                            collects (custom_cocoeval.py:265-349; coco_metric.py:219-283)
 *   uda_thr_objective_np  <- roc_metrics for the candidates of UncertOptimal._extract_optimal_params
 *                            (uncertainty_analysis.py:44-152)
 *   uda_thr_report_np     <- the curves, calc_jsd moments and removal counts of MainUncertViz._save_thr_performance and
 *                            _collect_thresh_results (uncertainty_analysis.py:517-749; utils_extra.py:25-36)
 *   uda_heat_maps_np      <- the ten spatial maps of MainUncertViz._plot_validheat, every `mask[y1:y2, x1:x2] += value[i]` loop
 *                            of one validation set in one launch (uncertainty_analysis.py:920-1019)
 *   uda_thr_post_np       <- the tallies of MainUncertViz._plot_metricsspider and the per-image counts behind
 *                            _collect_postthresholding (uncertainty_analysis.py:838-880, 1024-1068)
 *   uda_hash_neighbors_np <- the distance matrix, its maximum and the rows of near-duplicates of
 *                            ActiveLearning.extract_hash_matrix (active_learning_loop.py:240-270)
 *   uda_phash_np          <- the hashes that matrix is built from: Image.resize((512, 256)) and imagehash.phash of every pool
 *                            image (active_learning_loop.py:215-224)
 *   uda_nn_dist2_np       <- the four KD-tree queries of emp_KL_divergence for every (class, method) of
 *                            Similarity.calculate_set_similarity (active_learning_eval.py:481-487, 946-1029)
 *   uda_pseudo_audit_np   <- the matching, allocation and by-value tallies of Parent_SSL.extract_pseudo_gt_data and
 *                            _percls_analysis (ssl_utils/parent.py:1567-1813), read by ThreeDproblem.corrected_pseudo (3d.py:80-255)
 *   uda_uncert_report_np  <- the tallies of ValidUncertPlot.__init__ (utils_extra.py:378-445), RegressionCalib._conf_all
 *                            (calibrate_regression.py:231-349) and calc_ece / calc_nll / calc_rmse (utils_box.py:17-102)
 *   uda_class_report_np   <- the reliability bins, Brier and NLL sums of ClassificationCalib._calibr_bins and _calibr_plot
 *                            (calibrate_classification.py:97-143, 250-440)
 *   uda_resample_np       <- every Image.resize(.., Image.LANCZOS) and paste of Parent_SSL.crop_collage, the rare-class collage
 *                            (ssl_utils/parent.py:505-597; ssl_utils/rcc.py)
 *   uda_collage_np        <- the same with Parent_SSL.apply_manual_augmentation between resize and paste: Image.transpose,
 *                            ImageEnhance.Brightness / Contrast, ImageFilter.GaussianBlur and the noise add
 *                            (ssl_utils/parent.py:261-315, 534-537)
 *   uda_kde_eval_np       <- the scipy.stats.gaussian_kde evaluated on a mesh by EpistemicVSAleatoric.get_plot_grid
 *                            (uncertainty_ep_vs_al.py:361-375), for every configuration of a comparison in one call
 *
 * Conventions: every function returns 0 on success, non-zero on error (message via
 * uda_last_error); inputs are borrowed, outputs are caller-allocated; a handle owns one
 * GPU's weights, workspace and HIP stream, is not thread-safe, and every call that
 * returns data synchronises its stream before returning.  Host orchestration (config,
 * topology -> op list, weight packing) stays in Python (plan.py) exactly as the
 * reference keeps model building in Python above the TF runtime.
 */
#ifndef UDA_HIP_H_
#define UDA_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UDA_ABI_VERSION 5
#define UDA_MAX_LEVELS 8
#define UDA_MAX_FUSE_INPUTS 3

/* ---- activation buffers (NHWC float32) ---------------------------------------------- */
typedef struct uda_buf_desc {
  int32_t H, W, C;      /* one sample */
  int32_t per_sample;   /* 0: one row per image (shared by all MC samples); 1: one row per (image, sample) */
  int64_t offset;       /* float offset inside the per-chunk arena (liveness-planned by plan.py) */
  int32_t kind;         /* 0 arena, 1 network input image, 2 class head output, 3 box head output */
  int32_t level;        /* pyramid level index for kind 2/3 */
} uda_buf_desc_t;

/* ---- ops ------------------------------------------------------------------------------ */
enum uda_op_kind {
  UDA_OP_STEM = 1,  /* 3x3 stride-2 conv (Cin=3) + BN + swish          efficientnet_model.py:588-612 */
  UDA_OP_PW = 2,    /* 1x1 conv (+SE input scale)(+bias)(+BN)(+swish)(+dropout)(+residual)  :358-373,403-418,471-486 */
  UDA_OP_DW = 3,    /* depthwise kxk stride s SAME (+BN)(+swish)(+dropout)(+SE partial sums) :376-391,459-464 */
  UDA_OP_SE = 4,    /* mean -> fc+bias -> swish -> fc+bias -> sigmoid   :219-232 */
  UDA_OP_FUSE = 5,  /* BiFPN weighted fusion of resampled inputs + swish  efficientdet_keras.py:86-127,229-231 */
  UDA_OP_POOL = 6,  /* max pool (stride+1) x (stride+1), stride s, SAME   efficientdet_keras.py:280-290 */
  UDA_OP_MBX = 7,   /* fused MBConv front half: 1x1 expand + BN + swish + dropout -> depthwise kxk/s + BN + swish
                       + dropout + SE tile sums, the 6x-expanded tensor never leaves the CU
                       (efficientnet_model.py:446-464).  With se_scale >= 0 the op also absorbs the PREVIOUS block's
                       projection (efficientnet_model.py:471-486): in[0] is that block's gated-depthwise tensor D
                       [C0 <= 32 channels], se_scale its per-row gate [rows, C0], se_w1_off the projection kernel
                       [C0][se_mid], se_b1_off / se_w2_off its BN scale / shift, se_mid = 16 projected channels */
  UDA_OP_SEP = 8    /* fused SeparableConv2D: depthwise 3x3 stride 1 SAME (kernel at w2_off) -> 1x1 (kernel at w_off)
                       (+bias)(+BN)(+swish)(+dropout); the depthwise result never leaves the CU
                       (efficientdet_keras.py:207-227,421-446,584-626) */
};
/* utils.activation_fn (reference utils.py:42-59): swish / silu / swish_native are one function; srelu (it carries a trainable
 * beta) is refused by the planner (ValueError, as the reference raises for an unknown act_type) */
enum uda_act { UDA_ACT_NONE = 0, UDA_ACT_SWISH = 1, UDA_ACT_RELU = 2, UDA_ACT_RELU6 = 3, UDA_ACT_HSWISH = 4, UDA_ACT_MISH = 5 };
enum uda_resample { UDA_RS_NONE = 0, UDA_RS_NEAREST_UP = 1, UDA_RS_MAXPOOL = 2 };

typedef struct uda_op {
  int32_t kind;
  int32_t in[UDA_MAX_FUSE_INPUTS]; /* buffer ids, -1 = unused */
  int32_t out;                     /* buffer id */
  int32_t se_scale;                /* PW: buffer id of the [rows, Cin] SE gate applied to the input, or -1 */
  int32_t se_partial;              /* DW: buffer id receiving per-tile channel sums; SE: the same buffer as input */
  int32_t residual;                /* PW: buffer id added to the output, or -1 */
  int32_t k, stride;               /* DW / POOL / STEM */
  int32_t act;                     /* uda_act, applied after bias/BN, before dropout */
  int64_t w_off;                   /* float offsets into the weight blob; -1 = absent */
  int64_t bias_off;                /*   conv bias [Cout]                                */
  int64_t bn_scale_off;            /*   gamma * rsqrt(var + 1e-3)  [Cout]               */
  int64_t bn_shift_off;            /*   beta - mean * scale         [Cout]               */
  int64_t se_w1_off, se_b1_off, se_w2_off, se_b2_off; /* SE: [C][mid], [mid], [mid][C], [C] */
  int32_t se_mid;
  int32_t drop_site;               /* index of the MC-dropout site applied to the output, -1 = none */
  int32_t resample[UDA_MAX_FUSE_INPUTS]; /* FUSE: uda_resample per input */
  float fuse_w[UDA_MAX_FUSE_INPUTS];     /* FUSE: relu(w_i) / (sum relu(w) + 1e-4) */
  int32_t n_in;
  int32_t drop_site2;              /* MBX: dropout site after the depthwise stage (drop_site = after the expand stage).
                                      SEP (plain, not fuse_in): a DEFERRED site of the producing op - keep-scales [sample row][C] of
                                      this op's INPUT channels, which the producer (a per-image tensor shared by the T samples) did not
                                      apply: a per-channel factor commutes with the depthwise conv, so the op computes the depthwise
                                      result once per image and serves the T samples from it.  -1 = none */
  int64_t w2_off;                  /* MBX: depthwise kernel [k*k][Cmid]; SEP: depthwise kernel [9][C] */
  int64_t bn2_scale_off, bn2_shift_off; /* MBX: BN after the depthwise stage */
  int32_t launch_group;            /* SEP: n > 1 on the first of n consecutive, mutually independent ops of one shape class
                                      (same channels, activation, sample axes) that may share ONE launch - the pyramid levels
                                      of a head layer; the planner keeps every buffer they touch alive to the end of the run.
                                      0 / 1 elsewhere. */
  int32_t fuse_in;                 /* SEP: 1 = the conv input is the BiFPN fusion swish(sum_i fuse_w[i] * resample[i](in[i])) of in[0 .. n_in),
                                      computed on the fly for the tile (no fused tensor in memory); 0 elsewhere */
  int32_t fuse_act;                /* SEP with fuse_in: uda_act of that fusion (act_type; UDA_ACT_NONE under conv_bn_act_pattern,
                                      efficientdet_keras.py:229-236) */
} uda_op_t;

/* ---- MC dropout sites -------------------------------------------------------------------- */
typedef struct uda_drop_site {
  int32_t channels;
  float rate;            /* keep iff u >= rate, scale 1/(1-rate)  (SpatialDropout2D, noise shape [N,1,1,C]) */
} uda_drop_site_t;

/* ---- model / post-processing description ---------------------------------------------------- */
enum uda_decode { UDA_DECODE_PLAIN = 0, UDA_DECODE_LNORM = 1, UDA_DECODE_FALSEDEC = 2,
                  UDA_DECODE_SAMPLE = 3 /* utils_box.py:162-184: moments of decode_nsamples decoded Normal draws (Philox stream) */ };
enum uda_post_mode { UDA_POST_GLOBAL = 0, UDA_POST_PER_CLASS = 1 };
/* split-precision scheme of the 1x1 contractions (plan.PW_SCHEMES; the values are kernel template arguments) */
enum uda_pw_scheme {
  UDA_SPLIT_NONE = 0,     /* "f32": exact f32-input MFMA kernels, unfused */
  UDA_SPLIT_BF16X2 = 2,   /* "bf16x2": two bf16 pieces per operand, three cross terms (~2^-17 per product) */
  UDA_SPLIT_BF16X3 = 3,   /* "bf16x3": three bf16 pieces, six cross terms (~2^-24) */
  UDA_SPLIT_F16X2 = 4,    /* "f16x2": two fp16 pieces, three cross terms (~2^-22; operands must stay below 65504) */
  UDA_SPLIT_F16X1 = 5,    /* "f16": one fp16 piece, one product (~2^-11: Keras mixed_float16 operands; same range limit) */
  UDA_SPLIT_BF16X1 = 6    /* "bf16": one bf16 piece, one product (~2^-8: Keras mixed_bfloat16 operands; float32's range, nothing tracked) */
};

typedef struct uda_model {
  int32_t abi_version;
  int32_t image_h, image_w;         /* network input size (H, W) = parse_image_size(image_size) */
  float mean_rgb[3], stddev_rgb[3];
  int32_t num_levels;
  int32_t level_h[UDA_MAX_LEVELS], level_w[UDA_MAX_LEVELS];
  int32_t anchors_per_loc;          /* num_scales * len(aspect_ratios) */
  int32_t num_classes;
  int32_t loss_attenuation;         /* box head has 8*A channels: [4A box | 4A sigma]  (postprocess.py:448-462) */
  int32_t mc_samples;               /* T (1 when mc_dropout is off) */
  int32_t cls_stacked, box_stacked; /* head outputs carry the T axis                  (efficientdet_keras.py:1026-1049) */
  int32_t has_uncert;               /* loss_attenuation or mc_dropout: uncertainty columns are emitted (postprocess.py:443) */
  int32_t decode_method;            /* uda_decode */
  int32_t enable_softmax;           /* logits output present */
  /* nms (postprocess.py:373-400) */
  float nms_soft_sigma;             /* sigma/2 handed to NonMaxSuppressionV5; 0 = hard */
  float nms_iou_thresh, nms_score_thresh;
  int32_t max_output_size;
  int32_t max_nms_inputs;           /* 0: argmax per anchor; >0: top-k over anchors*classes (postprocess.py:96-121) */
  int32_t post_mode;                /* default uda_post_mode used by uda_run */
  /* planning */
  int32_t chunk_images;             /* images processed per pass of the op list */
  int32_t max_images;               /* capacity of one uda_run */
  int64_t arena_floats;             /* per-chunk arena size */
  int32_t n_drop_sites;
  int32_t decode_nsamples;          /* UDA_DECODE_SAMPLE: draws per (anchor, MC sample); config `decode_nsamples` (100) */
  int32_t pw_scheme;                /* uda_pw_scheme of the handle (plan.Plan.pw_scheme); anything else fails uda_create */
} uda_model_t;

typedef struct uda_ctx uda_ctx_t;

/* Build a handle on HIP device `device`: uploads `weights`, the anchor table, allocates
 * the arena, head-output and NMS workspaces.  Returns NULL-handle + error on failure. */
int uda_create(const uda_model_t* model, const uda_buf_desc_t* bufs, int32_t n_bufs,
               const uda_op_t* ops, int32_t n_ops, const uda_drop_site_t* sites,
               const float* weights, int64_t n_weights, const float* anchors /* [A_tot*4] */,
               int32_t device, uda_ctx_t** out);
void uda_destroy(uda_ctx_t* ctx);
/* last error of `ctx` (or of the last failed uda_create when ctx == NULL) */
const char* uda_last_error(const uda_ctx_t* ctx);

/* CRC-32C of a host buffer (continue from `crc`, 0 to start): the per-tensor checksum of the TensorFlow checkpoint bundles
 * `utils_keras.restore_ckpt` reads (utils_keras.py:125-235); host code, no GPU call. */
uint32_t uda_crc32c(const void* data, uint64_t n, uint32_t crc);

/* Raw uint8 images [n,h,w,3] from host memory into the handle's device staging buffer (replaces the feed of
 * ServingDriver.serve, infer_lib.py:139-151,232-249).  The bytes are gathered into a pinned host buffer owned by the
 * handle and leave by one DMA: the caller's array is free as soon as the call returns. */
int uda_set_images_u8(uda_ctx_t* ctx, const uint8_t* images, int32_t n, int32_t h, int32_t w);
/* A batch whose raw sizes differ per image - KITTI frames are 370-376 x 1224-1242 (dataset_data.py:105) and the
 * reference's callers feed them one file at a time (validate_model.py:479-483, infer_model.py:554-581): images[i] points
 * at [h[i], w[i], 3] bytes.  Every image gets its own resize scale / scaled size / image_scale, exactly as
 * dataloader.py:123-152 computes them per image. */
int uda_set_images_u8_ragged(uda_ctx_t* ctx, const uint8_t* const* images, int32_t n, const int32_t* h, const int32_t* w);
/* Feed hiding: upload the NEXT batch into the handle's second input slot on a copy stream while the current batch is
 * being processed (call it after uda_run has queued the current batch); uda_swap_prefetched then makes that batch the
 * input of the following uda_run (the compute stream waits for the upload event, no host synchronisation).  The reference
 * times serve() including its feed (validate_model.py:154-158); with these two calls the feed costs no device time. */
int uda_prefetch_images_u8(uda_ctx_t* ctx, const uint8_t* images, int32_t n, int32_t h, int32_t w);
int uda_prefetch_images_u8_ragged(uda_ctx_t* ctx, const uint8_t* const* images, int32_t n, const int32_t* h, const int32_t* w);
int uda_swap_prefetched(uda_ctx_t* ctx);
/* Same, from a device pointer the caller owns (device-to-device copy on the stream). */
int uda_set_images_u8_device(uda_ctx_t* ctx, const void* images_dev, int32_t n, int32_t h, int32_t w);
/* The handle's own device copy of the current uint8 batch (one raw size): lets the members of a deep ensemble share ONE
 * upload - member 0 takes the host batch, the others uda_set_images_u8_device from its buffer (BASELINE configs[3]). */
int uda_input_u8_device(uda_ctx_t* ctx, const void** images_dev, int32_t* n, int32_t* h, int32_t* w);
/* Preprocessed float images [n,H,W,3] (the `only_network` input); scales default to 1. */
int uda_set_images_f32(uda_ctx_t* ctx, const float* images, int32_t n, const float* image_scales);

/* Dropout masks: either generated on the device from `seed` (Philox4x32-10)
 * or injected: `masks` = concatenation over sites of float32 [n*T, channels] keep-scales. */
int uda_set_dropout_seed(uda_ctx_t* ctx, uint64_t seed);
/* Index of the handle's first image inside the global batch (multi-GPU image shards): the Philox row
 * of image n, sample t is (offset + n) * T + t, so a sharded batch draws the masks of the unsharded one. */
int uda_set_dropout_image_offset(uda_ctx_t* ctx, int64_t first_image);
/* MC samples sharded over ranks (north_star: "images (and optionally MC samples) shard"): the handle's T local samples are
 * samples t_first + j * t_stride (j < T) of a global axis of t_total samples - the Philox row of image n, local sample j is
 * (offset + n) * t_total + t_first + j * t_stride, so the ranks together draw exactly the masks of one handle that runs all
 * t_total samples.  t_total = 0 restores "this handle runs every sample".  (dist.serve_sample_sharded) */
int uda_set_dropout_sample_shard(uda_ctx_t* ctx, int32_t t_first, int32_t t_stride, int32_t t_total);
int uda_set_dropout_masks(uda_ctx_t* ctx, const float* masks, int64_t n_floats);
int uda_get_dropout_masks(uda_ctx_t* ctx, float* masks, int64_t n_floats);

/* preprocess (if uint8 images are set) -> network x T -> post-process, asynchronously on the
 * handle's stream.  post_mode < 0 uses the model default; run_post == 0 stops after the heads. */
int uda_run(uda_ctx_t* ctx, int32_t post_mode, int32_t run_post);
int uda_synchronize(uda_ctx_t* ctx);
/* Pipelined serving of a stream of batches (infer_lib.ServingDriver.serve_images called batch after batch,
 * infer_lib.py:504-540; the reference runs them strictly one after the other): uda_run_async queues network + post-process
 * of the current input like uda_run(ctx, post_mode, 1) but does NOT order the handle's main stream behind the
 * post-process - the next uda_run_async's network starts at once and only its first head-writing op waits for it, so the
 * ~4 ms of latency-bound aggregate / NMS / gather launches of batch k run beside the backbone of batch k + 1.
 * *ticket (0 | 1) names the run; at most two may be in flight.  uda_collect waits for that run's post-process only and
 * copies its detections (same arrays as uda_get_detections; NULL = skip) - the detection outputs and the image scales
 * exist once per ticket, so a run queued behind it cannot disturb them.  Typical loop:
 *     run_async(&t0);  for each further batch: { set / swap images; run_async(&t1); collect(t0, ...); t0 = t1; }  collect(t0, ...)
 * Failures are loud: a range / barrier flag raised by a run whose candidates a newer run has replaced fails the collect
 * (the batch has to be run again); entry points that rewrite head buffers refuse while a run is in flight.  Results are
 * bit-identical to uda_run's. */
int uda_run_async(uda_ctx_t* ctx, int32_t post_mode, int32_t* ticket);
/* Augmentation-consistency check (reference infer_model.py:768-848, model_params["consistency_ssl"], hparams_config.py:240;
 * set for the consistency-based SSL / SSAL datasets, inspector.py:127-128).  The n staged uint8 images (uniform or ragged)
 * and three variants of each, built on the device, run as ONE batch of 4n through preprocess, network and post-process:
 *   images n..2n-1   left-right flip (tf.image.flip_left_right, :775-776)
 *   images 2n..3n-1  cv2.GaussianBlur(im, (9, 9), 0) on uint8 as OpenCV's 8-bit fixed-point filter (:777-781;
 *                    taps 4 13 30 51 60 51 30 13 4 / 256, REFLECT_101 borders; DESIGN.md "Consistency check")
 *   images 3n..4n-1  im + N(0, 0.5) in float64, unclipped (:782-792): Philox normal stream, counter (raw pixel, image offset
 *                    + image, channel, tag 0x4E), keyed by the dropout seed
 * Variant n + N v keeps image n's raw size and scale; image j draws the dropout rows (offset + j) T + t, so the originals'
 * detections are bit-identical to uda_run's for the same seed.  Needs max_images >= 4n.  Afterwards the run's readers
 * (uda_get_detections, uda_get_class_probs, calibrators, uda_get_preprocessed) hold all 4n images, the originals first. */
int uda_run_consistency(uda_ctx_t* ctx, int32_t post_mode);
/* Scores of the last uda_run_consistency, [n, M] for its n originals, detection rank k (utils_box.py:56-89, :822-835):
 *   iou[k]   = mean over the three variants of max_j IoU(original box k, variant box j), all M rows of the variant (padded
 *              rows included), the flip's boxes un-flipped to [y1, W - x2, y2, W - x1] (W = raw width), float64
 *   agree[k] = 1 when the mean of the three variants' class ids at rank k is an integer (the reference's rank-wise test;
 *              the original's class is not consulted) */
int uda_get_consistency(uda_ctx_t* ctx, double* iou, uint8_t* agree);
/* The device-built flips then blurs of the current consistency input, packed like the originals (n_bytes = 2 x their bytes). */
int uda_get_augmented_u8(uda_ctx_t* ctx, uint8_t* out, int64_t n_bytes);
int uda_collect(uda_ctx_t* ctx, int32_t ticket, float* boxes, float* scores, float* classes, int32_t* valid, float* logits);
/* The same for the multi-GPU gather: the run's detections as ONE device-resident record buffer (see uda_detections_device
 * for the layout and `rows`); packed on a stream of its own, complete when the call returns; closes the ticket. */
int uda_collect_device(uda_ctx_t* ctx, int32_t ticket, int32_t rows, int32_t with_logits, void** dev_ptr, int32_t* cols);
/* Abandon every pipelined run in flight (results discarded, tickets closed, flags cleared): what a consumer that drops
 * ServingDriver.serve_stream half way, or whose uda_collect failed, calls before it uses the handle synchronously again. */
int uda_drain(uda_ctx_t* ctx);
/* The default scheme splits the operands of the 1x1 contractions into two fp16 pieces (float32-class products at the
 * matrix-core cost of bf16): an operand above 65504 cannot be split.  The reference computes in float32 and never rejects
 * an input on magnitude (utils.py:595-609), so neither does the handle: the op that saw such an operand is re-packed with
 * three bf16 pieces (float32 exponent range), the run is served again from its unchanged inputs before any reader sees
 * it, and the op stays that way.  This counts the ops re-packed so far (0 for every weight set the tests initialise). */
int64_t uda_range_demotions(const uda_ctx_t* ctx);
/* Debug: how op `op` of the handle's op list runs now (after any range demotion).  *scheme = its split scheme (UDA_SPLIT_*
 * of uda_internal.h; -1: no packed weights, the op has no split contraction), *w_scale = the power-of-two factor its packed
 * weights carry (1 unless fp16 pieces), *a_scale = the factor on its A operand (the pre-scaled depthwise taps of an fp16
 * separable conv; else 1), *out_f16 = 1 if its output tensor is stored in 16 bits (fp16 under
 * UDA_SPLIT_F16X1, bf16 under UDA_SPLIT_BF16X1: the op's scheme says which).  Any pointer may be NULL. */
int uda_debug_op_scheme(const uda_ctx_t* ctx, int32_t op, int32_t* scheme, float* w_scale, float* a_scale, int32_t* out_f16);
/* Global NMS over the whole anchor set runs on the score prefix that can be selected at all, checked on the
 * device; this counts the images / problems that failed the check and were redone on the full set (the results
 * are identical either way). */
int64_t uda_nms_prefix_fallbacks(const uda_ctx_t* ctx);
/* Global NMS over the whole anchor set normally runs as ONE launch of a co-resident grid whose blocks exchange keys
 * through memory with a bounded spin.  When a spin runs out (the grid was not co-resident: e.g.
 * another process interleaving such grids on the same GPU) the post-process is redone with two launches per epoch and
 * the handle stays on that version; this counts those redone post-process runs (0 in normal operation; results are
 * identical either way).  UDA_NMS_COOP_SPIN=<polls> shortens the bound (test hook). */
int64_t uda_nms_coop_fallbacks(const uda_ctx_t* ctx);
/* NMS runs that were eligible for the single-launch grid but did NOT get it (capacity query failed, grid larger than the
 * device holds, launch refused) and therefore ran the slower prefix / two-launches-per-epoch versions: 0 in normal
 * operation; a non-zero value explains a slow post-process that uda_nms_coop_fallbacks (time-outs only) would not show. */
int64_t uda_nms_coop_not_launched(const uda_ctx_t* ctx);

/* Detections of the last uda_run (synchronises).  Shapes for n images, M = max_output_size:
 *   boxes   [n, M, box_cols]   box_cols = 4 (+4 aleatoric sigma)(+4 epistemic sigma)
 *   scores  [n, M]
 *   classes [n, M, cls_cols]   cls_cols = 1 (+num_classes MC std of the logits)
 *   valid   [n] int32
 *   logits  [n, M, num_classes] (may be NULL)                       (postprocess.py:610-621) */
int uda_get_detections(uda_ctx_t* ctx, float* boxes, float* scores, float* classes,
                       int32_t* valid, float* logits);
int uda_detection_cols(const uda_ctx_t* ctx, int32_t post_mode, int32_t* box_cols, int32_t* cls_cols);
/* The detections of the last post-process as ONE device-resident float32 buffer [rows, max_output_size, cols], a row per
 * (image, detection): boxes (box_cols) | score | classes (cls_cols) | logits (num_classes, when with_logits and the global
 * post-process ran) | valid_len - the record of dist.pack_detections.  rows >= the images of the last post-process; the
 * rows beyond them are zero (padding of a ragged shard to the collective's common size).  The multi-GPU layer all-gathers
 * straight out of this buffer (RCCL): the detections do not cross PCIe before they have been collected (the
 * reference has no inference collective - infer_lib.py:337-343 returns host arrays of one process).  The buffer belongs to
 * the handle and is valid until its next call; the handle's stream has been synchronised when the call returns. */
int uda_detections_device(uda_ctx_t* ctx, int32_t rows, int32_t with_logits, void** dev_ptr, int32_t* cols);

/* What every caller of serve() computes next from `logits` (validate_model.py:159-166,
 * infer_model.py:585-600, utils_class.py:36-41), on the device: probs [n, M, num_classes] = stable softmax of the
 * selected rows' mean logits, entropy [n, M] = -sum p * log2(max(p, 1e-7)).  Global post-process only. */
int uda_get_class_probs(uda_ctx_t* ctx, float* probs, float* entropy);

/* Ground-truth assignment: what the reference's validate and calibrate modes do on the host right after serve() - give every
 * ground-truth (GT) box the detection that belongs to it (utils_extra.gt_box_assigner, utils_extra.py:44-64; callers
 * validate_model.py:314-339, calibrate_model.py:133-147) and keep that detection's row of every output column - done on the
 * detections RESIDENT in the handle after a global post-process (uda_run / uda_collect, the originals and variants of
 * uda_run_consistency, an ensemble's uda_postprocess_heads).
 *   uda_set_ground_truth     boxes [n, G, 4] (y1, x1, y2, x2 in raw-image pixels, the coordinates of the detections) and classes
 *                            [n, G], float32, padded with -1 rows (inspector.py:147-160); values must be finite (the Python
 *                            layer checks).  The handle's GT buffers hold max_images x G rows and grow only when G grows.
 *   uda_assign_ground_truth  method 0 "IoU": argmax_k calc_iou_np(gt, box_k) (utils_box.py:56-89; float32 differences, float64
 *                            products) over all M rows, padded ones included; 1 "MSE": argmin_k mean((gt - box_k)^2) in float32,
 *                            summed ((d0 + d1) + d2) + d3; 2: the GT row's own rank (the reference's else branch; a kept row
 *                            >= M is an error).  Ties go to the lowest rank, as np.argmax / np.argmin do.
 *                            keep 0 "validate": rows with class > 0 (validate_model.py:314); 1 "calibrate": rows < min(G, M) with
 *                            class >= 0 (calibrate_model.py:133-135).  Forces the deferred fix-ups every reader of detections
 *                            forces.  Refuses: no GT set, no global post-process yet, a per-class run, n different from the
 *                            run's image count, a pipelined run still in flight.
 *   uda_get_assignment       det_index [n, G] int32 (-1: row not kept), iou [n, G] float64 = calc_iou_np(gt, matched box) whatever
 *                            the method (0: not kept), count [n] int32 kept rows per image; any pointer may be NULL.
 *   uda_get_assigned_rows    the matched rows, K = sum(count) in (image, GT row) order - the order the reference appends in -
 *                            as one float32 table [K, cols]: box columns (box_cols of uda_detection_cols) | score | class
 *                            columns (cls_cols) | and with enable_softmax: logits (num_classes) | probab (num_classes) | entropy
 *                            (the buffers of uda_get_class_probs).  Values are copied unchanged: np.nan_to_num of the
 *                            uncertainty columns (validate_model.py:176-196) is the caller's (infer_lib does it).
 *                            n_floats must equal K * cols.
 *   uda_assigned_row_cols    cols of that table. */
int uda_set_ground_truth(uda_ctx_t* ctx, const float* boxes, const float* classes, int32_t n, int32_t G);
int uda_assign_ground_truth(uda_ctx_t* ctx, int32_t method, int32_t keep);
int uda_get_assignment(uda_ctx_t* ctx, int32_t* det_index, double* iou, int32_t* count);
int uda_get_assigned_rows(uda_ctx_t* ctx, float* rows, int64_t n_floats);
int uda_assigned_row_cols(const uda_ctx_t* ctx, int32_t* cols);
/* The same assignment without a handle, in the manner of uda_nms_np: host arrays det_boxes [n, M, 4], gt_boxes [n, G, 4],
 * gt_classes [n, G] in, the same kernel, det_index / iou [n, G] and count [n] out - gt_box_assigner for callers that hold
 * detections of their own.  M <= 4096, G <= 16384. */
int uda_assign_gt_np(int32_t device, const float* det_boxes, const float* gt_boxes, const float* gt_classes, int32_t n,
                     int32_t M, int32_t G, int32_t method, int32_t keep, int32_t* det_index, double* iou, int32_t* count);

/* Active-learning image scores: what the reference's active-learning loop does with the detections of the unlabeled pool
 * (ActiveLearning.score_image, active_learning_loop.py:528-733, on the lines Infer.iterate_infer wrote, infer_model.py:836-960) -
 * one to three uncertainty numbers per detection above min_score, reduced per image with mean or max - done on the detections
 * RESIDENT in the handle after a global post-process (uda_run / uda_collect, all 4n images of uda_run_consistency, an
 * ensemble's uda_postprocess_heads).  The dataset-wide part (:733-840) is the caller's (active_learning.py).
 * A row is kept iff score > min_score (the writer's filter; padded rows score 0).  A component of a kept row is
 * w0 * term0 (+ w1 * term1); a term is a source under a transform:
 *   UDA_SCORE_SCALAR    the value itself                                   (ENTROPY, DET_SCORE)
 *   UDA_SCORE_MEAN      the mean of the 4 (box) or the class-std columns   (ALBOX, MCBOX, MCCLASS)
 *   UDA_SCORE_REL_MEAN  relativize_uncert (utils_box.py:279-292): entries 0 and 2 divided by y2 - y1, entries 1 and 3 by
 *                       x2 - x1, then the mean of the four                 (ALBOX, MCBOX)
 * Every input is converted to float64 first and everything after that is float64; on float32 columns np.nan_to_num (NaN -> 0,
 * +-inf -> +-FLT_MAX) is applied to ALBOX / MCBOX / MCCLASS before the conversion (infer_model.py:607-631).  A zero side length
 * divides as IEEE does; NaN propagates through mean and max alike (np.max).  The reduction over the kept rows has a fixed order,
 * so equal values give bit-identical results on both entry points. */
enum uda_score_source { UDA_SCORE_ENTROPY = 0, UDA_SCORE_DET_SCORE = 1, UDA_SCORE_ALBOX = 2, UDA_SCORE_MCBOX = 3, UDA_SCORE_MCCLASS = 4 };
enum uda_score_transform { UDA_SCORE_SCALAR = 0, UDA_SCORE_MEAN = 1, UDA_SCORE_REL_MEAN = 2 };
#define UDA_SCORE_MAX_COMP 3
typedef struct uda_score_term {
  int32_t source;     /* uda_score_source */
  int32_t transform;  /* uda_score_transform */
  double weight;
} uda_score_term_t;
typedef struct uda_score_desc {
  int32_t n_comp;                        /* 1..UDA_SCORE_MAX_COMP */
  int32_t reduce_mean;                   /* 1: mean over the kept rows, 0: max */
  int32_t n_terms[UDA_SCORE_MAX_COMP];   /* 1 or 2 per component */
  int32_t reserved;
  uda_score_term_t term[UDA_SCORE_MAX_COMP][2];
} uda_score_desc_t;
/*   uda_score_images      queues the softmax / entropy kernel of uda_get_class_probs when a component reads ENTROPY, then the
 *                         score kernel, on the handle's stream; forces the deferred fix-ups every reader of detections forces.
 *                         Refuses: no global post-process yet, a per-class run, a pipelined run still in flight, a source the
 *                         model does not emit (ENTROPY without enable_softmax, ALBOX without loss attenuation, MCBOX / MCCLASS
 *                         without MC dropout on that head), max_output_size above 4096.
 *   uda_image_scores_shape  n (images of the scored run) and n_comp of the last uda_score_images.
 *   uda_get_image_scores  components [n, n_comp] float64 (0 where nothing is kept), count [n] int32 kept rows, class_counts
 *                         [n, num_classes] int32 kept rows per class id 1..num_classes; one copy; any pointer may be NULL.  A kept
 *                         row whose class id is not one of 1..num_classes is an error. */
int uda_score_images(uda_ctx_t* ctx, const uda_score_desc_t* desc, float min_score);
int uda_image_scores_shape(const uda_ctx_t* ctx, int32_t* n, int32_t* n_comp);
int uda_get_image_scores(uda_ctx_t* ctx, double* components, int32_t* count, int32_t* class_counts);
/* The same scores without a handle, in the manner of uda_assign_gt_np: float64 host arrays boxes [n, M, 4], scores [n, M],
 * classes [n, M]; optional (NULL: absent, a descriptor that reads it is refused) entropy [n, M], albox / mcbox [n, M, 4],
 * mcclass [n, M, mcclass_cols]; the same kernel in its float64 instantiation (no nan_to_num: the caller's columns are
 * finite), the same outputs.  For calibrated columns and for callers that hold detections of their own.  M <= 4096.
 * uda_score_images_np_f32: the same on float32 arrays, through the instantiation the handle runs. */
int uda_score_images_np(int32_t device, const uda_score_desc_t* desc, double min_score, const double* boxes, const double* scores,
                        const double* classes, const double* entropy, const double* albox, const double* mcbox,
                        const double* mcclass, int32_t n, int32_t M, int32_t num_classes, int32_t mcclass_cols,
                        double* components, int32_t* count, int32_t* class_counts);
int uda_score_images_np_f32(int32_t device, const uda_score_desc_t* desc, float min_score, const float* boxes, const float* scores,
                            const float* classes, const float* entropy, const float* albox, const float* mcbox,
                            const float* mcclass, int32_t n, int32_t M, int32_t num_classes, int32_t mcclass_cols,
                            double* components, int32_t* count, int32_t* class_counts);

/* Pseudo-labelling rows: the first half of the semi-supervised teacher's selection (STAC.score_image, SSL_stac.py:302-642, on the
 * lines Infer.iterate_infer wrote with min_score 0.1) - per detection above min_score ONE value v from a uda_score_desc_t, the
 * candidate rows and the per-image min / max of v - done on the detections RESIDENT in the handle after a global post-process.
 * The dataset-wide min-max normalisation, the final rule and the writers are the caller's (pseudo_labels.py).
 *   kept         score > min_score (the writer's filter; padded rows score 0); only the first max_rows kept rows of an image, in
 *                rank order, take part (the reference's max_detections_per_image = 99)
 *   v            invert 0: the descriptor's one component (terms, transforms, float32 nan_to_num exactly as uda_score_images;
 *                reduce_mean is not read); invert 1: 1.0 / (((c0 + c1) [+ c2]) / n_comp) over its 2 or 3 components
 *                (1 / np.mean([...], axis=0), SSL_stac.py:575-606).  IEEE throughout: a zero mean gives inf
 *   candidate    gate 0: det_score > tau (filter_based_on_sigmoid); gate 1: v > tau (the single-column branch); in float64
 *   min / max    over the rows that take part, candidates or not; NaN is ignored, +-inf take part; (+inf, -inf) where no row does
 * The order is fixed and nothing is accumulated with float atomics: equal values give bit-identical records on every entry point. */
typedef struct uda_pseudo_record {
  int32_t image, row;   /* image of the run, detection row */
  float box[4];         /* y1 x1 y2 x2 as stored */
  float det_score;
  int32_t cls;          /* class id 1..num_classes */
  double v;
} uda_pseudo_record_t;  /* 40 bytes */
/*   uda_pseudo_rows        queues the softmax / entropy kernel when a component reads ENTROPY, then the row kernel and the packing
 *                          kernel, on the handle's stream.  Refuses what uda_score_images refuses, and max_rows < 1, tau < 0 (or
 *                          NaN), invert with one component, no invert with several, gate 1 with invert 1.
 *   uda_pseudo_rows_shape  n (images of the run) and K = the sum of cand.  The first reader of a run waits for it and brings the
 *                          pack's head over in one copy: minmax, kept, cand and the error flag, 24 n + 8 bytes.
 *   uda_get_pseudo_rows    records [K] in (image, rank) order (n_records must be K), minmax [n, 2] float64, kept [n] int32 rows above
 *                          min_score (before the cap), cand [n] int32; any pointer may be NULL.  The K used records, which lie
 *                          behind the head, come over in one copy of 40 K bytes when `records` is given (the room for
 *                          n * min(M, max_rows) records is never copied).  A candidate whose class id is not one of
 *                          1..num_classes is an error. */
int uda_pseudo_rows(uda_ctx_t* ctx, const uda_score_desc_t* desc, int32_t invert, int32_t gate, float min_score, double tau,
                    int32_t max_rows);
int uda_pseudo_rows_shape(uda_ctx_t* ctx, int32_t* n, int64_t* K);
int uda_get_pseudo_rows(uda_ctx_t* ctx, void* records, int64_t n_records, double* minmax, int32_t* kept, int32_t* cand);
/* The same without a handle: the argument list of uda_score_images_np / _np_f32, then the five scalars and the outputs.  records
 * holds room for n * min(M, max_rows) records; *n_records receives K. */
int uda_pseudo_rows_np(int32_t device, const uda_score_desc_t* desc, double min_score, const double* boxes, const double* scores,
                       const double* classes, const double* entropy, const double* albox, const double* mcbox,
                       const double* mcclass, int32_t n, int32_t M, int32_t num_classes, int32_t mcclass_cols, int32_t invert,
                       int32_t gate, double tau, int32_t max_rows, void* records, int64_t* n_records, double* minmax,
                       int32_t* kept, int32_t* cand);
int uda_pseudo_rows_np_f32(int32_t device, const uda_score_desc_t* desc, float min_score, const float* boxes, const float* scores,
                           const float* classes, const float* entropy, const float* albox, const float* mcbox,
                           const float* mcclass, int32_t n, int32_t M, int32_t num_classes, int32_t mcclass_cols, int32_t invert,
                           int32_t gate, double tau, int32_t max_rows, void* records, int64_t* n_records, double* minmax,
                           int32_t* kept, int32_t* cand);

/* COCO evaluation: the matching half of the metric eval.py and the training-time COCOCallback hand their detections to
 * (coco_metric.EvaluationMetric, coco_metric.py:59-283, which runs pycocotools' COCOeval and custom_cocoeval.COCOeval_all) -
 * evaluateImg (custom_cocoeval.py:265-349) for every (image, category, area range, IoU threshold) at maxDets[-1] = 100 - done on
 * the detections RESIDENT in the handle after a post-process in either mode (per class is the main caller: eval.py:117-123).
 * accumulate / summarize (custom_cocoeval.py:351-545) are the caller's (coco_metric.py of the package), on the records.
 *   detections    a row is used iff class > -1 (coco_metric.py:235); its category is int(class); box [x1, y1, x2 - x1, y2 - y1] in
 *                 float32 (postprocess.transform_detections, postprocess.py:874-887), area = float32 w * h (pycocotools loadRes on
 *                 the float32 rows; stated from knowledge of pycocotools, which the reference imports but does not contain)
 *   ground truth  [n, G, 7] float32 rows y1, x1, y2, x2, is_crowd, area, class (coco_metric.py:256-275): rows with class <= -1 are
 *                 padding; box [x1, y1, x2 - x1, y2 - y1] and area (x2 - x1) * (y2 - y1) in float32, the area column is not read;
 *                 crowd = int(is_crowd) != 0.  G <= UDA_EVAL_MAX_GT rows per image (the reference's max_instances_per_image is
 *                 100); a larger G is refused, never truncated.  Classes must be whole numbers in 1..num_classes and all values
 *                 finite (the Python layer checks).
 *   IoU           pycocotools bbIou in float64 on the float32 values: iw = min(dx + dw, gx + gw) - max(dx, gx), ih likewise, 0 when
 *                 either is <= 0, else i = iw * ih and i / (crowd ? dw * dh : dw * dh + gw * gh - i)
 *   matching      detections of one (image, category) by score descending, stable, the first 100; ground truth non-ignored rows
 *                 first, stable, ignored = crowd or area outside [lo, hi] of (0, 1e10), (0, 1024), (1024, 9216), (9216, 1e10),
 *                 both ends inclusive; per threshold t the greedy scan of custom_cocoeval.py:307-330 from min(t, 1 - 1e-10): an
 *                 equal IoU moves the match to the later row, a crowd may be matched again, the scan stops at the ignored rows
 *                 once a non-ignored match is in hand; an unmatched detection whose own area is outside the range is ignored
 *   record        per detection row: rank inside its (image, category), 0-based, -1 when the row is unused or its category is not
 *                 one of 1..num_classes; bit t of matched[a] / ignored[a] per area range a; rows of rank >= 100 keep their rank
 *                 and carry zero masks */
#define UDA_EVAL_MAX_GT 256
#define UDA_EVAL_MAX_THRS 32
typedef struct uda_eval_record {
  float score;
  int32_t cls;
  int32_t rank;
  uint32_t matched[4];
  uint32_t ignored[4];
} uda_eval_record_t;   /* 44 bytes */
/*   uda_set_eval_ground_truth  gt [n, G, 7]; the handle's buffers hold max_images x G rows and grow only when G grows
 *                              (as uda_set_ground_truth's do).  Refuses n outside 1..max_images and G above UDA_EVAL_MAX_GT.
 *   uda_eval_match             iou_thrs [T] float64, T in 1..UDA_EVAL_MAX_THRS (pycocotools' linspace(0.5, 0.95, 10), COCOeval_all's
 *                              linspace(0.05, 0.95, 19), or both in one pass); queues the match kernel on the handle's stream;
 *                              forces the deferred fix-ups every reader of detections forces.  Refuses: no ground truth set, no
 *                              post-process yet, n different from the run's image count, a pipelined run still in flight, T out
 *                              of range, max_output_size above 4096.
 *   uda_get_eval_records       records [n, max_output_size] x 44 bytes, npig [n, num_classes, 4] int32 non-ignored ground-truth
 *                              rows per class id and area range, used [n] int32 used detection rows (an image with none is not
 *                              evaluated, coco_metric.py:237-238); one copy; any pointer may be NULL. */
int uda_set_eval_ground_truth(uda_ctx_t* ctx, const float* gt, int32_t n, int32_t G);
int uda_eval_match(uda_ctx_t* ctx, const double* iou_thrs, int32_t T);
int uda_get_eval_records(uda_ctx_t* ctx, void* records, int32_t* npig, int32_t* used);
/* The same match without a handle, in the manner of uda_assign_gt_np: host arrays det_rows [n, M, 7] float32 (image id, x, y, w, h,
 * score, class - what transform_detections returns and update_state takes, coco_metric.py:230-231; the image id is not read) and
 * gt [n, G, 7]; the same kernel in its legacy-row layout, the same outputs.  For the nms_np route and for callers that hold rows
 * of their own.  M <= 4096, G <= UDA_EVAL_MAX_GT, T in 1..UDA_EVAL_MAX_THRS, num_classes in 1..8192. */
int uda_eval_match_np(int32_t device, const float* det_rows, const float* gt, int32_t n, int32_t M, int32_t G, int32_t num_classes,
                      const double* iou_thrs, int32_t T, void* records, int32_t* npig, int32_t* used);

/* Thresholding: the objective of the failure-recognition search (UncertOptimal._extract_optimal_params / roc_metrics,
 * uncertainty_analysis.py:44-152) for P candidate weight vectors and K IoU thresholds in one call, without a handle.  Host arrays:
 * uncerts [U, N] float64, ious [N] float64, tp_class [N] uint8 (class == gt class), group [N] int32 in 0..G-1 or NULL with G = 0,
 * iou_thrs [K], params [P, U * max(G, 1)]; outputs thr / rate / auc [P, K] float64 (any may be NULL).
 *   score      u[i] = params[p, 0] * uncerts[0, i] + params[p, 1] * uncerts[1, i] + ...; with groups params[p, group[i] * U + j];
 *              float64, every product rounded, added left to right, never fused; -0.0 counts as 0.0
 *   labels     correct = (ious[i] >= iou_thrs[k]) && tp_class[i]; the curve's positive class is correct == 0 (pos_label=0)
 *   curve      sklearn's roc_curve with drop_intermediate=True (sklearn >= 1.3): scores descending, one point at the end of each
 *              run of equal scores (tps = positives so far, fps = 1 + index - tps); with more than 2 points a point stays iff it is
 *              first, last, or the second difference of fps or tps at it is non-zero; (0, 0) with threshold +inf in front;
 *              fpr = fps / fps[-1], tpr = tps / tps[-1]
 *   result     fix_cd != 0: rate = 1 - interp(1 - budget, fpr, tpr), thr = thresholds[argmin |1 - tpr - rate|]; else
 *              rate = interp(budget, tpr, fpr), thr = thresholds[argmin |fpr - rate|]; numpy.interp (the last j with xp[j] <= x;
 *              fp[j] when equal, else (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]) * (x - xp[j]) + fp[j]), the first minimum; auc = the
 *              trapezoid sum over the kept points.  A problem with one label only: thr = +inf, rate = auc = NaN.  budget must lie
 *              strictly between 0 and 1: there the two early branches of roc_metrics cannot be taken.
 *   limits     2 <= N <= UDA_THR_MAX_N, 1 <= U <= UDA_THR_MAX_U, 1 <= K <= UDA_THR_MAX_THRS, 1 <= P <= UDA_THR_MAX_P,
 *              0 <= G <= UDA_THR_MAX_G, group ids inside 0..G-1; anything else is refused, never truncated.  Values must be
 *              finite (the Python layer checks).
 *   scratch    allocated and freed inside the call.  Candidates go through in chunks; with Npad = max(2048, N rounded up to a
 *              power of two) one candidate takes 12 * Npad + 8 * N * K + 24 * K + 8 * U * max(G, 1) bytes, and a chunk is as many
 *              candidates as fit 64 MiB (at least one, which takes 70 MiB at the limits; at most 16384): scratch never exceeds
 *              70 MiB whatever P is.  On top: the inputs, 8 * N * (U + 1) + 5 * N bytes, and the mask, 4 * N. */
#define UDA_THR_MAX_N 262144
#define UDA_THR_MAX_U 4
#define UDA_THR_MAX_THRS 32
#define UDA_THR_MAX_P 65536
#define UDA_THR_MAX_G 8192
int uda_thr_objective_np(int32_t device, const double* uncerts, const double* ious, const uint8_t* tp_class, const int32_t* group,
                         int32_t N, int32_t U, int32_t G, const double* iou_thrs, int32_t K, const double* params, int32_t P,
                         int32_t fix_cd, double budget, double* thr, double* rate, double* auc);

/* Thresholding report: the judgement the reference makes of a failure-recognition score right after the search
 * (MainUncertViz._save_thr_performance / _collect_thresh_results, uncertainty_analysis.py:517-749, with calc_jsd,
 * utils_extra.py:25-36) for B segments of rows x S ready score columns x K IoU thresholds in one call, without a handle.  Host
 * arrays: scores [S, N] float64 (the caller forms the combinations), ious [N] float64, tp_class [N] uint8, iou_thrs [K], seg_lo /
 * seg_hi [B] int32: the half-open row ranges [lo, hi) with 0 <= lo <= hi <= N, which may nest, overlap or repeat (the Python layer
 * orders the rows by class, so "all rows" and every class are ranges).  Outputs, in the order the segments were given, any may be
 * NULL:
 *   roc        [B, S, K, 3] float64: thr, rate, auc of roc_metrics(scores[s, lo:hi], correct[lo:hi]) with exactly the semantics
 *              stated for uda_thr_objective_np (labels, pos_label 0, drop_intermediate, numpy.interp, the first argmin, -0.0 as
 *              0.0, the same kernels).  A segment of 0 or 1 rows, or with one label only, gives +inf, NaN, NaN
 *   n_label    [B, K, 2] int64: rows of the segment with correct, rows without
 *   moments    [B, S, K, 2, 2] float64: for the correct rows and for the wrong rows (sum, m2).  sum is the root of the tree
 *              uda_uncert_report_np documents over the segment's rows counted from lo (numpy: b = b[0::2] + b[1::2] over the terms
 *              zero-padded to a power of two, until one value is left); a row outside the subset contributes +0.0 and -0.0 counts
 *              as 0.0.  m2 is the same tree over (u - mean)^2 with mean = sum / n, one IEEE division done on the device, n the
 *              subset's size; the subtraction and the product are rounded on their own.  An empty subset gives 0, 0.  The caller
 *              takes std = sqrt(m2 / n)
 *   removed    [B, S, K, 3] int64, against the thr of the same (b, s, k): wrong && u >= thr (correctly removed), correct &&
 *              u >= thr (falsely removed), wrong && u < thr (falsely remaining).  With thr = +inf nothing is removed.  Wave
 *              ballots and popcounts; no atomics anywhere
 *   limits     2 <= N <= UDA_THR_MAX_N, 1 <= S <= UDA_THR_REPORT_MAX_S, 1 <= K <= UDA_THR_MAX_THRS, 1 <= B <=
 *              UDA_THR_REPORT_MAX_SEGS, ranges inside [0, N], budget strictly between 0 and 1; anything else is refused with a
 *              "uda_thr_report_np: " message, never truncated, and the outputs stay untouched.  Values must be finite (the Python
 *              layer checks)
 *   cost       one upload, one download, no host synchronisation between segments.  Launches are linear in B: per segment of
 *              n >= 2 rows the objective's sort and curve launches for ceil(S / chunk) chunks of columns, then one launch of
 *              B * S * K blocks for counts and moments
 *   scratch    allocated and freed inside the call.  With n the longest segment and Npad = max(2048, n rounded up to a power of
 *              two) one column takes 12 * Npad + 8 * n * K bytes of sort and curve scratch, shared by all segments; a chunk is as
 *              many columns as fit 64 MiB (at least one, which takes 70 MiB at the limits): never above 70 MiB whatever B and S
 *              are.  On top: the inputs, 8 * N * (S + 1) + N + 8 * S * S + 8 * B bytes, the mask, 4 * N, and the outputs,
 *              80 * B * S * K + 16 * B * K. */
#define UDA_THR_REPORT_MAX_S 8
#define UDA_THR_REPORT_MAX_SEGS 16384
int uda_thr_report_np(int32_t device, const double* scores, const double* ious, const uint8_t* tp_class, int32_t N, int32_t S,
                      const double* iou_thrs, int32_t K, const int32_t* seg_lo, const int32_t* seg_hi, int32_t B, int32_t fix_cd,
                      double budget, double* roc, int64_t* n_label, double* moments, int64_t* removed);

/* Heat maps: the spatial maps the reference draws after thresholding (MainUncertViz._plot_validheat, uncertainty_analysis.py:920-1019:
 * `mask[int(y1):int(y2), int(x1):int(x2)] += value[i]` once per row, ten maps over the same rows), M maps of H x W in one call,
 * without a handle.  Host arrays: rects [R, N, 4] int32 (r0, r1, c0, c1), half-open ranges the caller has already resolved the way
 * numpy resolves the slice (post_thresholding.box_slices), 0 <= r0, r1 <= H and 0 <= c0, c1 <= W; r1 <= r0 or c1 <= c0 covers
 * nothing.  values [V, N] float64, finite; sel [Q, N] uint8 row selectors.  Map m reads the rectangle set map_rect[m], the value
 * column map_value[m] (-1: every value is 1.0) and the selector map_sel[m] (-1: every row).
 *   heat       [M, H, W] float64: heat[m, y, x] = s after `s = +0.0; for i = 0 .. N-1: if row i is selected and its rectangle covers
 *              (y, x): s = s + v[i]` - every addition rounded on its own, in row order, which is numpy's slice += loop bit for bit.
 *              With map_mean[m] != 0 the stored value is count ? s / count : +0.0, one IEEE division (the reference's
 *              np.nan_to_num(mask / normalizer) for finite sums)
 *   count      [M, H, W] int32: the number of such rows; may be NULL
 *   limits     1 <= N <= UDA_THR_MAX_N, 1 <= M <= UDA_HEAT_MAX_MAPS, 1 <= R <= UDA_HEAT_MAX_RECTS, 0 <= V <= UDA_HEAT_MAX_VALUES,
 *              0 <= Q <= UDA_HEAT_MAX_SELS, 1 <= H, W and H * W <= UDA_HEAT_MAX_PIXELS, every table index inside its table, every
 *              rectangle inside the map (checked on the host inside the call); anything else is refused with a
 *              "uda_heat_maps_np: " message, never truncated, and the outputs stay untouched
 *   shape      one block of UDA_HEAT_CHUNK threads per (tile of UDA_HEAT_TILE_H x UDA_HEAT_TILE_W pixels, map), sums and counts in
 *              registers; the rows go through in chunks of UDA_HEAT_CHUNK in row order, the rows whose rectangle meets the tile
 *              are compacted into LDS in row order (ballot, popcount, prefix over the waves) and walked by all threads.  No
 *              atomics; the result does not depend on the launch shape.  Every block reads all N rows of its map's tables
 *   scratch    allocated and freed inside the call: the inputs, 16 * R * N + 8 * V * N + Q * N bytes, and the outputs,
 *              8 * M * H * W (+ 4 * M * H * W with count) */
#define UDA_HEAT_TILE_H 32
#define UDA_HEAT_TILE_W 64
#define UDA_HEAT_CHUNK 256
#define UDA_HEAT_MAX_MAPS 16
#define UDA_HEAT_MAX_RECTS 4
#define UDA_HEAT_MAX_VALUES 16
#define UDA_HEAT_MAX_SELS 8
#define UDA_HEAT_MAX_PIXELS 4194304
int uda_heat_maps_np(int32_t device, const int32_t* rects, int32_t R, const double* values, int32_t V, const uint8_t* sel, int32_t Q,
                     int32_t N, const int32_t* map_rect, const int32_t* map_value, const int32_t* map_sel, const int32_t* map_mean,
                     int32_t M, int32_t H, int32_t W, double* heat, int32_t* count);

/* Post-thresholding tallies: what MainUncertViz._plot_metricsspider (uncertainty_analysis.py:1024-1068) and
 * _collect_postthresholding (:838-880) count, given the thresholds uda_thr_report_np found, without a handle.  Host arrays: u [N]
 * float64 (the combined score), ious [N] float64, tp_class [N] uint8, iou_thrs / thrs [K] float64, image [N] int32 ids in 0..I-1
 * (read only with k_img >= 0).  correct = tp_class && iou >= iou_thrs[k]; side 0 is u >= thrs[k] (removed), side 1 is u < thrs[k]
 * (remaining).  Outputs, any may be NULL:
 *   counts     [K, 2, 4] int64: per side its rows, its tp_class rows, its correct rows, its wrong rows (ballots and popcounts)
 *   iou_sum    [K, 2] float64: the sum of iou over the side's rows - the root of the zero-padded pairwise tree
 *              uda_uncert_report_np documents, over all N rows from row 0; a row of the other side contributes +0.0 and -0.0
 *              counts as 0.0
 *   img_count  [I, 4] int32, at threshold k_img: the image's correctly removed (wrong, side 0), falsely removed (correct, side 0)
 *              and falsely remaining (wrong, side 1) rows, and its rows with u >= thr
 *   img_first  [I, 3] int32: the lowest row index of each of the three kinds, N where the image has none.  Both per-image outputs
 *              are built with integer atomicAdd / atomicMin only; k_img = -1 skips them
 *   limits     2 <= N <= UDA_THR_MAX_N, 1 <= K <= UDA_THR_MAX_THRS, -1 <= k_img < K, with k_img >= 0: 1 <= I <= N and every id
 *              inside 0..I-1.  thrs may be +inf (nothing is removed); a NaN in u, ious, iou_thrs or thrs is refused.  Anything else
 *              is refused with a "uda_thr_post_np: " message, never truncated, and the outputs stay untouched
 *   cost       one launch of K blocks, one packed download */
int uda_thr_post_np(int32_t device, const double* u, const double* ious, const uint8_t* tp_class, const int32_t* image, int32_t N,
                    int32_t I, const double* iou_thrs, const double* thrs, int32_t K, int32_t k_img, int64_t* counts,
                    double* iou_sum, int32_t* img_count, int32_t* img_first);

/* Dataset pruning: the quadratic part of the active-learning loop's `prune` strategies (ActiveLearning.extract_hash_matrix,
 * active_learning_loop.py:198-316) - for N image hashes the maximum Hamming distance over all pairs and, per image, the images
 * within a limit of it - without a handle and without the N x N matrix the reference builds (:240-245).  The draws, the removal
 * and the budget (:281-314) are the caller's (dataset_pruning.py).
 *   hashes     [N, W] uint64, W = 1..4 words of 64 hash bits (imagehash's hash_size 8 is W = 1, 16 is W = 4); any packing order,
 *              as long as every hash uses the same one.  1 <= N <= UDA_PRUNE_MAX_N
 *   distance   d(i, j) = sum over the W words of popcount(a ^ b) (ImageHash.__sub__); *max_dist = max over all i, j (:264)
 *   limit      max_distance >= 0: that many bits, prune_thr is not read; else the float64 product (double)*max_dist * prune_thr
 *              (:267), prune_thr >= 0 and finite.  Column j is in row i iff (double)d(i, j) <= limit: inclusive, i itself included
 *   result     CSR: row i is idx[row_off[i] .. row_off[i + 1]), ascending (np.where(...)[0]); row_off [N + 1] int64,
 *              *total = row_off[N].  max_dist, row_off and total are always written; idx is written only when it is not NULL and
 *              *total <= cap (its capacity in entries): NULL is a count-only call, a short cap leaves idx untouched and the
 *              caller comes back with cap = *total.  Integer-exact: the result does not depend on how the device cuts the work.
 *   scratch    allocated and freed inside the call: the hashes, 8 * N * W bytes, counts and cursors of 12 bytes per (row, column
 *              span) - at most 262144 + N of those - and 8 * (N + 1) for row_off; the index array, 4 * *total bytes, only after
 *              the total is known, and refused with both sizes in the message when the device does not have them free.
 * UDA_PRUNE_ROWS rows make a block, one per thread; UDA_PRUNE_COLS column hashes are staged in LDS at a time. */
#define UDA_PRUNE_ROWS 256
#define UDA_PRUNE_COLS 512
#define UDA_PRUNE_MAX_N 1048576
int uda_hash_neighbors_np(int32_t device, const uint64_t* hashes, int32_t N, int32_t W, double prune_thr, int32_t max_distance,
                          int64_t cap, int32_t* max_dist, int64_t* row_off, int32_t* idx, int64_t* total);

/* Dataset pruning, the hashes: what the reference computes for every pool image before the search above
 * (active_learning_loop.py:215-224) - Image.open(..).resize((512, 256)) and imagehash.phash - from the decoded pixels on, for N
 * ragged RGB images in one call, without a handle.  Decoding, and any image that is not RGB, stay the caller's
 * (dataset_pruning.py).
 *   wh, pix    wh [N, 2] int32 = (width, height); the packed RGB planes (row-major, 3 bytes a pixel) one after another in pix
 *   recipe     1. Image.resize((512, 256)) with Pillow's default filter for RGB, BICUBIC: the passes of uda_resample_np with the
 *                 table of uda_resample_coeffs_filter_np(.., UDA_FILTER_BICUBIC, ..) - along x first and rounded to uint8, a
 *                 pass whose axis keeps its length skipped, along y first for a plane more than 100 times as tall as wide whose
 *                 height shrinks.  Bit for bit Pillow's
 *              2. convert("L"): (R 19595 + G 38470 + B 7471 + 0x8000) >> 16
 *              3. resize((32, 32), Image.LANCZOS) of that plane, the same 8-bit arithmetic on one channel: thumb, bit for bit
 *                 Pillow's
 *              4. the 8 x 8 low corner of scipy.fftpack.dct (type 2, unnormalised) along axis 0 and then axis 1, in float64 as
 *                 direct sums with T[k][i] = 2.0 * cos(M_PI * k * (2 i + 1) / 64.0) (uda_phash_table_np hands out these 8 x 32
 *                 values; host only): a[k][j] = sum_i T[k][i] thumb[i][j], i ascending from 0.0, then low[k][l] = sum_j a[k][j]
 *                 T[l][j], j ascending; every product rounded, then every sum, never an FMA.  Bit-equal to a numpy loop in that
 *                 order; equal to scipy's FFT only to rounding
 *              5. med = the mean of the two middle values of low (numpy's median), bit 8 k + l = low[k][l] > med
 *   words      [N] uint64: the 64 bits row-major, the first bit the most significant - int(str(imagehash value), 16)
 *   margin     [N] doubles: min over the 64 values of |low - med|.  A bit whose value lies within rounding of the median is not
 *              determined by a direct sum or by an FFT: the caller compares margin with a bound of its own and settles such an
 *              image from thumb (dataset_pruning.PHASH_TIE).  A constant image has margin ~ 0: its AC terms are noise here
 *   thumb      [N, 32, 32] uint8, may be NULL;  low [N, 64] doubles, may be NULL
 *   limits     N >= 0 (N = 0 writes nothing), every side in 1 .. UDA_RESAMPLE_MAX_SIDE, and the call's device bytes - 393 216 an
 *              image for its 512 x 256 plane, its source, and 3 * 512 * h for the first pass's result when both axes change
 *              (3 * w * 256 where y goes first) - at most UDA_PHASH_MAX_BYTES.  A NULL wh, pix, words or margin and anything
 *              else is refused with a "uda_phash_np: " message, and the outputs stay untouched
 *   cost       one allocation, one upload of the pixels, up to three launches of the resample passes and one of the tail (a
 *              block an image, 37 648 bytes of LDS) on one stream without a host synchronisation in between, four downloads */
#define UDA_PHASH_PRE_W 512
#define UDA_PHASH_PRE_H 256
#define UDA_PHASH_SIDE 32
#define UDA_PHASH_LOW 8
#define UDA_PHASH_MAX_BYTES 4294967296LL           /* device bytes a call, 2^32 */
int uda_phash_np(int32_t device, int32_t N, const int32_t* wh, const uint8_t* pix, uint64_t* words, double* margin, uint8_t* thumb,
                 double* low);
int uda_phash_table_np(double* T);

/* Set similarity: the neighbour search of the active-learning evaluation's set-similarity analysis (emp_KL_divergence,
 * active_learning_eval.py:458-492, called twice per (class, method) by empirical_jensen_shannon_divergence :495-583 under
 * Similarity.calculate_set_similarity :946-1029) - for B independent problems in one call, the squared Euclidean distance from
 * every query point to its nearest reference point, in float64, without a handle and without the reference's KD-trees.  The KDE,
 * the resampling, the square root, the logarithms and the sums are the caller's (set_similarity.py).
 *   problems   problem b has n_b = q_off[b + 1] - q_off[b] query points, rows q_off[b].. of queries [q_off[B], D], and m_b =
 *              r_off[b + 1] - r_off[b] reference points, rows r_off[b].. of refs [r_off[B], D]; q_off[0] = r_off[0] = 0
 *   distance   d2(i, j) = ((x0 - y0)^2 + (x1 - y1)^2) + ... over the D coordinates in ascending order; every subtraction,
 *              product and sum is rounded on its own (never fused).  d2[q_off[b] + i] = min over j of d2(i, j); no square root
 *   self       self[b] != 0: the references ARE the queries (the caller passes the same points, m_b = n_b is not checked) and
 *              reference row j == query row i is left out - an exact copy elsewhere is not, and gives 0.  A self problem with
 *              m_b == 1 has no neighbour and yields +inf (KDTree.query(k=2)[:, 1]).  self == NULL: no problem is one
 *   result     a minimum does not depend on the order it is taken in: d2 does not depend on how the device cuts the work, and
 *              equals a sequential numpy sum with np.min bit for bit - for D <= 4 also scipy's cKDTree queried with eps=0
 *              (squared).  Differences whose squares overflow give +inf, as numpy does
 *   limits     1 <= D <= UDA_KNN_MAX_D, 1 <= B <= UDA_KNN_MAX_B, offsets ascending with 1 <= n_b, m_b <= UDA_KNN_MAX_N, and the
 *              sum of n_b * m_b at most UDA_KNN_MAX_PAIRS; anything else is refused, never truncated, and d2 stays untouched.
 *              UDA_KNN_MAX_PAIRS is there so that one call does not occupy a shared card for long; the time it corresponds to
 *              has NOT been measured.  Values must be finite (the Python layer checks)
 *   scratch    allocated and freed inside the call: the points, 8 * D * (q_off[B] + r_off[B]) bytes, the result, 8 * q_off[B],
 *              the tables, 16 * (B + 1) + B, and 16 bytes per work item - at most max(2047, the row blocks of all problems).
 * UDA_KNN_ROWS queries make a block, one per thread; UDA_KNN_COLS reference points are staged in LDS at a time. */
#define UDA_KNN_ROWS 256
#define UDA_KNN_COLS 512
#define UDA_KNN_MAX_D 4
#define UDA_KNN_MAX_N 1048576          /* points per set */
#define UDA_KNN_MAX_B 4096             /* problems per call */
#define UDA_KNN_MAX_PAIRS (1ll << 38)  /* sum of n_b * m_b per call */
int uda_nn_dist2_np(int32_t device, int32_t D, int32_t B, const double* queries, const int64_t* q_off, const double* refs,
                    const int64_t* r_off, const uint8_t* self, double* d2);

/* Gaussian KDE evaluation: the expensive step of the epistemic-vs-aleatoric comparison (EpistemicVSAleatoric.get_plot_grid,
 * uncertainty_ep_vs_al.py:361-375: scipy.stats.gaussian_kde on a 100 x 100 mesh) and `kde.pdf` in general - for B independent
 * problems in one call, the sum of Gaussian terms of every evaluation point over the problem's data rows, in float64, without a
 * handle.  Whitening and normalisation are the caller's, split as scipy splits them (epal.py): rows and points arrive as
 * solve_triangular(cho_cov, x, lower=True), and the caller multiplies the sum by (2 pi)^(-D/2) / prod(diag(cho_cov)).
 *   problems   problem b has n_b = d_off[b + 1] - d_off[b] data rows, rows d_off[b].. of data [d_off[B], D] and of weight
 *              [d_off[B]], and m_b = p_off[b + 1] - p_off[b] evaluation points, rows p_off[b].. of points [p_off[B], D];
 *              d_off[0] = p_off[0] = 0
 *   term       arg(i, j) = ((p0 - d0)^2 + (p1 - d1)^2) + ... over the D coordinates in ascending order; every subtraction,
 *              product and sum is rounded on its own (never fused).  term(i, j) = w_i * exp(arg * -0.5), exp in float64 (within
 *              an ulp; no fast or float variant); weight == NULL: every w_i is 1 and the multiplication is left out
 *   sum        sum[p_off[b] + j] = the sum of term(i, j) over the rows i of problem b, in an order that is a function of n_b
 *              alone: the rows are cut into runs of UDA_KDE_RUN, aligned to the problem's first row (the last run may be
 *              short); a run is summed sequentially from 0.0, row by row; the run sums are folded as the zero-padded pairwise
 *              tree of uda_uncert_report_np (numpy: b = b[0::2] + b[1::2] until one value is left).  Nothing depends on how
 *              points or rows are dealt to threads, blocks or launches: a point gives the same bits in a call of its own,
 *              inside a batch of other problems and at any position of `points`.  Terms that underflow count as what exp gives
 *   limits     1 <= D <= UDA_KDE_MAX_D, 1 <= B <= UDA_KDE_MAX_B, offsets ascending from 0 with 1 <= n_b <= UDA_KDE_MAX_N and
 *              0 <= m_b, and the sum of n_b * m_b at most UDA_KDE_MAX_PAIRS; anything else is refused, never truncated, and sum
 *              stays untouched.  UDA_KDE_MAX_PAIRS is there so that one call does not occupy a shared card for long; the time
 *              it corresponds to has NOT been measured.  Values must be finite (the Python layer checks)
 *   scratch    allocated and freed inside the call: rows, weights and points, 8 * ((D + 1) * d_off[B] + D * p_off[B]) bytes, the
 *              result, 8 * p_off[B], the run sums, 8 bytes per (run, point) of every problem - at most 8 * (UDA_KDE_MAX_PAIRS /
 *              UDA_KDE_RUN + p_off[B]) - the offsets, 24 * (B + 1), and 16 bytes per work item and 8 per block of points.
 * UDA_KDE_POINTS points make a block, one per thread; one run of data rows and weights is staged in LDS at a time. */
#define UDA_KDE_POINTS 256
#define UDA_KDE_RUN 256
#define UDA_KDE_MAX_D 4
#define UDA_KDE_MAX_N 1048576          /* data rows per problem */
#define UDA_KDE_MAX_B 4096             /* problems per call */
#define UDA_KDE_MAX_PAIRS (1ll << 36)  /* sum of n_b * m_b per call */
int uda_kde_eval_np(int32_t device, int32_t D, int32_t B, const double* data, const int64_t* d_off, const double* weight,
                    const double* points, const int64_t* p_off, double* sum);

/* Pseudo-label audit: how the STAC teacher's pseudo labels compare with the ground truth (Parent_SSL.extract_pseudo_gt_data and
 * _percls_analysis, ssl_utils/parent.py:1567-1813; its members feed ThreeDproblem.corrected_pseudo, 3d.py:80-255, and
 * Advanced_Pseudo_Labels._pls, pls.py:102-282) - for B ragged images in one call, without a handle.  Classes, the tallies per
 * class, the label files and the PLS scores are the caller's (pseudo_audit.py, writers.py).
 *   images     image b has G_b = gt_off[b + 1] - gt_off[b] ground-truth rows, rows gt_off[b].. of gt_boxes [gt_off[B], 4], and D_b =
 *              det_off[b + 1] - det_off[b] pseudo labels, rows det_off[b].. of det_boxes [det_off[B], 4]; gt_off[0] = det_off[0] = 0.
 *              Boxes are float64 in the order the reference's readers give (the IoU is symmetric in the two axes)
 *   iou        calc_iou_np (utils_box.py:56-89) in float64: (areaA + areaB) - inter, 0 where the union is 0; never fused
 *   per row    gt_max_iou[g] = max over the image's labels, gt_best_det[g] = the first label that reaches it (np.argmax,
 *              :1736-1737; index within the image).  The MATCHED PREDICTIONS of an image are the distinct gt_best_det of its
 *              rows with gt_max_iou >= gt_iou_thr (np.unique, :1736-1738), in ascending order; n_matches[b] counts them
 *   per label  det_max_iou[d] = max over the image's rows, det_best_gt[d] = the first row that reaches it (3d.py:150-152)
 *   allocation every matched prediction, in ascending order, takes the row of the best (IoU, lower row) among the rows not
 *              yet taken (:1744-1752): det_alloc_gt[d] is that row (-1: d is not a matched prediction), gt_alloc_det[g] the
 *              prediction that took row g (-1: none).  A prediction may take a row that did not choose it
 *   ious       det_alloc_pair_iou[d] = IoU of the allocated pair (_percls_analysis :1572-1581; 0 where not allocated);
 *              det_alloc_miou[d] = np.max of the row in the reference's MUTATED matrix (:1763-1765): the maximum over the
 *              labels e of IoU(row, e), where an entry counts as -1 iff e is a matched prediction after d, and (IoU(row, e),
 *              lower row) beats the row e took.  It may be below gt_max_iou of the row, and it may be -1
 *   flags      det_flags[d] & UDA_AUDIT_DET_EXTRA: the label's box equals no allocated label's box in all four coordinates
 *              (`pb[i] not in ab`, :1614-1619: the duplicate of an allocated box is not extra); gt_flags[g] &
 *              UDA_AUDIT_GT_NOMATCH: the row's box equals no allocated row's box (:1629-1636)
 *   empty      the reference raises on an image without a row or without a label.  Here such an image has no match: every
 *              label is extra, every row unmatched, the maxima are 0 and the best indices -1
 *   outputs    caller-allocated, length gt_off[B] per row, det_off[B] per label, B per image; any of them may be NULL.  Every
 *              output is exact and does not depend on how the device deals rows to waves
 *   limits     1 <= B <= UDA_AUDIT_MAX_B, offsets ascending from 0, at most UDA_AUDIT_MAX_G rows and UDA_AUDIT_MAX_D labels per
 *              image, gt_iou_thr finite; anything else is refused, never truncated, and the outputs stay untouched.  The
 *              allocation is sequential within an image (one wave, about G * D IoUs at worst); the caps bound it at about a
 *              million IoUs per image so that one call does not occupy a shared card for long - the time this corresponds to
 *              has NOT been measured.  Values must be finite (the Python layer checks); an IoU that is NaN orders as -1
 *   scratch    allocated and freed inside the call: the boxes, 32 * (gt_off[B] + det_off[B]) bytes, the offsets, 16 * (B + 1), and
 *              the results, 17 bytes per row, 33 per label and 4 per image. */
#define UDA_AUDIT_DET_EXTRA 1    /* det_flags */
#define UDA_AUDIT_GT_NOMATCH 1   /* gt_flags */
#define UDA_AUDIT_MAX_G 1024     /* ground-truth rows per image */
#define UDA_AUDIT_MAX_D 1024     /* pseudo labels per image */
#define UDA_AUDIT_MAX_B 1048576  /* images per call */
int uda_pseudo_audit_np(int32_t device, int32_t B, const double* gt_boxes, const int64_t* gt_off, const double* det_boxes,
                        const int64_t* det_off, double gt_iou_thr, double* gt_max_iou, int32_t* gt_best_det, int32_t* gt_alloc_det,
                        uint8_t* gt_flags, double* det_max_iou, int32_t* det_best_gt, int32_t* det_alloc_gt, double* det_alloc_miou,
                        double* det_alloc_pair_iou, uint8_t* det_flags, int32_t* n_matches);

/* Validation uncertainty report: the tallies from which the reference judges a box sigma - the header numbers and the ECE of
 * ValidUncertPlot.__init__ (utils_extra.py:378-445: % missing detections, misclassification rate, mIoU, RMSE, ECE), the line of
 * RegressionCalib._conf_all (calibrate_regression.py:231-349: share of rows inside +-sigma, ECE, NLL, RMSUE, sharpness) and
 * _relative_calc_ece (:46-61) - for B ragged segments of matched rows and K sigma columns in one call, without a handle.  The
 * divisions, square roots, roundings and the text are the caller's (uncertainty_report.py).
 *   segments   segment b is rows off[b] .. off[b + 1] of gt [rows, 4], pred [rows, 4], gt_class [rows], cls [rows] (all float64)
 *              and of every column of sigma [K, rows, 4]; rows = off[B].  A caller makes one segment per class, or one of all rows
 *   levels     z [L], computed by the caller as norm.ppf((1 - p_m) / 2); for np.linspace(0, 1, 100) z[0] = 0 and z[99] = -inf
 *   seg_counts [B, 4] int64: n_rows | n_iou_zero, the rows with calc_iou_np(gt, pred) == 0 (utils_box.py:56-89 in float64: (areaA +
 *              areaB) - inter, 0 where the union is 0; never fused) | n_misclassified, the rows with gt_class != cls |
 *              n_gt_nonzero, the ELEMENTS with gt != 0 (the mask of calc_rmse)
 *   col_counts [B, K, 3] int64: covered_all, the rows where all four coordinates have pred - sigma <= gt && gt <= pred + sigma
 *              (_conf_all:258-265) | n_res_nonzero, the elements with |gt - pred| != 0 (the mask of calc_rmse(residuals, sigma)) |
 *              n_degenerate, the sigma elements that are 0 or not finite
 *   ece_count  [B, K, 4, L] int64: for coordinate c and level i the rows with fabs(pred - gt) <= fabs(sigma * z[i]), evaluated
 *              in IEEE float64 level by level, the product rounded on its own.  NaN rule: a comparison with a NaN is false, as
 *              in numpy - sigma = 0 with z = -inf, an infinite sigma with z = 0 and a NaN sigma count for nothing.  Nothing is
 *              inferred from the order of the levels.  emp_conf = count / n and np.mean(np.abs(emp_conf - p_m)) are calc_ece's
 *              bit for bit, over the four coordinates together for its flattened form
 *   sums       float64.  Every sum is the root of a perfect binary tree over the segment's per-row terms, the sequence zero-
 *              padded to a power of two, a node being left + right (numpy: b = b[0::2] + b[1::2] until one value is left); a
 *              row's term is (t0 + t1) + (t2 + t3) of its four coordinates.  The result does not depend on how rows are dealt
 *              to waves, blocks or launches.  Apart from the log every operation is one correctly rounded IEEE operation
 *   seg_sums   [B, 2]: S_iou (a row's term is its IoU) | S_sqerr = sum (pred - gt)^2 [gt != 0]
 *   col_sums   [B, K, 3]: S_sigma2 = sum sigma^2 | S_ue = sum (sigma - |gt - pred|)^2 [|gt - pred| != 0] | S_nll = sum ((y * y / 2 +
 *              log(sigma)) + 0.9189385332046727) with y = |gt - pred| / sigma, over the elements that are not degenerate
 *   degenerate the reference's calc_nll turns sigma = 0 into +-1.8e308 through nan_to_num, an overflow artefact; here an element
 *              whose sigma is 0 or not finite is left out of S_nll and counted in n_degenerate.  A negative sigma is not
 *              degenerate: its log is NaN, as scipy's
 *   empty      an empty segment gives zeros and is not an error
 *   outputs    caller-allocated; any of them may be NULL
 *   limits     1 <= B <= UDA_REPORT_MAX_B, 1 <= K <= UDA_REPORT_MAX_K, 1 <= L <= UDA_REPORT_MAX_L, off ascending from 0, at most
 *              UDA_REPORT_MAX_ROWS rows; off and z not NULL, nor any input array when there are rows.  Anything else is refused
 *              with a "uda_uncert_report_np: " message, never truncated, and the outputs stay untouched
 *   scratch    allocated and freed inside the call: the inputs, (80 + 32 K) bytes a row, 16 (B + 1) + 8 L + 12 bytes a run of
 *              UDA_REPORT_ROWS rows; the results, 8 * B * (6 + K * (6 + 4 L)) bytes; and the run roots, 8 * (2 + 3 K) bytes for
 *              every slot - a segment has as many slots as runs, rounded up to a power of two. */
#define UDA_REPORT_ROWS 256          /* rows a block takes: an aligned run counted from the segment's start */
#define UDA_REPORT_MAX_K 16          /* sigma columns */
#define UDA_REPORT_MAX_L 128         /* levels */
#define UDA_REPORT_MAX_B 4096        /* segments */
#define UDA_REPORT_MAX_ROWS 4194304  /* rows per call, 2^22 */
int uda_uncert_report_np(int32_t device, int32_t B, int32_t K, int32_t L, const int64_t* off, const double* gt, const double* pred,
                         const double* gt_class, const double* cls, const double* sigma, const double* z, int64_t* seg_counts,
                         int64_t* col_counts, int64_t* ece_count, double* seg_sums, double* col_sums);

/* Classification calibration report: the tallies from which the reference draws its reliability diagrams and their titles -
 * ClassificationCalib._calibr_bins (calibrate_classification.py:97-143) as _calibr_plot calls it (:250-440), once per class and once
 * over the arg-max class, with ECE, MCE, Brier, NLL and SCE - for B ragged segments of rows, M probability tables (one per
 * configuration: uncalibrated, TS all, TS per class, isotonic all, isotonic per class) and all C + 1 targets in one call, without a
 * handle.  The divisions, roundings and the text are the caller's (class_report.py).
 *   segments   segment b is rows off[b] .. off[b + 1] of label [rows] (int32, the true class index: the reference's one-hot y_true
 *              is eye(C)[label]) and of every table of prob [M, rows, C] (float64); rows = off[B].  A caller makes one segment of the
 *              reference's 20 % evaluation split, or one per shard
 *   edges      [G, E] float64 with n_edges [G]: row g holds n_edges[g] strictly ascending edges, free of NaN (the rest of the row is
 *              not read).  G = 1: every target bins with row 0 (the reference's np.linspace(0, 1 + 1e-8, 11)); G = B * M * (C + 1):
 *              target t of table m of segment b bins with row (b * M + m) * (C + 1) + t (the quantile strategy; np.quantile and
 *              np.unique are the caller's)
 *   targets    t < C is class t: ypred = prob[m, i, t], ytrue = (label[i] == t).  t = C is the all_classes branch: a = the first
 *              index of row i that holds a NaN if there is one, else the first maximum (numpy.argmax); ypred = prob[m, i, a],
 *              ytrue = (label[i] == a)
 *   bin id     the number of edges e with !(ypred < e): np.digitize(ypred, edges) for ascending edges; a NaN lands in id n_edges.
 *              Ids run 0 .. n_edges, a (segment, table, target) has E + 1 slots; slots past n_edges stay 0.  The reference raises an
 *              IndexError when id n_edges is populated (a value at or above the last edge, or a NaN); here it is counted, and the
 *              caller decides
 *   bin_count  [B, M, C + 1, E + 1] int64: the rows of the bin
 *   bin_hits   [B, M, C + 1, E + 1] int64: the rows of the bin with ytrue set
 *   bin_sum    [B, M, C + 1, E + 1] float64: sum ypred over the bin
 *   brier_sum  [B, M, C] float64: sum (prob[m, i, t] - y)^2 with y = 1.0 or 0.0
 *   nll_sum    [B, M] float64: the row term of Keras's CategoricalCrossentropy() on probabilities, restated from Keras's backend
 *              (categorical_crossentropy, from_logits=False: output /= reduce_sum(output, axis); output = clip_by_value(output,
 *              epsilon, 1 - epsilon) with epsilon = 1e-7; -reduce_sum(target * log(output))) for a one-hot target, in float64 where
 *              TensorFlow would use the tensors' dtype: q = prob[m, i, label[i]] / rowsum, rowsum added left to right in class
 *              order from 0.0; q clipped to [1e-7, 1 - 1e-7]; the term is -log(q).  A row that holds a non-finite entry, or whose
 *              rowsum is 0, is left out of the sum.  The reference's UNCALIBRATED self.nll feeds logits to this loss, which expects
 *              probabilities: that is not reproduced - every table here holds probabilities
 *   tab_counts [B, M, 2] int64: the rows whose q was clipped | the rows left out of nll_sum
 *   sums       every float64 sum is the root of the tree uda_uncert_report_np documents, over the segment's rows with +0.0 as the
 *              term of a row outside the bin (or left out): the sequence zero-padded to a power of two, a node being left + right
 *              (numpy: b = b[0::2] + b[1::2] until one value is left), runs of UDA_CLASSREP_ROWS rows counted from the segment's
 *              start.  The result does not depend on how rows are dealt to waves, blocks or launches.  Apart from the log every
 *              operation is one correctly rounded IEEE operation, never fused.  Counts and hits are integer tallies (wave ballots,
 *              integer atomics); there are no floating-point atomics
 *   empty      an empty segment gives zeros and is not an error
 *   outputs    caller-allocated; any of them may be NULL
 *   limits     1 <= B <= UDA_CLASSREP_MAX_B, 1 <= M <= UDA_CLASSREP_MAX_M, 1 <= C <= UDA_CLASSREP_MAX_C, 2 <= n_edges[g] <= E <=
 *              UDA_CLASSREP_MAX_E, G as above, off ascending from 0, at most UDA_CLASSREP_MAX_ROWS rows, every label in [0, C); off,
 *              edges and n_edges not NULL, nor prob and label when there are rows.  Anything else is refused with a
 *              "uda_class_report_np: " message, never truncated, and the outputs stay untouched
 *   scratch    allocated and freed inside the call: the inputs, (8 M C + 4) bytes a row, 8 E + 4 bytes an edge row, 16 (B + 1) bytes,
 *              12 bytes a run and 4 bytes a segment of more than one run; the results, 8 * B * M * (3 (C + 1) (E + 1) + C + 3) bytes; and, for the segments of more than
 *              one run only, the run roots: 8 * M * ((C + 1) (E + 1) + C + 1) bytes for every slot - such a segment has as many
 *              slots as runs, rounded up to a power of two. */
#define UDA_CLASSREP_ROWS 256          /* rows a block takes: an aligned run counted from the segment's start */
#define UDA_CLASSREP_MAX_B 4096        /* segments */
#define UDA_CLASSREP_MAX_M 8           /* probability tables */
#define UDA_CLASSREP_MAX_C 128         /* classes */
#define UDA_CLASSREP_MAX_E 64          /* edges a row */
#define UDA_CLASSREP_MAX_ROWS 4194304  /* rows per call, 2^22 */
int uda_class_report_np(int32_t device, int32_t B, int32_t M, int32_t C, int32_t G, int32_t E, const int64_t* off, const double* prob,
                        const int32_t* label, const double* edges, const int32_t* n_edges, int64_t* bin_count, int64_t* bin_hits,
                        double* bin_sum, double* brier_sum, double* nll_sum, int64_t* tab_counts);

/* RCC collages: the pixel work of Parent_SSL.crop_collage (ssl_utils/parent.py:505-597) - every `img.resize(size, Image.LANCZOS)`
 * and `paste` of a collage run - as jobs on packed RGB uint8 planes, in one call.  The decisions (which crop goes where, at which
 * size) are the caller's (collage.py).  The result equals Pillow's 8-bit resize bit for bit.
 *   planes     ids 0 .. S - 1 are the S ragged source planes: src_wh [S, 2] = (width, height), their pixels one after another in
 *              src_pix (row-major, 3 bytes a pixel).  Ids S .. S + T - 1 are the T temporaries of tmp_wh [T, 2], scratch of the
 *              call.  Ids S + T .. S + T + N - 1 are the N output planes, each H x W, out [N, H, W, 3].  Temporaries and outputs
 *              start as zeros (Image.new)
 *   jobs       [K, 7] int32: level, source plane, destination plane, x, y, w, h.  A job reads its WHOLE source plane and writes
 *              its w x h resize (Image.resize((w, h), Image.LANCZOS)) into the destination at (x, y); what reaches past the
 *              destination's right or bottom edge is dropped, as Image.paste drops it.  A job whose w x h is its source's size is
 *              a copy, as in Pillow
 *   levels     ascend along the list.  The jobs of a level run together, a level after the one before it on one stream without a
 *              host synchronisation in between, so a job may read what an earlier level wrote.  Within a level no job reads a
 *              plane that a job of the level writes, and no two jobs write the same pixel
 *   arithmetic Pillow's (libImaging/Resample.c).  Per axis and output index xx: scale = in / out, filterscale = max(scale, 1),
 *              support = 3 filterscale, ksize = 2 ceil(support) + 1, center = (xx + 0.5) scale, the window [xmin, xmin + xmax) =
 *              [int(center - support + 0.5), int(center + support + 0.5)) cut to the plane; the weights sinc(x) sinc(x / 3) for
 *              -3 <= x < 3 at x = (i - center + 0.5) / filterscale, evaluated in double with the C library's sin on the host and
 *              divided by their running sum; each turned into fixed point by int(+-0.5 + k 2^22).  A pass accumulates
 *              2^21 + sum pixel * k in int32, shifts right arithmetically by 22 and clamps to 0..255.  The horizontal pass comes
 *              first and is rounded to uint8, then the vertical pass; a pass whose axis keeps its length is skipped
 *              (Image.resize's own rule is kept: a source more than 100 times as tall as wide whose height shrinks is resampled
 *              along y first, that result rounded to uint8, then along x)
 *   limits     S, T, K >= 0, N >= 1, every side of every plane in 1 .. UDA_RESAMPLE_MAX_SIDE, every w and h likewise, x and y
 *              inside the destination, the destination not a source plane; the temporaries and the horizontal passes' results
 *              together at most UDA_RESAMPLE_MAX_SCRATCH bytes.  Anything else is refused with a "uda_resample_np: " message, and
 *              out stays untouched
 *   scratch    allocated and freed inside the call: the planes, w x (source height) x 3 bytes for every job that resamples both
 *              axes ((source width) x h x 3 where y goes first), and the coefficient tables, one for each distinct (in, out) pair: 4 out (2 + ksize) bytes
 * uda_resample_coeffs_np is host only (no device is touched): the table of one axis.  *ksize is always written; bounds [out_size,
 * 2] = (xmin, xmax) and coeffs [out_size, ksize] (zeros past xmax) when they are not NULL, coeffs_cap being the int32 values
 * coeffs holds.
 * uda_resample_coeffs_filter_np is the same with the filter named (the values are Pillow's Image.LANCZOS and Image.BICUBIC):
 * UDA_FILTER_LANCZOS gives the table of uda_resample_coeffs_np; UDA_FILTER_BICUBIC has the support 2 filterscale and the weights
 * ((a + 2) x - (a + 3)) x x + 1 for |x| < 1, (((x - 5) x + 8) x - 4) a for |x| < 2, a = -0.5, every operation in double and
 * rounded on its own in this order - the table of Image.resize's default filter, which uda_phash_np resizes with.  Any other
 * filter is refused. */
#define UDA_FILTER_LANCZOS 1
#define UDA_FILTER_BICUBIC 3
#define UDA_RESAMPLE_TILE 32                       /* output positions a tile of a pass, at most */
#define UDA_RESAMPLE_MAX_SIDE 65536                /* pixels a side, planes and jobs */
#define UDA_RESAMPLE_MAX_SCRATCH 17179869184LL     /* bytes, 2^34 */
int uda_resample_np(int32_t device, int32_t S, const int32_t* src_wh, const uint8_t* src_pix, int32_t T, const int32_t* tmp_wh,
                    int32_t N, int32_t H, int32_t W, int32_t K, const int32_t* jobs, uint8_t* out);
int uda_resample_coeffs_np(int32_t in_size, int32_t out_size, int32_t* ksize, int32_t* bounds, int32_t* coeffs, int64_t coeffs_cap);
int uda_resample_coeffs_filter_np(int32_t in_size, int32_t out_size, int32_t filter, int32_t* ksize, int32_t* bounds, int32_t* coeffs,
                                  int64_t coeffs_cap);

/* RCC's manual augmentations (Parent_SSL.apply_manual_augmentation, ssl_utils/parent.py:261-315, applied at :534-537): the job
 * list of uda_resample_np with an operation per job, so that the augmentation of a resized crop runs between its resize and its
 * paste in the same call.  Planes, levels, limits and refusals are those of uda_resample_np; every pixel equals Pillow's.
 *   jobs       [K, 9] int32: level, source plane, destination plane, x, y, w, h, op, arg.  op 0 is the resize of uda_resample_np
 *              (arg is not read).  For the ops 1-5 w x h must be the source plane's size; the result is written at (x, y) with
 *              the paste's clipping
 *   params     [P] doubles; arg indexes it for the ops 2-4.  noise: the bytes of the op-5 jobs one after another in job-list
 *              order, 3 w h each (row-major, as the plane); noise_bytes is their total
 *   arithmetic channels are independent.  "f32" is IEEE binary32 with every operation rounded on its own: the device code does
 *              not contract a multiply and an add into an FMA (Pillow's x86 build does not, and a fused blend truncates
 *              differently)
 *     op 1  flip (Image.transpose(FLIP_LEFT_RIGHT)): dst[y, x] = src[y, w - 1 - x]
 *     op 2  brightness (ImageEnhance.Brightness(..).enhance(params[arg])): blend(0, factor)
 *     op 3  contrast (ImageEnhance.Contrast): blend(m, factor) with m = int(S / n + 0.5), division and addition in double on
 *           the device, S the exact integer sum over the WHOLE source plane of L = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16
 *           and n its pixel count
 *           blend(deg, factor) (ImagingBlend): a = f32(factor), t = f32(deg) + a * (f32(px) - f32(deg)) in f32; for 0 <= a <= 1
 *           the result is t truncated toward zero, otherwise 0 if t <= 0, 255 if t >= 255, else t truncated
 *     op 4  gaussian blur (ImageFilter.GaussianBlur(params[arg]), ImagingGaussianBlur with 3 passes).  On the host (this is
 *           uda_gauss_box_np): s2 = f32(f32(radius)^2 / 3); L = f32(sqrt(12.0 s2 + 1.0)) and l = f32(floor((L - 1.0) / 2.0)),
 *           the insides in double; a = f32((2 l + 1) (l (l + 1) - 3 s2)), a = f32(a / f32(6 (s2 - (l + 1)^2))), all f32;
 *           fr = f32(l + a).  Then r = int(fr), ww = uint32(f32(2^24) / (fr * 2 + 1)) (f32 division, truncated) and
 *           fw = (2^24 - (2 r + 1) ww) / 2 (integer division).  One pass along a line of length n:
 *             out[x] = (ww * sum_{d = -r..r} in[c(x + d)] + fw * (in[c(x - r - 1)] + in[c(x + r + 1)]) + 2^23) >> 24
 *           in uint32 with c(i) = clamp(i, 0, n - 1) - what Pillow's running accumulator gives, its edgeA > edgeB branch for
 *           windows wider than the line included.  Three passes along x, each rounded to uint8 and feeding the next, then
 *           three along y.  fr = 0 (radius 0) is a copy
 *     op 5  add bytes (np_image + noise on uint8): dst = (src + noise) mod 256; the reference's np.clip after it changes nothing
 *   refusals   as uda_resample_np, and: an op outside 0..5, an arg outside params for the ops 2-4, a parameter that is not
 *              finite or is negative, a radius above UDA_BLUR_MAX_RADIUS, a w x h that is not the source's size for the ops 1-5,
 *              a noise_bytes that is not the op-5 jobs' total.  Each with a "uda_collage_np: " message; out stays untouched
 *   scratch    as uda_resample_np, plus w x h x 3 bytes a blur job (the x stage's result, counted against
 *              UDA_RESAMPLE_MAX_SCRATCH), the noise, and 8 bytes a contrast job
 * A tile of the pointwise ops is UDA_AUGMENT_TILE pixels x 8 rows; a tile of a blur stage is UDA_AUGMENT_TILE positions x
 * UDA_AUGMENT_TILE lines with a halo of 3 (r + 1) positions a side in LDS, r + 1 <= UDA_BLUR_MAX_BOX + 1 for every radius up to
 * UDA_BLUR_MAX_RADIUS (the reference draws 1..3).
 * uda_gauss_box_np is host only (no device is touched, no cap on the radius): the box radius and the weights of one radius. */
#define UDA_AUGMENT_TILE 32
#define UDA_BLUR_MAX_RADIUS 16.0                   /* gaussian radius; box radius r <= UDA_BLUR_MAX_BOX */
#define UDA_BLUR_MAX_BOX 15
int uda_collage_np(int32_t device, int32_t S, const int32_t* src_wh, const uint8_t* src_pix, int32_t T, const int32_t* tmp_wh,
                   int32_t N, int32_t H, int32_t W, int32_t K, const int32_t* jobs /* [K, 9] */, int32_t P, const double* params,
                   int64_t noise_bytes, const uint8_t* noise, uint8_t* out);
int uda_gauss_box_np(double radius, float* fr, uint32_t* ww, uint32_t* fw);

/* Label correction (GLC): the verdicts of the reference's ground-truth label correction (AdvancedLabels, src/ssl_utils/glc.py) -
 * which ground-truth boxes are mistakes, which detections are missing labels, which noisy boxes are replaced by their detection -
 * done on the detections RESIDENT in the handle: the originals of the last uda_run_consistency (their cons_iou stays on the
 * device) against the ground truth of uda_set_ground_truth.  The label files are the caller's (writers.py).
 *   kept          detection k of an image is kept iff score > min_score, in float32 (the rows Infer.iterate_infer writes,
 *                 infer_model.py:842); only kept detections take part, in rank order
 *   counted       a ground-truth row counts iff its class is > 0 (padding rows carry -1, as in the validate mode)
 *   iou / match   iou[g] = max over the kept k of calc_iou_np(gt_g, box_k) (utils_box.py:56-89: float32 differences, float64
 *                 products, (areaA + areaB) - inter, 0 where the union is 0; never fused); det_rank[g] = the first kept k that
 *                 reaches it (np.argmax, glc.py:182-187).  A row that touches nothing is matched to the FIRST KEPT detection
 *   mistakes      UDA_LC_GT_MISTAKE: iou[g] == 0 (:551)
 *   md            UDA_LC_DET_MISSING: a kept detection whose maximum IoU over the counted rows == md_max_inter (np.equal,
 *                 :432-436; md_rule UDA_LC_MD_LE: <=, the synthetic branch :468-472) and cons_iou >= iou_consist
 *   noisy         UDA_LC_GT_NOISY: cons_iou[det_rank[g]] > iou_consist (strict), iou[g] <= correct_max_inter and
 *                 score[det_rank[g]] >= correct_score (float32) (:813-824).  For every detection matched by such a row the
 *                 FIRST counted row matched to it gets the detection's box and UDA_LC_GT_REPLACED - whether or not that row met
 *                 the conditions itself; a later row that did keeps its box (np.where(matched == k)[0][0], :828-833)
 * Two cases the reference does not reach: an image without a kept detection never appears in its file - all its rows get
 * det_rank -1, IoU 0 and no flag; an image without a counted row makes it raise (np.argmax of an empty list) - here every
 * detection's maximum IoU is 0 and the md rule is applied to that.  Every output is exact and does not depend on how the device
 * cuts rows and ranks into waves.  Values must be finite (the Python layer checks). */
#define UDA_LC_MD 1             /* methods: a bit set */
#define UDA_LC_MISTAKES 2
#define UDA_LC_NOISY 4
#define UDA_LC_MD_EQ 0          /* md_rule */
#define UDA_LC_MD_LE 1
#define UDA_LC_GT_MISTAKE 1     /* gt_flags */
#define UDA_LC_GT_NOISY 2
#define UDA_LC_GT_REPLACED 4
#define UDA_LC_DET_KEPT 1       /* det_flags */
#define UDA_LC_DET_MISSING 2
/*   uda_label_check      queues the kernel on the handle's stream; forces the deferred fix-ups every reader of detections forces.
 *                        Refuses: no ground truth set, the last post-process ran per class, a pipelined run still in flight, n
 *                        different from the run's originals, md or noisy asked for when the resident run was not a consistency
 *                        run (mistakes alone needs none), methods outside 1..7, an unknown md_rule, max_output_size above 4096.
 *                        The result buffers belong to the handle and grow only when G grows.
 *   uda_get_label_check  the first reader of a check waits for it and brings the results over in one copy; any pointer may be
 *                        NULL.  det_rank [n, G] int32 resident rank of the matched detection, -1: row not counted or no kept
 *                        detection; iou [n, G] float64; gt_flags [n, G] uint8; gt_boxes_out [n, G, 4] float32 the row's own box,
 *                        or the detection's where replaced; det_flags [n, M] uint8; det_max_iou [n, M] float64 (0: not kept);
 *                        counts [n, 5] int32 kept detections, counted rows, mistakes, replaced rows, missing labels. */
int uda_label_check(uda_ctx_t* ctx, float min_score, double iou_consist, double md_max_inter, int32_t md_rule,
                    double correct_max_inter, float correct_score, int32_t methods);
int uda_get_label_check(uda_ctx_t* ctx, int32_t* det_rank, double* iou, uint8_t* gt_flags, float* gt_boxes_out, uint8_t* det_flags,
                        double* det_max_iou, int32_t* counts);
/* The same without a handle, in the manner of uda_assign_gt_np / uda_score_images_np[_f32]: host arrays boxes [n, M, 4], scores
 * [n, M], cons_iou [n, M] (float64 in both; may be NULL for mistakes alone), gt_boxes [n, G, 4], gt_classes [n, G]; the same
 * kernel, the same outputs.  _np: float64 arrays and all-float64 arithmetic - fed with the values read back from a
 * prediction_data.txt it is the reference's arithmetic bit for bit; _np_f32: float32 arrays, the handle's arithmetic.
 * M <= 4096, G <= 16384, n >= 1; anything else is refused, never truncated, and the outputs stay untouched. */
int uda_label_check_np(int32_t device, const double* boxes, const double* scores, const double* cons_iou, const double* gt_boxes,
                       const double* gt_classes, int32_t n, int32_t M, int32_t G, double min_score, double iou_consist,
                       double md_max_inter, int32_t md_rule, double correct_max_inter, double correct_score, int32_t methods,
                       int32_t* det_rank, double* iou, uint8_t* gt_flags, float* gt_boxes_out, uint8_t* det_flags,
                       double* det_max_iou, int32_t* counts);
int uda_label_check_np_f32(int32_t device, const float* boxes, const float* scores, const double* cons_iou, const float* gt_boxes,
                           const float* gt_classes, int32_t n, int32_t M, int32_t G, float min_score, double iou_consist,
                           double md_max_inter, int32_t md_rule, double correct_max_inter, float correct_score, int32_t methods,
                           int32_t* det_rank, double* iou, uint8_t* gt_flags, float* gt_boxes_out, uint8_t* det_flags,
                           double* det_max_iou, int32_t* counts);

/* serve = set_images_u8 + run + get_detections */
int uda_serve(uda_ctx_t* ctx, const uint8_t* images, int32_t n, int32_t h, int32_t w,
              float* boxes, float* scores, float* classes, int32_t* valid, float* logits);

/* Calibrated box uncertainty of the last global post-process (CalibrateBoxUncert.calibrate_boxuncert,
 * utils_box.py:404-524), on the device.  col0 = first of the four uncertainty columns inside the boxes output (4:
 * aleatoric or the only one, 8: epistemic when both exist).  Isotonic tables are the fitted thresholds of the
 * reference's sklearn IsotonicRegression models: table t = xs/ys[tab_off[t] .. tab_off[t+1]); 1 table (ISO_ALL), 4
 * (ISO_PERCOO: ymin, xmin, ymax, xmax) or 4 * num_classes (ISO_PERCLSCOO, class-major, class ids 1..C);
 * relative != 0 = the rel_iso_perclscoo variant.  temps: 1 or 4 divisors for the TS modes.  out [n, M, 4]. */
enum uda_calib_mode { UDA_CALIB_TS_ALL = 0, UDA_CALIB_TS_PERCOO = 1, UDA_CALIB_ISO_ALL = 2, UDA_CALIB_ISO_PERCOO = 3,
                      UDA_CALIB_ISO_PERCLSCOO = 4 };
int uda_calibrate_box(uda_ctx_t* ctx, int32_t col0, int32_t mode, int32_t relative, int32_t n_tables,
                      const int32_t* tab_off, const double* xs, const double* ys, const float* temps, float* out);

/* Calibrated class probabilities of the last global post-process (class half; CalibrateClass._perform_class_calib /
 * calibrate_class, utils_class.py:109-272), on the device next to the logits they refine.  UDA_CLS_TS: logits / temps[c]
 * (ts_all: the same temperature num_classes times; ts_percls: one per class), stable softmax.  UDA_CLS_ISO_ALL / _PERCLS:
 * stable softmax, then the fitted isotonic table (1, or one per class; thresholds as in uda_calibrate_box), re-normalised to
 * sum 1.  draws == 0: the mean logits are calibrated (model without MC class uncertainty).  draws > 0 (the reference uses 10):
 * that many logit vectors ~ Normal(mean logits, MC std of the logits) are calibrated; probs = their mean, uncert = their
 * population std, entropy = entropy of the mean (needs the class-std columns: MC dropout on the class head, argmax path).
 * The draws come from the build's Philox stream with `seed` (TFP's stream cannot be reproduced).
 * probs [n, M, num_classes], entropy [n, M], uncert [n, M, num_classes] (may be NULL). */
enum uda_class_calib_mode { UDA_CLS_TS = 0, UDA_CLS_ISO_ALL = 1, UDA_CLS_ISO_PERCLS = 2 };
int uda_calibrate_class(uda_ctx_t* ctx, int32_t mode, int32_t n_tables, const int32_t* tab_off, const double* xs,
                        const double* ys, const float* temps, int32_t draws, uint64_t seed, float* probs, float* entropy,
                        float* uncert);

/* Raw head outputs of the last run, level `level`: class [T_c, n, h, w, A*C] and
 * box [T_b, n, h, w, 4A or 8A] in the reference's stacking order (T axis first; T_x = 1
 * and the axis is dropped by the caller when that head is not stacked). */
int uda_get_head_outputs(uda_ctx_t* ctx, int32_t level, float* cls, float* box);
/* Inject head outputs (same layout) and run only the post-process on them.  cls_floats / box_floats = number of floats
 * the host buffers hold; they must equal T_x * n * h * w * channels of the handle's layout (an error otherwise: the
 * caller passed an unstacked array to a stacked head or the other way round). */
int uda_set_head_outputs(uda_ctx_t* ctx, int32_t level, int32_t n, const float* cls, int64_t cls_floats,
                         const float* box, int64_t box_floats);
/* post-process (ServingDriver._postprocess, infer_lib.py:263-267) on the head outputs RESIDENT in the handle - injected
 * with uda_set_head_outputs / uda_copy_heads / written through uda_head_outputs_device, or left by the last uda_run. */
int uda_postprocess_heads(uda_ctx_t* ctx, int32_t n, const float* image_scales, int32_t post_mode);
/* Device address of the handle's head-output buffer of `level` (which: 0 class, 1 box): rows [image][sample], each of
 * *floats_per_row floats, *rows_per_image = T for a stacked head else 1; capacity max_images images.  For device-side
 * exchanges (RCCL over xGMI: ensemble re-shard) without a host hop; the caller orders its own stream against
 * the handle's with uda_synchronize.  uda_set_num_images tells the handle how many images such a write filled in. */
int uda_head_outputs_device(uda_ctx_t* ctx, int32_t level, int32_t which, void** dev_ptr, int64_t* floats_per_row,
                            int32_t* rows_per_image);
int uda_set_num_images(uda_ctx_t* ctx, int32_t n);
/* Deep ensembles (BASELINE configs[3]; the reference has no ensemble code): copy the
 * head outputs of the last run of `src` (a deterministic member network, T = 1) into sample slot
 * `sample` of `dst` (a handle whose model has mc_samples = number of members and stacked heads);
 * uda_postprocess_heads(dst) then aggregates the members exactly like MC samples (a8 / a14).
 * Device-to-device on dst's stream; both handles must live on the same GPU and share the geometry.  src is read like
 * any reader reads a run (uda_range_demotions): a member whose run raised the fp16 range flag is served again first. */
int uda_copy_heads(uda_ctx_t* dst, uda_ctx_t* src, int32_t n, int32_t sample);
/* predict = set_images_f32 + run(no post) ; read back with uda_get_head_outputs */
int uda_predict(uda_ctx_t* ctx, const float* images, int32_t n);

/* Pre-NMS candidates of the last run (debug / parity): boxes [n,K,4], scores [n,K], classes [n,K] int32 */
int uda_get_candidates(uda_ctx_t* ctx, float* boxes, float* scores, int32_t* classes,
                       float* u_cls, float* u_al, float* u_ep);
int32_t uda_num_candidates(const uda_ctx_t* ctx);

/* Read back activation buffer `buf` of the LAST chunk processed (debug / parity). */
int uda_read_buffer(uda_ctx_t* ctx, int32_t buf, float* host, int64_t n_floats);
int uda_get_preprocessed(uda_ctx_t* ctx, float* images /* [n,H,W,3] */, float* scales /* [n] */);

/* Standalone NMS on host arrays (parity tests of the NonMaxSuppressionV5 kernel):
 * boxes [n_img, k, 4], scores [n_img, k] -> idx [n_img, M], out_scores [n_img, M], valid [n_img]; M <= 128.
 * Bit-exact against the reference for finite boxes (inverted corners, zero area, identical and touching boxes included), any
 * iou_thresh (0, negative, >= 1), and scores that are finite, +-0.0 (the two zeros tie, the smaller index first, each keeps
 * its sign on the way out), +inf, -inf or NaN (the last two never enter the heap).  One case is REFUSED (non-zero return,
 * uda_last_error names the first offending score, nothing is computed): soft_sigma > 0 with score_thresh < 0 and a live
 * score below 0 (score_thresh < score < 0).  Soft weights raise such a score; the reference re-pushes it with a higher
 * priority, which the kernels' epoch rule - a cached exact score is an upper bound - cannot follow exactly (DESIGN.md
 * section 5).  Non-finite box coordinates are undefined (inf - inf: a NaN IoU). */
int uda_nms(uda_ctx_t* ctx, const float* boxes, const float* scores, int32_t n_img, int32_t k,
            int32_t max_out, float iou_thresh, float score_thresh, float soft_sigma, int32_t pad,
            int32_t* idx, float* out_scores, int32_t* valid);

/* Standalone 1x1 convolution on host arrays (op-level parity tests and timing of the pointwise kernels):
 * out[r, p, :] = (act(bn(in[r / in_div, p, :] * se[r / in_div, :] @ w + bias)) * mask[r, :]) + res[r, p, :]
 * in [rows/in_div, hw, cin], w [cin, cout], se [rows/in_div, cin], mask [rows, cout], res/out [rows, hw, cout];
 * optional arguments may be NULL.  terms: 0 = f32-input MFMA, 3 / 6 = split-bf16 MFMA with 3 / 6 cross terms, 16 = two fp16
 * pieces per operand with 3 cross terms (the default scheme of the network, UDA_PW_SCHEME=f16x2), 1 = one fp16 piece, one
 * product (UDA_PW_SCHEME=f16), 8 = one bf16 piece, one product (UDA_PW_SCHEME=bf16: weight scale 1, no range limit).
 * Both fp16 schemes pack the weights times split_weight_scale as the network does, and fail -
 * they do not return infinities - when an input exceeds fp16's 65504 (kernels_pwb.hip).  The launch is repeated `reps`
 * times for *avg_ms (HIP events). */
int uda_debug_pw(int32_t device, const float* in, const float* w, const float* bias, const float* bn_scale,
                 const float* bn_shift, const float* se, const float* mask, const float* res,
                 int32_t rows, int32_t in_div, int32_t hw, int32_t cin, int32_t cout, int32_t act,
                 int32_t terms, int32_t reps, float* out, float* avg_ms);

/* The numpy NMS family of the reference (row a18, src/nms_np.py:30-278): x1,y1,x2,y2 boxes with the +1 pixel
 * convention.  method: 0 hard_nms, 1 diou_nms, 2 soft_nms gaussian, 3 soft_nms linear (thresholds as the caller
 * resolved them: `iou_thresh or 0.5` ...).  uda_nms_np: float64 dets [n,5] -> kept rows out [<= n, 5] in selection
 * order, *n_out rows.  uda_per_class_nms_np = nms_np.per_class_nms on float32 inputs (boxes y1,x1,y2,x2; classes
 * 0-based): out [max_boxes, 7] rows [image_id, x1, y1, x2, y2, score, class + 1], dummy rows score -1e5, boxes
 * multiplied by image_scale. */
int uda_nms_np(int32_t device, const double* dets, int32_t n, int32_t method, double iou_thresh, double sigma,
               double score_thresh, double* out, int32_t* n_out);
int uda_per_class_nms_np(int32_t device, const float* boxes, const float* scores, const int32_t* classes, int32_t k,
                         float image_id, float image_scale, int32_t num_classes, int32_t max_boxes, int32_t method,
                         float iou_thresh, float sigma, float score_thresh, float* out);

/* Per-op-kind device timing with HIP events recorded on the handle's stream.
 * kind_mask: bit (1 << uda_op_kind) selects op kinds; bit 16 post-process aggregate, bit 17 NMS, bit 19 the score kernel of
 * uda_score_images (with its softmax / entropy kernel when ENTROPY is read), bit 20 the match kernel of uda_eval_match, bit 21
 * the row and packing kernels of uda_pseudo_rows (with the softmax / entropy kernel when ENTROPY is read). */
int uda_profile_enable(uda_ctx_t* ctx, uint32_t kind_mask);
int uda_profile_read(uda_ctx_t* ctx, int32_t kind, double* total_ms, int64_t* launches, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* UDA_HIP_H_ */
