// Host-only: the handle behind the C ABI (include/uda_hip.h) and what uda_api.hip (create / destroy, inputs, the executor, the
// post-process, pipelined runs, readers of detections) shares with uda_services.hip (the services that read the resident detections
// and the entry points that work on host arrays): the handle itself, the two owners of what a service keeps in it (ResultSlot,
// GtStaging), the error and profiling helpers.  No kernels.
#pragma once
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "uda_internal.h"

using namespace uda;

struct ProfSlot {
  double total_ms = 0;
  int64_t launches = 0;       // in units of PLANNED ops: a launch that covers a group of n ops counts n (plan.op_costs counts per op)
  struct Pending { hipEvent_t first, second; int weight; };
  std::vector<Pending> pending;
};

// What a service leaves on the device until somebody reads it: ONE buffer, packed so that one copy brings the result to the host,
// and the host copy the first reader makes (fetch_result, uda_services.hip).  Owns its device memory.
struct ResultSlot {
  char* d = nullptr;           // the pack
  void* aux = nullptr;         // a second device buffer that is sized, grown and freed with the pack
  int cap = 0;                 // rows per image the pack holds, where it grows with the ground truth
  std::vector<char> h;         // host copy of what the readers need of the pack
  bool fetched = false;        // `h` holds the result of the last queued run
  ResultSlot() = default;
  ResultSlot(const ResultSlot&) = delete;
  ResultSlot& operator=(const ResultSlot&) = delete;
  ~ResultSlot() { release(); }
  void release() {
    if (d) hipFree(d);
    if (aux) hipFree(aux);
    d = nullptr; aux = nullptr; cap = 0; fetched = false;
  }
};

// Per-image ground-truth rows on their way to the device: up to two device arrays of width[k] floats per row and ONE pinned staging
// buffer the rows are copied through, so that the upload is asynchronous.  Owns its memory and its event.
struct GtStaging {
  const int width[2];
  float* d[2] = {nullptr, nullptr};  // [max_images, cap, width[k]]
  float* h = nullptr;                // pinned, the arrays back to back
  hipEvent_t ev = nullptr;           // the upload out of `h` has been consumed
  int cap = 0, n = 0, G = 0;         // rows per image the buffers hold; images / rows per image of what is set (n 0: nothing)
  GtStaging(int w0, int w1) : width{w0, w1} {}
  GtStaging(const GtStaging&) = delete;
  GtStaging& operator=(const GtStaging&) = delete;
  ~GtStaging() {
    release();
    if (ev) hipEventDestroy(ev);
  }
  void release() {
    for (float*& p : d) {
      if (p) hipFree(p);
      p = nullptr;
    }
    if (h) hipHostFree(h);
    h = nullptr; cap = 0; n = 0;
  }
};

struct uda_ctx {
  uda_model_t model;
  std::vector<uda_buf_desc_t> bufs;
  std::vector<uda_op_t> ops;
  std::vector<uda_drop_site_t> sites;
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;

  float* d_weights = nullptr;
  int64_t n_weights = 0;
  // split-bf16 copies of the 1x1 kernels in MFMA fragment order (kernels_pwb.hip); -1 = op keeps the f32 path
  uint16_t* d_wsplit = nullptr;
  std::vector<int64_t> wsplit_off;
  std::vector<int64_t> wpar_off;   // MBX: offset (uint16 units) of the per-slab depthwise operand block inside d_wsplit
  int pw_parts = UDA_SPLIT_F16X2;  // requested split scheme of the 1x1 contractions (uda_model_t.pw_scheme)
  std::vector<int> wscheme;        // per op: the scheme its packed weights use (an op whose weights do not suit fp16 pieces keeps bf16 x3)
  std::vector<float> wunscale;     // per op: 1 / (power-of-two factor folded into the packed weights); 1 unless fp16 pieces
  std::vector<float> wascale;      // per op: factor on the A operand (fp16 separable conv: pre-scaled depthwise taps); part of wunscale
  int n_f16_ops = 0, n_f16_demoted = 0;
  std::vector<char> buf_f16;       // per buffer: stored in 16 bits in its float32-sized slot (set_f16_storage): 1 = fp16, 2 = bf16
  // fp16 pieces: a kernel that splits an operand above 65504 sets bit 0 of ITS OP's flag word.  Two arrays of n_ops + 1
  // words (index n_ops: launches outside the op list): pipelined run s raises its flags in array s, everything else in array 0.
  unsigned* d_oor = nullptr;
  unsigned* oor_cur = nullptr;     // the array the launches being queued raise their flags in
  int oor_half = 0;                // the array the readers of the current results look at (check_split_range)
  bool oor_armed = false;          // a run with fp16-piece ops has been queued since the flags were last read
  // An op that raises its flag is re-packed with three bf16 pieces (float32 exponent range) and the run is served again
  // on the same handle (demote_ops / replay_run): the reference computes in float32 and never rejects an input on magnitude.
  std::vector<float> h_weights;    // host copy of the weight blob (for the re-packing)
  std::vector<uint16_t*> wovr;     // per op: device copy of its re-packed weights (null: its slice of d_wsplit)
  std::vector<int64_t> wovr_par;   // per op: uint16 offset of the parameter block inside wovr (-1: none)
  int64_t range_demotions = 0;     // ops re-packed so far (uda_range_demotions)
  // What a run read, so that it can be served again: input slot / float image generation, seed, image offset, masks.
  struct RunRec {
    bool valid = false, do_post = false, have_u8 = false, masks_injected = false;
    int pm = 0, cur = 0, n = 0;
    uint64_t slot_gen = 0, f32_gen = 0, masks_gen = 0, seed = 0;
    int64_t image_offset = 0;
  };
  RunRec last_run;                 // the last synchronous uda_run
  const RunRec* replay_rec = nullptr;   // the run whose results the readers are looking at (null: cannot be served again)
  uint64_t f32_gen = 0, masks_gen = 0;
  float* d_arena = nullptr;
  uint4* d_w0frag[2] = {nullptr, nullptr};   // gated, split projection kernel per gate row for the fused block-1 kernel (launch_w0gate), per chunk lane
  size_t w0frag_cap[2] = {0, 0};
  // chunk lanes: consecutive chunks alternate between independent (stream, arena) pairs so that the
  // barrier-heavy kernels of one chunk overlap the streaming kernels of the other
  int n_lanes = 1;
  hipStream_t lane_stream[2] = {nullptr, nullptr};
  float* lane_arena[2] = {nullptr, nullptr};
  hipEvent_t ev_start = nullptr, ev_done[2] = {nullptr, nullptr};
  int last_lane = 0;
  // post-process of chunk i (aggregate, NMS, gather: small latency-bound launches) runs on its own stream
  // beside the conv stack of chunk i + 1; only the last chunk's post-process is exposed
  hipStream_t post_stream = nullptr;
  std::vector<hipEvent_t> ev_chunk;
  hipEvent_t ev_post = nullptr;
  int post_overlap = 1;
  float* d_anchors = nullptr;
  int A_tot = 0;
  int a_off[UDA_MAX_LEVELS + 1];

  // inputs.  uint8 batches go through one of two slots (device buffer + pinned host staging buffer each): `cur` feeds the
  // next uda_run; the other one takes a batch that is uploaded on the copy stream while the current one is being
  // processed (uda_prefetch_images_u8 / uda_swap_prefetched) - the feed then costs no device time.
  struct U8Slot {
    uint8_t* d = nullptr;        // device: geometry table, then the images back to back (image i at d_img + geo[i].off)
    size_t cap = 0;
    uint8_t* pinned = nullptr;   // host staging (hipHostMalloc): pageable caller memory is copied here, DMA reads this
    size_t pcap = 0;
    int n = 0;
    bool valid = false, uploaded = false;
    uint64_t gen = 0;            // bumped by every upload into this slot (a run can be served again only from unchanged inputs)
    std::vector<PreGeo> geo;     // per image: offset, raw size, scaled size, sampling ratios (dataloader.py:123-152)
    PreGeo* d_geo = nullptr;     // = d (the table leads the buffer)
    uint8_t* d_img = nullptr;    // = d + header
    std::vector<float> scales;   // image_scale per image (1 / resize scale)
    hipEvent_t ev = nullptr;     // upload complete (copy stream)
  } u8[2];
  int cur = 0;
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_pre_done[2] = {nullptr, nullptr};   // the preprocess kernel has consumed slot i (its buffer may be refilled)
  bool have_u8 = false;
  int stem_act = UDA_ACT_SWISH; // activation of the stem op (the uint8 stem is a swish kernel)
  bool stem_from_u8 = false;   // this run's stem ops read the uint8 slot (set by run_network)
  bool pre_valid = false;      // d_images holds the preprocessed current batch (false: the stem read the uint8 images itself)
  int stem_co = 0;             // output channels of the stem op (0: no stem op in the plan)
  float* d_images = nullptr;   // [max_images, H, W, 3]
  float* d_scales = nullptr;   // [max_images]
  // consistency check (uda_run_consistency): images [noise_from, n_images) of the run are the noise variant of images
  // [0, n_images - noise_from), preprocessed by the NOISE instantiation of the preprocess kernel (-1: an ordinary run)
  int noise_from = -1;
  std::vector<PreGeo> cons_geo;      // geometry table of the 4n images of the last consistency run
  double* d_cons_iou = nullptr;      // [max_images, M] cons_iou of the last consistency run (lazy)
  uint8_t* d_cons_agree = nullptr;   // [max_images, M] cons_cls
  int cons_n = 0;                    // originals of the last consistency run (0: none)
  std::vector<float> h_scales;
  int n_images = 0;
  int sh = 0, sw = 0;

  // dropout
  float* d_masks = nullptr;
  int64_t mask_cap = 0;        // floats
  int64_t sum_site_ch = 0;
  int max_c4 = 0;
  std::vector<int64_t> site_off;
  int64_t* d_site_off = nullptr;
  int32_t* d_site_ch = nullptr;
  float* d_site_rate = nullptr;
  bool masks_injected = false;
  int masks_rows = 0;
  uint64_t seed = 0;
  int64_t image_offset = 0;
  int t_first = 0, t_stride = 1, t_total = 0;      // this handle's samples inside the global sample axis (0: all of them; uda_set_dropout_sample_shard)

  // head outputs [max_images * Tx, hw, ch] per level
  float* d_cls[UDA_MAX_LEVELS] = {};
  float* d_box[UDA_MAX_LEVELS] = {};
  int cls_ch = 0, box_ch = 0;

  // candidates
  float *d_cboxes = nullptr, *d_cscores = nullptr, *d_clogits = nullptr;
  int32_t* d_cclasses = nullptr;
  float *d_ucls = nullptr, *d_ual = nullptr, *d_uep = nullptr;
  int Kc = 0;                  // candidates per image: A_tot, or max_nms_inputs on the top-k path
  float* d_clsmean = nullptr;  // [max_images, A_tot*C]  (top-k path)
  int32_t* d_cand_flat = nullptr;  // [max_images, Kc]   (top-k path)
  void* d_topk_ws = nullptr;       // scratch of the multi-block top-k selection
  // nms workspaces: [0] global mode (one problem per image), [1] per-class mode (images*classes problems)
  struct NmsWs {
    float *stale = nullptr, *tent = nullptr, *ub = nullptr, *sel_score = nullptr, *sel_box = nullptr;
    int32_t *ev = nullptr, *begin = nullptr, *sel_idx = nullptr, *nsel = nullptr, *done = nullptr;
    unsigned long long *bound = nullptr, *win = nullptr;
    bool ready = false;
  } ws[2];
  // NMS on a score prefix (global mode with the whole anchor set as candidates): sub-problem arrays + workspace
  struct PrefixWs {
    int32_t *sub_idx = nullptr, *bad = nullptr;
    float *sub_scores = nullptr, *sub_boxes = nullptr;
    uint32_t* excl = nullptr;
    NmsWs ws;
    int Lcap = 0;
  } pfx;
  std::vector<std::pair<int, int>> pfx_pending;   // image ranges whose prefix flags the host has not looked at yet
  bool pfx_off = false;                            // set while finish_post redoes rejected images
  int64_t pfx_fallbacks = 0;                       // images redone on the full candidate set so far
  int pfx_skip = 0, pfx_backoff = 0;               // runs left without the prefix / length of the last pause
  // cooperative single-launch NMS: per-problem barrier counters + one error word (barrier timed out)
  unsigned long long* d_coop_bar = nullptr;       // exchange slots, max_images x nms_coop_slot_words(max_output_size)
  int* d_coop_err = nullptr;
  bool coop_used = false;
  bool coop_off = false;                           // set after a barrier time-out: this handle stays on the two-launch version
  int64_t coop_fallbacks = 0;                      // post-process runs redone with two launches per epoch after such a time-out
  int64_t coop_not_launched = 0;                   // NMS runs that wanted the single-launch grid and did not get it (capacity query / launch refused)
  unsigned long long* d_merge_keys = nullptr;
  // outputs
  float *d_oboxes = nullptr, *d_oscores = nullptr, *d_oclasses = nullptr, *d_ologits = nullptr;
  float *d_oprobs = nullptr, *d_oentropy = nullptr;   // stable softmax / entropy of the selected rows (lazy)
  float* d_opacked = nullptr;                        // packed detection records for the multi-GPU gather (lazy, uda_detections_device)
  int32_t* d_ovalid = nullptr;
  // per-image ground truth, set before the service that reads it (stage_ground_truth, uda_services.hip): the buffers hold
  // max_images x cap rows and grow when a call brings more rows per image; nothing is allocated per call in the steady state
  GtStaging gt{4, 1};                // uda_set_ground_truth: boxes [n, G, 4] | classes [n, G] (assignment, label check)
  GtStaging egt{7, 0};               // uda_set_eval_ground_truth: rows [n, G, 7] (COCO matching)
  // the services' results (the *Pack structs of uda_services.hip name the layouts).  asg holds max_images x gt.cap rows and grows
  // with `gt`, lc max_images x lc.cap rows and grows when a check brings more; the others are sized once for max_images
  ResultSlot asg;                    // uda_assign_ground_truth (AssignPack); aux: the matched rows [max_images * cap, assigned_row_cols]
  int asg_n = 0, asg_G = 0;          // images / rows per image of the last assignment (0: none)
  int64_t asg_rows = 0;              // sum(count) of the last assignment, as its first reader found it
  ResultSlot score;                  // uda_score_images (ScorePack)
  int score_n = 0, score_nc = 0;     // images / components of the last scoring (0: none)
  ResultSlot pseudo;                 // uda_pseudo_rows (PseudoPack; the host copies the head, then the used records); aux: the
                                     // packing kernel's staging, [max_images, max_output_size] records
  int pseudo_n = 0, pseudo_cap = 0;  // images / record slots per image of the last uda_pseudo_rows (0: none)
  ResultSlot lc;                     // uda_label_check (LabelPack)
  int lc_n = 0, lc_G = 0;            // images / rows per image of the last check (0: none)
  ResultSlot eval;                   // uda_eval_match (EvalPack)
  int eval_n = 0;                    // images of the last match (0: none)
  int last_post_mode = 0;
  int last_n = 0;
  int last_chunk_i0 = 0, last_chunk_n = 0;
  // Pipelined runs (uda_run_async / uda_collect): the post-process of run k (aggregate, NMS, gather: ~4 ms of latency-bound
  // launches on the post stream) is NOT joined into the main stream; run k + 1's network starts at once and only its first
  // head-writing op waits for it.  What run k's post-process reads or writes and run k + 1 could touch exists twice, by
  // ticket: the detection outputs and the image scales (snapshot taken on the main stream when the run is queued).
  struct AsyncSlot {
    hipEvent_t ev = nullptr;             // post-process of this run done
    bool open = false;                   // queued, not collected yet
    bool joined = true;                  // the main stream has been made to wait for `ev`
    int64_t seq = 0;
    int n = 0, mode = 0;
    bool coop_used = false, oor_armed = false;
    bool cands_lost = false;             // an older run was served again after this one: its candidates are gone (no redo of its post-process)
    RunRec rec;                          // what this run read (replay_run)
    std::vector<std::pair<int, int>> pending;      // prefix-NMS ranges the host has not checked (rare path: no cooperative NMS)
    float *oboxes = nullptr, *oscores = nullptr, *oclasses = nullptr, *ologits = nullptr, *scales = nullptr;
    int32_t* ovalid = nullptr;
  };
  AsyncSlot as[2];
  int as_next = 0;
  int64_t as_seq = 0;
  bool as_ready = false;
  const float* d_scales_post = nullptr;  // what the post-process reads as image scales (null: d_scales)
  hipStream_t aux_stream = nullptr;      // uda_collect_device packs on it
  hipEvent_t gate_ev = nullptr;          // run_network: head-writing ops wait for this first (the previous run's post-process)

  uint32_t prof_mask = 0;
  ProfSlot prof[32];
};

// sets the handle's error text (`c` null: the text uda_last_error(NULL) returns, one per thread) and returns 1
int fail(uda_ctx* c, const char* fmt, ...);

// for code that owns nothing: a return here skips no clean-up
#define HIPC(ctx, expr)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(ctx, "%s: %s failed: %s (%s:%d)", __func__, #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

template <typename T>
inline hipError_t dalloc(T** p, size_t n) {
  return hipMalloc((void**)p, (n ? n : 1) * sizeof(T));
}

// ------------------------------------------------------------------------------------ profiling helpers
struct ProfScope {
  uda_ctx* c;
  int kind;
  hipStream_t st;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool on;
  int weight;
  ProfScope(uda_ctx* c_, int kind_, hipStream_t st_ = nullptr, int weight_ = 1)
      : c(c_), kind(kind_), st(st_ ? st_ : c_->stream), weight(weight_) {
    on = (c->prof_mask >> kind) & 1u;
    if (on) {
      hipEventCreate(&e0);
      hipEventCreate(&e1);
      hipEventRecord(e0, st);
    }
  }
  ~ProfScope() {
    if (on) {
      hipEventRecord(e1, st);
      c->prof[kind].pending.push_back({e0, e1, weight});
    }
  }
};

inline int box_cols_of(const uda_model_t& m, int post_mode) {
  if (post_mode == UDA_POST_PER_CLASS) return 4;
  int cols = 4;
  if (m.has_uncert && m.loss_attenuation) cols += 4;
  if (m.has_uncert && m.box_stacked) cols += 4;
  return cols;
}
inline int cls_cols_of(const uda_model_t& m, int post_mode) {
  if (post_mode == UDA_POST_PER_CLASS) return 1;
  // top-k path gathers ONE class-std value per (anchor, class) candidate (postprocess.py:117-121)
  return 1 + ((m.has_uncert && m.cls_stacked) ? (m.max_nms_inputs > 0 ? 1 : m.num_classes) : 0);
}

struct NmsCoop {           // scratch of the cooperative kernel; null members = never use it
  unsigned long long* bar = nullptr;    // exchange slots (per problem nms_coop_slot_words(M) words)
  int* err = nullptr;
  bool* used = nullptr;
  int64_t* not_launched = nullptr;      // counts the runs that wanted the single launch and fell through to the slower versions
};

// ------------------------------------------------------------------------------------ executor functions the services call (uda_api.hip)
int finish_post(uda_ctx* c);      // range replay / prefix redo / NMS fallback: afterwards the readers see final detections
int ensure_probs(uda_ctx* c, int rows);      // softmax and entropy of the first `rows` selected rows into d_oprobs / d_oentropy (lazy)
// Returns true when the problems were solved on their score prefix (flags in pw->bad[p0 ..] say which ones have to be
// redone on the full set, see finish_post); `pw` null = never.
bool run_nms(const NmsArgs& na, const float* scores, int M, hipStream_t st, uda_ctx::PrefixWs* pw = nullptr, size_t p0 = 0,
             NmsCoop coop = NmsCoop());
void nms_params(NmsArgs& a, float iou_thr, float score_thr, float soft_sigma);
int solo_limit();
int prefix_target();
hipError_t alloc_prefix_ws(uda_ctx::PrefixWs& w, size_t problems, int Lcap, size_t M);
void free_prefix_ws(uda_ctx::PrefixWs& w);
