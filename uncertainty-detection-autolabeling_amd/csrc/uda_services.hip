// The services of the C ABI (include/uda_hip.h) that run beside the executor of uda_api.hip: ground-truth assignment, image scores,
// COCO matching, the label check and the calibrations on the detections resident in a handle, and the entry points that take host arrays and work
// on scratch device memory of their own (the *_np twins, the thresholding objective and report, the post-thresholding heat maps and tallies, the pruning neighbours and hashes, the pseudo-label audit, the uncertainty report, the classification report, the collage resample and augmentations, uda_nms, uda_debug_pw,
// the numpy NMS family).
// Host code only: every kernel launched here lives in a kernels_*.hip.
//
// What the services share is stated once, ahead of them: the checks of the resident run (resident_ready, gt_covers_run), the
// pinned staging of per-image ground truth (stage_ground_truth), the result packs with their first-reader fetch (fetch_result
// over a ResultSlot of uda_ctx.h), the sources of a score descriptor (score_sources_missing, resident_score_sources,
// upload_score_sources), the tail of the entry points that own a DevScratch (scratch_done, fetch_pack) and the slots of a
// segment's tree fold (tree_slots).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <numeric>
#include <thread>
#include <vector>

#include "dev_scratch.h"
#include "uda_ctx.h"

static int hip_failed(uda_ctx* c, const char* who, hipError_t e) { return fail(c, "%s: %s", who, hipGetErrorString(e)); }

// ---- what the services on resident detections share
// No pipelined run is in flight and a post-process has run - the global one where `reads` ("the assignment reads", ...) is given.
static int resident_ready(uda_ctx* c, const char* who, const char* reads) {
  if (c->as[0].open || c->as[1].open) return fail(c, "%s: a pipelined run (uda_run_async) is in flight - uda_collect it first", who);
  if (c->last_n < 1) return fail(c, "%s: no %spost-process has run yet", who, reads ? "global " : "");
  if (reads && c->last_post_mode != UDA_POST_GLOBAL)
    return fail(c, "%s: the last post-process ran per class; %s the global post-process", who, reads);
  return 0;
}
// The handle's device is current and its detections are final (range replay / prefix redo / NMS fallback done).
static int settle_detections(uda_ctx* c) {
  HIPC(c, hipSetDevice(c->device));
  return finish_post(c);
}
// after a consistency run the handle holds 4n images, the n originals first
static bool holds_consistency_run(const uda_ctx* c) { return c->noise_from >= 0 && c->cons_n > 0 && c->last_n == 4 * c->cons_n; }
// The ground truth that is set covers the images the service reads: with `originals` those of a consistency run, to which the
// ground truth belongs, else every image of the last run.
static int gt_covers_run(uda_ctx* c, const char* who, int gt_n, bool originals) {
  const int held = originals && holds_consistency_run(c) ? c->cons_n : c->last_n;
  if (gt_n != held) return fail(c, "%s: ground truth of %d images, the last post-process holds %d", who, gt_n, held);
  return 0;
}

// Ground truth of n images x G rows into `st`: through its pinned buffer, so that the upload is queued on the handle's stream
// (a service queued behind a run finds it there) and the caller's arrays are free at once.  src[k]: [n, G, st.width[k]].
// Allocates only when G exceeds what the buffers hold, after a stream sync; *grew tells a caller whose buffers follow st.cap.
static int stage_ground_truth(uda_ctx* c, GtStaging& st, const float* const* src, int n, int G, bool* grew = nullptr) {
  HIPC(c, hipSetDevice(c->device));
  if (!st.ev) HIPC(c, hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
  else HIPC(c, hipEventSynchronize(st.ev));              // the previous upload has left the staging buffer
  const bool grow = G > st.cap || !st.d[0];
  if (grew) *grew = grow;
  if (grow) {
    HIPC(c, hipStreamSynchronize(c->stream));            // (growing is rare: nothing may still read the old buffers)
    st.release();
    const size_t rows = (size_t)c->model.max_images * std::max(G, 1);
    for (int k = 0; k < 2; ++k)
      if (st.width[k]) HIPC(c, dalloc(&st.d[k], rows * st.width[k]));
    HIPC(c, hipHostMalloc((void**)&st.h, rows * (st.width[0] + st.width[1]) * sizeof(float)));
    st.cap = std::max(G, 1);
  }
  float* h = st.h;
  for (int k = 0; k < 2; ++k)
    if (const size_t floats = (size_t)n * G * st.width[k]) {
      memcpy(h, src[k], floats * sizeof(float));
      HIPC(c, hipMemcpyAsync(st.d[k], h, floats * sizeof(float), hipMemcpyHostToDevice, c->stream));
      h += floats;
    }
  HIPC(c, hipEventRecord(st.ev, c->stream));
  st.n = n; st.G = G;
  return 0;
}

// The first reader of a result waits for it and brings `bytes` of the pack to the host in one copy; later readers find s.h.
static int fetch_result(uda_ctx* c, ResultSlot& s, size_t bytes) {
  if (s.fetched) return 0;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));
  s.h.resize(bytes);
  HIPC(c, hipMemcpy(s.h.data(), s.d, bytes, hipMemcpyDeviceToHost));
  s.fetched = true;
  return 0;
}

// ---- the tail of an entry point that owns a DevScratch
static int scratch_done(uda_ctx* c, const char* who, const DevScratch& s) { return s.ok() ? 0 : hip_failed(c, who, s.err); }
// the handle-free twins: the launches' error, the end of the work, then `bytes` of the device pack as the host copy `h`
static int fetch_pack(const char* who, DevScratch& s, const void* d_pack, size_t bytes, std::vector<char>& h) {
  s.sync();
  h.resize(bytes);
  s.download(h.data(), d_pack, bytes);
  return scratch_done(nullptr, who, s);
}

// ---- the slots a segment of `runs` run roots takes for the in-place tree fold (fold_slots_in_place of wave_fold.h): none
// for no runs, else the power of two at or above `runs`; the slots past the runs stay zero, the tree's padding
static int64_t tree_slots(int64_t runs) {
  int64_t slots = runs ? 1 : 0;
  while (slots < runs) slots <<= 1;
  return slots;
}

// ---- result packs: one device buffer per service, so that ONE copy brings a result to the host.  Built over the device buffer
// where the kernel arguments are filled and over the host copy where the results are handed out.
struct AssignPack {      // iou [n G] float64 | det_index [n G] int32 | count [n] int32 | error flag int32
  char* base;
  size_t n, G;
  AssignPack(void* b, size_t n_, size_t G_) : base((char*)b), n(n_), G(G_) {}
  size_t bytes() const { return n * G * (sizeof(double) + sizeof(int32_t)) + (n + 1) * sizeof(int32_t); }
  double* iou() const { return (double*)base; }
  int32_t* det_index() const { return (int32_t*)(base + n * G * sizeof(double)); }
  int32_t* count() const { return det_index() + n * G; }
  int32_t* err() const { return count() + n; }
  void fill(AssignArgs& a, int M, int method, int keep) const {       // where the kernel writes, and the problem's scalars
    a.det_index = det_index(); a.iou = iou(); a.count = count(); a.err = err();
    a.n = (int)n; a.M = M; a.G = (int)G; a.method = method; a.keep = keep;
  }
  int copy_out(uda_ctx* c, const char* who, int M, int32_t* det_index_out, double* iou_out, int32_t* count_out) const {
    if (*err())
      return fail(c, M > 0 ? "%s: the rank method met a kept ground-truth row beyond the %d detections"
                           : "%s: a kept ground-truth row and %d detections to match it with", who, M);
    if (iou_out && n * G) memcpy(iou_out, iou(), n * G * sizeof(double));
    if (det_index_out && n * G) memcpy(det_index_out, det_index(), n * G * sizeof(int32_t));
    if (count_out) memcpy(count_out, count(), n * sizeof(int32_t));
    return 0;
  }
};

struct ScorePack {       // components [n, nc] float64 | count [n] int32 | class_counts [n, C] int32 | error flag int32
  char* base;
  size_t n, nc, C;
  ScorePack(void* b, size_t n_, size_t nc_, size_t C_) : base((char*)b), n(n_), nc(nc_), C(C_) {}
  size_t bytes() const { return n * nc * sizeof(double) + (n + n * C + 1) * sizeof(int32_t); }
  double* comp() const { return (double*)base; }
  int32_t* count() const { return (int32_t*)(base + n * nc * sizeof(double)); }
  int32_t* class_counts() const { return count() + n; }
  int32_t* err() const { return class_counts() + n * C; }
  int copy_out(uda_ctx* c, const char* who, double* components, int32_t* count_out, int32_t* class_counts_out) const {
    if (*err()) return fail(c, "%s: a kept detection has a class id outside 1..%d", who, (int)C);
    if (components) memcpy(components, comp(), n * nc * sizeof(double));
    if (count_out) memcpy(count_out, count(), n * sizeof(int32_t));
    if (class_counts_out) memcpy(class_counts_out, class_counts(), n * C * sizeof(int32_t));
    return 0;
  }
};

static_assert(sizeof(uda_pseudo_record_t) == sizeof(PseudoRecord), "the record is 40 bytes on both sides");
struct PseudoPack {      // head: minmax [n, 2] float64 | kept [n] | cand [n] | error flag, padded to 8 bytes; then records [n, cap] x 40
  char* base;            // bytes, the first sum(cand) used - the host copies the head, then only the used records
  size_t n, cap;
  PseudoPack(void* b, size_t n_, size_t cap_) : base((char*)b), n(n_), cap(cap_) {}
  size_t head_bytes() const { return (n * 2 * sizeof(double) + (2 * n + 1) * sizeof(int32_t) + 7) & ~(size_t)7; }
  size_t bytes() const { return head_bytes() + n * cap * sizeof(PseudoRecord); }
  double* minmax() const { return (double*)base; }
  int32_t* kept() const { return (int32_t*)(base + n * 2 * sizeof(double)); }
  int32_t* cand() const { return kept() + n; }
  int32_t* err() const { return cand() + n; }
  PseudoRecord* rec() const { return (PseudoRecord*)(base + head_bytes()); }
  int64_t total() const { return std::accumulate(cand(), cand() + n, (int64_t)0); }
  // `base` is a host copy of the head; `recs` a host copy of the first total() records (null: none were asked for)
  int copy_out(uda_ctx* c, const char* who, int C, const void* recs, void* records, int64_t n_records, double* minmax_out,
               int32_t* kept_out, int32_t* cand_out) const {
    if (*err()) return fail(c, "%s: a candidate has a class id outside 1..%d", who, C);
    if (records && n_records != total()) return fail(c, "%s: %lld candidate records, not %lld", who, (long long)total(), (long long)n_records);
    if (records && n_records) memcpy(records, recs, (size_t)n_records * sizeof(PseudoRecord));
    if (minmax_out) memcpy(minmax_out, minmax(), n * 2 * sizeof(double));
    if (kept_out) memcpy(kept_out, kept(), n * sizeof(int32_t));
    if (cand_out) memcpy(cand_out, cand(), n * sizeof(int32_t));
    return 0;
  }
};

static_assert(sizeof(uda_eval_record_t) == 44, "the record is 11 words");
struct EvalPack {        // records [n, M] x 44 bytes | npig [n, C, 4] int32 | used [n] int32
  char* base;
  size_t n, M, C;
  EvalPack(void* b, size_t n_, size_t M_, size_t C_) : base((char*)b), n(n_), M(M_), C(C_) {}
  size_t bytes() const { return n * M * sizeof(uda_eval_record_t) + (n * C * 4 + n) * sizeof(int32_t); }
  uda_eval_record_t* rec() const { return (uda_eval_record_t*)base; }
  int32_t* npig() const { return (int32_t*)(base + n * M * sizeof(uda_eval_record_t)); }
  int32_t* used() const { return npig() + n * C * 4; }
  void copy_out(void* records, int32_t* npig_out, int32_t* used_out) const {
    if (records) memcpy(records, rec(), n * M * sizeof(uda_eval_record_t));
    if (npig_out) memcpy(npig_out, npig(), n * C * 4 * sizeof(int32_t));
    if (used_out) memcpy(used_out, used(), n * sizeof(int32_t));
  }
};

struct LabelPack {       // iou [n G] float64 | det_max_iou [n M] float64 | det_rank [n G] int32 | counts [n 5] int32 | gt_boxes_out
  char* base;            // [n G 4] float32 | gt_flags [n G] uint8 | det_flags [n M] uint8; behind what is copied, from the next
  size_t n, G, M;        // multiple of 4 bytes: the kernel's first-row words [n M] int32
  LabelPack(void* b, size_t n_, size_t G_, size_t M_) : base((char*)b), n(n_), G(G_), M(M_) {}
  double* iou() const { return (double*)base; }
  double* det_max() const { return iou() + n * G; }
  int32_t* det_rank() const { return (int32_t*)(det_max() + n * M); }
  int32_t* counts() const { return det_rank() + n * G; }
  float* gt_boxes() const { return (float*)(counts() + n * 5); }
  uint8_t* gt_flags() const { return (uint8_t*)(gt_boxes() + n * G * 4); }
  uint8_t* det_flags() const { return gt_flags() + n * G; }
  size_t copy_bytes() const { return (size_t)(det_flags() + n * M - (uint8_t*)base); }
  int32_t* first_row() const { return (int32_t*)(base + ((copy_bytes() + 3) & ~(size_t)3)); }
  size_t bytes() const { return ((copy_bytes() + 3) & ~(size_t)3) + n * M * sizeof(int32_t); }
  template <typename T>      // where the kernel writes, and the problem's scalars
  void fill(LabelCheckArgs<T>& a, int methods, int md_rule, T min_score, T correct_score, double iou_consist, double md_max_inter,
            double correct_max_inter) const {
    a.iou = iou(); a.det_max_iou = det_max(); a.det_rank = det_rank(); a.counts = counts(); a.gt_boxes_out = gt_boxes();
    a.gt_flags = gt_flags(); a.det_flags = det_flags(); a.first_row = first_row();
    a.n = (int)n; a.M = (int)M; a.G = (int)G; a.methods = methods; a.md_rule = md_rule;
    a.min_score = min_score; a.correct_score = correct_score;
    a.iou_consist = iou_consist; a.md_max_inter = md_max_inter; a.correct_max_inter = correct_max_inter;
  }
  void copy_out(int32_t* det_rank_out, double* iou_out, uint8_t* gt_flags_out, float* gt_boxes_out, uint8_t* det_flags_out,
                double* det_max_out, int32_t* counts_out) const {
    if (det_rank_out && n * G) memcpy(det_rank_out, det_rank(), n * G * sizeof(int32_t));
    if (iou_out && n * G) memcpy(iou_out, iou(), n * G * sizeof(double));
    if (gt_flags_out && n * G) memcpy(gt_flags_out, gt_flags(), n * G);
    if (gt_boxes_out && n * G) memcpy(gt_boxes_out, gt_boxes(), n * G * 4 * sizeof(float));
    if (det_flags_out && n * M) memcpy(det_flags_out, det_flags(), n * M);
    if (det_max_out && n * M) memcpy(det_max_out, det_max(), n * M * sizeof(double));
    if (counts_out) memcpy(counts_out, counts(), n * 5 * sizeof(int32_t));
  }
};

struct AuditPack {       // float64 gt_max_iou [NG] | det_max_iou [ND] | det_alloc_miou [ND] | det_alloc_pair_iou [ND]; int32 gt_best_det
  char* base;            // [NG] | gt_alloc_det [NG] | det_best_gt [ND] | det_alloc_gt [ND] | n_matches [B]; uint8 gt_flags [NG] |
  size_t NG, ND, B;      // det_flags [ND].  Read where it lies: every array the caller asked for is copied straight out of it
  AuditPack(void* b, size_t NG_, size_t ND_, size_t B_) : base((char*)b), NG(NG_), ND(ND_), B(B_) {}
  size_t n64() const { return NG + 3 * ND; }
  size_t n32() const { return 2 * NG + 2 * ND + B; }
  size_t bytes() const { return n64() * sizeof(double) + n32() * sizeof(int32_t) + NG + ND; }
  void fill(AuditArgs& a) const {
    double* f = (double*)base;
    int32_t* i = (int32_t*)(f + n64());
    uint8_t* u = (uint8_t*)(i + n32());
    a.gt_max_iou = f; a.det_max_iou = f + NG; a.det_alloc_miou = f + NG + ND; a.det_alloc_pair_iou = f + NG + 2 * ND;
    a.gt_best_det = i; a.gt_alloc_det = i + NG; a.det_best_gt = i + 2 * NG; a.det_alloc_gt = i + 2 * NG + ND;
    a.n_matches = i + 2 * NG + 2 * ND;
    a.gt_flags = u; a.det_flags = u + NG;
  }
};

// ---- ground-truth assignment (reference utils_extra.py:44-64; validate_model.py:314-339, calibrate_model.py:133-147)
// Width of a matched row: every column the global post-process produced, then what uda_get_class_probs adds.
static int assigned_row_cols_of(const uda_model_t& m) {
  return box_cols_of(m, UDA_POST_GLOBAL) + 1 + cls_cols_of(m, UDA_POST_GLOBAL) + (m.enable_softmax ? 2 * m.num_classes + 1 : 0);
}
// LDS of the two kernels: M boxes of 16 bytes, G row numbers of 4 bytes, and 4 static bytes each - 65540 at either cap, which the
// runtime grants a gfx950 block as it is (tests/test_gpu_service_edges.py launches M = 4095 and 4096)
static const int kAssignMaxM = 4096, kAssignMaxG = 16384;

extern "C" int uda_assigned_row_cols(const uda_ctx_t* c, int32_t* cols) {
  if (!c || !cols) return 1;
  *cols = assigned_row_cols_of(c->model);
  return 0;
}

extern "C" int uda_set_ground_truth(uda_ctx_t* c, const float* boxes, const float* classes, int32_t n, int32_t G) {
  if (!c || !boxes || !classes) return c ? fail(c, "set_ground_truth: NULL argument") : 1;
  const uda_model_t& m = c->model;
  if (n < 1 || n > m.max_images) return fail(c, "set_ground_truth: %d images, the handle holds 1..%d", n, m.max_images);
  if (G < 0 || G > kAssignMaxG) return fail(c, "set_ground_truth: %d ground-truth rows per image, at most %d", G, kAssignMaxG);
  const float* src[] = {boxes, classes};
  bool grew = false;
  if (int rc = stage_ground_truth(c, c->gt, src, n, G, &grew)) return rc;
  if (grew) {              // the assignment's pack and row table hold gt.cap rows per image as well: the last assignment is gone
    c->asg.release();
    c->asg_n = 0;
    const size_t cap = (size_t)c->gt.cap;
    float* rows = nullptr;
    hipError_t e = dalloc(&c->asg.d, AssignPack(nullptr, (size_t)m.max_images, cap).bytes());
    if (e == hipSuccess) e = dalloc(&rows, (size_t)m.max_images * cap * (size_t)assigned_row_cols_of(m));
    c->asg.aux = rows;
    if (e != hipSuccess) {
      c->gt.n = 0;         // (nothing may be assigned into a pack that is not there)
      return hip_failed(c, "set_ground_truth", e);
    }
  }
  return 0;
}

extern "C" int uda_assign_ground_truth(uda_ctx_t* c, int32_t method, int32_t keep) {
  if (!c) return 1;
  const uda_model_t& m = c->model;
  if (method < ASSIGN_IOU || method > ASSIGN_RANK) return fail(c, "assign_ground_truth: unknown method %d", method);
  if (keep != ASSIGN_KEEP_VALIDATE && keep != ASSIGN_KEEP_CALIBRATE) return fail(c, "assign_ground_truth: unknown keep rule %d", keep);
  if (c->gt.n < 1) return fail(c, "assign_ground_truth: no ground truth is set (uda_set_ground_truth)");
  if (int rc = resident_ready(c, "assign_ground_truth", "the assignment reads")) return rc;
  if (int rc = gt_covers_run(c, "assign_ground_truth", c->gt.n, true)) return rc;
  if (m.max_output_size > kAssignMaxM) return fail(c, "assign_ground_truth: max_output_size %d above %d", m.max_output_size, kAssignMaxM);
  if (int rc = settle_detections(c)) return rc;
  const int n = c->gt.n, M = m.max_output_size, G = c->gt.G, C = m.enable_softmax ? m.num_classes : 0;
  if (C)
    if (int rc = ensure_probs(c, n * M)) return rc;
  const AssignPack pack(c->asg.d, (size_t)n, (size_t)G);
  HIPC(c, hipMemsetAsync(pack.err(), 0, sizeof(int32_t), c->stream));
  AssignArgs a{};
  a.det_boxes = c->d_oboxes; a.det_stride = box_cols_of(m, UDA_POST_GLOBAL);
  a.gt_boxes = c->gt.d[0]; a.gt_classes = c->gt.d[1];
  pack.fill(a, M, method, keep);
  launch_assign_gt(a, c->stream);
  AssignRowsArgs r{};
  r.det_index = pack.det_index(); r.count = pack.count();
  r.boxes = c->d_oboxes; r.scores = c->d_oscores; r.classes = c->d_oclasses;
  r.logits = c->d_ologits; r.probs = c->d_oprobs; r.entropy = c->d_oentropy;
  r.rows = (float*)c->asg.aux;
  r.n = n; r.M = M; r.G = G; r.bc = a.det_stride; r.cc = cls_cols_of(m, UDA_POST_GLOBAL); r.C = C; r.cols = assigned_row_cols_of(m);
  launch_gather_assigned(r, c->stream);
  HIPC(c, hipGetLastError());
  c->asg_n = n; c->asg_G = G; c->asg.fetched = false;
  return 0;
}

// The host copy of the last assignment's pack (fetch_result), its error word checked and its matched rows counted.
static int fetch_assignment(uda_ctx* c) {
  AssignPack h(nullptr, (size_t)c->asg_n, (size_t)c->asg_G);
  if (int rc = fetch_result(c, c->asg, h.bytes())) return rc;
  h.base = c->asg.h.data();
  if (int rc = h.copy_out(c, "assign_ground_truth", c->model.max_output_size, nullptr, nullptr, nullptr)) return rc;      // (the error word)
  c->asg_rows = std::accumulate(h.count(), h.count() + h.n, (int64_t)0);
  return 0;
}

extern "C" int uda_get_assignment(uda_ctx_t* c, int32_t* det_index, double* iou, int32_t* count) {
  if (!c) return 1;
  if (c->asg_n < 1) return fail(c, "get_assignment: no assignment (uda_assign_ground_truth)");
  if (int rc = fetch_assignment(c)) return rc;
  return AssignPack(c->asg.h.data(), (size_t)c->asg_n, (size_t)c->asg_G)
      .copy_out(c, "assign_ground_truth", c->model.max_output_size, det_index, iou, count);
}

extern "C" int uda_get_assigned_rows(uda_ctx_t* c, float* rows, int64_t n_floats) {
  if (!c) return 1;
  if (c->asg_n < 1) return fail(c, "get_assigned_rows: no assignment (uda_assign_ground_truth)");
  if (int rc = fetch_assignment(c)) return rc;
  const int64_t want = c->asg_rows * assigned_row_cols_of(c->model);
  if (n_floats != want) return fail(c, "get_assigned_rows: the %lld matched rows take %lld floats, not %lld", (long long)c->asg_rows, (long long)want, (long long)n_floats);
  if (want && !rows) return fail(c, "get_assigned_rows: NULL output");
  HIPC(c, hipSetDevice(c->device));
  if (want) HIPC(c, hipMemcpy(rows, c->asg.aux, (size_t)want * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// gt_box_assigner for callers that hold detections of their own: host arrays in, the same kernel, host arrays out
extern "C" int uda_assign_gt_np(int32_t device, const float* det_boxes, const float* gt_boxes, const float* gt_classes, int32_t n,
                                int32_t M, int32_t G, int32_t method, int32_t keep, int32_t* det_index, double* iou, int32_t* count) {
  if (n < 0 || M < 0 || G < 0 || M > kAssignMaxM || G > kAssignMaxG || method < ASSIGN_IOU || method > ASSIGN_RANK ||
      (keep != ASSIGN_KEEP_VALIDATE && keep != ASSIGN_KEEP_CALIBRATE) || !count ||
      ((size_t)n * G && (!gt_boxes || !gt_classes || !det_index || !iou)) || ((size_t)n * M && !det_boxes))
    return fail(nullptr, "uda_assign_gt_np: bad argument");
  if (n == 0) return 0;
  const size_t nm = (size_t)n * M, ng = (size_t)n * G;
  DevScratch s(device);
  AssignArgs a{};
  a.det_boxes = s.upload(det_boxes, nm * 4); a.det_stride = 4;
  a.gt_boxes = s.upload(gt_boxes, ng * 4); a.gt_classes = s.upload(gt_classes, ng);
  AssignPack pack(nullptr, (size_t)n, (size_t)G);
  pack.base = s.alloc<char>(pack.bytes());
  s.zero(pack.count(), ((size_t)n + 1) * sizeof(int32_t));
  pack.fill(a, M, method, keep);
  if (s.ok()) launch_assign_gt(a, nullptr);
  std::vector<char> h;
  if (int rc = fetch_pack("uda_assign_gt_np", s, pack.base, pack.bytes(), h)) return rc;
  return AssignPack(h.data(), pack.n, pack.G).copy_out(nullptr, "uda_assign_gt_np", M, det_index, iou, count);
}

// ---- active-learning image scores (reference active_learning_loop.py:528-733 on the lines of infer_model.py:836-960)
static const int kScoreMaxM = 4096, kScoreMaxC = 8192;      // rows a block walks; class counters in LDS (4 bytes each)

// what a descriptor reads: bit (1 << uda_score_source); 0 with *why set when it is malformed
static unsigned score_desc_sources(const uda_score_desc_t* d, const char** why) {
  *why = nullptr;
  if (!d) { *why = "NULL descriptor"; return 0; }
  if (d->n_comp < 1 || d->n_comp > UDA_SCORE_MAX_COMP) { *why = "n_comp outside 1..3"; return 0; }
  unsigned mask = 0;
  for (int k = 0; k < d->n_comp; ++k) {
    if (d->n_terms[k] < 1 || d->n_terms[k] > 2) { *why = "a component has 1 or 2 terms"; return 0; }
    for (int t = 0; t < d->n_terms[k]; ++t) {
      const int src = d->term[k][t].source, tr = d->term[k][t].transform;
      const bool scalar = src == UDA_SCORE_ENTROPY || src == UDA_SCORE_DET_SCORE;
      const bool box = src == UDA_SCORE_ALBOX || src == UDA_SCORE_MCBOX;
      if (!scalar && !box && src != UDA_SCORE_MCCLASS) { *why = "unknown source"; return 0; }
      if (scalar ? tr != UDA_SCORE_SCALAR : !(tr == UDA_SCORE_MEAN || (box && tr == UDA_SCORE_REL_MEAN))) {
        *why = "transform does not fit the source (SCALAR: entropy / det_score; MEAN: albox / mcbox / mcclass; REL_MEAN: albox / mcbox)";
        return 0;
      }
      mask |= 1u << src;
    }
  }
  return mask;
}

// the refusal when the model does not emit a source the descriptor reads; null when it emits them all
static const char* score_sources_missing(const uda_model_t& m, unsigned need) {
  if ((need & (1u << UDA_SCORE_ENTROPY)) && !m.enable_softmax) return "the model emits no entropy (enable_softmax is off)";
  if ((need & (1u << UDA_SCORE_ALBOX)) && !(m.has_uncert && m.loss_attenuation))
    return "the model emits no aleatoric box uncertainty (no loss attenuation)";
  if ((need & (1u << UDA_SCORE_MCBOX)) && !(m.has_uncert && m.box_stacked))
    return "the model emits no epistemic box uncertainty (no MC dropout on the box head)";
  if ((need & (1u << UDA_SCORE_MCCLASS)) && !(m.has_uncert && m.cls_stacked))
    return "the model emits no epistemic class uncertainty (no MC dropout on the class head)";
  return nullptr;
}

// The problem a descriptor poses on the run resident in the handle: the columns of the global post-process as its sources (after
// ensure_probs where it reads the entropy), every image of the last run.
static int resident_score_sources(uda_ctx* c, unsigned need, const uda_score_desc_t* desc, float min_score, ScoreArgs<float>& a) {
  const uda_model_t& m = c->model;
  a.n = c->last_n; a.M = m.max_output_size; a.C = m.num_classes; a.min_score = min_score; a.desc = *desc;
  if (need & (1u << UDA_SCORE_ENTROPY))
    if (int rc = ensure_probs(c, a.n * a.M)) return rc;
  const int bc = box_cols_of(m, UDA_POST_GLOBAL), cc = cls_cols_of(m, UDA_POST_GLOBAL);
  a.boxes = c->d_oboxes; a.scores = c->d_oscores; a.classes = c->d_oclasses; a.entropy = c->d_oentropy;
  a.albox = c->d_oboxes + 4;                                               // box | aleatoric std | MC std, as each exists
  a.mcbox = c->d_oboxes + ((m.has_uncert && m.loss_attenuation) ? 8 : 4);
  a.mcclass = c->d_oclasses + 1;
  a.box_stride = a.al_stride = a.mc_stride = bc; a.cls_stride = a.mcc_stride = cc; a.mcc_w = cc - 1;
  return 0;
}

// The same problem on host columns [n, M, width]: refuses a source the descriptor reads and the caller did not give, then
// uploads what is given.  host: boxes, scores, classes, entropy, albox, mcbox, mcclass (mcw columns).
template <typename T>
static int upload_score_sources(const char* who, DevScratch& s, unsigned need, const T* const (&host)[7], int n, int M, int C, int mcw,
                                const uda_score_desc_t* desc, T min_score, ScoreArgs<T>& a) {
  static const char* names[] = {"boxes", "scores", "classes", "entropy", "albox", "mcbox", "mcclass"};
  static const int source[] = {-1, UDA_SCORE_DET_SCORE, -1, UDA_SCORE_ENTROPY, UDA_SCORE_ALBOX, UDA_SCORE_MCBOX, UDA_SCORE_MCCLASS};
  const size_t nm = (size_t)n * M, widths[] = {4, 1, 1, 1, 4, 4, (size_t)(mcw > 0 ? mcw : 0)};
  for (int k = 0; k < 7; ++k)
    if (source[k] >= 0 && (need & (1u << source[k])) && nm && !host[k])
      return fail(nullptr, "%s: the descriptor reads %s, which is not given", who, names[k]);
  if ((need & (1u << UDA_SCORE_MCCLASS)) && mcw < 1) return fail(nullptr, "%s: mcclass_cols must be at least 1", who);
  const T* dev[7] = {};
  for (int k = 0; k < 7; ++k)
    if (nm * widths[k]) dev[k] = s.upload(host[k], nm * widths[k]);
  a.boxes = dev[0]; a.scores = dev[1]; a.classes = dev[2]; a.entropy = dev[3]; a.albox = dev[4]; a.mcbox = dev[5]; a.mcclass = dev[6];
  a.box_stride = a.al_stride = a.mc_stride = 4; a.cls_stride = 1; a.mcc_stride = a.mcc_w = (int)widths[6];
  a.n = n; a.M = M; a.C = C; a.min_score = min_score; a.desc = *desc;
  return 0;
}

extern "C" int uda_score_images(uda_ctx_t* c, const uda_score_desc_t* desc, float min_score) {
  if (!c) return 1;
  const uda_model_t& m = c->model;
  const char* why = nullptr;
  const unsigned need = score_desc_sources(desc, &why);
  if (why) return fail(c, "score_images: %s", why);
  if (int rc = resident_ready(c, "score_images", "the scores read")) return rc;
  if (const char* lacks = score_sources_missing(m, need)) return fail(c, "score_images: %s", lacks);
  if (m.max_output_size > kScoreMaxM) return fail(c, "score_images: max_output_size %d above %d", m.max_output_size, kScoreMaxM);
  if (m.num_classes < 1 || m.num_classes > kScoreMaxC) return fail(c, "score_images: num_classes %d outside 1..%d", m.num_classes, kScoreMaxC);
  if (int rc = settle_detections(c)) return rc;
  const int n = c->last_n, nc = desc->n_comp;
  if (!c->score.d) HIPC(c, dalloc(&c->score.d, ScorePack(nullptr, (size_t)m.max_images, UDA_SCORE_MAX_COMP, (size_t)m.num_classes).bytes()));
  {
    ProfScope ps(c, 19);
    const ScorePack pack(c->score.d, (size_t)n, (size_t)nc, (size_t)m.num_classes);
    ScoreArgs<float> a{};
    if (int rc = resident_score_sources(c, need, desc, min_score, a)) return rc;
    a.comp = pack.comp(); a.count = pack.count(); a.class_counts = pack.class_counts(); a.err = pack.err();
    HIPC(c, hipMemsetAsync(a.err, 0, sizeof(int32_t), c->stream));
    launch_score_images(a, c->stream);
  }
  HIPC(c, hipGetLastError());
  c->score_n = n; c->score_nc = nc; c->score.fetched = false;
  return 0;
}

extern "C" int uda_image_scores_shape(const uda_ctx_t* c, int32_t* n, int32_t* n_comp) {
  if (!c || !n || !n_comp) return 1;
  *n = c->score_n; *n_comp = c->score_nc;
  return 0;
}

extern "C" int uda_get_image_scores(uda_ctx_t* c, double* components, int32_t* count, int32_t* class_counts) {
  if (!c) return 1;
  if (c->score_n < 1) return fail(c, "get_image_scores: no scores (uda_score_images)");
  ScorePack h(nullptr, (size_t)c->score_n, (size_t)c->score_nc, (size_t)c->model.num_classes);
  if (int rc = fetch_result(c, c->score, h.bytes())) return rc;
  h.base = c->score.h.data();
  return h.copy_out(c, "score_images", components, count, class_counts);
}

// score_image for callers that hold detections of their own (calibrated columns, a gathered multi-GPU batch): host arrays in,
// the same kernel, host arrays out; its own allocations
template <typename T>
static int score_images_np(const char* who, int32_t device, const uda_score_desc_t* desc, T min_score, const T* boxes, const T* scores,
                           const T* classes, const T* entropy, const T* albox, const T* mcbox, const T* mcclass, int32_t n, int32_t M,
                           int32_t C, int32_t mcw, double* components, int32_t* count, int32_t* class_counts) {
  const char* why = nullptr;
  const unsigned need = score_desc_sources(desc, &why);
  if (why) return fail(nullptr, "%s: %s", who, why);
  if (n < 0 || M < 0 || M > kScoreMaxM || C < 1 || C > kScoreMaxC || ((size_t)n * M && (!boxes || !scores || !classes)))
    return fail(nullptr, "%s: bad argument", who);
  const T* host[] = {boxes, scores, classes, entropy, albox, mcbox, mcclass};
  DevScratch s(device);
  ScoreArgs<T> a{};
  if (int rc = upload_score_sources(who, s, need, host, n, M, C, mcw, desc, min_score, a)) return rc;
  if (n == 0) return 0;
  ScorePack pack(nullptr, (size_t)n, (size_t)desc->n_comp, (size_t)C);
  pack.base = s.alloc<char>(pack.bytes());
  s.zero(pack.base, pack.bytes());
  a.comp = pack.comp(); a.count = pack.count(); a.class_counts = pack.class_counts(); a.err = pack.err();
  if (s.ok()) launch_score_images(a, nullptr);
  std::vector<char> h;
  if (int rc = fetch_pack(who, s, pack.base, pack.bytes(), h)) return rc;
  return ScorePack(h.data(), pack.n, pack.nc, pack.C).copy_out(nullptr, who, components, count, class_counts);
}

extern "C" int uda_score_images_np(int32_t device, const uda_score_desc_t* desc, double min_score, const double* boxes,
                                   const double* scores, const double* classes, const double* entropy, const double* albox,
                                   const double* mcbox, const double* mcclass, int32_t n, int32_t M, int32_t num_classes,
                                   int32_t mcclass_cols, double* components, int32_t* count, int32_t* class_counts) {
  return score_images_np<double>("uda_score_images_np", device, desc, min_score, boxes, scores, classes, entropy, albox, mcbox, mcclass, n,
                                 M, num_classes, mcclass_cols, components, count, class_counts);
}

extern "C" int uda_score_images_np_f32(int32_t device, const uda_score_desc_t* desc, float min_score, const float* boxes,
                                       const float* scores, const float* classes, const float* entropy, const float* albox,
                                       const float* mcbox, const float* mcclass, int32_t n, int32_t M, int32_t num_classes,
                                       int32_t mcclass_cols, double* components, int32_t* count, int32_t* class_counts) {
  return score_images_np<float>("uda_score_images_np_f32", device, desc, min_score, boxes, scores, classes, entropy, albox, mcbox, mcclass,
                                n, M, num_classes, mcclass_cols, components, count, class_counts);
}

// ---- pseudo-labelling rows (reference SSL_stac.py:302-642 on the lines of infer_model.py:836-960)
// what the five scalars must satisfy beside a well-formed descriptor; null when they do
static const char* pseudo_args_bad(const uda_score_desc_t* d, int invert, int gate, double tau, int max_rows) {
  if (max_rows < 1) return "max_rows must be at least 1";
  if (!(tau >= 0.0)) return "tau must not be negative";
  if ((invert != 0 && invert != 1) || (gate != 0 && gate != 1)) return "invert and gate are 0 or 1";
  if (invert && d->n_comp < 2) return "invert needs 2 or 3 components";
  if (!invert && d->n_comp != 1) return "several components need invert";
  if (invert && gate) return "gate 1 (v > tau) belongs to the single-column branch, not to invert";
  return nullptr;
}

extern "C" int uda_pseudo_rows(uda_ctx_t* c, const uda_score_desc_t* desc, int32_t invert, int32_t gate, float min_score, double tau,
                               int32_t max_rows) {
  if (!c) return 1;
  const uda_model_t& m = c->model;
  const char* why = nullptr;
  const unsigned need = score_desc_sources(desc, &why);
  if (!why) why = pseudo_args_bad(desc, invert, gate, tau, max_rows);
  if (why) return fail(c, "pseudo_rows: %s", why);
  if (int rc = resident_ready(c, "pseudo_rows", "the pseudo-labels read")) return rc;
  if (const char* lacks = score_sources_missing(m, need)) return fail(c, "pseudo_rows: %s", lacks);
  if (m.max_output_size > kScoreMaxM) return fail(c, "pseudo_rows: max_output_size %d above %d", m.max_output_size, kScoreMaxM);
  if (m.num_classes < 1) return fail(c, "pseudo_rows: num_classes %d below 1", m.num_classes);
  if (int rc = settle_detections(c)) return rc;
  const int n = c->last_n, M = m.max_output_size, cap = std::min(M, max_rows);
  if (!c->pseudo.d) {
    HIPC(c, dalloc(&c->pseudo.d, PseudoPack(nullptr, (size_t)m.max_images, (size_t)M).bytes()));
    HIPC(c, hipMalloc(&c->pseudo.aux, (size_t)m.max_images * M * sizeof(PseudoRecord)));
  }
  {
    ProfScope ps(c, 21);
    const PseudoPack pack(c->pseudo.d, (size_t)n, (size_t)cap);
    PseudoArgs<float> a{};
    if (int rc = resident_score_sources(c, need, desc, min_score, a.s)) return rc;
    a.s.err = pack.err();
    a.tau = tau; a.invert = invert; a.gate = gate; a.max_rows = max_rows; a.cap = cap;
    a.minmax = pack.minmax(); a.kept = pack.kept(); a.cand = pack.cand(); a.records = pack.rec();
    a.slots = (PseudoRecord*)c->pseudo.aux;
    HIPC(c, hipMemsetAsync(a.s.err, 0, sizeof(int32_t), c->stream));
    launch_pseudo_rows(a, c->stream);
  }
  HIPC(c, hipGetLastError());
  c->pseudo_n = n; c->pseudo_cap = cap; c->pseudo.fetched = false;
  return 0;
}

// The host copy of the pack's head (fetch_result): the records stay on the device until uda_get_pseudo_rows asks for the used ones.
static int fetch_pseudo(uda_ctx* c, const char* who) {
  if (c->pseudo_n < 1) return fail(c, "%s: no pseudo-label rows (uda_pseudo_rows)", who);
  return fetch_result(c, c->pseudo, PseudoPack(nullptr, (size_t)c->pseudo_n, (size_t)c->pseudo_cap).head_bytes());
}

extern "C" int uda_pseudo_rows_shape(uda_ctx_t* c, int32_t* n, int64_t* K) {
  if (!c || !n || !K) return 1;
  if (int rc = fetch_pseudo(c, "pseudo_rows_shape")) return rc;
  *n = c->pseudo_n;
  *K = PseudoPack(c->pseudo.h.data(), (size_t)c->pseudo_n, (size_t)c->pseudo_cap).total();
  return 0;
}

extern "C" int uda_get_pseudo_rows(uda_ctx_t* c, void* records, int64_t n_records, double* minmax, int32_t* kept, int32_t* cand) {
  if (!c) return 1;
  if (int rc = fetch_pseudo(c, "get_pseudo_rows")) return rc;
  const PseudoPack h(c->pseudo.h.data(), (size_t)c->pseudo_n, (size_t)c->pseudo_cap);
  if (int rc = h.copy_out(c, "pseudo_rows", c->model.num_classes, nullptr, nullptr, 0, minmax, kept, cand)) return rc;
  if (!records) return 0;
  if (n_records != h.total()) return fail(c, "pseudo_rows: %lld candidate records, not %lld", (long long)h.total(), (long long)n_records);
  // the used records only, straight into the caller's array (the stream was waited for when the head was fetched)
  if (n_records)
    HIPC(c, hipMemcpy(records, PseudoPack(c->pseudo.d, h.n, h.cap).rec(), (size_t)n_records * sizeof(PseudoRecord), hipMemcpyDeviceToHost));
  return 0;
}

// score_image's first half for callers that hold detections of their own (calibrated columns, a gathered multi-GPU batch): host
// arrays in, the same kernels, host arrays out; its own allocations
template <typename T>
static int pseudo_rows_np(const char* who, int32_t device, const uda_score_desc_t* desc, T min_score, const T* boxes, const T* scores,
                          const T* classes, const T* entropy, const T* albox, const T* mcbox, const T* mcclass, int32_t n, int32_t M,
                          int32_t C, int32_t mcw, int32_t invert, int32_t gate, double tau, int32_t max_rows, void* records,
                          int64_t* n_records, double* minmax, int32_t* kept, int32_t* cand) {
  const char* why = nullptr;
  const unsigned need = score_desc_sources(desc, &why);
  if (!why) why = pseudo_args_bad(desc, invert, gate, tau, max_rows);
  if (why) return fail(nullptr, "%s: %s", who, why);
  if (n < 0 || M < 0 || M > kScoreMaxM || C < 1 || ((size_t)n * M && (!boxes || !scores || !classes)) || (records && !n_records))
    return fail(nullptr, "%s: bad argument", who);
  const T* host[] = {boxes, scores, classes, entropy, albox, mcbox, mcclass};
  DevScratch s(device);
  PseudoArgs<T> a{};
  if (int rc = upload_score_sources(who, s, need, host, n, M, C, mcw, desc, min_score, a.s)) return rc;
  if (n_records) *n_records = 0;
  if (n == 0) return 0;
  const size_t cap = (size_t)std::min(M, max_rows);
  PseudoPack pack(nullptr, (size_t)n, cap);
  pack.base = s.alloc<char>(pack.bytes());
  s.zero(pack.base, pack.bytes());
  a.s.err = pack.err();
  a.tau = tau; a.invert = invert; a.gate = gate; a.max_rows = max_rows; a.cap = (int)cap;
  a.minmax = pack.minmax(); a.kept = pack.kept(); a.cand = pack.cand(); a.records = pack.rec();
  a.slots = s.alloc<PseudoRecord>((size_t)n * cap);
  if (s.ok()) launch_pseudo_rows(a, nullptr);
  std::vector<char> h;
  if (int rc = fetch_pack(who, s, pack.base, pack.head_bytes(), h)) return rc;
  const PseudoPack hp(h.data(), pack.n, pack.cap);
  const int64_t K = hp.total();
  std::vector<char> recs;
  if (records && K && !*hp.err()) {
    recs.resize((size_t)K * sizeof(PseudoRecord));
    s.download(recs.data(), pack.rec(), recs.size());
    if (!s.ok()) return hip_failed(nullptr, who, s.err);
  }
  if (n_records) *n_records = K;
  return hp.copy_out(nullptr, who, C, recs.data(), records, K, minmax, kept, cand);
}

extern "C" int uda_pseudo_rows_np(int32_t device, const uda_score_desc_t* desc, double min_score, const double* boxes,
                                  const double* scores, const double* classes, const double* entropy, const double* albox,
                                  const double* mcbox, const double* mcclass, int32_t n, int32_t M, int32_t num_classes,
                                  int32_t mcclass_cols, int32_t invert, int32_t gate, double tau, int32_t max_rows, void* records,
                                  int64_t* n_records, double* minmax, int32_t* kept, int32_t* cand) {
  return pseudo_rows_np<double>("uda_pseudo_rows_np", device, desc, min_score, boxes, scores, classes, entropy, albox, mcbox, mcclass, n, M,
                                num_classes, mcclass_cols, invert, gate, tau, max_rows, records, n_records, minmax, kept, cand);
}

extern "C" int uda_pseudo_rows_np_f32(int32_t device, const uda_score_desc_t* desc, float min_score, const float* boxes,
                                      const float* scores, const float* classes, const float* entropy, const float* albox,
                                      const float* mcbox, const float* mcclass, int32_t n, int32_t M, int32_t num_classes,
                                      int32_t mcclass_cols, int32_t invert, int32_t gate, double tau, int32_t max_rows, void* records,
                                      int64_t* n_records, double* minmax, int32_t* kept, int32_t* cand) {
  return pseudo_rows_np<float>("uda_pseudo_rows_np_f32", device, desc, min_score, boxes, scores, classes, entropy, albox, mcbox, mcclass, n,
                               M, num_classes, mcclass_cols, invert, gate, tau, max_rows, records, n_records, minmax, kept, cand);
}

// ---- label correction (reference ssl_utils/glc.py:182-187, 432-436, 551, 813-834)
// what the scalars must satisfy; null when they do
static const char* label_check_args_bad(int methods, int md_rule) {
  if (methods < 1 || methods > (LC_MD | LC_MISTAKES | LC_NOISY)) return "methods is a bit set of md (1), mistakes (2) and noisy (4), at least one";
  if (md_rule != LC_MD_EQ && md_rule != LC_MD_LE) return "md_rule is 0 (==) or 1 (<=)";
  return nullptr;
}

extern "C" int uda_label_check(uda_ctx_t* c, float min_score, double iou_consist, double md_max_inter, int32_t md_rule,
                               double correct_max_inter, float correct_score, int32_t methods) {
  if (!c) return 1;
  const uda_model_t& m = c->model;
  if (const char* why = label_check_args_bad(methods, md_rule)) return fail(c, "label_check: %s", why);
  if (c->gt.n < 1) return fail(c, "label_check: no ground truth is set (uda_set_ground_truth)");
  if (int rc = resident_ready(c, "label_check", "the label check reads")) return rc;
  if (int rc = gt_covers_run(c, "label_check", c->gt.n, true)) return rc;
  const bool cons = holds_consistency_run(c);
  if ((methods & (LC_MD | LC_NOISY)) && !cons)
    return fail(c, "label_check: md and noisy read cons_iou, and the resident run is not a consistency run (uda_run_consistency)");
  if (m.max_output_size > kAssignMaxM) return fail(c, "label_check: max_output_size %d above %d", m.max_output_size, kAssignMaxM);
  if (int rc = settle_detections(c)) return rc;
  const int n = c->gt.n, M = m.max_output_size, G = c->gt.G;
  if (!c->lc.d || G > c->lc.cap) {
    HIPC(c, hipStreamSynchronize(c->stream));              // (growing is rare: nothing may still read the old buffer)
    c->lc.release();
    c->lc_n = 0;
    const int cap = std::max(G, 1);
    HIPC(c, dalloc(&c->lc.d, LabelPack(nullptr, (size_t)m.max_images, (size_t)cap, (size_t)M).bytes()));
    c->lc.cap = cap;
  }
  LabelCheckArgs<float> a{};
  a.det_boxes = c->d_oboxes; a.det_stride = box_cols_of(m, UDA_POST_GLOBAL); a.scores = c->d_oscores;
  a.cons_iou = cons ? c->d_cons_iou : nullptr;
  a.gt_boxes = c->gt.d[0]; a.gt_classes = c->gt.d[1];
  LabelPack(c->lc.d, (size_t)n, (size_t)G, (size_t)M).fill(a, methods, md_rule, min_score, correct_score, iou_consist, md_max_inter, correct_max_inter);
  launch_label_check(a, c->stream);
  HIPC(c, hipGetLastError());
  c->lc_n = n; c->lc_G = G; c->lc.fetched = false;
  return 0;
}

extern "C" int uda_get_label_check(uda_ctx_t* c, int32_t* det_rank, double* iou, uint8_t* gt_flags, float* gt_boxes_out,
                                   uint8_t* det_flags, double* det_max_iou, int32_t* counts) {
  if (!c) return 1;
  if (c->lc_n < 1) return fail(c, "get_label_check: no label check (uda_label_check)");
  LabelPack h(nullptr, (size_t)c->lc_n, (size_t)c->lc_G, (size_t)c->model.max_output_size);
  if (int rc = fetch_result(c, c->lc, h.copy_bytes())) return rc;
  h.base = c->lc.h.data();
  h.copy_out(det_rank, iou, gt_flags, gt_boxes_out, det_flags, det_max_iou, counts);
  return 0;
}

// the label check for callers that hold detections of their own (a parsed prediction_data.txt, a gathered multi-GPU batch): host
// arrays in, the same kernel, host arrays out; its own allocations
template <typename T>
static int label_check_np(const char* who, int32_t device, const T* boxes, const T* scores, const double* cons_iou, const T* gt_boxes,
                          const T* gt_classes, int32_t n, int32_t M, int32_t G, T min_score, double iou_consist, double md_max_inter,
                          int32_t md_rule, double correct_max_inter, T correct_score, int32_t methods, int32_t* det_rank, double* iou,
                          uint8_t* gt_flags, float* gt_boxes_out, uint8_t* det_flags, double* det_max_iou, int32_t* counts) {
  if (const char* why = label_check_args_bad(methods, md_rule)) return fail(nullptr, "%s: %s", who, why);
  if (n < 1) return fail(nullptr, "%s: %d images, at least 1", who, n);
  if (M < 0 || M > kAssignMaxM) return fail(nullptr, "%s: %d detection rows per image, at most %d", who, M, kAssignMaxM);
  if (G < 0 || G > kAssignMaxG) return fail(nullptr, "%s: %d ground-truth rows per image, at most %d", who, G, kAssignMaxG);
  const size_t nm = (size_t)n * M, ng = (size_t)n * G;
  if ((nm && (!boxes || !scores)) || (ng && (!gt_boxes || !gt_classes))) return fail(nullptr, "%s: NULL input", who);
  if ((methods & (LC_MD | LC_NOISY)) && nm && !cons_iou) return fail(nullptr, "%s: md and noisy read cons_iou, which is not given", who);
  DevScratch s(device);
  LabelCheckArgs<T> a{};
  a.det_boxes = s.upload(boxes, nm * 4); a.det_stride = 4; a.scores = s.upload(scores, nm);
  a.cons_iou = (methods & (LC_MD | LC_NOISY)) ? s.upload(cons_iou, nm) : nullptr;
  a.gt_boxes = s.upload(gt_boxes, ng * 4); a.gt_classes = s.upload(gt_classes, ng);
  LabelPack pack(nullptr, (size_t)n, (size_t)G, (size_t)M);
  pack.base = s.alloc<char>(pack.bytes());
  pack.fill(a, methods, md_rule, min_score, correct_score, iou_consist, md_max_inter, correct_max_inter);
  if (s.ok()) launch_label_check(a, nullptr);
  std::vector<char> h;
  if (int rc = fetch_pack(who, s, pack.base, pack.copy_bytes(), h)) return rc;
  LabelPack(h.data(), pack.n, pack.G, pack.M).copy_out(det_rank, iou, gt_flags, gt_boxes_out, det_flags, det_max_iou, counts);
  return 0;
}

extern "C" int uda_label_check_np(int32_t device, const double* boxes, const double* scores, const double* cons_iou,
                                  const double* gt_boxes, const double* gt_classes, int32_t n, int32_t M, int32_t G, double min_score,
                                  double iou_consist, double md_max_inter, int32_t md_rule, double correct_max_inter,
                                  double correct_score, int32_t methods, int32_t* det_rank, double* iou, uint8_t* gt_flags,
                                  float* gt_boxes_out, uint8_t* det_flags, double* det_max_iou, int32_t* counts) {
  return label_check_np<double>("uda_label_check_np", device, boxes, scores, cons_iou, gt_boxes, gt_classes, n, M, G, min_score,
                                iou_consist, md_max_inter, md_rule, correct_max_inter, correct_score, methods, det_rank, iou, gt_flags,
                                gt_boxes_out, det_flags, det_max_iou, counts);
}

extern "C" int uda_label_check_np_f32(int32_t device, const float* boxes, const float* scores, const double* cons_iou,
                                      const float* gt_boxes, const float* gt_classes, int32_t n, int32_t M, int32_t G, float min_score,
                                      double iou_consist, double md_max_inter, int32_t md_rule, double correct_max_inter,
                                      float correct_score, int32_t methods, int32_t* det_rank, double* iou, uint8_t* gt_flags,
                                      float* gt_boxes_out, uint8_t* det_flags, double* det_max_iou, int32_t* counts) {
  return label_check_np<float>("uda_label_check_np_f32", device, boxes, scores, cons_iou, gt_boxes, gt_classes, n, M, G, min_score,
                               iou_consist, md_max_inter, md_rule, correct_max_inter, correct_score, methods, det_rank, iou, gt_flags,
                               gt_boxes_out, det_flags, det_max_iou, counts);
}

// ---- COCO matching (reference custom_cocoeval.py:265-349 on the containers of coco_metric.py:219-283)
static const int kEvalMaxC = 8192;

static const char* eval_thrs_bad(const double* thrs, int32_t T) {
  if (T < 1 || T > COCO_MAX_T) return "T outside 1..32 thresholds";
  if (!thrs) return "NULL thresholds";
  return nullptr;
}

extern "C" int uda_set_eval_ground_truth(uda_ctx_t* c, const float* gt, int32_t n, int32_t G) {
  if (!c || !gt) return c ? fail(c, "set_eval_ground_truth: NULL argument") : 1;
  const uda_model_t& m = c->model;
  if (n < 1 || n > m.max_images) return fail(c, "set_eval_ground_truth: %d images, the handle holds 1..%d", n, m.max_images);
  if (G < 0 || G > COCO_MAX_G) return fail(c, "set_eval_ground_truth: %d ground-truth rows per image, at most %d", G, (int)COCO_MAX_G);
  const float* src[] = {gt, nullptr};
  return stage_ground_truth(c, c->egt, src, n, G);
}

extern "C" int uda_eval_match(uda_ctx_t* c, const double* iou_thrs, int32_t T) {
  if (!c) return 1;
  const uda_model_t& m = c->model;
  if (const char* why = eval_thrs_bad(iou_thrs, T)) return fail(c, "eval_match: %s", why);
  if (c->egt.n < 1) return fail(c, "eval_match: no ground truth is set (uda_set_eval_ground_truth)");
  if (int rc = resident_ready(c, "eval_match", nullptr)) return rc;
  if (int rc = gt_covers_run(c, "eval_match", c->egt.n, false)) return rc;
  if (m.max_output_size > COCO_MAX_M) return fail(c, "eval_match: max_output_size %d above %d", m.max_output_size, (int)COCO_MAX_M);
  if (m.num_classes < 1 || m.num_classes > kEvalMaxC) return fail(c, "eval_match: num_classes %d outside 1..%d", m.num_classes, kEvalMaxC);
  if (int rc = settle_detections(c)) return rc;
  const int n = c->last_n, M = m.max_output_size, C = m.num_classes;
  if (!c->eval.d) HIPC(c, dalloc(&c->eval.d, EvalPack(nullptr, (size_t)m.max_images, (size_t)M, (size_t)C).bytes()));
  {
    ProfScope ps(c, 20);
    CocoMatchArgs a{};
    a.boxes = c->d_oboxes; a.scores = c->d_oscores; a.classes = c->d_oclasses;
    a.box_stride = box_cols_of(m, c->last_post_mode); a.cls_stride = cls_cols_of(m, c->last_post_mode);
    a.gt = c->egt.d[0];
    const EvalPack pack(c->eval.d, (size_t)n, (size_t)M, (size_t)C);
    a.rec = pack.rec(); a.npig = pack.npig(); a.used = pack.used();
    a.n = n; a.M = M; a.G = c->egt.G; a.C = C; a.T = T; a.legacy = 0;
    for (int t = 0; t < T; ++t) a.thr[t] = iou_thrs[t];
    launch_coco_match(a, c->stream);
  }
  HIPC(c, hipGetLastError());
  c->eval_n = n; c->eval.fetched = false;
  return 0;
}

extern "C" int uda_get_eval_records(uda_ctx_t* c, void* records, int32_t* npig, int32_t* used) {
  if (!c) return 1;
  if (c->eval_n < 1) return fail(c, "get_eval_records: no match (uda_eval_match)");
  EvalPack h(nullptr, (size_t)c->eval_n, (size_t)c->model.max_output_size, (size_t)c->model.num_classes);
  if (int rc = fetch_result(c, c->eval, h.bytes())) return rc;
  h.base = c->eval.h.data();
  h.copy_out(records, npig, used);
  return 0;
}

// evaluateImg for callers that hold legacy rows of their own (the nms_np route, gathered detections): host arrays in, the same
// kernel in its legacy-row layout, host arrays out; its own allocations
extern "C" int uda_eval_match_np(int32_t device, const float* det_rows, const float* gt, int32_t n, int32_t M, int32_t G,
                                 int32_t num_classes, const double* iou_thrs, int32_t T, void* records, int32_t* npig, int32_t* used) {
  if (const char* why = eval_thrs_bad(iou_thrs, T)) return fail(nullptr, "uda_eval_match_np: %s", why);
  if (G > COCO_MAX_G) return fail(nullptr, "uda_eval_match_np: %d ground-truth rows per image, at most %d", G, (int)COCO_MAX_G);
  if (M > COCO_MAX_M) return fail(nullptr, "uda_eval_match_np: %d detection rows per image, at most %d", M, (int)COCO_MAX_M);
  if (n < 0 || M < 0 || G < 0 || num_classes < 1 || num_classes > kEvalMaxC || ((size_t)n * M && !det_rows) || ((size_t)n * G && !gt))
    return fail(nullptr, "uda_eval_match_np: bad argument");
  if (n == 0) return 0;
  DevScratch s(device);
  CocoMatchArgs a{};
  a.rows = s.upload(det_rows, (size_t)n * M * 7); a.gt = s.upload(gt, (size_t)n * G * 7);
  EvalPack pack(nullptr, (size_t)n, (size_t)M, (size_t)num_classes);
  pack.base = s.alloc<char>(pack.bytes());
  s.zero(pack.base, pack.bytes());
  a.rec = pack.rec(); a.npig = pack.npig(); a.used = pack.used();
  a.n = n; a.M = M; a.G = G; a.C = num_classes; a.T = T; a.legacy = 1;
  for (int t = 0; t < T; ++t) a.thr[t] = iou_thrs[t];
  if (s.ok()) launch_coco_match(a, nullptr);
  std::vector<char> h;
  if (int rc = fetch_pack("uda_eval_match_np", s, pack.base, pack.bytes(), h)) return rc;
  EvalPack(h.data(), pack.n, pack.M, pack.C).copy_out(records, npig, used);
  return 0;
}

// the objective of the thresholding search for P candidates: host arrays in, chunks of candidates through the device (scratch of
// at most kThrScratchBytes, or one candidate's), host arrays out; its own allocations
static const size_t kThrScratchBytes = (size_t)64 << 20;
extern "C" int uda_thr_objective_np(int32_t device, const double* uncerts, const double* ious, const uint8_t* tp_class,
                                    const int32_t* group, int32_t N, int32_t U, int32_t G, const double* iou_thrs, int32_t K,
                                    const double* params, int32_t P, int32_t fix_cd, double budget, double* thr, double* rate,
                                    double* auc) {
  const char* who = "uda_thr_objective_np";
  if (N < 2 || N > THR_MAX_N) return fail(nullptr, "%s: %d rows, 2..%d are taken", who, N, (int)THR_MAX_N);
  if (U < 1 || U > THR_MAX_U) return fail(nullptr, "%s: %d uncertainties, 1..%d are taken", who, U, (int)THR_MAX_U);
  if (K < 1 || K > THR_MAX_K) return fail(nullptr, "%s: %d IoU thresholds, 1..%d are taken", who, K, (int)THR_MAX_K);
  if (P < 1 || P > THR_MAX_P) return fail(nullptr, "%s: %d candidates, 1..%d are taken", who, P, (int)THR_MAX_P);
  if (G < 0 || G > THR_MAX_G) return fail(nullptr, "%s: %d groups, 0..%d are taken", who, G, (int)THR_MAX_G);
  if (!uncerts || !ious || !tp_class || !iou_thrs || !params) return fail(nullptr, "%s: NULL input", who);
  if ((G > 0) != (group != nullptr)) return fail(nullptr, "%s: group ids and G > 0 go together", who);
  if (!(budget > 0.0 && budget < 1.0)) return fail(nullptr, "%s: budget %g is not strictly between 0 and 1", who, budget);
  for (int i = 0; group && i < N; ++i)
    if (group[i] < 0 || group[i] >= G) return fail(nullptr, "%s: group id %d of row %d outside 0..%d", who, group[i], i, G - 1);
  int Npad = THR_TILE;
  while (Npad < N) Npad <<= 1;
  const size_t n = (size_t)N, stride = (size_t)U * (size_t)(G > 0 ? G : 1);
  const size_t per = 12 * (size_t)Npad + 8 * n * K + 24 * (size_t)K + 8 * stride;
  size_t fit = kThrScratchBytes / per;
  const int Pc = (int)std::min<size_t>(std::max<size_t>(fit, 1), std::min<size_t>((size_t)P, THR_MAX_CHUNK));
  DevScratch s(device);
  ThrArgs a{};
  a.uncerts = s.upload(uncerts, n * U); a.ious = s.upload(ious, n); a.tp_class = s.upload(tp_class, n); a.group = s.upload(group, n);
  a.mask = s.alloc<uint32_t>(n);
  double* d_par = s.alloc<double>((size_t)Pc * stride);
  a.params = d_par;
  a.keys = s.alloc<uint64_t>((size_t)Pc * Npad); a.rows = s.alloc<int32_t>((size_t)Pc * Npad);
  a.runs = s.alloc<int32_t>((size_t)Pc * K * 2 * n); a.out = s.alloc<double>((size_t)Pc * K * 3);
  a.N = N; a.Npad = Npad; a.U = U; a.G = G; a.K = K; a.fix_cd = fix_cd != 0; a.budget = budget;
  for (int k = 0; k < K; ++k) a.thr[k] = iou_thrs[k];
  if (s.ok()) launch_thr_mask(a, nullptr);
  std::vector<double> h((size_t)Pc * K * 3);
  for (int p0 = 0; s.ok() && p0 < P; p0 += Pc) {
    a.Pc = std::min(Pc, P - p0);
    s.err = hipMemcpy(d_par, params + (size_t)p0 * stride, (size_t)a.Pc * stride * sizeof(double), hipMemcpyHostToDevice);
    if (s.ok()) launch_thr_objective(a, nullptr);
    if (s.ok()) s.err = hipGetLastError();
    s.download(h.data(), a.out, (size_t)a.Pc * K * 3 * sizeof(double));
    if (!s.ok()) break;
    for (size_t q = 0; q < (size_t)a.Pc * K; ++q) {
      const size_t o = (size_t)p0 * K + q;
      if (thr) thr[o] = h[3 * q];
      if (rate) rate[o] = h[3 * q + 1];
      if (auc) auc[o] = h[3 * q + 2];
    }
  }
  return scratch_done(nullptr, who, s);
}

// the thresholding report for B row segments x S ready score columns: one packed upload, the curves of every segment through the
// objective's kernels on offset pointers (the S columns as S unit-weight candidates: 1.0 * u + 0.0 * u' is u for finite values),
// in chunks of columns that fit kThrScratchBytes, then one launch for counts and moments, one packed download.  All launches go
// to the null stream in order, so segments share the sort scratch and nothing waits on the host between them
extern "C" int uda_thr_report_np(int32_t device, const double* scores, const double* ious, const uint8_t* tp_class, int32_t N,
                                 int32_t S, const double* iou_thrs, int32_t K, const int32_t* seg_lo, const int32_t* seg_hi,
                                 int32_t B, int32_t fix_cd, double budget, double* roc, int64_t* n_label, double* moments,
                                 int64_t* removed) {
  const char* who = "uda_thr_report_np";
  if (N < 2 || N > THR_MAX_N) return fail(nullptr, "%s: %d rows, 2..%d are taken", who, N, (int)THR_MAX_N);
  if (S < 1 || S > THRREP_MAX_S) return fail(nullptr, "%s: %d score columns, 1..%d are taken", who, S, (int)THRREP_MAX_S);
  if (K < 1 || K > THR_MAX_K) return fail(nullptr, "%s: %d IoU thresholds, 1..%d are taken", who, K, (int)THR_MAX_K);
  if (B < 1 || B > THRREP_MAX_B) return fail(nullptr, "%s: %d segments, 1..%d are taken", who, B, (int)THRREP_MAX_B);
  if (!scores || !ious || !tp_class || !iou_thrs || !seg_lo || !seg_hi) return fail(nullptr, "%s: NULL input", who);
  if (!(budget > 0.0 && budget < 1.0)) return fail(nullptr, "%s: budget %g is not strictly between 0 and 1", who, budget);
  int n_max = 0;
  for (int b = 0; b < B; ++b) {
    if (seg_lo[b] < 0 || seg_hi[b] < seg_lo[b] || seg_hi[b] > N)
      return fail(nullptr, "%s: segment %d is [%d, %d), not a range inside [0, %d]", who, b, seg_lo[b], seg_hi[b], N);
    n_max = std::max(n_max, seg_hi[b] - seg_lo[b]);
  }
  int Npad_max = THR_TILE;
  while (Npad_max < n_max) Npad_max <<= 1;
  const size_t n = (size_t)N, per = 12 * (size_t)Npad_max + 8 * (size_t)n_max * K;
  const int Sc = (int)std::min<size_t>(std::max<size_t>(kThrScratchBytes / per, 1), (size_t)S);

  // the inputs as one pack: float64 scores | ious | unit weights, int32 seg_lo | seg_hi, uint8 tp_class
  const size_t o_iou = 8 * n * S, o_eye = o_iou + 8 * n, o_lo = o_eye + 8 * (size_t)S * S, o_hi = o_lo + 4 * (size_t)B,
               o_tp = o_hi + 4 * (size_t)B, in_bytes = o_tp + n;
  std::vector<char> in(in_bytes);
  memcpy(in.data(), scores, o_iou);
  memcpy(in.data() + o_iou, ious, 8 * n);
  for (int i = 0; i < S * S; ++i) ((double*)(in.data() + o_eye))[i] = i / S == i % S ? 1.0 : 0.0;
  memcpy(in.data() + o_lo, seg_lo, 4 * (size_t)B);
  memcpy(in.data() + o_hi, seg_hi, 4 * (size_t)B);
  memcpy(in.data() + o_tp, tp_class, n);

  DevScratch s(device);
  char* d_in = s.upload(in.data(), in_bytes);
  ThrArgs t{};
  t.mask = s.alloc<uint32_t>(n);
  t.keys = s.alloc<uint64_t>((size_t)Sc * Npad_max); t.rows = s.alloc<int32_t>((size_t)Sc * Npad_max);
  t.runs = s.alloc<int32_t>((size_t)Sc * K * 2 * (size_t)n_max);
  // the outputs as one pack of 8-byte values: roc | moments | removed | n_label
  const size_t slots = (size_t)B * S * K, n_pack = slots * (3 + 4 + 3) + (size_t)B * K * 2;
  double* pack = s.alloc<double>(n_pack);
  if (int rc = scratch_done(nullptr, who, s)) return rc;
  s.zero(pack, n_pack * sizeof(double));
  const double* d_scores = (const double*)d_in;
  const double* d_eye = (const double*)(d_in + o_eye);
  ThrRepArgs r{};
  r.scores = d_scores; r.mask = t.mask; r.seg_lo = (const int32_t*)(d_in + o_lo); r.seg_hi = (const int32_t*)(d_in + o_hi);
  r.roc = pack; r.moments = pack + 3 * slots; r.removed = (long long*)(pack + 7 * slots); r.n_label = (long long*)(pack + 10 * slots);
  r.N = N; r.S = S; r.K = K; r.B = B;
  t.uncerts = d_scores; t.ious = (const double*)(d_in + o_iou); t.tp_class = (const uint8_t*)(d_in + o_tp);
  t.N = N; t.K = K; t.U = S; t.G = 0; t.ld = N; t.fix_cd = fix_cd != 0; t.budget = budget;
  for (int k = 0; k < K; ++k) t.thr[k] = iou_thrs[k];
  if (s.ok()) {
    launch_thr_mask(t, nullptr);
    launch_thr_report_fill(r, nullptr);
    const uint32_t* d_mask = t.mask;
    for (int b = 0; b < B; ++b) {
      const int lo = seg_lo[b], nb = seg_hi[b] - lo;
      if (nb < 2) continue;                                 // no curve: the slot keeps +inf, NaN, NaN
      ThrArgs c = t;
      c.uncerts = d_scores + lo; c.mask = const_cast<uint32_t*>(d_mask) + lo; c.N = nb;
      c.Npad = THR_TILE;
      while (c.Npad < nb) c.Npad <<= 1;
      for (int s0 = 0; s0 < S; s0 += Sc) {
        c.Pc = std::min(Sc, S - s0);
        c.params = d_eye + (size_t)s0 * S;
        c.out = pack + (((size_t)b * S + s0) * K) * 3;
        launch_thr_objective(c, nullptr);
      }
    }
    launch_thr_report(r, nullptr);
  }
  std::vector<char> h;
  if (int rc = fetch_pack(who, s, pack, n_pack * sizeof(double), h)) return rc;
  const double* hp = (const double*)h.data();
  if (roc) memcpy(roc, hp, 3 * slots * 8);
  if (moments) memcpy(moments, hp + 3 * slots, 4 * slots * 8);
  if (removed) memcpy(removed, hp + 7 * slots, 3 * slots * 8);
  if (n_label) memcpy(n_label, hp + 10 * slots, (size_t)B * K * 2 * 8);
  return 0;
}

// the heat maps of the post-thresholding analysis: everything is checked on the host first (a rectangle outside the map would be
// harmless to the kernel, which writes its own pixels only, but it is not what the caller meant), then one upload per table, one
// launch of tiles x M blocks, one download per output
extern "C" int uda_heat_maps_np(int32_t device, const int32_t* rects, int32_t R, const double* values, int32_t V, const uint8_t* sel,
                                int32_t Q, int32_t N, const int32_t* map_rect, const int32_t* map_value, const int32_t* map_sel,
                                const int32_t* map_mean, int32_t M, int32_t H, int32_t W, double* heat, int32_t* count) {
  const char* who = "uda_heat_maps_np";
  if (N < 1 || N > THR_MAX_N) return fail(nullptr, "%s: %d rows, 1..%d are taken", who, N, (int)THR_MAX_N);
  if (M < 1 || M > HEAT_MAX_M) return fail(nullptr, "%s: %d maps, 1..%d are taken", who, M, (int)HEAT_MAX_M);
  if (R < 1 || R > HEAT_MAX_R) return fail(nullptr, "%s: %d rectangle sets, 1..%d are taken", who, R, (int)HEAT_MAX_R);
  if (V < 0 || V > HEAT_MAX_V) return fail(nullptr, "%s: %d value columns, 0..%d are taken", who, V, (int)HEAT_MAX_V);
  if (Q < 0 || Q > HEAT_MAX_Q) return fail(nullptr, "%s: %d selectors, 0..%d are taken", who, Q, (int)HEAT_MAX_Q);
  if (H < 1 || W < 1 || (int64_t)H * W > HEAT_MAX_PIXELS)
    return fail(nullptr, "%s: a map of %d x %d, at least 1 x 1 and at most %d pixels are taken", who, H, W, (int)HEAT_MAX_PIXELS);
  if (!rects || !map_rect || !map_value || !map_sel || !map_mean || (V > 0 && !values) || (Q > 0 && !sel))
    return fail(nullptr, "%s: NULL input", who);
  for (int m = 0; m < M; ++m) {
    if (map_rect[m] < 0 || map_rect[m] >= R) return fail(nullptr, "%s: map %d reads rectangle set %d of %d", who, m, map_rect[m], R);
    if (map_value[m] < -1 || map_value[m] >= V) return fail(nullptr, "%s: map %d reads value column %d of %d", who, m, map_value[m], V);
    if (map_sel[m] < -1 || map_sel[m] >= Q) return fail(nullptr, "%s: map %d reads selector %d of %d", who, m, map_sel[m], Q);
  }
  const size_t n = (size_t)N, px = (size_t)H * W;
  for (size_t i = 0; i < (size_t)R * n; ++i) {
    const int32_t* q = rects + 4 * i;
    if (q[0] < 0 || q[0] > H || q[1] < 0 || q[1] > H || q[2] < 0 || q[2] > W || q[3] < 0 || q[3] > W)
      return fail(nullptr, "%s: rectangle %d of set %d is rows [%d, %d) x columns [%d, %d), outside the %d x %d map", who,
                  (int)(i % n), (int)(i / n), q[0], q[1], q[2], q[3], H, W);
  }
  DevScratch s(device);
  HeatArgs a{};
  a.rects = (const int4*)s.upload(rects, 4 * (size_t)R * n);
  a.values = V ? s.upload(values, (size_t)V * n) : nullptr;
  a.sel = Q ? s.upload(sel, (size_t)Q * n) : nullptr;
  a.heat = s.alloc<double>((size_t)M * px);
  a.count = count ? s.alloc<int32_t>((size_t)M * px) : nullptr;
  a.N = N; a.H = H; a.W = W; a.tiles_x = (W + HEAT_TILE_W - 1) / HEAT_TILE_W;
  for (int m = 0; m < M; ++m) {
    a.map_rect[m] = map_rect[m]; a.map_value[m] = map_value[m]; a.map_sel[m] = map_sel[m]; a.map_mean[m] = map_mean[m] != 0;
  }
  const int tiles = a.tiles_x * ((H + HEAT_TILE_H - 1) / HEAT_TILE_H);
  if (s.ok()) launch_heat_maps(a, tiles, M, nullptr);
  s.sync();
  if (int rc = scratch_done(nullptr, who, s)) return rc;
  // (the outputs are written only from here on; a copy that fails half way is HIP's failure, not a refusal)
  if (heat) s.download(heat, a.heat, (size_t)M * px * sizeof(double));
  if (count) s.download(count, a.count, (size_t)M * px * sizeof(int32_t));
  return scratch_done(nullptr, who, s);
}

// the tallies of the post-thresholding analysis: one packed upload of the float64 columns, one launch of K blocks, one packed
// download (counts | iou_sum | img_count | img_first)
extern "C" int uda_thr_post_np(int32_t device, const double* u, const double* ious, const uint8_t* tp_class, const int32_t* image,
                               int32_t N, int32_t I, const double* iou_thrs, const double* thrs, int32_t K, int32_t k_img,
                               int64_t* counts, double* iou_sum, int32_t* img_count, int32_t* img_first) {
  const char* who = "uda_thr_post_np";
  if (N < 2 || N > THR_MAX_N) return fail(nullptr, "%s: %d rows, 2..%d are taken", who, N, (int)THR_MAX_N);
  if (K < 1 || K > THR_MAX_K) return fail(nullptr, "%s: %d IoU thresholds, 1..%d are taken", who, K, (int)THR_MAX_K);
  if (k_img < -1 || k_img >= K) return fail(nullptr, "%s: k_img %d, -1..%d are taken", who, k_img, K - 1);
  if (!u || !ious || !tp_class || !iou_thrs || !thrs) return fail(nullptr, "%s: NULL input", who);
  const bool images = k_img >= 0;
  if (images) {
    if (!image) return fail(nullptr, "%s: k_img %d without image ids", who, k_img);
    if (I < 1 || I > N) return fail(nullptr, "%s: %d images for %d rows, 1..%d are taken", who, I, N, N);
    for (int i = 0; i < N; ++i)
      if (image[i] < 0 || image[i] >= I) return fail(nullptr, "%s: image id %d of row %d outside 0..%d", who, image[i], i, I - 1);
  }
  for (int k = 0; k < K; ++k)
    if (iou_thrs[k] != iou_thrs[k] || thrs[k] != thrs[k]) return fail(nullptr, "%s: threshold %d is NaN", who, k);
  for (int i = 0; i < N; ++i)
    if (u[i] != u[i] || ious[i] != ious[i]) return fail(nullptr, "%s: row %d holds NaN", who, i);
  const size_t n = (size_t)N, ni = images ? (size_t)I : 0;
  std::vector<double> in(2 * n);
  memcpy(in.data(), u, 8 * n);
  memcpy(in.data() + n, ious, 8 * n);
  DevScratch s(device);
  const double* d_in = s.upload(in.data(), 2 * n);
  ThrPostArgs a{};
  a.u = d_in; a.ious = d_in + n;
  a.tp = s.upload(tp_class, n);
  a.image = images ? s.upload(image, n) : nullptr;
  // the outputs as one pack: 8-byte values counts [K, 8] | iou_sum [K, 2], then int32 img_count [I, 4] | img_first [I, 3]
  const size_t n8 = 10 * (size_t)K, pack_bytes = 8 * n8 + 4 * 7 * ni;
  char* pack = s.alloc<char>(pack_bytes);
  if (int rc = scratch_done(nullptr, who, s)) return rc;
  a.counts = (long long*)pack; a.iou_sum = (double*)pack + 8 * (size_t)K;
  a.img_count = (int32_t*)(pack + 8 * n8); a.img_first = a.img_count + 4 * ni;
  a.N = N; a.K = K; a.k_img = k_img;
  for (int k = 0; k < K; ++k) { a.iou_thr[k] = iou_thrs[k]; a.thr[k] = thrs[k]; }
  if (images) {
    s.zero(a.img_count, 4 * 4 * ni);
    std::vector<int32_t> none(3 * ni, N);
    if (s.ok()) s.err = hipMemcpy(a.img_first, none.data(), 4 * 3 * ni, hipMemcpyHostToDevice);
  }
  if (s.ok()) launch_thr_post(a, nullptr);
  std::vector<char> h;
  if (int rc = fetch_pack(who, s, pack, pack_bytes, h)) return rc;
  if (counts) memcpy(counts, h.data(), 8 * 8 * (size_t)K);
  if (iou_sum) memcpy(iou_sum, h.data() + 8 * 8 * (size_t)K, 8 * 2 * (size_t)K);
  if (images && img_count) memcpy(img_count, h.data() + 8 * n8, 4 * 4 * ni);
  if (images && img_first) memcpy(img_first, h.data() + 8 * n8 + 4 * 4 * ni, 4 * 3 * ni);
  return 0;
}

// the neighbour rows of the pruning step: host hashes in, four passes with a launch boundary between them (max, count, scan,
// fill), CSR rows out; its own allocations, the index array only once the total is known.  A grid of about kPruneBlocks blocks:
// the columns are cut into as many spans as that takes, which decides who counts a hit and nothing about the result.
static const int kPruneBlocks = 1024;
extern "C" int uda_hash_neighbors_np(int32_t device, const uint64_t* hashes, int32_t N, int32_t W, double prune_thr,
                                     int32_t max_distance, int64_t cap, int32_t* max_dist, int64_t* row_off, int32_t* idx,
                                     int64_t* total) {
  const char* who = "uda_hash_neighbors_np";
  if (N < 1 || N > UDA_PRUNE_MAX_N) return fail(nullptr, "%s: %d hashes, 1..%d are taken", who, N, (int)UDA_PRUNE_MAX_N);
  if (W < 1 || W > PRUNE_MAX_W) return fail(nullptr, "%s: %d words per hash, 1..%d are taken", who, W, (int)PRUNE_MAX_W);
  if (!hashes || !max_dist || !row_off || !total) return fail(nullptr, "%s: NULL input", who);
  if (cap < 0) return fail(nullptr, "%s: cap %lld is negative", who, (long long)cap);
  if (max_distance < 0 && !(prune_thr >= 0.0 && prune_thr <= 1.79769313486231570e308))
    return fail(nullptr, "%s: prune_thr %g is negative or not finite", who, prune_thr);
  PruneArgs a{};
  a.N = N; a.W = W;
  a.n_chunks = (N + PRUNE_COLS - 1) / PRUNE_COLS;
  const int row_blocks = (N + PRUNE_ROWS - 1) / PRUNE_ROWS;
  const int want_spans = std::min(a.n_chunks, std::max(1, (kPruneBlocks + row_blocks - 1) / row_blocks));
  a.chunks_per_span = (a.n_chunks + want_spans - 1) / want_spans;
  a.spans = (a.n_chunks + a.chunks_per_span - 1) / a.chunks_per_span;      // no empty span
  a.n_slots = (int64_t)N * a.spans;
  a.n_tiles = (int)((a.n_slots + PRUNE_SCAN_TILE - 1) / PRUNE_SCAN_TILE);
  if (a.n_tiles > PRUNE_SCAN_MAX_TILES) return fail(nullptr, "%s: %d scan tiles, at most %d (internal)", who, a.n_tiles, (int)PRUNE_SCAN_MAX_TILES);
  DevScratch s(device);
  a.hashes = s.upload(hashes, (size_t)N * W);
  a.max_dist = s.alloc<int32_t>(1);
  a.counts = s.alloc<int32_t>((size_t)a.n_slots);
  a.tile_sums = s.alloc<int64_t>((size_t)a.n_tiles + 1);
  a.cursor = s.alloc<int64_t>((size_t)a.n_slots);
  a.row_off = s.alloc<int64_t>((size_t)N + 1);
  s.zero(a.max_dist, sizeof(int32_t));
  if (s.ok()) launch_prune_max(a, nullptr);
  s.sync();
  int32_t md = 0;
  s.download(&md, a.max_dist, sizeof md);
  if (!s.ok()) return hip_failed(nullptr, who, s.err);
  a.limit = max_distance >= 0 ? (double)max_distance : (double)md * prune_thr;
  launch_prune_count(a, nullptr);
  launch_prune_scan(a, nullptr);
  s.sync();
  int64_t tot = 0;
  s.download(&tot, a.tile_sums + a.n_tiles, sizeof tot);
  s.download(row_off, a.row_off, ((size_t)N + 1) * sizeof(int64_t));
  if (!s.ok()) return hip_failed(nullptr, who, s.err);
  *max_dist = md;
  *total = tot;
  if (!idx || tot > cap) return 0;
  size_t free_b = 0, all_b = 0;
  s.err = hipMemGetInfo(&free_b, &all_b);
  if (!s.ok()) return hip_failed(nullptr, who, s.err);
  if ((size_t)tot * sizeof(int32_t) > free_b)
    return fail(nullptr, "%s: %lld neighbour entries take %zu bytes of device memory, %zu of %zu are free", who, (long long)tot,
                (size_t)tot * sizeof(int32_t), free_b, all_b);
  a.idx = s.alloc<int32_t>((size_t)tot);
  if (s.ok()) launch_prune_fill(a, nullptr);
  s.sync();
  s.download(idx, a.idx, (size_t)tot * sizeof(int32_t));
  return scratch_done(nullptr, who, s);
}

// the neighbour search of the set-similarity analysis: B ragged problems in, one launch over a table of (problem, row block,
// column span) work items, the squared distances out; its own allocations.  A call with fewer row blocks than kKnnBlocks cuts
// every problem's reference chunks into as many spans as fill that many blocks, as the pruning step does; the spans meet by an
// integer atomicMin, so the cut decides who finds a minimum and nothing about its value.
static const int kKnnBlocks = 1024;
extern "C" int uda_nn_dist2_np(int32_t device, int32_t D, int32_t B, const double* queries, const int64_t* q_off, const double* refs,
                               const int64_t* r_off, const uint8_t* self, double* d2) {
  const char* who = "uda_nn_dist2_np";
  if (D < 1 || D > KNN_MAX_D) return fail(nullptr, "%s: %d coordinates, 1..%d are taken", who, D, (int)KNN_MAX_D);
  if (B < 1 || B > UDA_KNN_MAX_B) return fail(nullptr, "%s: %d problems, 1..%d are taken", who, B, (int)UDA_KNN_MAX_B);
  if (!queries || !q_off || !refs || !r_off || !d2) return fail(nullptr, "%s: NULL input", who);
  if (q_off[0] != 0 || r_off[0] != 0) return fail(nullptr, "%s: offsets start at %lld and %lld, not at 0", who, (long long)q_off[0], (long long)r_off[0]);
  int64_t pairs = 0, row_blocks = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t n = q_off[b + 1] - q_off[b], m = r_off[b + 1] - r_off[b];
    if (n < 0 || m < 0) return fail(nullptr, "%s: the offsets of problem %d descend", who, b);
    if (n == 0 || m == 0) return fail(nullptr, "%s: problem %d has an empty set (%lld queries, %lld references)", who, b, (long long)n, (long long)m);
    if (n > UDA_KNN_MAX_N || m > UDA_KNN_MAX_N)
      return fail(nullptr, "%s: problem %d has %lld queries and %lld references, at most %d each", who, b, (long long)n, (long long)m, (int)UDA_KNN_MAX_N);
    pairs += n * m;                                            // at most 2^40 a problem, 2^52 a call
    row_blocks += (n + KNN_ROWS - 1) / KNN_ROWS;
  }
  if (pairs > UDA_KNN_MAX_PAIRS)
    return fail(nullptr, "%s: %lld pairs of points in one call, at most %lld", who, (long long)pairs, (long long)UDA_KNN_MAX_PAIRS);
  const int64_t want_spans = std::max<int64_t>(1, (kKnnBlocks + row_blocks - 1) / row_blocks);
  if (row_blocks > KNN_MAX_ITEMS) return fail(nullptr, "%s: %lld row blocks, at most %d (internal)", who, (long long)row_blocks, (int)KNN_MAX_ITEMS);
  std::vector<KnnItem> items;
  items.reserve((size_t)std::max<int64_t>(row_blocks, 2 * kKnnBlocks));
  for (int b = 0; b < B; ++b) {
    const int n = (int)(q_off[b + 1] - q_off[b]), m = (int)(r_off[b + 1] - r_off[b]);
    const int n_chunks = (m + KNN_COLS - 1) / KNN_COLS;
    const int spans = (int)std::min<int64_t>(n_chunks, want_spans);
    const int per = (n_chunks + spans - 1) / spans;            // chunks per span; no empty span below
    for (int row0 = 0; row0 < n; row0 += KNN_ROWS)
      for (int c0 = 0; c0 < n_chunks; c0 += per) items.push_back(KnnItem{b, row0, c0, std::min(n_chunks, c0 + per)});
  }
  DevScratch s(device);
  KnnArgs a{};
  a.D = D; a.n_items = (int)items.size(); a.total = q_off[B];
  a.queries = s.upload(queries, (size_t)q_off[B] * D); a.refs = s.upload(refs, (size_t)r_off[B] * D);
  a.q_off = s.upload(q_off, (size_t)B + 1); a.r_off = s.upload(r_off, (size_t)B + 1);
  a.self = s.upload(self, (size_t)B);
  a.items = s.upload(items.data(), items.size());
  a.d2_bits = s.alloc<unsigned long long>((size_t)a.total);
  if (s.ok()) launch_knn_min(a, nullptr);
  s.sync();
  s.download(d2, a.d2_bits, (size_t)a.total * sizeof(double));
  return scratch_done(nullptr, who, s);
}

// Gaussian KDE evaluation: B ragged problems in, one launch over a table of (problem, point tile, span of runs) work items, a
// second over the point tiles, the sums out; its own allocations.  A call with fewer point tiles than kKdeBlocks cuts every
// problem's runs into as many spans as fill that many blocks (a 100 x 100 mesh is 40 tiles).  Every run's sum has its own slot in
// the scratch, so the cut decides who sums a run and nothing about the result.
static const int kKdeBlocks = 2048;
extern "C" int uda_kde_eval_np(int32_t device, int32_t D, int32_t B, const double* data, const int64_t* d_off, const double* weight,
                               const double* points, const int64_t* p_off, double* sum) {
  const char* who = "uda_kde_eval_np";
  if (D < 1 || D > KDE_MAX_D) return fail(nullptr, "%s: %d coordinates, 1..%d are taken", who, D, (int)KDE_MAX_D);
  if (B < 1 || B > UDA_KDE_MAX_B) return fail(nullptr, "%s: %d problems, 1..%d are taken", who, B, (int)UDA_KDE_MAX_B);
  if (!data || !d_off || !points || !p_off || !sum) return fail(nullptr, "%s: NULL input", who);
  if (d_off[0] != 0 || p_off[0] != 0) return fail(nullptr, "%s: offsets start at %lld and %lld, not at 0", who, (long long)d_off[0], (long long)p_off[0]);
  int64_t pairs = 0, tiles = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t n = d_off[b + 1] - d_off[b], m = p_off[b + 1] - p_off[b];
    if (n < 0 || m < 0) return fail(nullptr, "%s: the offsets of problem %d descend", who, b);
    if (n == 0) return fail(nullptr, "%s: problem %d has no data row", who, b);
    if (n > UDA_KDE_MAX_N) return fail(nullptr, "%s: problem %d has %lld data rows, at most %d", who, b, (long long)n, (int)UDA_KDE_MAX_N);
    if (m > UDA_KDE_MAX_PAIRS / n || (pairs += n * m) > UDA_KDE_MAX_PAIRS)
      return fail(nullptr, "%s: more than %lld pairs of a point and a data row in one call (reached at problem %d)", who,
                  (long long)UDA_KDE_MAX_PAIRS, b);
    tiles += (m + KDE_POINTS - 1) / KDE_POINTS;
  }
  if (tiles > KDE_MAX_ITEMS) return fail(nullptr, "%s: %lld blocks of points, at most %d (internal)", who, (long long)tiles, (int)KDE_MAX_ITEMS);
  const int64_t want_spans = tiles > 0 ? std::max<int64_t>(1, (kKdeBlocks + tiles - 1) / tiles) : 1;   // no tile: no point anywhere, nothing is launched
  std::vector<KdeItem> items;
  std::vector<KdeTile> tile_tab;
  std::vector<int64_t> s_off((size_t)B + 1, 0);
  items.reserve((size_t)std::max<int64_t>(tiles, 2 * kKdeBlocks));
  tile_tab.reserve((size_t)tiles);
  for (int b = 0; b < B; ++b) {
    const int n = (int)(d_off[b + 1] - d_off[b]), m = (int)(p_off[b + 1] - p_off[b]);   // m < KDE_MAX_ITEMS * KDE_POINTS = 2^30
    const int runs = (n + KDE_RUN - 1) / KDE_RUN;
    const int spans = (int)std::min<int64_t>(runs, want_spans);
    const int per = (runs + spans - 1) / spans;                // runs per span; no empty span below
    s_off[b + 1] = s_off[b] + (int64_t)runs * m;
    for (int point0 = 0; point0 < m; point0 += KDE_POINTS) {
      tile_tab.push_back(KdeTile{b, point0});
      for (int r0 = 0; r0 < runs; r0 += per) items.push_back(KdeItem{b, point0, r0, std::min(runs, r0 + per)});
    }
  }
  DevScratch s(device);
  KdeArgs a{};
  a.D = D; a.n_items = (int)items.size(); a.n_tiles = (int)tile_tab.size();
  a.data = s.upload(data, (size_t)d_off[B] * D); a.weight = s.upload(weight, (size_t)d_off[B]);
  a.points = s.upload(points, (size_t)p_off[B] * D);
  a.d_off = s.upload(d_off, (size_t)B + 1); a.p_off = s.upload(p_off, (size_t)B + 1); a.s_off = s.upload(s_off.data(), s_off.size());
  a.items = s.upload(items.data(), items.size()); a.tiles = s.upload(tile_tab.data(), tile_tab.size());
  a.run_sums = s.alloc<double>((size_t)s_off[B]);
  a.sum = s.alloc<double>((size_t)p_off[B]);
  if (s.ok()) launch_kde_eval(a, nullptr);
  s.sync();
  s.download(sum, a.sum, (size_t)p_off[B] * sizeof(double));
  return scratch_done(nullptr, who, s);
}

// the pseudo-label audit: B ragged images in, one block each, the results in ONE device allocation, each array the caller asked
// for copied out of it; its own allocations
extern "C" int uda_pseudo_audit_np(int32_t device, int32_t B, const double* gt_boxes, const int64_t* gt_off, const double* det_boxes,
                                   const int64_t* det_off, double gt_iou_thr, double* gt_max_iou, int32_t* gt_best_det,
                                   int32_t* gt_alloc_det, uint8_t* gt_flags, double* det_max_iou, int32_t* det_best_gt,
                                   int32_t* det_alloc_gt, double* det_alloc_miou, double* det_alloc_pair_iou, uint8_t* det_flags,
                                   int32_t* n_matches) {
  const char* who = "uda_pseudo_audit_np";
  if (B < 1 || B > UDA_AUDIT_MAX_B) return fail(nullptr, "%s: %d images, 1..%d are taken", who, B, (int)UDA_AUDIT_MAX_B);
  if (!gt_off || !det_off) return fail(nullptr, "%s: NULL offsets", who);
  if (!(gt_iou_thr - gt_iou_thr == 0.0)) return fail(nullptr, "%s: gt_iou_thr %g is not finite", who, gt_iou_thr);
  if (gt_off[0] != 0 || det_off[0] != 0)
    return fail(nullptr, "%s: offsets start at %lld and %lld, not at 0", who, (long long)gt_off[0], (long long)det_off[0]);
  int64_t max_g = 0, max_d = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t g = gt_off[b + 1] - gt_off[b], d = det_off[b + 1] - det_off[b];
    if (g < 0 || d < 0) return fail(nullptr, "%s: the offsets of image %d do not ascend", who, b);
    if (g > UDA_AUDIT_MAX_G || d > UDA_AUDIT_MAX_D)
      return fail(nullptr, "%s: image %d has %lld ground-truth rows and %lld pseudo labels, at most %d and %d", who, b, (long long)g,
                  (long long)d, (int)UDA_AUDIT_MAX_G, (int)UDA_AUDIT_MAX_D);
    max_g = std::max(max_g, g); max_d = std::max(max_d, d);
  }
  const size_t NG = (size_t)gt_off[B], ND = (size_t)det_off[B];
  if ((NG && !gt_boxes) || (ND && !det_boxes)) return fail(nullptr, "%s: NULL boxes", who);
  DevScratch s(device);
  AuditArgs a{};
  a.B = B; a.max_g = (int)max_g; a.max_d = (int)max_d; a.gt_iou_thr = gt_iou_thr;
  a.gt_boxes = s.upload(gt_boxes, NG * 4); a.det_boxes = s.upload(det_boxes, ND * 4);
  a.gt_off = s.upload(gt_off, (size_t)B + 1); a.det_off = s.upload(det_off, (size_t)B + 1);
  AuditPack pack(nullptr, NG, ND, (size_t)B);
  pack.base = s.alloc<char>(pack.bytes());
  if (int rc = scratch_done(nullptr, who, s)) return rc;
  pack.fill(a);
  launch_pseudo_audit(a, nullptr);
  s.sync();
  // every array the caller asked for, straight from its place in the pack (no staging copy on the host)
  s.download(gt_max_iou, a.gt_max_iou, gt_max_iou ? NG * sizeof(double) : 0);
  s.download(gt_best_det, a.gt_best_det, gt_best_det ? NG * sizeof(int32_t) : 0);
  s.download(gt_alloc_det, a.gt_alloc_det, gt_alloc_det ? NG * sizeof(int32_t) : 0);
  s.download(gt_flags, a.gt_flags, gt_flags ? NG : 0);
  s.download(det_max_iou, a.det_max_iou, det_max_iou ? ND * sizeof(double) : 0);
  s.download(det_best_gt, a.det_best_gt, det_best_gt ? ND * sizeof(int32_t) : 0);
  s.download(det_alloc_gt, a.det_alloc_gt, det_alloc_gt ? ND * sizeof(int32_t) : 0);
  s.download(det_alloc_miou, a.det_alloc_miou, det_alloc_miou ? ND * sizeof(double) : 0);
  s.download(det_alloc_pair_iou, a.det_alloc_pair_iou, det_alloc_pair_iou ? ND * sizeof(double) : 0);
  s.download(det_flags, a.det_flags, det_flags ? ND : 0);
  s.download(n_matches, a.n_matches, n_matches ? (size_t)B * sizeof(int32_t) : 0);
  return scratch_done(nullptr, who, s);
}

// the validation uncertainty report: B ragged segments x K sigma columns in, two launches (run x column blocks, then the fold of
// the run roots), the results in ONE zeroed device allocation; its own allocations
extern "C" int uda_uncert_report_np(int32_t device, int32_t B, int32_t K, int32_t L, const int64_t* off, const double* gt,
                                    const double* pred, const double* gt_class, const double* cls, const double* sigma,
                                    const double* z, int64_t* seg_counts, int64_t* col_counts, int64_t* ece_count, double* seg_sums,
                                    double* col_sums) {
  const char* who = "uda_uncert_report_np";
  if (B < 1 || B > UDA_REPORT_MAX_B) return fail(nullptr, "%s: %d segments, 1..%d are taken", who, B, (int)UDA_REPORT_MAX_B);
  if (K < 1 || K > UDA_REPORT_MAX_K) return fail(nullptr, "%s: %d sigma columns, 1..%d are taken", who, K, (int)UDA_REPORT_MAX_K);
  if (L < 1 || L > UDA_REPORT_MAX_L) return fail(nullptr, "%s: %d levels, 1..%d are taken", who, L, (int)UDA_REPORT_MAX_L);
  if (!off || !z) return fail(nullptr, "%s: NULL offsets or levels", who);
  if (off[0] != 0) return fail(nullptr, "%s: offsets start at %lld, not at 0", who, (long long)off[0]);
  for (int b = 0; b < B; ++b) {
    if (off[b + 1] < off[b]) return fail(nullptr, "%s: the offsets of segment %d do not ascend", who, b);
    if (off[b + 1] > UDA_REPORT_MAX_ROWS)
      return fail(nullptr, "%s: %lld rows up to segment %d, at most %d a call", who, (long long)off[b + 1], b, (int)UDA_REPORT_MAX_ROWS);
  }
  const size_t rows = (size_t)off[B];
  if (rows && (!gt || !pred || !gt_class || !cls || !sigma)) return fail(nullptr, "%s: NULL input array", who);
  // the runs of every segment and where their roots go: a segment holds a power of two of slots, an empty one none
  std::vector<int64_t> pbase((size_t)B + 1, 0);
  std::vector<ReportItem> items;
  items.reserve(rows / REPORT_ROWS + (size_t)B);
  for (int b = 0; b < B; ++b) {
    const int64_t n = off[b + 1] - off[b], runs = (n + REPORT_ROWS - 1) / REPORT_ROWS;
    for (int64_t r = 0; r < runs; ++r) items.push_back(ReportItem{b, (int32_t)(r * REPORT_ROWS), (int32_t)(pbase[b] + r)});
    pbase[b + 1] = pbase[b] + tree_slots(runs);
  }
  const size_t n_sums = REPORT_SEG_SUMS + (size_t)REPORT_COL_SUMS * K;
  const size_t n_seg = (size_t)B * 4, n_col = (size_t)B * K * 3, n_ece = (size_t)B * K * 4 * L, n_ssum = (size_t)B * REPORT_SEG_SUMS,
               n_csum = (size_t)B * K * REPORT_COL_SUMS;
  DevScratch s(device);
  ReportArgs a{};
  a.B = B; a.K = K; a.L = L; a.n_items = (int)items.size(); a.rows = (int64_t)rows; a.slots = pbase[B];
  a.gt = s.upload(gt, rows * 4); a.pred = s.upload(pred, rows * 4);
  a.gt_class = s.upload(gt_class, rows); a.cls = s.upload(cls, rows);
  a.sigma = s.upload(sigma, rows * 4 * K); a.z = s.upload(z, (size_t)L);
  a.off = s.upload(off, (size_t)B + 1); a.pbase = s.upload(pbase.data(), pbase.size());
  a.items = s.upload(items.data(), items.size());
  // int64 seg_counts | col_counts | ece_count, then float64 seg_sums | col_sums: zeroed, so that an empty segment reads zeros
  unsigned long long* pack = s.alloc<unsigned long long>(n_seg + n_col + n_ece + n_ssum + n_csum);
  a.partials = s.alloc<double>(n_sums * (size_t)a.slots);
  if (int rc = scratch_done(nullptr, who, s)) return rc;
  s.zero(pack, (n_seg + n_col + n_ece + n_ssum + n_csum) * sizeof(double));
  s.zero(a.partials, std::max<size_t>(n_sums * (size_t)a.slots, 1) * sizeof(double));
  a.seg_counts = pack; a.col_counts = pack + n_seg; a.ece_count = a.col_counts + n_col;
  a.seg_sums = (double*)(a.ece_count + n_ece); a.col_sums = a.seg_sums + n_ssum;
  if (s.ok()) launch_uncert_report(a, nullptr);
  s.sync();
  std::vector<int64_t> h_seg(seg_counts ? n_seg : 0);
  s.download(h_seg.data(), a.seg_counts, h_seg.size() * sizeof(int64_t));
  s.download(col_counts, a.col_counts, col_counts ? n_col * sizeof(int64_t) : 0);
  s.download(ece_count, a.ece_count, ece_count ? n_ece * sizeof(int64_t) : 0);
  s.download(seg_sums, a.seg_sums, seg_sums ? n_ssum * sizeof(double) : 0);
  s.download(col_sums, a.col_sums, col_sums ? n_csum * sizeof(double) : 0);
  if (int rc = scratch_done(nullptr, who, s)) return rc;
  for (int b = 0; seg_counts && b < B; ++b) {                  // n_rows is the host's: the offsets say it
    h_seg[(size_t)b * 4] = off[b + 1] - off[b];
    memcpy(seg_counts + (size_t)b * 4, h_seg.data() + (size_t)b * 4, 4 * sizeof(int64_t));
  }
  return 0;
}

// the classification calibration report: B ragged segments x M probability tables in, two launches (run x table blocks that walk
// the C + 1 targets, then the fold of the run roots of the segments of more than one run), the results in ONE zeroed device
// allocation; its own allocations
extern "C" int uda_class_report_np(int32_t device, int32_t B, int32_t M, int32_t C, int32_t G, int32_t E, const int64_t* off,
                                   const double* prob, const int32_t* label, const double* edges, const int32_t* n_edges,
                                   int64_t* bin_count, int64_t* bin_hits, double* bin_sum, double* brier_sum, double* nll_sum,
                                   int64_t* tab_counts) {
  const char* who = "uda_class_report_np";
  if (B < 1 || B > UDA_CLASSREP_MAX_B) return fail(nullptr, "%s: %d segments, 1..%d are taken", who, B, (int)UDA_CLASSREP_MAX_B);
  if (M < 1 || M > UDA_CLASSREP_MAX_M) return fail(nullptr, "%s: %d probability tables, 1..%d are taken", who, M, (int)UDA_CLASSREP_MAX_M);
  if (C < 1 || C > UDA_CLASSREP_MAX_C) return fail(nullptr, "%s: %d classes, 1..%d are taken", who, C, (int)UDA_CLASSREP_MAX_C);
  if (E < 2 || E > UDA_CLASSREP_MAX_E) return fail(nullptr, "%s: %d edges a row, 2..%d are taken", who, E, (int)UDA_CLASSREP_MAX_E);
  const int64_t G_each = (int64_t)B * M * (C + 1);
  if (G != 1 && G != G_each)
    return fail(nullptr, "%s: %d edge rows, 1 (shared) or B * M * (C + 1) = %lld (one a target) are taken", who, G, (long long)G_each);
  if (!off || !edges || !n_edges) return fail(nullptr, "%s: NULL offsets or edges", who);
  if (off[0] != 0) return fail(nullptr, "%s: offsets start at %lld, not at 0", who, (long long)off[0]);
  for (int b = 0; b < B; ++b) {
    if (off[b + 1] < off[b]) return fail(nullptr, "%s: the offsets of segment %d do not ascend", who, b);
    if (off[b + 1] > UDA_CLASSREP_MAX_ROWS)
      return fail(nullptr, "%s: %lld rows up to segment %d, at most %d a call", who, (long long)off[b + 1], b, (int)UDA_CLASSREP_MAX_ROWS);
  }
  for (int g = 0; g < G; ++g) {
    const double* e = edges + (size_t)g * E;
    if (n_edges[g] < 2 || n_edges[g] > E) return fail(nullptr, "%s: edge row %d holds %d edges, 2..%d are taken", who, g, n_edges[g], E);
    for (int i = 0; i + 1 < n_edges[g]; ++i)                    // (a NaN fails the comparison too)
      if (!(e[i] < e[i + 1])) return fail(nullptr, "%s: the edges of row %d do not ascend strictly at %d (or hold a NaN)", who, g, i);
  }
  const size_t rows = (size_t)off[B];
  if (rows && (!prob || !label)) return fail(nullptr, "%s: NULL input array", who);
  for (size_t i = 0; i < rows; ++i)
    if (label[i] < 0 || label[i] >= C) return fail(nullptr, "%s: the label of row %lld is %d, outside 0..%d", who, (long long)i, label[i], C - 1);
  // the runs of every segment and where their roots go: a segment of more than one run holds a power of two of slots
  std::vector<int64_t> pbase((size_t)B + 1, 0);
  std::vector<int32_t> tree_segs;
  std::vector<ClassRepItem> items;
  items.reserve(rows / CLASSREP_ROWS + (size_t)B);
  for (int b = 0; b < B; ++b) {
    const int64_t n = off[b + 1] - off[b], runs = (n + CLASSREP_ROWS - 1) / CLASSREP_ROWS;
    for (int64_t r = 0; r < runs; ++r)
      items.push_back(ClassRepItem{b, (int32_t)(r * CLASSREP_ROWS), runs > 1 ? (int32_t)(pbase[b] + r) : -1});
    if (runs > 1) tree_segs.push_back(b);
    pbase[b + 1] = pbase[b] + (runs > 1 ? tree_slots(runs) : 0);
  }
  const size_t S = (size_t)(C + 1) * (E + 1) + C + 1;
  const size_t n_bin = (size_t)B * M * (C + 1) * (E + 1), n_tab = (size_t)B * M * 2, n_bri = (size_t)B * M * C, n_nll = (size_t)B * M;
  DevScratch s(device);
  ClassRepArgs a{};
  a.B = B; a.M = M; a.C = C; a.G = G; a.E = E; a.n_items = (int)items.size(); a.n_tree = (int)tree_segs.size();
  a.rows = (int64_t)rows; a.slots = pbase[B];
  a.prob = s.upload(prob, rows * (size_t)C * M); a.label = s.upload(label, rows);
  a.edges = s.upload(edges, (size_t)G * E); a.n_edges = s.upload(n_edges, (size_t)G);
  a.off = s.upload(off, (size_t)B + 1); a.pbase = s.upload(pbase.data(), pbase.size());
  a.tree_segs = s.upload(tree_segs.data(), tree_segs.size()); a.items = s.upload(items.data(), items.size());
  // int64 bin_count | bin_hits | tab_counts, then float64 bin_sum | brier_sum | nll_sum: zeroed, so that an empty segment and a bin
  // slot past a row's edges read zeros
  const size_t n_pack = 3 * n_bin + n_tab + n_bri + n_nll;
  unsigned long long* pack = s.alloc<unsigned long long>(n_pack);
  a.partials = s.alloc<double>(M * S * (size_t)a.slots);
  if (int rc = scratch_done(nullptr, who, s)) return rc;
  s.zero(pack, n_pack * sizeof(double));
  s.zero(a.partials, std::max<size_t>(M * S * (size_t)a.slots, 1) * sizeof(double));
  a.bin_count = pack; a.bin_hits = pack + n_bin; a.tab_counts = a.bin_hits + n_bin;
  a.bin_sum = (double*)(a.tab_counts + n_tab); a.brier_sum = a.bin_sum + n_bin; a.nll_sum = a.brier_sum + n_bri;
  if (s.ok()) launch_class_report(a, nullptr);
  s.sync();
  if (int rc = scratch_done(nullptr, who, s)) return rc;
  s.download(bin_count, a.bin_count, bin_count ? n_bin * sizeof(int64_t) : 0);
  s.download(bin_hits, a.bin_hits, bin_hits ? n_bin * sizeof(int64_t) : 0);
  s.download(tab_counts, a.tab_counts, tab_counts ? n_tab * sizeof(int64_t) : 0);
  s.download(bin_sum, a.bin_sum, bin_sum ? n_bin * sizeof(double) : 0);
  s.download(brier_sum, a.brier_sum, brier_sum ? n_bri * sizeof(double) : 0);
  s.download(nll_sum, a.nll_sum, nll_sum ? n_nll * sizeof(double) : 0);
  return scratch_done(nullptr, who, s);
}

// ---- RCC collages: Pillow's resize and paste as jobs on packed RGB planes (kernels_collage.hip)
static int resample_coeffs_entry(const char* who, int32_t in_size, int32_t out_size, int32_t filter, int32_t* ksize, int32_t* bounds,
                                 int32_t* coeffs, int64_t coeffs_cap) {
  if (filter != UDA_FILTER_LANCZOS && filter != UDA_FILTER_BICUBIC)
    return fail(nullptr, "%s: filter %d, UDA_FILTER_LANCZOS (%d) and UDA_FILTER_BICUBIC (%d) are built", who, filter, (int)UDA_FILTER_LANCZOS,
                (int)UDA_FILTER_BICUBIC);
  if (in_size < 1 || in_size > UDA_RESAMPLE_MAX_SIDE || out_size < 1 || out_size > UDA_RESAMPLE_MAX_SIDE)
    return fail(nullptr, "%s: an axis of %d to %d pixels, 1..%d are taken", who, in_size, out_size, (int)UDA_RESAMPLE_MAX_SIDE);
  if (!ksize) return fail(nullptr, "%s: NULL ksize", who);
  *ksize = resample_ksize(in_size, out_size, filter);
  if (!bounds && !coeffs) return 0;
  if (!bounds || !coeffs) return fail(nullptr, "%s: bounds and coeffs go together", who);
  if (coeffs_cap < (int64_t)out_size * *ksize)
    return fail(nullptr, "%s: coeffs holds %lld values, %lld are needed", who, (long long)coeffs_cap, (long long)out_size * *ksize);
  resample_coeffs(in_size, out_size, filter, bounds, coeffs);
  return 0;
}
extern "C" int uda_resample_coeffs_np(int32_t in_size, int32_t out_size, int32_t* ksize, int32_t* bounds, int32_t* coeffs,
                                      int64_t coeffs_cap) {
  return resample_coeffs_entry("uda_resample_coeffs_np", in_size, out_size, UDA_FILTER_LANCZOS, ksize, bounds, coeffs, coeffs_cap);
}
extern "C" int uda_resample_coeffs_filter_np(int32_t in_size, int32_t out_size, int32_t filter, int32_t* ksize, int32_t* bounds,
                                             int32_t* coeffs, int64_t coeffs_cap) {
  return resample_coeffs_entry("uda_resample_coeffs_filter_np", in_size, out_size, filter, ksize, bounds, coeffs, coeffs_cap);
}

namespace {
struct ResamplePlane { int64_t off; int32_t w, h; };
struct ResampleTables {          // one table for each distinct (filter, in, out) of the call, in one int32 pool
  struct Table { int64_t key, off; };                  // key: filter << 56 | in << 32 | out (a side is at most 2^16)
  std::vector<int32_t> pool;
  std::vector<Table> index, fresh;                     // index: sorted by key; fresh: the latest, not yet merged
  std::vector<Table> todo;                             // reserved in the pool, not yet filled
  size_t reserved = 0;
  // where the table of (in, out) under `filter` is (or will be: fill() makes what get() reserved)
  int64_t get(int in, int out, int filter) {
    const int64_t key = ((int64_t)filter << 56) | ((int64_t)in << 32) | (uint32_t)out;
    for (const Table& f : fresh) if (f.key == key) return f.off;
    auto it = std::lower_bound(index.begin(), index.end(), key, [](const Table& t, int64_t k) { return t.key < k; });
    if (it != index.end() && it->key == key) return it->off;
    const Table t{key, (int64_t)reserved};
    reserved += (size_t)out * (2 + (in == out ? 1 : resample_ksize(in, out, filter)));
    todo.push_back(t);
    fresh.push_back(t);
    if (fresh.size() >= 64) {
      index.insert(index.end(), fresh.begin(), fresh.end());
      std::sort(index.begin(), index.end(), [](const Table& a, const Table& b) { return a.key < b.key; });
      fresh.clear();
    }
    return t.off;
  }
  // the tables are independent of each other: a few host threads share them out (thousands of sin calls a table)
  void fill() {
    pool.resize(reserved);
    std::atomic<size_t> next{0};
    auto work = [&]() {
      for (size_t i; (i = next.fetch_add(1)) < todo.size();) {
        const int filter = (int)(todo[i].key >> 56), in = (int)(todo[i].key >> 32) & 0xFFFFFF, out = (int)(uint32_t)todo[i].key;
        int32_t* b = pool.data() + todo[i].off;
        if (in == out) {                               // the identity: a copy is a pass like any other
          for (int k = 0; k < out; ++k) { b[2 * k] = k; b[2 * k + 1] = 1; b[2 * (size_t)out + k] = 1 << RESAMPLE_BITS; }
        } else {
          resample_coeffs(in, out, filter, b, b + 2 * (size_t)out);
        }
      }
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t n_thr = std::min<size_t>({(size_t)(hw ? hw : 1), 8, todo.size() / 16});
    std::vector<std::thread> pool_thr;
    for (size_t t = 0; t < n_thr; ++t) pool_thr.emplace_back(work);
    work();
    for (std::thread& t : pool_thr) t.join();
    todo.clear();
  }
};
}  // namespace

// Image.resize's own rule (PIL/Image.py): a plane more than 100 times as tall as wide that gets shorter is resized along y first,
// then along x - the one case where the vertical result, not the horizontal one, is what gets rounded to uint8 in between.
static bool resample_vertical_first(int src_w, int src_h, int h) { return (int64_t)src_h > (int64_t)src_w * 100 && h < src_h; }

// One pass over `in_size` -> table `out_full`, of which n_out positions and n_lines lines are written; its table is reserved.
static ResamplePass resample_pass(ResampleTables& tabs, int64_t src, int64_t src_stride, int64_t dst, int64_t dst_stride, int in_size,
                                  int out_full, int n_out, int n_lines, int filter = UDA_FILTER_LANCZOS) {
  ResamplePass p{};
  p.src = src; p.dst = dst; p.src_stride = src_stride; p.dst_stride = dst_stride;
  p.coef_off = tabs.get(in_size, out_full, filter);
  p.in_size = in_size; p.out_full = out_full; p.n_out = n_out; p.n_lines = n_lines;
  p.ksize = in_size == out_full ? 1 : resample_ksize(in_size, out_full, filter);
  return p;
}
// The tiles of a pass, once the tables are filled.  tw: the largest power of two <= RESAMPLE_TW whose every tile's span (last xmin
// - first xmin + a chunk) fits RESAMPLE_SPAN_PER_POS * tw pixels, and no wider than the output needs.  A tile of one position
// always fits.
static void resample_tiles(ResamplePass& p, const ResampleTables& tabs, bool vertical, int* n_tiles) {
  const int32_t* bounds = tabs.pool.data() + p.coef_off;
  int tw = vertical ? 8 : RESAMPLE_TW;                 // along y a tile is wide rather than tall: its rows are runs of 3 * 256 / tw bytes
  while (tw > 1 && tw / 2 >= p.n_out) tw /= 2;
  for (; tw > 1; tw /= 2) {
    bool fits = true;
    for (int o0 = 0; o0 < p.n_out && fits; o0 += tw)
      fits = bounds[2 * (std::min(o0 + tw, p.n_out) - 1)] - bounds[2 * o0] + RESAMPLE_KCH <= RESAMPLE_SPAN_PER_POS * tw;
    if (fits) break;
  }
  p.tw = tw;
  p.tiles_pos = (p.n_out + tw - 1) / tw;
  const int lines = RESAMPLE_THREADS / tw;
  p.tile0 = *n_tiles;
  *n_tiles += p.tiles_pos * ((p.n_lines + lines - 1) / lines);
}

extern "C" int uda_gauss_box_np(double radius, float* fr, uint32_t* ww, uint32_t* fw) {
  const char* who = "uda_gauss_box_np";
  if (!fr || !ww || !fw) return fail(nullptr, "%s: NULL output", who);
  if (!std::isfinite(radius) || radius < 0) return fail(nullptr, "%s: a radius of %g, finite and >= 0 is taken", who, radius);
  gauss_box(radius, fr, ww, fw);
  return 0;
}

// Both collage entry points: a job row has JS = 7 values (uda_resample_np: every job is a resize) or 9 (uda_collage_np: op, arg).
static int collage_run(const char* who, int JS, int32_t device, int32_t S, const int32_t* src_wh, const uint8_t* src_pix, int32_t T,
                       const int32_t* tmp_wh, int32_t N, int32_t H, int32_t W, int32_t K, const int32_t* jobs, int32_t n_params,
                       const double* params, int64_t noise_bytes, const uint8_t* noise, uint8_t* out) {
  const int MAXS = UDA_RESAMPLE_MAX_SIDE;
  auto op_of = [&](int k) { return JS == 9 ? jobs[JS * (size_t)k + 7] : 0; };
  if (n_params < 0 || noise_bytes < 0 || (n_params && !params) || (noise_bytes && !noise))
    return fail(nullptr, "%s: %d parameters, %lld noise bytes, or a NULL array of them", who, n_params, (long long)noise_bytes);
  if (S < 0 || T < 0 || K < 0 || N < 1) return fail(nullptr, "%s: %d source planes, %d temporaries, %d output planes, %d jobs", who, S, T, N, K);
  if (H < 1 || H > MAXS || W < 1 || W > MAXS) return fail(nullptr, "%s: output planes of %d x %d, sides of 1..%d are taken", who, W, H, MAXS);
  if (!out || (S && (!src_wh || !src_pix)) || (T && !tmp_wh) || (K && !jobs)) return fail(nullptr, "%s: NULL array", who);
  const int P = S + T + N;
  std::vector<ResamplePlane> pl((size_t)P);
  int64_t bytes = 0;
  for (int i = 0; i < S + T; ++i) {
    const int32_t* wh = i < S ? src_wh + 2 * (size_t)i : tmp_wh + 2 * (size_t)(i - S);
    if (wh[0] < 1 || wh[1] < 1 || wh[0] > MAXS || wh[1] > MAXS)
      return fail(nullptr, "%s: plane %d is %d x %d, an empty plane or a side above %d is not taken", who, i, wh[0], wh[1], MAXS);
    pl[i] = ResamplePlane{bytes, wh[0], wh[1]};
    bytes += (int64_t)wh[0] * wh[1] * 3;
  }
  const int64_t src_bytes = S ? pl[S - 1].off + (int64_t)pl[S - 1].w * pl[S - 1].h * 3 : 0;
  int64_t scratch = bytes - src_bytes;
  const int64_t out_off = bytes, out_bytes = (int64_t)N * H * W * 3;
  for (int i = 0; i < N; ++i) pl[S + T + i] = ResamplePlane{out_off + (int64_t)i * H * W * 3, W, H};
  bytes += out_bytes;
  // the jobs: ids, sizes, levels; per level no read of a plane the level writes, no pixel written twice
  std::vector<int> wrote((size_t)P, -1);
  std::vector<int> order;
  int64_t noise_need = 0;
  for (int k0 = 0; k0 < K;) {
    int k1 = k0;
    const int level = jobs[JS * (size_t)k0];
    if (k0 && level < jobs[JS * (size_t)(k0 - 1)]) return fail(nullptr, "%s: the level of job %d is %d after %d: levels ascend", who, k0, level, jobs[JS * (size_t)(k0 - 1)]);
    for (; k1 < K && jobs[JS * (size_t)k1] == level; ++k1) {
      const int32_t* j = jobs + JS * (size_t)k1;
      if (j[1] < 0 || j[1] >= P) return fail(nullptr, "%s: job %d reads plane %d, there are %d", who, k1, j[1], P);
      if (j[2] < S || j[2] >= P) return fail(nullptr, "%s: job %d writes plane %d, the planes %d..%d can be written", who, k1, j[2], S, P - 1);
      if (j[5] < 1 || j[6] < 1 || j[5] > MAXS || j[6] > MAXS) return fail(nullptr, "%s: job %d resizes to %d x %d, sides of 1..%d are taken", who, k1, j[5], j[6], MAXS);
      const ResamplePlane& d = pl[j[2]];
      if (j[3] < 0 || j[4] < 0 || j[3] >= d.w || j[4] >= d.h)
        return fail(nullptr, "%s: job %d pastes at (%d, %d), outside its destination of %d x %d", who, k1, j[3], j[4], d.w, d.h);
      wrote[j[2]] = k0;
      const ResamplePlane& f = pl[j[1]];
      const int op = op_of(k1);
      if (op < 0 || op > 5) return fail(nullptr, "%s: job %d has op %d, 0..5 are known", who, k1, op);
      if (op && (j[5] != f.w || j[6] != f.h))
        return fail(nullptr, "%s: job %d (op %d) writes %d x %d from a plane of %d x %d: an augmentation keeps the size", who, k1, op, j[5], j[6], f.w, f.h);
      if (op >= 2 && op <= 4) {
        if (j[8] < 0 || j[8] >= n_params) return fail(nullptr, "%s: job %d (op %d) has arg %d, there are %d parameters", who, k1, op, j[8], n_params);
        const double v = params[j[8]];
        if (!std::isfinite(v) || v < 0) return fail(nullptr, "%s: job %d (op %d) has the parameter %g, finite and >= 0 is taken", who, k1, op, v);
        if (op == 4 && v > UDA_BLUR_MAX_RADIUS)
          return fail(nullptr, "%s: job %d blurs with radius %g, at most %g is taken", who, k1, v, (double)UDA_BLUR_MAX_RADIUS);
        if (op == 4) scratch += (int64_t)std::min(j[5], d.w - j[3]) * f.h * 3;
      }
      if (op == 5) noise_need += (int64_t)j[5] * j[6] * 3;
      if (op == 0 && j[5] != f.w && j[6] != f.h)
        scratch +=resample_vertical_first(f.w, f.h, j[6]) ? (int64_t)f.w * std::min(j[6], d.h - j[4]) * 3 : (int64_t)std::min(j[5], d.w - j[3]) * f.h * 3;
    }
    order.clear();
    for (int k = k0; k < k1; ++k) {
      if (wrote[jobs[JS * (size_t)k + 1]] == k0)
        return fail(nullptr, "%s: job %d reads plane %d, which a job of its own level %d writes", who, k, jobs[JS * (size_t)k + 1], level);
      order.push_back(k);
    }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return jobs[JS * (size_t)a + 2] < jobs[JS * (size_t)b + 2]; });
    for (size_t a = 0; a < order.size(); ++a)
      for (size_t b = a + 1; b < order.size() && jobs[JS * (size_t)order[b] + 2] == jobs[JS * (size_t)order[a] + 2]; ++b) {
        const int32_t *ja = jobs + JS * (size_t)order[a], *jb = jobs + JS * (size_t)order[b];
        if (ja[3] < jb[3] + jb[5] && jb[3] < ja[3] + ja[5] && ja[4] < jb[4] + jb[6] && jb[4] < ja[4] + ja[6])
          return fail(nullptr, "%s: jobs %d and %d of level %d write the same pixels of plane %d", who, std::min(order[a], order[b]),
                      std::max(order[a], order[b]), level, ja[2]);
      }
    k0 = k1;
  }
  if (scratch > UDA_RESAMPLE_MAX_SCRATCH)
    return fail(nullptr, "%s: %lld bytes of scratch, at most %lld a call", who, (long long)scratch, (long long)UDA_RESAMPLE_MAX_SCRATCH);
  if (noise_need != noise_bytes)
    return fail(nullptr, "%s: %lld noise bytes, the op-5 jobs take %lld", who, (long long)noise_bytes, (long long)noise_need);
  // the passes, level by level: the horizontal ones of a level, then its vertical ones; then the level's augmentations - the
  // contrast means, the pointwise jobs (which read the means), the blurs' x stages and their y stages
  ResampleTables tabs;
  std::vector<ResamplePass> passes;
  std::vector<AugMeanJob> means;
  std::vector<AugJob> points;
  std::vector<BlurPass> blurs;
  enum { L_RESAMPLE, L_MEAN, L_POINT, L_BLUR };
  struct Launch { int first, count, tiles; bool vertical; int what = L_RESAMPLE; };
  std::vector<Launch> launches;
  int64_t noise_at = 0;
  int n_means = 0;
  for (int k0 = 0; k0 < K;) {
    int k1 = k0;
    while (k1 < K && jobs[JS * (size_t)k1] == jobs[JS * (size_t)k0]) ++k1;
    std::vector<ResamplePass> vert, late;
    std::vector<AugMeanJob> lvl_means;
    std::vector<AugJob> lvl_points;
    std::vector<BlurPass> blur_x, blur_y;
    const int first = (int)passes.size();
    for (int k = k0; k < k1; ++k) {
      const int32_t* j = jobs + JS * (size_t)k;
      const ResamplePlane &s = pl[j[1]], &d = pl[j[2]];
      const int w = j[5], h = j[6], cw = std::min(w, d.w - j[3]), ch = std::min(h, d.h - j[4]);
      const int64_t to = d.off + ((int64_t)j[4] * d.w + j[3]) * 3;
      if (const int op = op_of(k)) {
        float fr = 0.0f;
        uint32_t ww = 0, fw = 0;
        if (op == 4) gauss_box(params[j[8]], &fr, &ww, &fw);
        if (op == 4 && fr != 0.0f) {                    // the x stage's result, cw x h, in scratch; the y stage reads it
          if ((int)fr > UDA_BLUR_MAX_BOX) return fail(nullptr, "%s: job %d blurs with a box of %d, at most %d fit a tile", who, k, (int)fr, (int)UDA_BLUR_MAX_BOX);
          BlurPass bx{s.off, bytes, (int64_t)s.w * 3, (int64_t)cw * 3, ww, fw, (int)fr, s.w, cw, s.h, 0, 0};
          BlurPass by{bytes, to, (int64_t)cw * 3, (int64_t)d.w * 3, ww, fw, (int)fr, s.h, ch, cw, 0, 0};
          blur_x.push_back(bx);
          blur_y.push_back(by);
          bytes += (int64_t)cw * s.h * 3;
          continue;
        }
        AugJob a{};
        a.src = s.off; a.dst = to; a.src_stride = (int64_t)s.w * 3; a.dst_stride = (int64_t)d.w * 3;
        a.n_pix = (int64_t)s.w * s.h; a.w = s.w; a.cw = cw; a.ch = ch; a.mean = -1;
        a.kind = op == 1 ? AUG_FLIP : op == 5 ? AUG_ADD : AUG_COPY;
        if (op == 2 || op == 3) {
          a.a = (float)params[j[8]];
          a.kind = a.a >= 0.0f && a.a <= 1.0f ? AUG_BLEND : AUG_BLEND_CLIP;
        }
        if (op == 3) {
          a.mean = n_means++;
          lvl_means.push_back(AugMeanJob{s.off, a.n_pix, a.mean, 0});
        }
        if (op == 5) { a.noise = noise_at; noise_at += (int64_t)w * h * 3; }
        lvl_points.push_back(a);
        continue;
      }
      if (w != s.w && h != s.h && resample_vertical_first(s.w, s.h, h)) {   // the vertical result, s.w x ch, in scratch; x after it
        vert.push_back(resample_pass(tabs, s.off, (int64_t)s.w * 3, bytes, (int64_t)s.w * 3, s.h, h, ch, s.w));
        late.push_back(resample_pass(tabs, bytes, (int64_t)s.w * 3, to, (int64_t)d.w * 3, s.w, w, cw, ch));
        bytes += (int64_t)s.w * ch * 3;
      } else if (w != s.w && h != s.h) {                // both: the horizontal result, cw x s.h, rounded to uint8 in scratch
        passes.push_back(resample_pass(tabs, s.off, (int64_t)s.w * 3, bytes, (int64_t)cw * 3, s.w, w, cw, s.h));
        vert.push_back(resample_pass(tabs, bytes, (int64_t)cw * 3, to, (int64_t)d.w * 3, s.h, h, ch, cw));
        bytes += (int64_t)cw * s.h * 3;
      } else if (h != s.h) {
        vert.push_back(resample_pass(tabs, s.off, (int64_t)s.w * 3, to, (int64_t)d.w * 3, s.h, h, ch, cw));
      } else {                                          // along x only, or the copy (the identity table)
        passes.push_back(resample_pass(tabs, s.off, (int64_t)s.w * 3, to, (int64_t)d.w * 3, s.w, w, cw, ch));
      }
    }
    if ((int)passes.size() > first) launches.push_back(Launch{first, (int)passes.size() - first, 0, false});
    if (!vert.empty()) launches.push_back(Launch{(int)passes.size(), (int)vert.size(), 0, true});
    passes.insert(passes.end(), vert.begin(), vert.end());
    if (!late.empty()) launches.push_back(Launch{(int)passes.size(), (int)late.size(), 0, false});
    passes.insert(passes.end(), late.begin(), late.end());
    if (!lvl_means.empty()) {
      Launch l{(int)means.size(), (int)lvl_means.size(), 0, false, L_MEAN};
      for (AugMeanJob& m : lvl_means) {
        m.tile0 = l.tiles;
        l.tiles += (int)((m.n_pix + AUG_MEAN_PIX - 1) / AUG_MEAN_PIX);
      }
      means.insert(means.end(), lvl_means.begin(), lvl_means.end());
      launches.push_back(l);
    }
    if (!lvl_points.empty()) {
      Launch l{(int)points.size(), (int)lvl_points.size(), 0, false, L_POINT};
      for (AugJob& a : lvl_points) {
        a.tile0 = l.tiles;
        a.tiles_x = (a.cw + AUG_TILE - 1) / AUG_TILE;
        l.tiles += a.tiles_x * ((a.ch + AUG_ROWS - 1) / AUG_ROWS);
      }
      points.insert(points.end(), lvl_points.begin(), lvl_points.end());
      launches.push_back(l);
    }
    for (int vertical = 0; vertical < 2; ++vertical) {
      std::vector<BlurPass>& stage = vertical ? blur_y : blur_x;
      if (stage.empty()) continue;
      Launch l{(int)blurs.size(), (int)stage.size(), 0, vertical != 0, L_BLUR};
      for (BlurPass& b : stage) {
        b.tile0 = l.tiles;
        b.tiles_pos = (b.n_out + AUG_TILE - 1) / AUG_TILE;
        l.tiles += b.tiles_pos * ((b.n_lines + BLUR_LINES - 1) / BLUR_LINES);
      }
      blurs.insert(blurs.end(), stage.begin(), stage.end());
      launches.push_back(l);
    }
    k0 = k1;
  }
  tabs.fill();
  for (Launch& l : launches)
    if (l.what == L_RESAMPLE)
      for (int i = 0; i < l.count; ++i) resample_tiles(passes[l.first + i], tabs, l.vertical, &l.tiles);
  DevScratch s(device);
  hipStream_t st = s.stream();
  uint8_t* base = s.alloc<uint8_t>((size_t)bytes);
  const ResamplePass* d_pass = s.upload(passes.data(), passes.size(), st);
  const int32_t* d_pool = s.upload(tabs.pool.data(), tabs.pool.size(), st);
  const AugMeanJob* d_means = s.upload(means.data(), means.size(), st);
  const AugJob* d_points = s.upload(points.data(), points.size(), st);
  const BlurPass* d_blurs = s.upload(blurs.data(), blurs.size(), st);
  const uint8_t* d_noise = noise_bytes ? s.upload(noise, (size_t)noise_bytes, st) : nullptr;
  unsigned long long* d_sums = n_means ? s.alloc<unsigned long long>((size_t)n_means) : nullptr;
  if (int rc = scratch_done(nullptr, who, s)) return rc;
  if (src_bytes && s.ok()) s.err = hipMemcpyAsync(base, src_pix, (size_t)src_bytes, hipMemcpyHostToDevice, st);
  s.zero(base + src_bytes, (size_t)(out_off + out_bytes - src_bytes), st);
  if (n_means) s.zero(d_sums, (size_t)n_means * sizeof(unsigned long long), st);
  for (const Launch& l : launches) {
    if (!s.ok()) break;
    if (l.what == L_RESAMPLE) launch_resample_passes(d_pass + l.first, l.count, l.tiles, l.vertical, d_pool, base, st);
    else if (l.what == L_MEAN) launch_augment_means(d_means + l.first, l.count, l.tiles, d_sums, base, st);
    else if (l.what == L_POINT) launch_augment_points(d_points + l.first, l.count, l.tiles, d_sums, d_noise, base, st);
    else launch_blur_stages(d_blurs + l.first, l.count, l.tiles, l.vertical, base, st);
  }
  s.sync(st);
  if (int rc = scratch_done(nullptr, who, s)) return rc;
  s.download(out, base + out_off, (size_t)out_bytes);
  return scratch_done(nullptr, who, s);
}

extern "C" int uda_resample_np(int32_t device, int32_t S, const int32_t* src_wh, const uint8_t* src_pix, int32_t T, const int32_t* tmp_wh,
                               int32_t N, int32_t H, int32_t W, int32_t K, const int32_t* jobs, uint8_t* out) {
  return collage_run("uda_resample_np", 7, device, S, src_wh, src_pix, T, tmp_wh, N, H, W, K, jobs, 0, nullptr, 0, nullptr, out);
}

extern "C" int uda_collage_np(int32_t device, int32_t S, const int32_t* src_wh, const uint8_t* src_pix, int32_t T, const int32_t* tmp_wh,
                              int32_t N, int32_t H, int32_t W, int32_t K, const int32_t* jobs, int32_t P, const double* params,
                              int64_t noise_bytes, const uint8_t* noise, uint8_t* out) {
  return collage_run("uda_collage_np", 9, device, S, src_wh, src_pix, T, tmp_wh, N, H, W, K, jobs, P, params, noise_bytes, noise, out);
}

// ---- the pruning step's perceptual hash: the passes of kernels_collage.hip with bicubic tables, then kernels_phash.hip
extern "C" int uda_phash_table_np(double* T) {
  if (!T) return fail(nullptr, "uda_phash_table_np: NULL table");
  phash_dct_table(T);
  return 0;
}

extern "C" int uda_phash_np(int32_t device, int32_t N, const int32_t* wh, const uint8_t* pix, uint64_t* words, double* margin,
                            uint8_t* thumb, double* low) {
  const char* who = "uda_phash_np";
  const int MAXS = UDA_RESAMPLE_MAX_SIDE, PW = UDA_PHASH_PRE_W, PH = UDA_PHASH_PRE_H, F = UDA_FILTER_BICUBIC;
  const int64_t plane = (int64_t)PW * PH * 3;
  if (N < 0) return fail(nullptr, "%s: %d images", who, N);
  if (N == 0) return 0;
  if (!wh || !pix || !words || !margin) return fail(nullptr, "%s: NULL array", who);
  // one device allocation: the N planes of 512 x 256 first (the tail reads them in 16-byte words), the sources, the first passes' results
  const int64_t src_off = (int64_t)N * plane;
  int64_t bytes = src_off, mid_bytes = 0;
  for (int i = 0; i < N && bytes + mid_bytes <= UDA_PHASH_MAX_BYTES; ++i) {
    const int w = wh[2 * (size_t)i], h = wh[2 * (size_t)i + 1];
    if (w < 1 || h < 1 || w > MAXS || h > MAXS)
      return fail(nullptr, "%s: image %d is %d x %d, an empty image or a side above %d is not taken", who, i, w, h, MAXS);
    bytes += (int64_t)w * h * 3;
    if (w != PW && h != PH) mid_bytes += resample_vertical_first(w, h, PH) ? (int64_t)w * PH * 3 : (int64_t)PW * h * 3;
  }
  if (bytes + mid_bytes > UDA_PHASH_MAX_BYTES)
    return fail(nullptr, "%s: %d images take more than %lld bytes on the device (planes of %d x %d, sources, first passes): split the call",
                who, N, (long long)UDA_PHASH_MAX_BYTES, PW, PH);
  const int64_t src_bytes = bytes - src_off;
  PhashTables pt;
  if (resample_ksize(PW, PHASH_SIDE, UDA_FILTER_LANCZOS) != PHASH_KX || resample_ksize(PH, PHASH_SIDE, UDA_FILTER_LANCZOS) != PHASH_KY)
    return fail(nullptr, "%s: the thumbnail's tables do not have %d and %d coefficients a row", who, (int)PHASH_KX, (int)PHASH_KY);
  resample_coeffs(PW, PHASH_SIDE, UDA_FILTER_LANCZOS, pt.bx, pt.kx);
  resample_coeffs(PH, PHASH_SIDE, UDA_FILTER_LANCZOS, pt.by, pt.ky);
  phash_dct_table(pt.T);
  // Image.resize((512, 256)) of every image: along x first, rounded to uint8; a pass whose axis keeps its length is skipped
  ResampleTables tabs;
  std::vector<ResamplePass> passes, vert, late;
  int64_t s = src_off;
  for (int i = 0; i < N; ++i) {
    const int w = wh[2 * (size_t)i], h = wh[2 * (size_t)i + 1];
    const int64_t to = (int64_t)i * plane;
    if (w != PW && h != PH && resample_vertical_first(w, h, PH)) {
      vert.push_back(resample_pass(tabs, s, (int64_t)w * 3, bytes, (int64_t)w * 3, h, PH, PH, w, F));
      late.push_back(resample_pass(tabs, bytes, (int64_t)w * 3, to, (int64_t)PW * 3, w, PW, PW, PH, F));
      bytes += (int64_t)w * PH * 3;
    } else if (w != PW && h != PH) {
      passes.push_back(resample_pass(tabs, s, (int64_t)w * 3, bytes, (int64_t)PW * 3, w, PW, PW, h, F));
      vert.push_back(resample_pass(tabs, bytes, (int64_t)PW * 3, to, (int64_t)PW * 3, h, PH, PH, PW, F));
      bytes += (int64_t)PW * h * 3;
    } else if (h != PH) {
      vert.push_back(resample_pass(tabs, s, (int64_t)w * 3, to, (int64_t)PW * 3, h, PH, PH, PW, F));
    } else {                                            // along x only, or the copy (the identity table)
      passes.push_back(resample_pass(tabs, s, (int64_t)w * 3, to, (int64_t)PW * 3, w, PW, PW, PH, F));
    }
    s += (int64_t)w * h * 3;
  }
  const int n_x = (int)passes.size(), n_y = (int)vert.size(), n_late = (int)late.size();
  passes.insert(passes.end(), vert.begin(), vert.end());
  passes.insert(passes.end(), late.begin(), late.end());
  tabs.fill();
  int tiles_x = 0, tiles_y = 0, tiles_late = 0;
  for (int i = 0; i < n_x; ++i) resample_tiles(passes[i], tabs, false, &tiles_x);
  for (int i = 0; i < n_y; ++i) resample_tiles(passes[n_x + i], tabs, true, &tiles_y);
  for (int i = 0; i < n_late; ++i) resample_tiles(passes[n_x + n_y + i], tabs, false, &tiles_late);
  DevScratch d(device);
  hipStream_t st = d.stream();
  uint8_t* base = d.alloc<uint8_t>((size_t)bytes);
  const ResamplePass* d_pass = d.upload(passes.data(), passes.size(), st);
  const int32_t* d_pool = d.upload(tabs.pool.data(), tabs.pool.size(), st);
  const PhashTables* d_pt = d.upload(&pt, 1, st);
  unsigned long long* d_words = d.alloc<unsigned long long>((size_t)N);
  double* d_margin = d.alloc<double>((size_t)N);
  uint8_t* d_thumb = d.alloc<uint8_t>((size_t)N * PHASH_SIDE * PHASH_SIDE);
  double* d_low = d.alloc<double>((size_t)N * PHASH_LOW * PHASH_LOW);
  if (int rc = scratch_done(nullptr, who, d)) return rc;
  d.err = hipMemcpyAsync(base + src_off, pix, (size_t)src_bytes, hipMemcpyHostToDevice, st);
  if (d.ok()) launch_resample_passes(d_pass, n_x, tiles_x, false, d_pool, base, st);
  if (d.ok()) launch_resample_passes(d_pass + n_x, n_y, tiles_y, true, d_pool, base, st);
  if (d.ok()) launch_resample_passes(d_pass + n_x + n_y, n_late, tiles_late, false, d_pool, base, st);
  if (d.ok()) launch_phash_tail(base, N, d_pt, d_words, d_margin, d_thumb, d_low, st);
  d.sync(st);
  if (int rc = scratch_done(nullptr, who, d)) return rc;
  d.download(words, d_words, (size_t)N * sizeof(uint64_t));
  d.download(margin, d_margin, (size_t)N * sizeof(double));
  d.download(thumb, d_thumb, thumb ? (size_t)N * PHASH_SIDE * PHASH_SIDE : 0);
  d.download(low, d_low, low ? (size_t)N * PHASH_LOW * PHASH_LOW * sizeof(double) : 0);
  return scratch_done(nullptr, who, d);
}

extern "C" int uda_calibrate_box(uda_ctx_t* c, int32_t col0, int32_t mode, int32_t relative, int32_t n_tables,
                                 const int32_t* tab_off, const double* xs, const double* ys, const float* temps, float* out) {
  if (!c || !out) return c ? fail(c, "calibrate_box: NULL out") : 1;
  if (c->last_post_mode != UDA_POST_GLOBAL) return fail(c, "calibrate_box: needs the global post-process (uncertainty columns)");
  const int bc = box_cols_of(c->model, UDA_POST_GLOBAL), cc = cls_cols_of(c->model, UDA_POST_GLOBAL);
  if (col0 < 4 || col0 + 4 > bc || (col0 & 3)) return fail(c, "calibrate_box: columns %d..%d outside the %d box columns", col0, col0 + 3, bc);
  const bool iso = mode >= UDA_CALIB_ISO_ALL;
  if (mode < 0 || mode > UDA_CALIB_ISO_PERCLSCOO) return fail(c, "calibrate_box: unknown mode %d", mode);
  if (!iso && !temps) return fail(c, "calibrate_box: temperature scaling needs temps");
  if (relative && mode != UDA_CALIB_ISO_PERCLSCOO) return fail(c, "calibrate_box: the relative variant exists per class and coordinate only");
  const int want = mode == UDA_CALIB_ISO_ALL ? 1 : (mode == UDA_CALIB_ISO_PERCOO ? 4 : 4 * c->model.num_classes);
  if (iso && (n_tables != want || !tab_off || !xs || !ys))
    return fail(c, "calibrate_box: mode %d needs %d tables, got %d", mode, want, n_tables);
  if (int rc = settle_detections(c)) return rc;
  for (int t = 0; iso && t < n_tables; ++t)
    if (tab_off[t + 1] < tab_off[t]) return fail(c, "calibrate_box: table offsets must be non-decreasing");
  const size_t rows = (size_t)c->last_n * c->model.max_output_size;
  DevScratch s(c->device);
  CalibArgs a{};
  if (iso) {
    const size_t tot = (size_t)tab_off[n_tables];
    a.xs = s.upload(xs, tot, c->stream); a.ys = s.upload(ys, tot, c->stream); a.tab_off = s.upload(tab_off, (size_t)n_tables + 1, c->stream);
  }
  float* d_out = s.alloc<float>(rows * 4);
  a.boxes = c->d_oboxes; a.classes = c->d_oclasses; a.out = d_out;
  for (int j = 0; j < 4; ++j) a.temps[j] = temps ? temps[mode == UDA_CALIB_TS_ALL ? 0 : j] : 1.f;
  a.rows = (int)rows; a.box_cols = bc; a.cls_cols = cc; a.col0 = col0;
  a.mode = mode; a.relative = relative; a.n_tables = n_tables;
  if (s.ok()) launch_calib(a, c->stream);
  s.sync(c->stream);
  s.download(out, d_out, rows * 4 * sizeof(float));
  return scratch_done(c, "calibrate_box", s);
}

extern "C" int uda_calibrate_class(uda_ctx_t* c, int32_t mode, int32_t n_tables, const int32_t* tab_off, const double* xs,
                                   const double* ys, const float* temps, int32_t draws, uint64_t seed, float* probs,
                                   float* entropy, float* uncert) {
  if (!c || !probs || !entropy) return c ? fail(c, "calibrate_class: NULL output") : 1;
  const uda_model_t& m = c->model;
  if (c->last_post_mode != UDA_POST_GLOBAL || !m.enable_softmax)
    return fail(c, "calibrate_class: needs the logits of the global post-process (enable_softmax)");
  if (mode < UDA_CLS_TS || mode > UDA_CLS_ISO_PERCLS) return fail(c, "calibrate_class: unknown mode %d", mode);
  const int C = m.num_classes;
  if (C > 128) return fail(c, "calibrate_class: more than 128 classes");
  if (mode == UDA_CLS_TS && !temps) return fail(c, "calibrate_class: temperature scaling needs %d temperatures", C);
  const int want = mode == UDA_CLS_ISO_ALL ? 1 : C;
  if (mode != UDA_CLS_TS && (n_tables != want || !tab_off || !xs || !ys))
    return fail(c, "calibrate_class: mode %d needs %d isotonic tables, got %d", mode, want, n_tables);
  const int cc = cls_cols_of(m, UDA_POST_GLOBAL);
  if (draws < 0 || draws > 1000) return fail(c, "calibrate_class: draws %d outside [0, 1000]", draws);
  if (draws > 0 && cc != 1 + C)
    return fail(c, "calibrate_class: sampling needs the MC std of every class logit (MC dropout on the class head, max_nms_inputs = 0)");
  if (int rc = settle_detections(c)) return rc;
  const size_t rows = (size_t)c->last_n * m.max_output_size;
  for (int t = 0; mode != UDA_CLS_TS && t < n_tables; ++t)
    if (tab_off[t + 1] <= tab_off[t]) return fail(c, "calibrate_class: every isotonic table needs at least one threshold");
  DevScratch s(c->device);
  ClsCalibArgs k{};
  if (mode != UDA_CLS_TS) {
    const size_t tot = (size_t)tab_off[n_tables];
    k.xs = s.upload(xs, tot, c->stream); k.ys = s.upload(ys, tot, c->stream); k.tab_off = s.upload(tab_off, (size_t)n_tables + 1, c->stream);
  } else {
    k.temps = s.upload(temps, (size_t)C, c->stream);
  }
  float *d_p = s.alloc<float>(rows * C), *d_e = s.alloc<float>(rows), *d_u = uncert ? s.alloc<float>(rows * C) : nullptr;
  k.logits = c->d_ologits; k.classes = c->d_oclasses; k.probs = d_p; k.entropy = d_e; k.uncert = d_u;
  k.rows = (int)rows; k.C = C; k.cls_cols = cc; k.mode = mode; k.draws = draws; k.seed = seed;
  if (s.ok()) launch_class_calib(k, c->stream);
  s.sync(c->stream);
  s.download(probs, d_p, rows * C * sizeof(float));
  s.download(entropy, d_e, rows * sizeof(float));
  if (uncert && draws > 0) s.download(uncert, d_u, rows * C * sizeof(float));
  if (!s.ok()) return hip_failed(c, "calibrate_class", s.err);
  if (uncert && draws <= 0) memset(uncert, 0, rows * C * sizeof(float));
  return 0;
}

// CRC-32C (Castagnoli, reflected polynomial 0x82F63B78), slicing-by-8 on the host: the per-tensor checksum of TensorFlow
// checkpoint bundles (ckpt_reader.py verifies every tensor it restores; a pure-Python table CRC manages ~1 MB/s).
extern "C" uint32_t uda_crc32c(const void* data, uint64_t n, uint32_t crc) {
  struct Tables {
    uint32_t t[8][256];
    Tables() {
      for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
        t[0][i] = c;
      }
      for (uint32_t i = 0; i < 256; ++i)
        for (int k = 1; k < 8; ++k) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 0xFFu];
    }
  };
  static const Tables tables;          // function-local static: initialised once, thread-safe (C++11) - ctypes releases the GIL
  const uint32_t (*T)[256] = tables.t;
  const uint8_t* p = (const uint8_t*)data;
  crc = ~crc;
  while (n >= 8) {
    uint64_t w;
    memcpy(&w, p, 8);
    w ^= crc;
    crc = T[7][w & 0xFF] ^ T[6][(w >> 8) & 0xFF] ^ T[5][(w >> 16) & 0xFF] ^ T[4][(w >> 24) & 0xFF] ^
          T[3][(w >> 32) & 0xFF] ^ T[2][(w >> 40) & 0xFF] ^ T[1][(w >> 48) & 0xFF] ^ T[0][(w >> 56) & 0xFF];
    p += 8; n -= 8;
  }
  while (n--) crc = T[0][(crc ^ *p++) & 0xFFu] ^ (crc >> 8);
  return ~crc;
}

// ------------------------------------------------------------------------------------ standalone NMS
extern "C" int uda_nms(uda_ctx_t* c, const float* boxes, const float* scores, int32_t n_img, int32_t k,
                       int32_t max_out, float iou_thresh, float score_thresh, float soft_sigma, int32_t pad,
                       int32_t* idx, float* out_scores, int32_t* valid) {
  if (!c || !boxes || !scores || !idx || !out_scores || !valid) return c ? fail(c, "uda_nms: NULL argument") : 1;
  if (n_img < 1 || k < 0 || max_out < 1 || max_out > 128) return fail(c, "uda_nms: bad sizes (max_out must be in [1, 128])");
  const size_t NK = (size_t)n_img * (k ? k : 1), NM = (size_t)n_img * max_out;
  // The epoch rule of the kernels needs scores that only shrink: a cached exact score is an upper
  // bound, a candidate below the last winner cannot be popped.  Soft NMS moves a live NEGATIVE score up (a weight below 1
  // times a negative number), the reference re-pushes it with a higher priority and the selections differ - refused, not
  // answered differently.  (Host arrays: the scan is free here; the serve path scores are sigmoids and never negative.)
  if (soft_sigma > 0.0f && score_thresh < 0.0f) {
    for (size_t i = 0; i < (size_t)n_img * (size_t)k; ++i)
      if (scores[i] < 0.0f && scores[i] > score_thresh)
        return fail(c, "uda_nms: soft NMS (soft_sigma %g) with score_thresh %g < 0 over a live negative score (problem %lld, "
                       "candidate %lld: %g) is not supported: its weights raise such a score, which the kernels' epoch rule "
                       "cannot follow exactly.  Use score_thresh >= 0, hard NMS, or non-negative scores",
                    (double)soft_sigma, (double)score_thresh, (long long)(i / (size_t)k), (long long)(i % (size_t)k), (double)scores[i]);
  }
  DevScratch s(c->device);
  float* d_boxes = k ? s.upload(boxes, NK * 4, c->stream) : s.alloc<float>(NK * 4);
  float* d_scores = k ? s.upload(scores, NK, c->stream) : s.alloc<float>(NK);
  NmsArgs a{};
  a.boxes = d_boxes; a.stale = s.alloc<float>(NK); a.tent = s.alloc<float>(NK); a.ub = s.alloc<float>(NK);
  a.ev = s.alloc<int32_t>(NK); a.begin = s.alloc<int32_t>(NK);
  a.sel_idx = s.alloc<int32_t>(NM); a.sel_score = s.alloc<float>(NM); a.sel_box = s.alloc<float>(NM * 4);
  a.bound_key = s.alloc<unsigned long long>(NM); a.win_key = s.alloc<unsigned long long>(NM);
  a.nsel = s.alloc<int32_t>((size_t)n_img); a.done = s.alloc<int32_t>((size_t)n_img);
  a.n_img = n_img; a.K = k; a.M = max_out;
  a.segs = 1; a.classes = nullptr;
  nms_params(a, iou_thresh, score_thresh, soft_sigma);
  struct Prefix {          // the workspace of the score-prefix NMS, as the handle's own: alloc_prefix_ws / free_prefix_ws
    uda_ctx::PrefixWs ws;
    ~Prefix() { free_prefix_ws(ws); }
  } owned;
  uda_ctx::PrefixWs& pw = owned.ws;
  const int lp = prefix_target();
  if (s.ok() && lp > 0 && k > solo_limit() && k > 2 * lp) s.err = alloc_prefix_ws(pw, (size_t)n_img, 2 * lp, (size_t)max_out);
  if (!s.ok()) return hip_failed(c, "uda_nms", s.err);
  bool prefix = false;
  {
    ProfScope ps(c, 17);
    NmsCoop coop;
    if ((size_t)n_img * nms_coop_slot_words(max_out) <= (size_t)c->model.max_images * nms_coop_slot_words(c->model.max_output_size) && !c->coop_off) { coop.bar = c->d_coop_bar; coop.err = c->d_coop_err; coop.used = &c->coop_used; coop.not_launched = &c->coop_not_launched; }
    if (k > 0) prefix = run_nms(a, d_scores, max_out, c->stream, pw.Lcap ? &pw : nullptr, 0, coop);
    else launch_nms_init(a, d_scores, c->stream);
  }
  s.sync(c->stream);
  if (prefix) {            // problems whose prefix was not sufficient: the full candidate set, one problem at a time
    std::vector<int32_t> bad((size_t)n_img);
    s.download(bad.data(), pw.bad, (size_t)n_img * sizeof(int32_t));
    for (int p = 0; s.ok() && p < n_img; ++p) {
      if (!bad[(size_t)p]) continue;
      const size_t pk = (size_t)p * k, pm = (size_t)p * max_out;
      NmsArgs f = a;
      f.boxes += pk * 4; f.stale += pk; f.begin += pk; f.tent += pk; f.ub += pk; f.ev += pk;
      f.sel_idx += pm; f.sel_score += pm; f.sel_box += pm * 4; f.bound_key += pm; f.win_key += pm;
      f.nsel += p; f.done += p; f.n_img = 1;
      ProfScope ps(c, 17);
      NmsCoop coop;
      if (!c->coop_off) { coop.bar = c->d_coop_bar; coop.err = c->d_coop_err; coop.used = &c->coop_used; coop.not_launched = &c->coop_not_launched; }
      run_nms(f, d_scores + pk, max_out, c->stream, nullptr, 0, coop);
      ++c->pfx_fallbacks;
    }
    s.sync(c->stream);
  }
  if (s.ok() && c->coop_used) {
    c->coop_used = false;
    int e = 0;
    hipMemcpy(&e, c->d_coop_err, sizeof(int), hipMemcpyDeviceToHost);
    if (e) {           // barrier time-out: redo with the two-launch version (see finish_post)
      hipMemset(c->d_coop_err, 0, sizeof(int));
      c->coop_off = true;
      ++c->coop_fallbacks;
      fprintf(stderr, "[uda] cooperative NMS: grid barrier timed out; falling back to two launches per epoch\n");
      run_nms(a, d_scores, max_out, c->stream);
      s.sync(c->stream);
    }
  }
  s.download(valid, a.nsel, n_img * sizeof(int32_t));
  s.download(idx, a.sel_idx, NM * sizeof(int32_t));
  s.download(out_scores, a.sel_score, NM * sizeof(float));
  (void)pad;  // slots >= valid already hold index 0 / score 0.0 (the padded form); callers slice when pad == 0
  return scratch_done(c, "uda_nms", s);
}

// ------------------------------------------------------------------------------------ standalone 1x1 conv
extern "C" int uda_debug_pw(int32_t device, const float* in, const float* w, const float* bias, const float* bn_scale,
                            const float* bn_shift, const float* se, const float* mask, const float* res,
                            int32_t rows, int32_t in_div, int32_t hw, int32_t cin, int32_t cout, int32_t act,
                            int32_t terms, int32_t reps, float* out, float* avg_ms) {
  if (!in || !w || !out || rows < 1 || in_div < 1 || rows % in_div || hw < 1 || cin < 4 || cin % 4 || cout < 1)
    return fail(nullptr, "uda_debug_pw: bad argument");
  if (terms != 0 && terms != 1 && terms != 3 && terms != 6 && terms != 8 && terms != 16)
    return fail(nullptr, "uda_debug_pw: terms must be 0 (f32 MFMA), 1 (fp16 x1), 3 (bf16 x2), 6 (bf16 x3), 8 (bf16 x1) or 16 (fp16 x2)");
  const size_t rows_in = rows / in_div;
  DevScratch s(device);
  PwArgs a{};
  a.in = s.upload(in, rows_in * hw * cin);
  a.w = s.upload(w, (size_t)cin * cout);
  a.bias = s.upload(bias, cout);
  a.bn_scale = s.upload(bn_scale, cout);
  a.bn_shift = s.upload(bn_shift, cout);
  a.se = s.upload(se, rows_in * cin);
  a.mask = s.upload(mask, (size_t)rows * cout);
  a.res = s.upload(res, (size_t)rows * hw * cout);
  float* d_out = s.alloc<float>((size_t)rows * hw * cout);
  a.out = d_out;
  a.HW = hw; a.Cin = cin; a.Cout = cout; a.in_div = in_div; a.res_div = 1; a.se_div = in_div; a.act = act;
  unsigned* d_oor = nullptr;
  if (terms) {
    const int scheme = terms == 6 ? UDA_SPLIT_BF16X3 : (terms == 16 ? UDA_SPLIT_F16X2 : (terms == 1 ? UDA_SPLIT_F16X1 : (terms == 8 ? UDA_SPLIT_BF16X1 : UDA_SPLIT_BF16X2)));
    // (as uda_create packs a 1x1 conv: fp16 pieces, one or two, carry the power-of-two weight scale)
    const float scale = uda_split_f16(scheme) ? split_weight_scale(w, (size_t)cin * cout) : 1.0f;
    std::vector<uint16_t> packed(pwb_packed_elems(cin, cout, scheme));
    pwb_pack_weights(w, cin, cout, scheme, packed.data(), scale);
    a.wsplit = s.upload(packed.data(), packed.size());
    a.wparts = scheme;
    a.wunscale = 1.0f / scale;
    a.oor = d_oor = s.alloc<unsigned>(1);
    s.zero(d_oor, sizeof(unsigned));
  }
  hipStream_t st = s.stream();
  hipEvent_t e0 = s.event(), e1 = s.event();
  float ms = 0;
  if (s.ok()) {
    auto go = [&]() { if (terms) launch_pwb(a, rows, st); else launch_pw(a, rows, st); };
    go();                                   // warm-up (and the result that is read back)
    hipEventRecord(e0, st);
    for (int i = 0; i < reps; ++i) go();
    hipEventRecord(e1, st);
    s.sync(st);
    hipEventElapsedTime(&ms, e0, e1);
  }
  if (avg_ms) *avg_ms = reps > 0 ? ms / reps : 0.f;
  s.download(out, d_out, (size_t)rows * hw * cout * sizeof(float));
  unsigned oor = 0;
  if (d_oor) s.download(&oor, d_oor, sizeof(unsigned));
  if (!s.ok()) return hip_failed(nullptr, "uda_debug_pw", s.err);
  if (oor) return fail(nullptr, "uda_debug_pw: an input above 65504 cannot be split into fp16 pieces (terms = %d)", terms);
  return 0;
}

// ------------------------------------------------------------------------------------ numpy NMS family (a18)
template <typename T>
static int run_nmsnp(const char* who, int device, const std::vector<T>& dets, const std::vector<int32_t>& off, int method, double iou_thr,
                     double sigma, double score_thr, std::vector<T>& out, std::vector<int32_t>& n_out) {
  const int problems = (int)off.size() - 1;
  const size_t total = (size_t)off.back();
  out.assign(total * 5, (T)0);
  n_out.assign(problems > 0 ? problems : 0, 0);
  if (problems <= 0 || total == 0) return 0;
  DevScratch s(device);
  NmsNpArgs<T> a{};
  a.dets = s.upload(dets.data(), total * 5); a.score = s.alloc<T>(total); a.out = s.alloc<T>(total * 5);
  a.off = s.upload(off.data(), off.size()); a.state = s.alloc<int32_t>(total); a.n_out = s.alloc<int32_t>((size_t)problems);
  a.method = method; a.iou_thr = (T)iou_thr; a.sigma = (T)sigma; a.score_thr = (T)score_thr;
  if (s.ok()) launch_nmsnp<T>(a, problems, nullptr);
  s.sync();
  s.download(out.data(), a.out, total * 5 * sizeof(T));
  s.download(n_out.data(), a.n_out, (size_t)problems * sizeof(int32_t));
  return scratch_done(nullptr, who, s);
}

// rows sorted by score, descending (what `dets[:, 4].argsort()[::-1]` yields for distinct scores; ties: later index first)
template <typename T>
static void sort_desc(std::vector<T>& dets, int begin, int n) {
  std::vector<int> idx(n);
  std::iota(idx.begin(), idx.end(), 0);
  std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) {
    const T sx = dets[(size_t)(begin + x) * 5 + 4], sy = dets[(size_t)(begin + y) * 5 + 4];
    return sx > sy || (sx == sy && x > y);
  });
  std::vector<T> tmp((size_t)n * 5);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 5; ++k) tmp[(size_t)i * 5 + k] = dets[(size_t)(begin + idx[i]) * 5 + k];
  std::copy(tmp.begin(), tmp.end(), dets.begin() + (size_t)begin * 5);
}

extern "C" int uda_nms_np(int32_t device, const double* dets, int32_t n, int32_t method, double iou_thresh, double sigma,
                          double score_thresh, double* out, int32_t* n_out) {
  if (!dets || !out || !n_out || n < 0 || method < 0 || method > 3) return fail(nullptr, "uda_nms_np: bad argument");
  std::vector<double> d(dets, dets + (size_t)n * 5), o;
  std::vector<int32_t> off = {0, n}, no;
  if (method <= 1) sort_desc(d, 0, n);
  const int rc = run_nmsnp<double>("uda_nms_np", device, d, off, method, iou_thresh, sigma, score_thresh, o, no);
  if (rc) return rc;
  *n_out = n ? no[0] : 0;
  std::copy(o.begin(), o.begin() + (size_t)*n_out * 5, out);
  return 0;
}

extern "C" int uda_per_class_nms_np(int32_t device, const float* boxes, const float* scores, const int32_t* classes, int32_t k,
                                    float image_id, float image_scale, int32_t num_classes, int32_t max_boxes, int32_t method,
                                    float iou_thresh, float sigma, float score_thresh, float* out) {
  if (!boxes || !scores || !classes || !out || k < 0 || num_classes < 1 || max_boxes < 1 || method < 0 || method > 3)
    return fail(nullptr, "uda_per_class_nms_np: bad argument");
  std::vector<float> d;
  std::vector<int32_t> off = {0}, cls_of;
  for (int c = 0; c < num_classes; ++c) {
    const int begin = off.back();
    int n = 0;
    for (int i = 0; i < k; ++i)
      if (classes[i] == c) {           // boxes arrive y1,x1,y2,x2 -> x1,y1,x2,y2 (nms_np.py:234)
        d.insert(d.end(), {boxes[i * 4 + 1], boxes[i * 4 + 0], boxes[i * 4 + 3], boxes[i * 4 + 2], scores[i]});
        ++n;
      }
    if (!n) continue;
    if (method <= 1) sort_desc(d, begin, n);
    off.push_back(begin + n);
    cls_of.push_back(c);
  }
  std::vector<float> o;
  std::vector<int32_t> no;
  const int rc = run_nmsnp<float>("uda_per_class_nms_np", device, d, off, method, iou_thresh, sigma, score_thresh, o, no);
  if (rc) return rc;
  struct Row { float v[7]; };
  std::vector<Row> rows;
  for (size_t p = 0; p + 1 < off.size(); ++p)
    for (int i = 0; i < no[p]; ++i) {
      const float* r = o.data() + ((size_t)off[p] + i) * 5;
      rows.push_back(Row{{image_id, r[0], r[1], r[2], r[3], r[4], (float)(cls_of[p] + 1)}});
    }
  std::stable_sort(rows.begin(), rows.end(), [](const Row& x, const Row& y) { return x.v[5] > y.v[5]; });
  for (int i = 0; i < max_boxes; ++i) {
    float* dst = out + (size_t)i * 7;
    if (i < (int)rows.size()) {
      for (int j = 0; j < 7; ++j) dst[j] = rows[i].v[j];
    } else {                           // dummy rows: score -1e5 (nms_np.py:256-274)
      for (int j = 0; j < 7; ++j) dst[j] = 0.f;
      dst[0] = image_id;
      dst[5] = -1e5f;
    }
    for (int j = 1; j < 5; ++j) dst[j] *= image_scale;
  }
  return 0;
}
