// Pseudo-label audit: the reference's comparison of the STAC teacher's pseudo labels with the ground truth
// (Parent_SSL.extract_pseudo_gt_data and _percls_analysis, src/ssl_utils/parent.py:1567-1813) for a batch of ragged images -
// uda_pseudo_audit_np (include/uda_hip.h).  Built without FMA contraction (csrc/Makefile): the IoUs are compared with the
// reference's bit for bit.
//
//   pseudo_audit_kernel   one block of 256 threads per image, six phases; a block barrier wherever a phase reads what an
//                         earlier one wrote
//
// An image has G ground-truth rows (read from global memory) and D pseudo labels (staged in LDS).  The G x D IoU matrix of the
// reference is never stored: a phase computes the IoUs it needs again - the same operands give the same bits.
//   phase 0  stages the D pseudo boxes, clears the matched-prediction bits and the rows' orders, and writes the "not allocated"
//            values of the per-row and per-label outputs.
//   phase 1  one wave per row g, its lanes striding over the labels: gt_max_iou[g] = max_d IoU and gt_best_det[g] = the first d
//            that reaches it (np.argmax, :1736-1737) - the lexicographic best of (IoU, lower index), in the lane's own sweep
//            and in every step of the wave reduction alike.  gt_max_iou[g] >= gt_iou_thr sets bit gt_best_det[g] of the
//            matched-prediction set (an integer atomic OR in LDS): np.unique of :1736-1738.
//            The first wave then packs the set bits in ascending order (ballots): mp[p] is the p-th matched prediction and
//            pos[d] its position, -1 for a label that is not one.
//   phase 2  one wave per label d over the rows: det_max_iou[d] and det_best_gt[d], the first row that reaches it
//            (np.argmax(np.asarray(perim_ious).T[selector], axis=-1), 3d.py:150-152).
//   phase 3  the allocation loop of :1744-1752, one wave.  For the p-th matched prediction i the lanes stride over the rows
//            not yet taken and the wave reduces to the best (IoU(r, i), lower r); that row is taken with order p.  This is
//            what the reference's `while idx in matched_gt: ious[idx, i] = -1` arrives at: it discards taken rows one by one,
//            best first, until an untaken row is the column's argmax.  Lane r % 64 owns row r in every sweep, so order[r] is
//            written and read by one lane only.  There are at most G matched predictions, so an untaken row always exists.
//   phase 4  one wave per allocated pair (p: prediction i, row r): alloc_pair_iou = IoU(r, i) (the elementwise calc_iou_np of
//            _percls_analysis :1572-1581) and alloc_miou = np.max(ious[r]) on the reference's MUTATED matrix (:1763-1765): the
//            maximum over d of IoU(r, d), where entry (r, d) counts as -1 iff d is a matched prediction at a position q > p
//            (r was taken before d's turn) and (IoU(r, d), lower r) beats d's winner w - those are the entries the while loop
//            invalidated.  A prediction may take a row that did not choose it, and alloc_miou may be below the row's maximum,
//            even -1: both are the reference's behaviour.
//   phase 5  the by-value flags of _percls_analysis :1614-1646: a label is extra iff its box equals no allocated label's box in
//            all four coordinates (`pb[i] not in ab`), a row is unmatched iff its box equals no allocated row's box.
// Only integer atomics, no floating-point accumulation: every output is exact and the same however rows are dealt to waves.
// An image without a row or without a label (the reference raises on both) has no match: every label is extra, every row
// unmatched, maxima 0 and best indices -1.  An IoU that is NaN (non-finite input; the Python layer refuses it) orders as -1, so
// that no index is ever taken from a comparison that failed.
#include "box_iou.h"
#include "uda_internal.h"
#include "wave_fold.h"

namespace uda {

#define AUDIT_FREE 0x7fffffff

__device__ __forceinline__ double audit_iou(const double* a, const double* b) {
  const double v = glc_iou(a, b);
  return v == v ? v : -1.0;
}

// dynamic LDS of a block, for the call's largest image: boxes [Dm][4] f64 | win [Dm] f64 | mp [Dm] | pos [Dm] | mg [Dm] |
// order [Gm] int32 | bits [(Dm + 31) / 32] uint32.  57 472 bytes at the caps.
static size_t audit_lds(int Gm, int Dm) {
  return (size_t)Dm * (5 * sizeof(double) + 3 * sizeof(int32_t)) + (size_t)Gm * sizeof(int32_t) + (size_t)((Dm + 31) / 32) * sizeof(uint32_t);
}

__global__ __launch_bounds__(256) void pseudo_audit_kernel(AuditArgs a) {
  extern __shared__ double audit_smem[];
  __shared__ int P_s;
  const int b = blockIdx.x, Gm = a.max_g, Dm = a.max_d;
  const size_t g0 = (size_t)a.gt_off[b], d0 = (size_t)a.det_off[b];
  const int G = (int)(a.gt_off[b + 1] - a.gt_off[b]), D = (int)(a.det_off[b + 1] - a.det_off[b]);
  double* box = audit_smem;                                 // [D][4] the image's pseudo boxes
  double* win = box + (size_t)Dm * 4;                       // [P] IoU of the p-th matched prediction with the row it took
  int32_t* mp = (int32_t*)(win + Dm);                       // [P] the matched predictions, ascending
  int32_t* pos = mp + Dm;                                   // [D] position in mp, -1: not a matched prediction
  int32_t* mg = pos + Dm;                                   // [P] the row the p-th matched prediction took
  int32_t* order = mg + Dm;                                 // [G] the p a row was taken at, AUDIT_FREE: not taken
  uint32_t* bits = (uint32_t*)(order + Gm);                 // bit d: label d is a matched prediction
  const double* gtb = a.gt_boxes + g0 * 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;

  // ---- phase 0
  for (int e = threadIdx.x; e < D * 4; e += blockDim.x) box[e] = a.det_boxes[d0 * 4 + e];
  for (int w = threadIdx.x; w < (D + 31) / 32; w += blockDim.x) bits[w] = 0u;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    pos[d] = -1;
    a.det_alloc_gt[d0 + d] = -1; a.det_alloc_miou[d0 + d] = 0.0; a.det_alloc_pair_iou[d0 + d] = 0.0;
    if (G == 0) { a.det_max_iou[d0 + d] = 0.0; a.det_best_gt[d0 + d] = -1; }
  }
  for (int g = threadIdx.x; g < G; g += blockDim.x) {
    order[g] = AUDIT_FREE;
    a.gt_alloc_det[g0 + g] = -1;
    if (D == 0) { a.gt_max_iou[g0 + g] = 0.0; a.gt_best_det[g0 + g] = -1; }
  }
  __syncthreads();

  // ---- phase 1
  if (D > 0)
    for (int g = wave; g < G; g += waves) {                 // (wave-uniform: the shuffles below see all 64 lanes)
      const double gt[4] = {gtb[g * 4], gtb[g * 4 + 1], gtb[g * 4 + 2], gtb[g * 4 + 3]};
      double key = -2.0;                                    // below every IoU, the -1 of a NaN included
      int best = AUDIT_FREE;
      for (int d = lane; d < D; d += 64) {
        const double v = audit_iou(gt, box + d * 4);
        if (v > key) { key = v; best = d; }                 // (d ascends: an equal key never replaces a lower index)
      }
      wave_best_max(key, best);
      if (lane == 0) {
        a.gt_max_iou[g0 + g] = key;
        a.gt_best_det[g0 + g] = best;
        if (key >= a.gt_iou_thr) atomicOr(bits + (best >> 5), 1u << (best & 31));
      }
    }
  __syncthreads();
  if (wave == 0) {
    int base = 0;
    for (int k0 = 0; k0 < D; k0 += 64) {                    // (wave-uniform: the ballot sees all 64 lanes)
      const int d = k0 + lane;
      const bool in = d < D && ((bits[d >> 5] >> (d & 31)) & 1u);
      const unsigned long long mask = __ballot(in);
      if (in) {
        const int p = base + __popcll(mask & ((1ull << lane) - 1ull));
        mp[p] = d; pos[d] = p;
      }
      base += __popcll(mask);
    }
    if (lane == 0) P_s = base;
  }
  __syncthreads();
  const int P = P_s;

  // ---- phase 2 (reads the staged boxes only)
  if (G > 0)
    for (int d = wave; d < D; d += waves) {
      const double* bd = box + d * 4;
      double key = -2.0;
      int best = AUDIT_FREE;
      for (int g = lane; g < G; g += 64) {
        const double v = audit_iou(gtb + g * 4, bd);
        if (v > key) { key = v; best = g; }
      }
      wave_best_max(key, best);
      if (lane == 0) { a.det_max_iou[d0 + d] = key; a.det_best_gt[d0 + d] = best; }
    }

  // ---- phase 3
  if (wave == 0)
    for (int p = 0; p < P; ++p) {
      const double* bi = box + mp[p] * 4;
      double key = -2.0;
      int best = AUDIT_FREE;
      for (int r = lane; r < G; r += 64) {
        if (order[r] != AUDIT_FREE) continue;
        const double v = audit_iou(gtb + r * 4, bi);
        if (v > key) { key = v; best = r; }
      }
      wave_best_max(key, best);                           // P <= G: an untaken row exists, so best < G
      if ((best & 63) == lane) order[best] = p;             // the lane that owns the row
      if (lane == 0) { mg[p] = best; win[p] = key; }
    }
  __syncthreads();

  // ---- phase 4
  for (int p = wave; p < P; p += waves) {
    const int i = mp[p], r = mg[p];
    const double gt[4] = {gtb[r * 4], gtb[r * 4 + 1], gtb[r * 4 + 2], gtb[r * 4 + 3]};
    double key = -2.0;
    for (int d = lane; d < D; d += 64) {
      double v = audit_iou(gt, box + d * 4);
      const int q = pos[d];
      if (q > p) {                                          // d's turn came after r was taken
        const double wv = win[q];
        if (v > wv || (v == wv && r < mg[q])) v = -1.0;     // r beat d's winner: the while loop invalidated (r, d)
      }
      key = fmax(key, v);
    }
    for (int o = 32; o > 0; o >>= 1) key = fmax(key, __shfl_xor(key, o));
    if (lane == 0) {
      a.det_alloc_gt[d0 + i] = r;
      a.det_alloc_miou[d0 + i] = key;
      a.det_alloc_pair_iou[d0 + i] = win[p];
      a.gt_alloc_det[g0 + r] = i;
    }
  }

  // ---- phase 5 (reads what phases 0 to 3 left in LDS)
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    bool extra = pos[d] < 0;
    const double* bd = box + d * 4;
    for (int p = 0; extra && p < P; ++p) {
      const double* o = box + mp[p] * 4;
      if (bd[0] == o[0] && bd[1] == o[1] && bd[2] == o[2] && bd[3] == o[3]) extra = false;
    }
    a.det_flags[d0 + d] = extra ? UDA_AUDIT_DET_EXTRA : 0;
  }
  for (int g = threadIdx.x; g < G; g += blockDim.x) {
    bool nomatch = order[g] == AUDIT_FREE;
    if (nomatch && P > 0) {
      const double c[4] = {gtb[g * 4], gtb[g * 4 + 1], gtb[g * 4 + 2], gtb[g * 4 + 3]};
      for (int p = 0; nomatch && p < P; ++p) {
        const double* o = gtb + mg[p] * 4;
        if (c[0] == o[0] && c[1] == o[1] && c[2] == o[2] && c[3] == o[3]) nomatch = false;
      }
    }
    a.gt_flags[g0 + g] = nomatch ? UDA_AUDIT_GT_NOMATCH : 0;
  }
  if (threadIdx.x == 0) a.n_matches[b] = P;
}

void launch_pseudo_audit(const AuditArgs& a, hipStream_t s) {
  const size_t lds = audit_lds(a.max_g, a.max_d);
  if (lds > 65536) hipFuncSetAttribute((const void*)pseudo_audit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(pseudo_audit_kernel, dim3((unsigned)a.B), dim3(256), lds, s, a);
}

}  // namespace uda
