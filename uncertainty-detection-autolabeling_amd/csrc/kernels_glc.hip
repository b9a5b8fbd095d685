// Ground-truth label correction (GLC): the three verdicts of the reference's AdvancedLabels (src/ssl_utils/glc.py) on the
// detections and the ground truth of a batch of labelled images - uda_label_check and its host-array twins (include/uda_hip.h).
// Built without FMA contraction (csrc/Makefile): the IoUs are compared with the reference's bit for bit.
//
//   label_check_kernel<float | double>   one block per image, four phases; a block barrier wherever a phase reads what an
//                                        earlier one wrote (phases 2 and 3 touch different words and share one)
//
// The detections of an image are its KEPT rows, score > min_score in rank order (the rows of prediction_data.txt,
// infer_model.py:842); the ground truth its COUNTED rows, class > 0 (padding rows carry -1).
//   phase 0  the first wave packs the kept ranks in rank order (ballots); the block stages their boxes in LDS and clears the
//            per-detection words.  Packing keeps the order, so "lower packed index" and "lower rank" are the same thing.
//   phase 1  one wave per counted row g, its lanes striding over the K kept boxes: iou[g] = max_k calc_iou_np(gt_g, box_k) and
//            matched[g] = the first k that reaches it (glc.py:182-187) - the lexicographic best of (IoU, packed index), in the
//            lane's own sweep and in every step of the wave reduction alike, so the winner does not depend on how the indices
//            were dealt to lanes.  A row that touches nothing has IoU 0 everywhere and is matched to the first kept detection.
//            On the way every positive IoU goes into the detection's maximum over the rows with an integer atomicMax: IoUs
//            are >= 0, so their float64 bit patterns order like unsigned integers, and a maximum does not depend on order
//            (zeros are skipped: the word starts at 0).  The row's lane 0 then writes mistake (iou == 0, :551) and the noisy
//            conditions (:813-824), raises the matched detection's `better` bit (an OR) and lowers its first-row word (a
//            minimum over row indices).
//   phase 2  one thread per row: the row is replaced iff its detection is in `better` and the row is the detection's first
//            matched row (np.where(matched == k)[0][0], :832) - whether or not the row itself met the conditions.
//   phase 3  one thread per kept detection: missing label iff its maximum IoU == md_max_inter (np.equal, :432-436; <= under
//            the synthetic rule, :468-472) and cons_iou >= iou_consist.
// The five counts are integer atomics in LDS.  Nothing is accumulated in floating point: every output is exact and the same
// however rows and ranks are cut into waves.
// Two cases the reference does not reach are defined here: an image without a kept detection gives every row det_rank -1,
// IoU 0 and no flag; an image without a counted row (the reference raises on np.argmax of an empty list) leaves every
// detection's maximum at 0, and the missing-label rule is applied to that.
#include "box_iou.h"
#include "uda_internal.h"
#include "wave_fold.h"

namespace uda {

// (glc_iou, the reference's calc_iou_np on float32 and on float64 boxes, is in box_iou.h)

// dynamic LDS of a block: boxes [M][4] of T | packed ranks [M] int32 | `better` bits [(M + 31) / 32] uint32
template <typename T>
static size_t label_check_lds(int M) {
  return (size_t)M * (4 * sizeof(T) + sizeof(int32_t)) + (size_t)((M + 31) / 32) * sizeof(uint32_t);
}

template <typename T>
__global__ __launch_bounds__(256) void label_check_kernel(LabelCheckArgs<T> a) {
  extern __shared__ double glc_lds[];                       // (double: the boxes of either type are aligned)
  __shared__ int K_s, cnt[4];                               // kept detections; counted rows, mistakes, replaced rows, missing labels
  const int i = blockIdx.x, M = a.M, G = a.G;
  T* box = (T*)glc_lds;                                     // [K][4] the kept detections' boxes, in rank order
  int32_t* rank = (int32_t*)(box + (size_t)M * 4);          // [K] resident rank of the packed detection
  uint32_t* better = (uint32_t*)(rank + M);                 // bit e: packed detection e is in `better`
  const T* scores = a.scores + (size_t)i * M;
  const double* cons = a.cons_iou ? a.cons_iou + (size_t)i * M : nullptr;
  unsigned long long* det_max = (unsigned long long*)(a.det_max_iou + (size_t)i * M);   // by rank; float64 bits
  int32_t* first = a.first_row + (size_t)i * M;             // by packed index
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;

  // ---- phase 0
  if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
  if (wave == 0) {
    int base = 0;
    for (int k0 = 0; k0 < M; k0 += 64) {                   // (wave-uniform: the ballot sees all 64 lanes)
      const int k = k0 + lane;
      const bool kept = k < M && scores[k] > a.min_score;
      const unsigned long long mask = __ballot(kept);
      if (kept) rank[base + __popcll(mask & ((1ull << lane) - 1ull))] = k;
      base += __popcll(mask);
    }
    if (lane == 0) K_s = base;
  }
  for (int k = threadIdx.x; k < M; k += blockDim.x) {
    det_max[k] = 0ull;
    first[k] = 0x7fffffff;
    a.det_flags[(size_t)i * M + k] = 0;
  }
  for (int w = threadIdx.x; w < (M + 31) / 32; w += blockDim.x) better[w] = 0u;
  __syncthreads();
  const int K = K_s;
  for (int e = threadIdx.x; e < K * 4; e += blockDim.x)
    box[e] = a.det_boxes[((size_t)i * M + rank[e >> 2]) * a.det_stride + (e & 3)];
  __syncthreads();

  // ---- phase 1
  int rows = 0, mistakes = 0;
  for (int g = wave; g < G; g += waves) {                   // (wave-uniform: the shuffles below see all 64 lanes)
    const size_t row = (size_t)i * G + g;
    const T* gp = a.gt_boxes + row * 4;
    const T gt[4] = {gp[0], gp[1], gp[2], gp[3]};
    const bool counted = a.gt_classes[row] > (T)0;
    if (!counted || K == 0) {
      if (lane == 0) {
        a.det_rank[row] = -1; a.iou[row] = 0.0; a.gt_flags[row] = 0;
        if (counted) ++rows;
      }
      continue;
    }
    double key = -1.0;                                      // below every IoU
    int best = 0x7fffffff;
    for (int e = lane; e < K; e += 64) {
      const double v = glc_iou(gt, box + e * 4);
      if (v > key) { key = v; best = e; }                   // (e ascends: an equal key never replaces a lower index)
      if (v > 0.0) atomicMax(det_max + rank[e], (unsigned long long)__double_as_longlong(v));
    }
    wave_best_max(key, best);
    if (lane == 0) {
      if (best >= K) { best = 0; key = glc_iou(gt, box); }  // every IoU was NaN (non-finite input): nothing is indexed with the sentinel
      const int r = rank[best];
      uint8_t f = 0;
      if ((a.methods & LC_MISTAKES) && key == 0.0) { f |= LC_GT_MISTAKE; ++mistakes; }
      if (a.methods & LC_NOISY) {
        if (cons[r] > a.iou_consist && key <= a.correct_max_inter && scores[r] >= a.correct_score) {
          f |= LC_GT_NOISY;
          atomicOr(better + (best >> 5), 1u << (best & 31));
        }
        atomicMin(first + best, g);
      }
      a.det_rank[row] = best;                               // the packed index until phase 2 turns it into the rank
      a.iou[row] = key;
      a.gt_flags[row] = f;
      ++rows;
    }
  }
  if (lane == 0) {
    if (rows) atomicAdd(&cnt[0], rows);
    if (mistakes) atomicAdd(&cnt[1], mistakes);
  }
  __syncthreads();

  // ---- phase 2
  int replaced = 0;
  for (int g = threadIdx.x; g < G; g += blockDim.x) {
    const size_t row = (size_t)i * G + g;
    const T* gp = a.gt_boxes + row * 4;
    const int e = a.det_rank[row];
    const T* src = gp;
    if (e >= 0) {
      a.det_rank[row] = rank[e];
      // (the word was lowered by atomics of other waves: read it where they were done)
      if (((better[e >> 5] >> (e & 31)) & 1u) && __hip_atomic_load(first + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == g) {
        src = box + e * 4;
        a.gt_flags[row] |= LC_GT_REPLACED;
        ++replaced;
      }
    }
    for (int q = 0; q < 4; ++q) a.gt_boxes_out[row * 4 + q] = (float)src[q];
  }
  if (replaced) atomicAdd(&cnt[2], replaced);

  // ---- phase 3
  int md = 0;
  for (int e = threadIdx.x; e < K; e += blockDim.x) {
    const int r = rank[e];
    uint8_t f = LC_DET_KEPT;
    if (a.methods & LC_MD) {
      const double mx = __longlong_as_double((long long)__hip_atomic_load(det_max + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      if ((a.md_rule == LC_MD_LE ? mx <= a.md_max_inter : mx == a.md_max_inter) && cons[r] >= a.iou_consist) {
        f |= LC_DET_MISSING;
        ++md;
      }
    }
    a.det_flags[(size_t)i * M + r] = f;
  }
  if (md) atomicAdd(&cnt[3], md);
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t* c = a.counts + (size_t)i * 5;
    c[0] = K; c[1] = cnt[0]; c[2] = cnt[1]; c[3] = cnt[2]; c[4] = cnt[3];
  }
}

template <typename T>
static void launch_label_check_t(const LabelCheckArgs<T>& a, hipStream_t s) {
  const size_t lds = label_check_lds<T>(a.M);
  if (lds > 65536) hipFuncSetAttribute((const void*)label_check_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(label_check_kernel<T>, dim3((unsigned)a.n), dim3(256), lds, s, a);
}
void launch_label_check(const LabelCheckArgs<float>& a, hipStream_t s) { launch_label_check_t(a, s); }
void launch_label_check(const LabelCheckArgs<double>& a, hipStream_t s) { launch_label_check_t(a, s); }

}  // namespace uda
