// Pre/post-processing kernels (gfx950).  Compiled with -ffp-contract=off: every float
// operation here is an individually rounded IEEE op in the order written, so results are
// comparable bit for bit with the CPU oracle's statement of the same arithmetic.
//
//   preprocess_kernel  normalise + bilinear resize (half-pixel centres) + zero pad
//                      (reference dataloader.py:69-75,123-152; efficientdet_keras.py:1076-1100); its NOISE
//                      instantiation serves the noise variant of the consistency check (infer_model.py:784-793)
//   augment_u8_kernel  flip + 9x9 Gaussian blur of the staged uint8 images (consistency check, infer_model.py:775-783)
//   consistency_kernel IoU / class agreement of the originals' detections with the variants' (infer_model.py:768-848,
//                      utils_box.py:56-89)
//   assign_gt_kernel   the detection that belongs to each ground-truth box (utils_extra.py:44-64, validate_model.py:314-339,
//                      calibrate_model.py:133-147); gather_assigned_kernel packs the matched rows of every output column
//   aggregate_kernel   MC mean / population std of the class logits, argmax + sigmoid,
//                      per-sample anchor decode (plain f32 or variance-propagating f64),
//                      mean / std over samples of the decoded corners, mean of decoded sigma
//                      (utils_extra.py:220-244; postprocess.py:75-141,284-331; anchors.py:41-75;
//                       utils_box.py:105-276)
//   (NMS itself: kernels_nms.hip)
//   gather_kernel     gathers by selected index, clips, rescales, packs the output tuple
//                      (postprocess.py:402-413,599-621)
//
// Pinned-down numerics shared with the oracle (oracle/post_ref.py header):
//   exp32(x) = float(exp(double(x))), sigmoid(x) = float(1/(1+exp(-double(x)))),
//   MC reductions are sequential float32 sums over t = 0..T-1.
#include <type_traits>
#include <hip/hip_fp16.h>

#include "post_common.h"
#include "wave_fold.h"

namespace uda {

// ------------------------------------------------------------------------------------ preprocess
// Raw value of channel c of raw pixel `px` of image `img` (index in the batch).  NOISE (the consistency check's noise variant,
// infer_model.py:784-793: im + np.random.normal(0, sqrt(0.5)), summed in float64, neither clipped nor rounded, served as a
// float image that preprocessing casts to float32): the draw is philox_normal(seed, px, image offset + img, c, tag 0x4E),
// keyed by the run's dropout seed - a property of the noisy RAW image, so the bilinear taps of one raw pixel agree.
template <bool NOISE>
__device__ __forceinline__ float raw_px(const uint8_t* img, size_t px, int c, int n, const PreprocArgs& a) {
  if constexpr (NOISE)
    return (float)((double)img[px * 3 + c] +
                   0.70710678118654752440 * philox_normal(a.noise_seed, (uint32_t)px, a.noise_img0 + (uint32_t)n, (uint32_t)c, 0x4Eu));
  else
    return (float)img[px * 3 + c];
}

template <bool NOISE>
__device__ __forceinline__ float norm_px(const uint8_t* img, size_t px, int c, int n, const PreprocArgs& a) {
  return (raw_px<NOISE>(img, px, c, n, a) - a.mean[c]) / a.stdv[c];
}

template <bool NOISE>
__global__ __launch_bounds__(256) void preprocess_kernel(PreprocArgs a) {
  const int64_t total = (int64_t)a.n * a.H * a.W;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= total) return;
  const int x = (int)(gid % a.W);
  const int y = (int)((gid / a.W) % a.H);
  const int n = (int)(gid / ((int64_t)a.W * a.H));
  float* o = a.out + (size_t)gid * 3;
  const PreGeo g = a.geo[n];                    // (uniform per image: one 40-byte scalar load for most waves)
  if (y >= g.sh || x >= g.sw) {
    o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
    return;
  }
  const uint8_t* img = a.in + g.off;
  if (g.sh == g.h && g.sw == g.w) {
    const size_t p = (size_t)y * g.w + x;
    for (int c = 0; c < 3; ++c) o[c] = norm_px<NOISE>(img, p, c, n, a);
    return;
  }
  const float fy = ((float)y + 0.5f) * g.scale_y - 0.5f;
  const float fx = ((float)x + 0.5f) * g.scale_x - 0.5f;
  const float fly = floorf(fy), flx = floorf(fx);
  const int ylo = (int)fmaxf(fly, 0.f), yhi = min((int)ceilf(fy), g.h - 1);
  const int xlo = (int)fmaxf(flx, 0.f), xhi = min((int)ceilf(fx), g.w - 1);
  const float ly = fy - fly, lx = fx - flx;
  const size_t ptl = (size_t)ylo * g.w + xlo;
  const size_t ptr = (size_t)ylo * g.w + xhi;
  const size_t pbl = (size_t)yhi * g.w + xlo;
  const size_t pbr = (size_t)yhi * g.w + xhi;
  for (int c = 0; c < 3; ++c) {
    const float tl = norm_px<NOISE>(img, ptl, c, n, a), tr = norm_px<NOISE>(img, ptr, c, n, a);
    const float bl = norm_px<NOISE>(img, pbl, c, n, a), br = norm_px<NOISE>(img, pbr, c, n, a);
    const float top = tl + (tr - tl) * lx;
    const float bot = bl + (br - bl) * lx;
    o[c] = top + (bot - top) * ly;
  }
}

void launch_preprocess(const PreprocArgs& a, hipStream_t s) {
  const int64_t total = (int64_t)a.n * a.H * a.W;
  if (a.noise)
    hipLaunchKernelGGL(preprocess_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(preprocess_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------------------------ consistency check: flip + blur
// cv2.GaussianBlur(im, (9, 9), 0) on uint8 (infer_model.py:779-781).  sigma 0 means 0.3 ((9 - 1) / 2 - 1) + 0.8 = 1.7; OpenCV's
// 8-bit path filters with fixed-point taps of 8 fractional bits (getGaussianKernelBitExact + getGaussianKernelFixedPoint_ED):
// c[i] = exp(-i^2 / (2 sigma^2)) / sum, times 256, rounded from the outside in with the rounding error carried to the next
// tap, the centre tap taking what is left so that the taps sum to exactly 256.  That gives 4 13 30 51 60 51 30 13 4.  Row pass
// r = sum c[i] p (exact, < 2^16), column pass s = sum c[j] r (exact, < 2^24), output (s + 32768) >> 16.  Borders: REFLECT_101
// (BORDER_DEFAULT) with borderInterpolate's iteration for images narrower than the 4-pixel halo.  The numpy restatement
// (tests) reproduces this bit for bit; agreement with cv2 itself is not verified here (cv2 is not a dependency).
constexpr int AUG_TX = 64, AUG_TY = 16, AUG_R = 4;
__device__ __forceinline__ int blur_tap(int i) {
  return i == 0 ? 60 : (i == 1 || i == -1) ? 51 : (i == 2 || i == -2) ? 30 : (i == 3 || i == -3) ? 13 : 4;
}
__device__ __forceinline__ int reflect101(int p, int len) {
  if (len == 1) return 0;
  while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

// One block per 64 x 16 output tile of one image: the tile and its 4-pixel halo are staged in LDS once; the flip copies
// the tile's centre mirrored, the blur filters rows then columns.  Images may differ in raw size (grid = the largest).
__global__ __launch_bounds__(256) void augment_u8_kernel(AugArgs a) {
  constexpr int LW = AUG_TX + 2 * AUG_R, LH = AUG_TY + 2 * AUG_R;
  __shared__ uint8_t tile[LH][LW * 3];
  __shared__ int rowp[LH][AUG_TX * 3];
  const PreGeo g = a.geo[blockIdx.z];
  const int x0 = blockIdx.x * AUG_TX, y0 = blockIdx.y * AUG_TY;
  if (x0 >= g.w || y0 >= g.h) return;                  // (block-uniform)
  const uint8_t* src = a.img + g.off;
  for (int e = threadIdx.x; e < LH * LW; e += blockDim.x) {
    const int ly = e / LW, lx = e - ly * LW;
    const int sy = reflect101(y0 + ly - AUG_R, g.h), sx = reflect101(x0 + lx - AUG_R, g.w);
    const uint8_t* p = src + ((size_t)sy * g.w + sx) * 3;
    tile[ly][lx * 3 + 0] = p[0];
    tile[ly][lx * 3 + 1] = p[1];
    tile[ly][lx * 3 + 2] = p[2];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < LH * AUG_TX * 3; e += blockDim.x) {
    const int ly = e / (AUG_TX * 3), r = e - ly * (AUG_TX * 3);
    int s = 0;
#pragma unroll
    for (int i = -AUG_R; i <= AUG_R; ++i) s += blur_tap(i) * (int)tile[ly][r + (AUG_R + i) * 3];
    rowp[ly][r] = s;
  }
  __syncthreads();
  uint8_t* flip = a.img + a.variant_stride + g.off;
  uint8_t* blur = a.img + 2 * a.variant_stride + g.off;
  for (int e = threadIdx.x; e < AUG_TY * AUG_TX * 3; e += blockDim.x) {
    const int ly = e / (AUG_TX * 3), r = e - ly * (AUG_TX * 3);
    const int lx = r / 3, ch = r - lx * 3;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= g.h || x >= g.w) continue;
    int s = 0;
#pragma unroll
    for (int j = -AUG_R; j <= AUG_R; ++j) s += blur_tap(j) * rowp[ly + AUG_R + j][r];
    blur[((size_t)y * g.w + x) * 3 + ch] = (uint8_t)((s + 32768) >> 16);
    flip[((size_t)y * g.w + (g.w - 1 - x)) * 3 + ch] = tile[ly + AUG_R][(lx + AUG_R) * 3 + ch];
  }
}

void launch_augment_u8(const AugArgs& a, int max_h, int max_w, hipStream_t s) {
  const dim3 grid((unsigned)((max_w + AUG_TX - 1) / AUG_TX), (unsigned)((max_h + AUG_TY - 1) / AUG_TY), (unsigned)a.n);
  hipLaunchKernelGGL(augment_u8_kernel, grid, dim3(256), 0, s, a);
}

// ------------------------------------------------------------------------------------ consistency check: scores
// Per original image (one block) and detection rank k (one thread), against all M rows of each variant, padded rows included
// (infer_model.py:811-827): the flip variant's boxes are un-flipped to [y1, W - x2, y2, W - x1] in float32 (W = raw width);
// IoU = calc_iou_np (utils_box.py:56-89): float32 coordinate differences, float64 products, union = (areaA + areaB) - inter,
// 0 where the union is 0; cons_iou = ((max_flip + max_blur) + max_noise) / 3 in float64 (np.mean of three);
// cons_cls = np.mean of the three variants' classes at rank k in float32 .is_integer() - the original's class is not
// consulted (the reference's rank-wise comparison, reproduced as it is).
__device__ __forceinline__ double iou_np(const float* a, const float* b) {
  const float yA = fmaxf(a[0], b[0]), xA = fmaxf(a[1], b[1]);
  const float yB = fminf(a[2], b[2]), xB = fminf(a[3], b[3]);
  const double inter = (double)fmaxf(0.0f, xB - xA) * (double)fmaxf(0.0f, yB - yA);
  const double areaA = (double)fabsf(a[3] - a[1]) * (double)fabsf(a[2] - a[0]);
  const double areaB = (double)fabsf(b[3] - b[1]) * (double)fabsf(b[2] - b[0]);
  const double uni = (areaA + areaB) - inter;
  return uni != 0.0 ? inter / uni : 0.0;
}

__global__ __launch_bounds__(128) void consistency_kernel(ConsArgs a) {
  __shared__ float vb[3][128][4];
  const int i = blockIdx.x, k = threadIdx.x, M = a.M;
  const float W = (float)a.geo[i].w;
  for (int e = k; e < 3 * M; e += blockDim.x) {
    const int v = e / M, j = e - v * M;
    const float* b = a.boxes + ((size_t)(v + 1) * a.n + i) * M * a.bc + (size_t)j * a.bc;
    if (v == 0) {
      vb[0][j][0] = b[0]; vb[0][j][1] = W - b[3]; vb[0][j][2] = b[2]; vb[0][j][3] = W - b[1];
    } else {
      for (int q = 0; q < 4; ++q) vb[v][j][q] = b[q];
    }
  }
  __syncthreads();
  if (k >= M) return;
  const float* ob = a.boxes + ((size_t)i * M + k) * a.bc;
  const float box[4] = {ob[0], ob[1], ob[2], ob[3]};
  double best[3];
  for (int v = 0; v < 3; ++v) {
    double m = iou_np(box, vb[v][0]);
    for (int j = 1; j < M; ++j) m = fmax(m, iou_np(box, vb[v][j]));
    best[v] = m;
  }
  a.iou[(size_t)i * M + k] = ((best[0] + best[1]) + best[2]) / 3.0;
  float cls[3];
  for (int v = 0; v < 3; ++v) cls[v] = a.classes[(((size_t)(v + 1) * a.n + i) * M + k) * a.cc];
  const float mean = ((cls[0] + cls[1]) + cls[2]) / 3.0f;
  a.agree[(size_t)i * M + k] = (uint8_t)(isfinite(mean) && mean == truncf(mean));
}

void launch_consistency(const ConsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(consistency_kernel, dim3((unsigned)a.n), dim3(128), 0, s, a);
}

// ------------------------------------------------------------------------------------ ground-truth assignment
// gt_box_assigner (utils_extra.py:44-64) for every kept ground-truth row of every image.  One block per image; the image's M
// detection boxes are staged in LDS once; a wave owns GT rows wave, wave + waves, ... and its lanes stride over the M ranks.
//   IoU  argmax_k calc_iou_np(gt, box_k) (iou_np above), all M rows, padded ones included
//   MSE  argmin_k np.mean(np.square(gt - box_k)) in float32: differences, squares, ((s0 + s1) + s2) + s3 (numpy's order for a
//        4-element inner axis), times 0.25f (= / 4 exactly); no contraction in this file
//   else rank i itself (the reference's else branch); a kept row i >= M raises *err, and so does any kept row when M == 0
// np.argmax / np.argmin return the first occurrence: a candidate replaces the best one only when its key is strictly better, or
// equal with a lower rank - in the lane's own sweep and in every step of the wave reduction alike, so the winner is the
// lexicographic best of (key, rank) however the ranks were dealt to lanes.  This decides real cases: padded slots carry row
// 0's box, and a GT box that overlaps nothing has IoU 0 with every row.
// Kept rows: ASSIGN_KEEP_VALIDATE class > 0 (validate_model.py:314); ASSIGN_KEEP_CALIBRATE row < min(G, M) and class >= 0
// (calibrate_model.py:133-135).  Outputs: det_index (-1: not kept), iou = calc_iou_np(gt, matched box) whatever the method
// (0: not kept), count = kept rows of the image.
__device__ __forceinline__ bool gt_row_kept(float cls, int g, int M, int keep) {
  return keep == ASSIGN_KEEP_CALIBRATE ? (g < M && cls >= 0.0f) : cls > 0.0f;
}

__device__ __forceinline__ float mse_np(const float* a, const float* b) {
  const float d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2], d3 = a[3] - b[3];
  return (((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3) * 0.25f;
}

__global__ __launch_bounds__(256) void assign_gt_kernel(AssignArgs a) {
  extern __shared__ float det[];           // [M][4]
  __shared__ int kept_rows;
  const int i = blockIdx.x, M = a.M, G = a.G;
  if (threadIdx.x == 0) kept_rows = 0;
  for (int e = threadIdx.x; e < M * 4; e += blockDim.x) det[e] = a.det_boxes[((size_t)i * M + (e >> 2)) * a.det_stride + (e & 3)];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  int mine = 0;
  for (int g = wave; g < G; g += waves) {                 // (wave-uniform: the shuffles below see all 64 lanes)
    const size_t row = (size_t)i * G + g;
    const float* gp = a.gt_boxes + row * 4;
    const float gt[4] = {gp[0], gp[1], gp[2], gp[3]};
    if (!gt_row_kept(a.gt_classes[row], g, M, a.keep)) {
      if (lane == 0) { a.det_index[row] = -1; a.iou[row] = 0.0; }
      continue;
    }
    int best = 0x7fffffff;
    if (a.method == ASSIGN_IOU) {
      double key = -1.0;                                   // below every IoU
      for (int k = lane; k < M; k += 64) {
        const double v = iou_np(gt, det + k * 4);
        if (v > key) { key = v; best = k; }               // (k ascends: an equal key never replaces a lower rank)
      }
      wave_best_max(key, best);
    } else if (a.method == ASSIGN_MSE) {
      float key = __builtin_inff();
      for (int k = lane; k < M; k += 64) {
        const float v = mse_np(gt, det + k * 4);
        if (v < key || best == 0x7fffffff) { key = v; best = k; }
      }
      for (int o = 32; o > 0; o >>= 1) {
        const float ok = __shfl_xor(key, o);
        const int ob = __shfl_xor(best, o);
        if (ob != 0x7fffffff && (best == 0x7fffffff || ok < key || (ok == key && ob < best))) { key = ok; best = ob; }
      }
    } else {
      best = g;
    }
    if (lane == 0) {
      if (best >= M) {                                     // rank branch beyond the detections, or no detection at all (M == 0)
        *a.err = 1;
        best = 0;
      }
      a.det_index[row] = best;
      a.iou[row] = M > 0 ? iou_np(gt, det + best * 4) : 0.0;
      ++mine;
    }
  }
  if (lane == 0 && mine) atomicAdd(&kept_rows, mine);
  __syncthreads();
  if (threadIdx.x == 0) a.count[i] = kept_rows;
}

void launch_assign_gt(const AssignArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(assign_gt_kernel, dim3((unsigned)a.n), dim3(256), (size_t)a.M * 4 * sizeof(float), s, a);
}

// The matched rows as one compact float32 table, K = sum(count) rows in (image, GT row) order - the order the reference
// appends in (validate_model.py:314-470).  Row = the matched detection's box columns (box 4, then aleatoric / MC std as the
// configuration has them) | score | class columns (id, then the MC std of the logits) | logits C | probab C | entropy (the
// last three when the handle has logits).  The values are copied as they are: the reference's nan_to_num of the uncertainty
// columns (validate_model.py:176-196) is done by the host that splits the table (infer_lib.split_assigned_rows).
// One block per image: its row offset is the exclusive scan of count (n is at most a few dozen), the kept rows are ranked by
// the first wave with ballots.
__global__ __launch_bounds__(256) void gather_assigned_kernel(AssignRowsArgs a) {
  extern __shared__ int src_g[];           // [G] GT row of the image's r-th kept row
  __shared__ int row0;
  const int i = blockIdx.x, G = a.G, M = a.M;
  if (threadIdx.x == 0) {
    int s = 0;
    for (int j = 0; j < i; ++j) s += a.count[j];
    row0 = s;
  }
  if (threadIdx.x < 64) {
    int run = 0;
    for (int base = 0; base < G; base += 64) {            // (wave-uniform trip count)
      const int g = base + (int)threadIdx.x;
      const bool kept = g < G && a.det_index[(size_t)i * G + g] >= 0;
      const unsigned long long m = __ballot(kept);
      if (kept) src_g[run + __popcll(m & ((1ull << threadIdx.x) - 1ull))] = g;
      run += __popcll(m);
    }
  }
  __syncthreads();
  const int cnt = a.count[i], W = a.cols;
  const int sc0 = a.bc, cl0 = sc0 + 1, lg0 = cl0 + a.cc, pr0 = lg0 + a.C, en0 = pr0 + a.C;
  for (int e = threadIdx.x; e < cnt * W; e += blockDim.x) {
    const int r = e / W, col = e - r * W;
    const size_t d = (size_t)i * M + a.det_index[(size_t)i * G + src_g[r]];
    float v;
    if (col < sc0) v = a.boxes[d * a.bc + col];
    else if (col < cl0) v = a.scores[d];
    else if (col < lg0) v = a.classes[d * a.cc + (col - cl0)];
    else if (col < pr0) v = a.logits[d * a.C + (col - lg0)];
    else if (col < en0) v = a.probs[d * a.C + (col - pr0)];
    else v = a.entropy[d];
    a.rows[((size_t)row0 + r) * W + col] = v;
  }
}

void launch_gather_assigned(const AssignRowsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(gather_assigned_kernel, dim3((unsigned)a.n), dim3(256), (size_t)(a.G > 0 ? a.G : 1) * sizeof(int), s, a);
}

// ------------------------------------------------------------------------------------ active-learning image scores
// ActiveLearning.score_image (active_learning_loop.py:528-733) without the text file in between: per kept detection one to three
// uncertainty numbers, per image their mean or max.  One block of 256 threads per image over all M rows; a row is kept iff
// score > min_score in the input type (np.where(scores[0] > min_score), infer_model.py:836; padded rows score 0).
// A component of a row is w0 * term0 (+ w1 * term1, the `combo` strategy); a term is a source under a transform (uda_hip.h).
// Every input is converted to double first.  The float instantiation cleans ALBOX / MCBOX / MCCLASS as np.nan_to_num does in
// float32 (infer_model.py:607-631) before that; the double one reads the caller's columns as they are.
// The sums of a row follow numpy's add.reduce of a contiguous float64 vector (sum_np) - np.mean of the 4 relativized entries
// and of the C class stds.
// The reduction over the rows has a fixed order: the thread's rows ascending, an xor butterfly inside the wave, the four waves
// in wave order through LDS; NaN wins every max, as in np.max.  No float atomics: class_counts are integer LDS adds.
__device__ __forceinline__ double score_in(float v) {
  if (v != v) return 0.0;
  if (v == __builtin_inff()) return (double)3.402823466e+38f;
  if (v == -__builtin_inff()) return -(double)3.402823466e+38f;
  return (double)v;
}
__device__ __forceinline__ double score_in(double v) { return v; }

// np.add.reduce over the contiguous float64 vector v[0 .. n), n <= 128: numpy's pairwise_sum - sequential below 8 elements, 8
// running sums combined as a tree above, the n % 8 last elements added one by one.  (Beyond 128 elements numpy splits the
// vector in halves first; this keeps the 8 running sums, which differs by rounding only.)
template <typename T>
__device__ double sum_np(const T* v, int n) {
  if (n < 8) {
    double res = score_in(v[0]);
    for (int i = 1; i < n; ++i) res += score_in(v[i]);
    return res;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = score_in(v[j]);
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += score_in(v[i + j]);
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += score_in(v[i]);
  return res;
}

template <typename T>
__device__ double score_term(const ScoreArgs<T>& a, size_t row, int source, int transform) {
  if (source == UDA_SCORE_ENTROPY) return (double)a.entropy[row];
  if (source == UDA_SCORE_DET_SCORE) return (double)a.scores[row];
  if (source == UDA_SCORE_MCCLASS) return sum_np(a.mcclass + row * a.mcc_stride, a.mcc_w) / (double)a.mcc_w;
  const T* u = source == UDA_SCORE_ALBOX ? a.albox + row * a.al_stride : a.mcbox + row * a.mc_stride;
  double v[4] = {score_in(u[0]), score_in(u[1]), score_in(u[2]), score_in(u[3])};
  if (transform == UDA_SCORE_REL_MEAN) {
    const T* b = a.boxes + row * a.box_stride;
    const double h = (double)b[2] - (double)b[0], w = (double)b[3] - (double)b[1];
    v[0] /= h; v[1] /= w; v[2] /= h; v[3] /= w;
  }
  return sum_np(v, 4) / 4.0;
}

// component k of a row: w0 * term0 (+ w1 * term1) - the one place both the image scores and the pseudo-labelling rows build it
template <typename T>
__device__ __forceinline__ double score_component(const ScoreArgs<T>& a, size_t row, int k) {
  const uda_score_term_t* t = a.desc.term[k];
  double v = t[0].weight * score_term(a, row, t[0].source, t[0].transform);
  if (a.desc.n_terms[k] > 1) v = v + t[1].weight * score_term(a, row, t[1].source, t[1].transform);
  return v;
}

__device__ __forceinline__ double max_np(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

template <typename T>
__global__ __launch_bounds__(256) void score_images_kernel(ScoreArgs<T> a) {
  extern __shared__ int cls_cnt[];         // [C]
  __shared__ double wave_acc[4][UDA_SCORE_MAX_COMP];
  __shared__ int wave_cnt[4];
  const int i = blockIdx.x, M = a.M, C = a.C, nc = a.desc.n_comp;
  const bool mean = a.desc.reduce_mean != 0;
  for (int c = threadIdx.x; c < C; c += blockDim.x) cls_cnt[c] = 0;
  __syncthreads();
  double acc[UDA_SCORE_MAX_COMP];
  for (int k = 0; k < UDA_SCORE_MAX_COMP; ++k) acc[k] = mean ? 0.0 : -(double)__builtin_inff();
  int cnt = 0;
  for (int r = threadIdx.x; r < M; r += blockDim.x) {
    const size_t row = (size_t)i * M + r;
    if (!(a.scores[row] > a.min_score)) continue;
    ++cnt;
    const double cid = (double)a.classes[row * a.cls_stride];
    const int ci = cid >= 1.0 && cid <= (double)C ? (int)cid : 0;
    if (ci < 1 || (double)ci != cid) *a.err = 1;
    else atomicAdd(&cls_cnt[ci - 1], 1);
#pragma unroll
    for (int k = 0; k < UDA_SCORE_MAX_COMP; ++k) {         // (unrolled: acc stays in registers)
      if (k >= nc) break;
      const double v = score_component(a, row, k);
      acc[k] = mean ? acc[k] + v : max_np(acc[k], v);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    for (int k = 0; k < UDA_SCORE_MAX_COMP; ++k) {
      const double other = __shfl_xor(acc[k], o);
      acc[k] = mean ? acc[k] + other : max_np(acc[k], other);
    }
    cnt += __shfl_xor(cnt, o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    for (int k = 0; k < UDA_SCORE_MAX_COMP; ++k) wave_acc[wave][k] = acc[k];
    wave_cnt[wave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = (wave_cnt[0] + wave_cnt[1]) + (wave_cnt[2] + wave_cnt[3]);
    for (int k = 0; k < nc; ++k) {
      double v = wave_acc[0][k];
      for (int w = 1; w < 4; ++w) v = mean ? v + wave_acc[w][k] : max_np(v, wave_acc[w][k]);
      a.comp[(size_t)i * nc + k] = total ? (mean ? v / (double)total : v) : 0.0;
    }
    a.count[i] = total;
  }
  for (int c = threadIdx.x; c < C; c += blockDim.x) a.class_counts[(size_t)i * C + c] = cls_cnt[c];
}

template <typename T>
static void launch_score_images_t(const ScoreArgs<T>& a, hipStream_t s) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(score_images_kernel<T>, dim3((unsigned)a.n), dim3(256), (size_t)(a.C > 0 ? a.C : 1) * sizeof(int), s, a);
}
void launch_score_images(const ScoreArgs<float>& a, hipStream_t s) { launch_score_images_t(a, s); }
void launch_score_images(const ScoreArgs<double>& a, hipStream_t s) { launch_score_images_t(a, s); }

// ------------------------------------------------------------------------------------ pseudo-labelling rows
// STAC.score_image (SSL_stac.py:302-642) up to its dataset-wide normalisation, without the text file in between: the per-row form
// of the image scores above.  One block of 256 threads per image walks the M rows in chunks of 256, row r of a chunk on thread r.
//   kept         score > min_score in the input type (the writer's filter); its rank among the image's kept rows is an exclusive
//                scan of the flags: ballot + popcount inside a wave, the four wave totals through LDS, a running base over chunks
//   takes part   rank < max_rows (the reference's [:99])
//   v            the descriptor's one component, or 1 / (((c0 + c1) [+ c2]) / n_comp) - np.mean over axis 0, then the divide
//   candidate    det_score > tau (gate 0) or v > tau (gate 1), float64; ranked by a second scan of the same shape
// Two barriers per chunk are enough: a chunk's kept totals are read between its two barriers and written again only after the
// second, its candidate totals are read before the next chunk's first barrier and written again only after it.  min / max over the rows that
// take part: b < a / b > a never takes a NaN b (the reference's running min(global_min, item)); a thread's rows ascending, an xor
// butterfly in the wave, the waves in wave order.  No float atomics.  The candidates go to the image's `cap` slots; the packing
// kernel moves them behind the candidates of the images before (the order the reference appends in).
template <typename T>
__global__ __launch_bounds__(256) void pseudo_rows_kernel(PseudoArgs<T> a) {
  __shared__ int kept_tot[4], cand_tot[4];
  __shared__ double wave_min[4], wave_max[4];
  const int i = blockIdx.x, M = a.s.M, C = a.s.C, nc = a.s.desc.n_comp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  int kept_base = 0, cand_base = 0;
  double vmin = (double)__builtin_inff(), vmax = -(double)__builtin_inff();
  for (int r0 = 0; r0 < M; r0 += 256) {      // (uniform trip count: every thread reaches the ballots and barriers)
    const int r = r0 + (int)threadIdx.x;
    const size_t row = (size_t)i * M + (r < M ? r : 0);
    const bool kept = r < M && a.s.scores[row] > a.s.min_score;
    const unsigned long long km = __ballot(kept);
    if (lane == 0) kept_tot[wave] = __popcll(km);
    __syncthreads();
    int rank = kept_base + __popcll(km & below);
    for (int w = 0; w < wave; ++w) rank += kept_tot[w];
    kept_base += (kept_tot[0] + kept_tot[1]) + (kept_tot[2] + kept_tot[3]);
    const bool part = kept && rank < a.max_rows;
    double v = 0.0;
    bool cand = false;
    if (part) {
      if (a.invert) {
        double sum = score_component(a.s, row, 0) + score_component(a.s, row, 1);
        if (nc > 2) sum = sum + score_component(a.s, row, 2);
        v = 1.0 / (sum / (double)nc);
      } else {
        v = score_component(a.s, row, 0);
      }
      vmin = v < vmin ? v : vmin;
      vmax = v > vmax ? v : vmax;
      cand = a.gate ? v > a.tau : (double)a.s.scores[row] > a.tau;
    }
    const unsigned long long cm = __ballot(cand);
    if (lane == 0) cand_tot[wave] = __popcll(cm);
    __syncthreads();
    int slot = cand_base + __popcll(cm & below);
    for (int w = 0; w < wave; ++w) slot += cand_tot[w];
    cand_base += (cand_tot[0] + cand_tot[1]) + (cand_tot[2] + cand_tot[3]);
    if (cand && slot < a.cap) {                              // (slot <= rank < min(M, max_rows) = cap: always true)
      const double cid = (double)a.s.classes[row * a.s.cls_stride];
      const int ci = cid >= 1.0 && cid <= (double)C ? (int)cid : 0;
      if (ci < 1 || (double)ci != cid) *a.s.err = 1;
      const T* b = a.s.boxes + row * a.s.box_stride;
      PseudoRecord rec;
      rec.image = i; rec.row = r;
      rec.box[0] = (float)b[0]; rec.box[1] = (float)b[1]; rec.box[2] = (float)b[2]; rec.box[3] = (float)b[3];
      rec.det_score = (float)a.s.scores[row];
      rec.cls = ci;
      rec.v = v;
      a.slots[(size_t)i * a.cap + slot] = rec;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double lo = __shfl_xor(vmin, o), hi = __shfl_xor(vmax, o);
    vmin = lo < vmin ? lo : vmin;
    vmax = hi > vmax ? hi : vmax;
  }
  if (lane == 0) { wave_min[wave] = vmin; wave_max[wave] = vmax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double lo = wave_min[0], hi = wave_max[0];
    for (int w = 1; w < 4; ++w) {
      lo = wave_min[w] < lo ? wave_min[w] : lo;
      hi = wave_max[w] > hi ? wave_max[w] : hi;
    }
    a.minmax[2 * (size_t)i] = lo; a.minmax[2 * (size_t)i + 1] = hi;
    a.kept[i] = kept_base; a.cand[i] = cand_base;
  }
}

// records of image i -> records[sum(cand[0 .. i)) ...]: one block per image; the offset is an integer sum in a fixed order
__global__ __launch_bounds__(256) void pseudo_pack_kernel(const int32_t* cand, const PseudoRecord* slots, PseudoRecord* records, int cap) {
  __shared__ int wave_sum[4];
  const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int off = 0;
  for (int k = threadIdx.x; k < i; k += 256) off += cand[k];
  for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o);
  if (lane == 0) wave_sum[wave] = off;
  __syncthreads();
  off = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
  const int words = (cand[i] < cap ? cand[i] : cap) * (int)(sizeof(PseudoRecord) / sizeof(int32_t));
  const int32_t* src = (const int32_t*)(slots + (size_t)i * cap);
  int32_t* dst = (int32_t*)(records + off);
  for (int w = threadIdx.x; w < words; w += 256) dst[w] = src[w];
}

template <typename T>
static void launch_pseudo_rows_t(const PseudoArgs<T>& a, hipStream_t s) {
  if (a.s.n <= 0) return;
  hipLaunchKernelGGL(pseudo_rows_kernel<T>, dim3((unsigned)a.s.n), dim3(256), 0, s, a);
  hipLaunchKernelGGL(pseudo_pack_kernel, dim3((unsigned)a.s.n), dim3(256), 0, s, a.cand, a.slots, a.records, a.cap);
}
void launch_pseudo_rows(const PseudoArgs<float>& a, hipStream_t s) { launch_pseudo_rows_t(a, s); }
void launch_pseudo_rows(const PseudoArgs<double>& a, hipStream_t s) { launch_pseudo_rows_t(a, s); }

// ------------------------------------------------------------------------------------ COCO matching
// COCOeval_all.evaluateImg (custom_cocoeval.py:265-349) at maxDets[-1] = 100 for the containers EvaluationMetric.update_state
// builds (coco_metric.py:219-283).  One block of two waves per (image, class id c in 1..C):
//   wave 0 compacts the rows of class c in row order (ballots) and counts the image's used rows (class > -1, :235); a row's
//          category is int(class) as loadNumpyAnnotations takes it, so c <= class < c + 1
//   wave 1 compacts the ground-truth rows of class c: box [x1, y1, x2 - x1, y2 - y1] and area (x2 - x1) * (y2 - y1) in float32
//          (:258-270; the area column is not read), crowd = int(is_crowd) != 0, ignore per area range = crowd or area outside
//          [lo, hi], both ends inclusive
//   rank   of a row = #{j : s_j > s_i or (s_j == s_i and j < i)} among the class's rows: the stable argsort of -score (:289).
//          Ranks below 100 are staged with box and area = float32 w * h (what pycocotools' loadRes computes on the float32 rows;
//          stated from knowledge of pycocotools, which the reference imports but does not contain)
//   order  per area range: non-ignored rows first, stable (:287)
//   scan   thread p = area * T + t walks the ranked detections and, per detection, the ground truth in that order (:307-330);
//          IoUs are recomputed from the staged boxes in float64 (pycocotools bbIou; no contraction in this file); its
//          "ground truth taken" bits live in a column of LDS words of its own; matched / ignored bits meet in LDS words per
//          (area, detection) through integer OR, which has no order to depend on
// Every detection row gets exactly one record: from its class's block, or from the block of class 1 when it is unused or its
// class lies outside 1..C (rank -1).  Rows of rank >= 100 keep their rank and carry zero masks.
__device__ __forceinline__ double bb_iou(const float* d, const float* g, bool crowd) {
  const double dx = d[0], dy = d[1], dw = d[2], dh = d[3], gx = g[0], gy = g[1], gw = g[2], gh = g[3];
  const double w = fmin(dw + dx, gw + gx) - fmax(dx, gx);
  if (w <= 0.0) return 0.0;
  const double h = fmin(dh + dy, gh + gy) - fmax(dy, gy);
  if (h <= 0.0) return 0.0;
  const double i = w * h, da = dw * dh, ga = gw * gh;
  const double u = crowd ? da : da + ga - i;
  return i / u;
}

__device__ __forceinline__ bool coco_area_out(float area, int ar) {
  const double lo = ar < 2 ? 0.0 : (ar == 2 ? 1024.0 : 9216.0), hi = ar == 1 ? 1024.0 : (ar == 2 ? 9216.0 : 1e10);
  return (double)area < lo || (double)area > hi;
}

__device__ __forceinline__ int coco_class_field(float k) {
  return !(k > -1.0f) ? -1 : (k < 2147483520.0f ? (int)k : 2147483647);
}

__device__ __forceinline__ void coco_write(uda_eval_record_t* o, float score, int cls, int rank, const unsigned* mm, const unsigned* im) {
  o->score = score; o->cls = cls; o->rank = rank;
  for (int k = 0; k < 4; ++k) { o->matched[k] = mm ? mm[k] : 0u; o->ignored[k] = im ? im[k] : 0u; }
}

template <bool LEGACY>
__global__ __launch_bounds__(128) void coco_match_kernel(CocoMatchArgs a) {
  __shared__ float sc[COCO_MAX_M];                 // score of the class's r-th row
  __shared__ unsigned short row[COCO_MAX_M];       // its row in the image
  __shared__ float dbox[COCO_MAX_DET][4], darea[COCO_MAX_DET], dscore[COCO_MAX_DET];
  __shared__ unsigned short drow[COCO_MAX_DET];
  __shared__ float gbox[COCO_MAX_G][4];
  __shared__ unsigned char gflag[COCO_MAX_G];      // bit ar: ignored in area range ar; bit 4: crowd
  __shared__ unsigned short order[4][COCO_MAX_G];
  __shared__ unsigned taken[COCO_MAX_G / 32][128];
  __shared__ unsigned mm[COCO_MAX_DET][4], im[COCO_MAX_DET][4];
  __shared__ int s_mc, s_gc, s_used;
  const int i = blockIdx.x / a.C, c = blockIdx.x % a.C + 1;
  const int M = a.M, G = a.G, T = a.T, tid = threadIdx.x;
  const float clo = (float)c, chi = (float)(c + 1);
  const size_t r0 = (size_t)i * M;
  auto cls_of = [&](int r) { return LEGACY ? a.rows[(r0 + r) * 7 + 6] : a.classes[(r0 + r) * a.cls_stride]; };
  auto score_of = [&](int r) { return LEGACY ? a.rows[(r0 + r) * 7 + 5] : a.scores[r0 + r]; };

  if (tid < 64) {                                  // (wave-uniform branch: the ballots below see whole waves)
    int run = 0, used = 0;
    for (int base = 0; base < M; base += 64) {
      const int r = base + tid;
      const float k = r < M ? cls_of(r) : -1.0f;
      const bool u = r < M && k > -1.0f;
      const bool mine = u && k >= clo && k < chi;
      const unsigned long long bm = __ballot(mine);
      if (mine) {
        const int p = run + __popcll(bm & ((1ull << tid) - 1ull));
        row[p] = (unsigned short)r;
        sc[p] = score_of(r);
      }
      run += __popcll(bm);
      used += __popcll(__ballot(u));
    }
    if (tid == 0) { s_mc = run; s_used = used; }
  } else {
    const int lane = tid - 64;
    int run = 0;
    for (int base = 0; base < G; base += 64) {
      const int g = base + lane;
      const float* gp = a.gt + ((size_t)i * G + (g < G ? g : 0)) * 7;
      const float k = g < G ? gp[6] : -1.0f;
      const bool mine = g < G && k > -1.0f && k >= clo && k < chi;
      const unsigned long long bm = __ballot(mine);
      if (mine) {
        const int p = run + __popcll(bm & ((1ull << lane) - 1ull));
        const float w = gp[3] - gp[1], h = gp[2] - gp[0];
        gbox[p][0] = gp[1]; gbox[p][1] = gp[0]; gbox[p][2] = w; gbox[p][3] = h;
        const float area = w * h;
        const bool crowd = gp[4] >= 1.0f || gp[4] <= -1.0f;      // int(is_crowd) != 0
        unsigned f = crowd ? 0x1fu : 0u;
        for (int ar = 0; ar < 4; ++ar)
          if (coco_area_out(area, ar)) f |= 1u << ar;
        gflag[p] = (unsigned char)f;
      }
      run += __popcll(bm);
    }
    if (lane == 0) s_gc = run;
  }
  for (int e = tid; e < COCO_MAX_DET * 4; e += 128) { (&mm[0][0])[e] = 0u; (&im[0][0])[e] = 0u; }
  for (int w = 0; w < COCO_MAX_G / 32; ++w) taken[w][tid] = 0u;
  __syncthreads();
  const int mc = s_mc, gc = s_gc, D = mc < COCO_MAX_DET ? mc : COCO_MAX_DET;

  if (tid < 4) {                                   // non-ignored rows first, stable; their count is npig
    int p = 0;
    for (int g = 0; g < gc; ++g)
      if (!((gflag[g] >> tid) & 1)) order[tid][p++] = (unsigned short)g;
    a.npig[((size_t)i * a.C + (c - 1)) * 4 + tid] = p;
    for (int g = 0; g < gc; ++g)
      if ((gflag[g] >> tid) & 1) order[tid][p++] = (unsigned short)g;
  }
  for (int r = tid; r < mc; r += 128) {
    const float s = sc[r];
    int rank = 0;
    for (int j = 0; j < mc; ++j) {
      const float t = sc[j];
      rank += (t > s || (t == s && j < r)) ? 1 : 0;
    }
    const int R = row[r];
    if (rank < COCO_MAX_DET) {
      float x, y, w, h;
      if (LEGACY) {
        const float* p = a.rows + (r0 + R) * 7;
        x = p[1]; y = p[2]; w = p[3]; h = p[4];
      } else {
        const float* p = a.boxes + (r0 + R) * a.box_stride;
        x = p[1]; y = p[0]; w = p[3] - p[1]; h = p[2] - p[0];     // transform_detections, float32
      }
      dbox[rank][0] = x; dbox[rank][1] = y; dbox[rank][2] = w; dbox[rank][3] = h;
      darea[rank] = w * h;
      dscore[rank] = s;
      drow[rank] = (unsigned short)R;
    } else {
      coco_write(a.rec + r0 + R, s, c, rank, nullptr, nullptr);
    }
  }
  __syncthreads();

  if (tid < 4 * T) {
    const int ar = tid / T, t = tid - ar * T;
    const double start = fmin(a.thr[t], 1.0 - 1e-10);
    for (int d = 0; d < D; ++d) {
      double best = start;
      int m = -1;
      bool m_ig = false;
      for (int gi = 0; gi < gc; ++gi) {
        const int g = order[ar][gi];
        const unsigned f = gflag[g];
        const bool ig = (f >> ar) & 1, crowd = (f >> 4) & 1;
        if (((taken[g >> 5][tid] >> (g & 31)) & 1u) && !crowd) continue;
        if (m >= 0 && !m_ig && ig) break;
        const double v = bb_iou(dbox[d], gbox[g], crowd);
        if (v < best) continue;
        best = v; m = g; m_ig = ig;
      }
      bool ign;
      if (m < 0) {
        ign = coco_area_out(darea[d], ar);
      } else {
        taken[m >> 5][tid] |= 1u << (m & 31);
        atomicOr(&mm[d][ar], 1u << t);
        ign = m_ig;
      }
      if (ign) atomicOr(&im[d][ar], 1u << t);
    }
  }
  __syncthreads();
  for (int d = tid; d < D; d += 128) coco_write(a.rec + r0 + drow[d], dscore[d], c, d, mm[d], im[d]);

  if (c == 1) {                                    // the rows no class's block owns
    for (int r = tid; r < M; r += 128) {
      const float k = cls_of(r);
      if (!(k > -1.0f && k >= 1.0f && k < (float)(a.C + 1))) coco_write(a.rec + r0 + r, score_of(r), coco_class_field(k), -1, nullptr, nullptr);
    }
    if (tid == 0) a.used[i] = s_used;
  }
}

void launch_coco_match(const CocoMatchArgs& a, hipStream_t s) {
  if (a.n <= 0 || a.C <= 0) return;
  const dim3 grid((unsigned)a.n * (unsigned)a.C);
  if (a.legacy)
    hipLaunchKernelGGL(coco_match_kernel<true>, grid, dim3(128), 0, s, a);
  else
    hipLaunchKernelGGL(coco_match_kernel<false>, grid, dim3(128), 0, s, a);
}

// ------------------------------------------------------------------------------------ thresholding: batched ROC objective
// roc_metrics(sum(param * uncert), (ious >= iou_thr) * tps_class) of the reference (uncertainty_analysis.py:44-152) for a chunk of
// candidate weight vectors.  The order of a candidate's combined score does not depend on the IoU threshold, so a candidate is
// sorted once (bitonic network on (key, row): tiles of THR_TILE in LDS, the wider strides in global memory) and its K curves are
// scans over that order.  Counts are integers, the few float64 operations are the reference's, in its order (this file is built
// with FMA contraction off).
enum { THR_SORT_THREADS = THR_TILE / 2, THR_CURVE_THREADS = 512 };

__global__ void __launch_bounds__(256) thr_mask_kernel(ThrArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  const double iou = a.ious[i];
  const bool tp = a.tp_class[i] != 0;
  uint32_t m = 0;
  for (int k = 0; k < a.K; ++k) m |= (uint32_t)(tp && iou >= a.thr[k]) << k;
  a.mask[i] = m;
}

// ~(bits that order like the value): an ascending sort of the key is a descending sort of the score
__device__ __forceinline__ uint64_t thr_key_of(double u) {
  if (u == 0.0) u = 0.0;     // -0.0 and 0.0 are one value
  const uint64_t b = (uint64_t)__double_as_longlong(u);
  return ~(b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull));
}
__device__ __forceinline__ double thr_score_of(uint64_t key) {
  const uint64_t o = ~key;
  return __longlong_as_double((long long)(o ^ ((o >> 63) ? 0x8000000000000000ull : ~0ull)));
}

// compare-exchange steps k, j = j0 .. 1 of the bitonic network on one tile held in LDS; `base` is the tile's first position
__device__ __forceinline__ void thr_tile_steps(uint64_t* sk, int32_t* si, int base, int k, int j0) {
  const int t = threadIdx.x;
  for (int j = j0; j > 0; j >>= 1) {
    const int i = 2 * t - (t & (j - 1)), l = i + j;
    const bool asc = ((base + i) & k) == 0;
    const uint64_t x = sk[i], y = sk[l];
    if ((x > y) == asc) {
      sk[i] = y; sk[l] = x;
      const int32_t r = si[i]; si[i] = si[l]; si[l] = r;
    }
    __syncthreads();
  }
}

// combined score of the tile's rows -> keys, then the tile sorted (ascending or descending by its place in the network)
__global__ void __launch_bounds__(THR_SORT_THREADS) thr_sort_tile_kernel(ThrArgs a) {
  __shared__ uint64_t sk[THR_TILE];
  __shared__ int32_t si[THR_TILE];
  const int base = blockIdx.x * THR_TILE, p = blockIdx.y;
  const int stride = a.U * (a.G > 0 ? a.G : 1);
  const size_t ld = a.ld ? (size_t)a.ld : (size_t)a.N;
  const double* w = a.params + (size_t)p * stride;
  for (int e = threadIdx.x; e < THR_TILE; e += THR_SORT_THREADS) {
    const int i = base + e;
    uint64_t key = ~0ull;
    if (i < a.N) {
      const double* wi = a.group ? w + (size_t)a.group[i] * a.U : w;
      double u = __dmul_rn(wi[0], a.uncerts[i]);          // every product rounded on its own: a fused one moves the ties
      for (int j = 1; j < a.U; ++j) u = __dadd_rn(u, __dmul_rn(wi[j], a.uncerts[(size_t)j * ld + i]));
      key = thr_key_of(u);
    }
    sk[e] = key;
    si[e] = i < a.N ? i : -1;
  }
  __syncthreads();
  for (int k = 2; k <= THR_TILE; k <<= 1) thr_tile_steps(sk, si, base, k, k >> 1);
  const size_t o = (size_t)p * a.Npad + base;
  for (int e = threadIdx.x; e < THR_TILE; e += THR_SORT_THREADS) {
    a.keys[o + e] = sk[e];
    a.rows[o + e] = si[e];
  }
}

// one step (k, j) with j >= THR_TILE: partners lie in different tiles
__global__ void __launch_bounds__(256) thr_merge_global_kernel(ThrArgs a, int k, int j) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= a.Npad / 2) return;
  const int i = 2 * t - (t & (j - 1)), l = i + j;
  uint64_t* keys = a.keys + (size_t)blockIdx.y * a.Npad;
  int32_t* rows = a.rows + (size_t)blockIdx.y * a.Npad;
  const uint64_t x = keys[i], y = keys[l];
  if ((x > y) == ((i & k) == 0)) {
    keys[i] = y; keys[l] = x;
    const int32_t r = rows[i]; rows[i] = rows[l]; rows[l] = r;
  }
}

// the steps j = THR_TILE / 2 .. 1 of stage k, inside one tile
__global__ void __launch_bounds__(THR_SORT_THREADS) thr_merge_tile_kernel(ThrArgs a, int k) {
  __shared__ uint64_t sk[THR_TILE];
  __shared__ int32_t si[THR_TILE];
  const int base = blockIdx.x * THR_TILE;
  const size_t o = (size_t)blockIdx.y * a.Npad + base;
  for (int e = threadIdx.x; e < THR_TILE; e += THR_SORT_THREADS) {
    sk[e] = a.keys[o + e];
    si[e] = a.rows[o + e];
  }
  __syncthreads();
  thr_tile_steps(sk, si, base, k, THR_TILE / 2);
  for (int e = threadIdx.x; e < THR_TILE; e += THR_SORT_THREADS) {
    a.keys[o + e] = sk[e];
    a.rows[o + e] = si[e];
  }
}

// inclusive sums of two counters over the block (wave shuffles, then the wave totals through LDS); sw: 2 * waves ints
__device__ __forceinline__ void thr_block_scan_add2(int& x, int& y, int* sw) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const int tx = __shfl_up(x, d, 64), ty = __shfl_up(y, d, 64);
    if (lane >= d) { x += tx; y += ty; }
  }
  __syncthreads();               // sw may still be read from the previous use
  if (lane == 63) { sw[2 * wave] = x; sw[2 * wave + 1] = y; }
  __syncthreads();
  for (int v = 0; v < wave; ++v) { x += sw[2 * v]; y += sw[2 * v + 1]; }
}

// a point of the curve survives drop_intermediate iff it is first, last, or its run and the next differ in positives or negatives
__device__ __forceinline__ bool thr_kept(const int32_t* E, const int32_t* T, int r, int M) {
  if (r == 0 || r == M - 1) return true;
  const int e0 = E[r - 1], e = E[r], e1 = E[r + 1], t0 = T[r - 1], t = T[r], t1 = T[r + 1];
  const int dt = t - t0, dtn = t1 - t;
  return dt != dtn || (e - e0) - dt != (e1 - e) - dtn;
}

// one block per (IoU threshold, candidate) over the candidate's sorted order
__global__ void __launch_bounds__(THR_CURVE_THREADS) thr_curve_kernel(ThrArgs a) {
  constexpr int B = THR_CURVE_THREADS, W = B / 64;
  __shared__ int sw[2 * W];
  __shared__ int s_incl[B];
  __shared__ int s_tot[2];
  __shared__ double s_d[B];
  __shared__ int s_i[B];
  __shared__ double s_rate;
  const int tid = threadIdx.x, k = blockIdx.x, p = blockIdx.y, N = a.N;
  const uint64_t* keys = a.keys + (size_t)p * a.Npad;
  const int32_t* rows = a.rows + (size_t)p * a.Npad;
  int32_t* E = a.runs + ((size_t)p * a.K + k) * 2 * (size_t)N;
  int32_t* T = E + N;
  double* out = a.out + ((size_t)p * a.K + k) * 3;

  // 1. runs of equal scores: E[r] = last position of run r, T[r] = positives (correct == 0) up to it
  int runs = 0, npos = 0;
  for (int base = 0; base < N; base += B) {
    const int i = base + tid;
    int flag = 0, pos = 0;
    if (i < N) {
      flag = i + 1 == N || keys[i] != keys[i + 1];
      const int row = rows[i];              // a padding row cannot come before N for finite scores
      pos = row >= 0 && !((a.mask[row] >> k) & 1u);
    }
    int f = flag, q = pos;
    thr_block_scan_add2(f, q, sw);
    if (flag) {
      const int r = runs + f - 1;
      E[r] = i;
      T[r] = npos + q;
    }
    if (tid == B - 1) { s_tot[0] = f; s_tot[1] = q; }
    __syncthreads();
    runs += s_tot[0];
    npos += s_tot[1];
    __syncthreads();
  }
  const int M = runs, nneg = N - npos;
  if (npos == 0 || nneg == 0) {       // one label only: fpr or tpr is 0 / 0 throughout
    if (tid == 0) {
      out[0] = __longlong_as_double(0x7ff0000000000000ll);
      out[1] = out[2] = __longlong_as_double(0x7ff8000000000000ll);
    }
    return;
  }
  const double dpos = (double)npos, dneg = (double)nneg;
  const double x = a.fix_cd ? 1.0 - a.budget : a.budget;

  // 2. kept points: trapezoid terms against the previous kept point, and the segment of interp that brackets x
  int prev_carry = -1, jmax = -1, j1min = 0x7fffffff;
  double area = 0.0;
  for (int base = 0; base < M; base += B) {
    const int r = base + tid;
    const bool kept = r < M && thr_kept(E, T, r, M);
    int v = kept ? r : -1;
    for (int d = 1; d < 64; d <<= 1) v = max(v, __shfl_up(v, d, 64));    // lanes below d read their own value
    s_incl[tid] = v;
    __syncthreads();
    int prev = prev_carry;
    for (int wv = 0; wv < (tid >> 6); ++wv) prev = max(prev, s_incl[wv * 64 + 63]);
    if (tid & 63) prev = max(prev, s_incl[tid - 1]);
    int last = prev_carry;
    for (int wv = 0; wv < W; ++wv) last = max(last, s_incl[wv * 64 + 63]);
    prev_carry = last;
    __syncthreads();
    if (kept) {
      const int t = T[r];
      const double fpr = (double)(E[r] + 1 - t) / dneg, tpr = (double)t / dpos;
      double fpr0 = 0.0, tpr0 = 0.0;
      if (prev >= 0) {
        const int t0 = T[prev];
        fpr0 = (double)(E[prev] + 1 - t0) / dneg;
        tpr0 = (double)t0 / dpos;
      }
      area += (fpr - fpr0) * (tpr + tpr0) / 2.0;
      if ((a.fix_cd ? fpr : tpr) <= x) jmax = max(jmax, r); else j1min = min(j1min, r);
    }
  }
  s_d[tid] = area;
  s_incl[tid] = jmax;
  s_i[tid] = j1min;
  __syncthreads();
  for (int h = B / 2; h > 0; h >>= 1) {
    if (tid < h) {
      s_d[tid] += s_d[tid + h];
      s_incl[tid] = max(s_incl[tid], s_incl[tid + h]);
      s_i[tid] = min(s_i[tid], s_i[tid + h]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int j = s_incl[0], j1 = s_i[0];     // j = -1: the point (0, 0) in front; j1 exists, the last point has xp = 1 > x
    double xj = 0.0, fj = 0.0;
    if (j >= 0) {
      const int t = T[j];
      const double fpr = (double)(E[j] + 1 - t) / dneg, tpr = (double)t / dpos;
      xj = a.fix_cd ? fpr : tpr;
      fj = a.fix_cd ? tpr : fpr;
    }
    double res = fj;
    if (x != xj && j1 < M) {
      const int t = T[j1];
      const double fpr = (double)(E[j1] + 1 - t) / dneg, tpr = (double)t / dpos;
      const double x1 = a.fix_cd ? fpr : tpr, f1 = a.fix_cd ? tpr : fpr;
      const double slope = (f1 - fj) / (x1 - xj);
      res = slope * (x - xj) + fj;
    }
    s_rate = a.fix_cd ? 1.0 - res : res;
    out[2] = s_d[0];
  }
  __syncthreads();
  const double rate = s_rate;

  // 3. the kept point nearest to the rate, the first of equals; r = -1 is the point in front, whose threshold is +inf
  double best = a.fix_cd ? fabs(1.0 - 0.0 - rate) : fabs(0.0 - rate);
  int best_r = -1;
  if (tid != 0) { best = __longlong_as_double(0x7ff0000000000000ll); best_r = 0x7fffffff; }
  for (int r = tid; r < M; r += B) {
    if (!thr_kept(E, T, r, M)) continue;
    const int t = T[r];
    const double fpr = (double)(E[r] + 1 - t) / dneg, tpr = (double)t / dpos;
    const double val = a.fix_cd ? fabs(1.0 - tpr - rate) : fabs(fpr - rate);
    if (val < best) { best = val; best_r = r; }
  }
  s_d[tid] = best;
  s_i[tid] = best_r;
  __syncthreads();
  for (int h = B / 2; h > 0; h >>= 1) {
    if (tid < h) {
      const double ov = s_d[tid + h];
      const int orr = s_i[tid + h];
      if (ov < s_d[tid] || (ov == s_d[tid] && orr < s_i[tid])) { s_d[tid] = ov; s_i[tid] = orr; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = s_i[0] < 0 ? __longlong_as_double(0x7ff0000000000000ll) : thr_score_of(keys[E[s_i[0]]]);
    out[1] = rate;
  }
}

void launch_thr_mask(const ThrArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(thr_mask_kernel, dim3((a.N + 255) / 256), dim3(256), 0, s, a);
}

void launch_thr_objective(const ThrArgs& a, hipStream_t s) {
  const dim3 tiles(a.Npad / THR_TILE, a.Pc);
  hipLaunchKernelGGL(thr_sort_tile_kernel, tiles, dim3(THR_SORT_THREADS), 0, s, a);
  for (int k = 2 * THR_TILE; k <= a.Npad; k <<= 1) {
    for (int j = k >> 1; j >= THR_TILE; j >>= 1)
      hipLaunchKernelGGL(thr_merge_global_kernel, dim3(a.Npad / 2 / 256, a.Pc), dim3(256), 0, s, a, k, j);
    hipLaunchKernelGGL(thr_merge_tile_kernel, tiles, dim3(THR_SORT_THREADS), 0, s, a, k);
  }
  hipLaunchKernelGGL(thr_curve_kernel, dim3(a.K, a.Pc), dim3(THR_CURVE_THREADS), 0, s, a);
}

// ------------------------------------------------------------------------------------ aggregate + decode
__device__ __forceinline__ float exp32(float x) { return (float)exp((double)x); }

struct Dec {
  float box[4];
  float sig[4];
};

__device__ __forceinline__ void decode_plain(const float* t, const float* an, Dec& d) {
  const float ya = (an[0] + an[2]) / 2.0f, xa = (an[1] + an[3]) / 2.0f;
  const float ha = an[2] - an[0], wa = an[3] - an[1];
  const float w = exp32(t[3]) * wa;
  const float h = exp32(t[2]) * ha;
  const float yc = t[0] * ha + ya;
  const float xc = t[1] * wa + xa;
  d.box[0] = yc - h / 2.0f;
  d.box[1] = xc - w / 2.0f;
  d.box[2] = yc + h / 2.0f;
  d.box[3] = xc + w / 2.0f;
}

// method "sample" (utils_box.py:162-184): S draws from Normal(loc = (ty, tx, th, tw), scale = sqrt(sigma^2)), each decoded like
// a plain box, mean and population variance (tf.nn.moments) of the four corners over the draws, all in float64.  TFP's
// stream cannot be reproduced: the draws come from the build's Philox normal stream (counter (anchor, sample row, 2 s + {0, 1}),
// tag 0xD5: (y, x) from the first call, (h, w) from the second), shared with the oracle.  Welford's update keeps the variance
// accurate at box coordinates ~1e3 with sigma ~1e-1.
__device__ __forceinline__ void decode_sample(const float* t, const float* sg, const float* an, int S, uint64_t seed,
                                              uint32_t id0, uint32_t id1, Dec& d) {
  const double a0 = an[0], a1 = an[1], a2 = an[2], a3 = an[3];
  const double ya = (a0 + a2) / 2, xa = (a1 + a3) / 2;
  const double ha = a2 - a0, wa = a3 - a1;
  const double ty = t[0], tx = t[1], th = t[2], tw = t[3];
  double sc[4];
  for (int k = 0; k < 4; ++k) { const double s = sg[k]; sc[k] = sqrt(s * s); }
  double mean[4] = {0, 0, 0, 0}, m2[4] = {0, 0, 0, 0};
  for (int s = 0; s < S; ++s) {
    double zy, zx, zh, zw;
    philox_normal2(seed, id0, id1, (uint32_t)(2 * s), 0xD5u, zy, zx);
    philox_normal2(seed, id0, id1, (uint32_t)(2 * s + 1), 0xD5u, zh, zw);
    const double sy = ty + sc[0] * zy, sx = tx + sc[1] * zx, sh = th + sc[2] * zh, sw = tw + sc[3] * zw;
    const double w = exp(sw) * wa, h = exp(sh) * ha;
    const double yc = sy * ha + ya, xc = sx * wa + xa;
    const double v[4] = {yc - h / 2.0, xc - w / 2.0, yc + h / 2.0, xc + w / 2.0};
    const double n = (double)(s + 1);
    for (int k = 0; k < 4; ++k) {
      const double dl = v[k] - mean[k];
      mean[k] += dl / n;
      m2[k] += dl * (v[k] - mean[k]);
    }
  }
  for (int k = 0; k < 4; ++k) {
    d.box[k] = (float)mean[k];
    d.sig[k] = (float)sqrt(m2[k] / (double)S);
  }
}

__device__ __forceinline__ void decode_uncert(const float* t, const float* sg, const float* an,
                                              int method, Dec& d) {
  const double a0 = an[0], a1 = an[1], a2 = an[2], a3 = an[3];
  const double ya = (a0 + a2) / 2, xa = (a1 + a3) / 2;
  const double ha = a2 - a0, wa = a3 - a1;
  const double ty = t[0], tx = t[1], th = t[2], tw = t[3];
  const double s0 = sg[0], s1 = sg[1], s2 = sg[2], s3 = sg[3];
  const double dty = s0 * s0, dtx = s1 * s1, dth = s2 * s2, dtw = s3 * s3;
  double w, h, yc, xc, dymin, dxmin, dymax, dxmax;
  if (method == UDA_DECODE_LNORM) {
    w = exp(tw + dtw / 2) * wa;
    h = exp(th + dth / 2) * ha;
    yc = ty * ha + ya;
    xc = tx * wa + xa;
    const double dw = (exp(dtw) - 1) * exp(2 * tw + dtw) * (wa * wa);
    const double dh = (exp(dth) - 1) * exp(2 * th + dth) * (ha * ha);
    const double dyc = dty * (ha * ha);
    const double dxc = dtx * (wa * wa);
    dymin = dyc + dh / 4.0;
    dxmin = dxc + dw / 4.0;
    dymax = dymin;
    dxmax = dxmin;
  } else {  // falsedec
    w = exp(tw) * wa;
    h = exp(th) * ha;
    yc = ty * ha + ya;
    xc = tx * wa + xa;
    const double dw = exp(dtw) * wa;
    const double dh = exp(dth) * ha;
    const double dyc = dty * ha + ya;
    const double dxc = dtx * wa + xa;
    dymin = fabs(dyc - dh / 2.0);
    dxmin = fabs(dxc - dw / 2.0);
    dymax = dyc + dh / 2.0;
    dxmax = dxc + dw / 2.0;
  }
  d.box[0] = (float)(yc - h / 2.0);
  d.box[1] = (float)(xc - w / 2.0);
  d.box[2] = (float)(yc + h / 2.0);
  d.box[3] = (float)(xc + w / 2.0);
  d.sig[0] = (float)sqrt(dymin);
  d.sig[1] = (float)sqrt(dxmin);
  d.sig[2] = (float)sqrt(dymax);
  d.sig[3] = (float)sqrt(dxmax);
}

// SAMPLE is a compile-time flag: the Philox / Box-Muller code of the "sample" method would otherwise cost the common
// kernels registers (measured: aggregate_reg_kernel 0.94 -> 1.25 ms with the branch inside).
template <bool SAMPLE = false>
__device__ __forceinline__ void decode_one(const AggArgs& a, const float* bp, int A, const float* an,
                                           Dec& d, uint32_t id0 = 0, uint32_t id1 = 0) {
  float t[4] = {bp[0], bp[1], bp[2], bp[3]};
  if (a.loss_att) {
    const float* sp = bp + 4 * A;
    float sg[4] = {sp[0], sp[1], sp[2], sp[3]};
    if constexpr (SAMPLE) decode_sample(t, sg, an, a.decode_nsamples, a.decode_seed, id0, id1, d);
    else decode_uncert(t, sg, an, a.decode, d);
  } else {
    decode_plain(t, an, d);
    d.sig[0] = d.sig[1] = d.sig[2] = d.sig[3] = 0.f;
  }
}

// One thread per candidate, 64-thread blocks.  Every head value is read from HBM exactly ONCE: the T class
// logits and the T decoded boxes of the candidate are parked in LDS ([slot][lane], conflict-free) between
// the mean pass and the deviation pass, so the two-pass population std keeps the oracle's arithmetic order
// (bit-exact) without a second trip to memory and without decoding twice.
constexpr int AGG_BLOCK = 64;

template <bool SAMPLE>
__global__ __launch_bounds__(AGG_BLOCK) void aggregate_kernel(AggArgs a) {
  extern __shared__ float park[];          // [Tc * C + Tb * 4][AGG_BLOCK]
  const int lane = threadIdx.x;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)a.n_img * a.K) return;
  const int n = (int)(gid / a.K);
  const int C = a.C;
  int ai = (int)(gid % a.K), fixed_c = -1;
  if (a.cand_flat) {            // top-k path: this candidate is one (anchor, class) pair
    const int flat = a.cand_flat[gid];
    ai = flat / C;
    fixed_c = flat % C;
  }
  int lvl = 0;
  while (lvl + 1 < a.lv.num_levels && ai >= a.lv.a_off[lvl + 1]) ++lvl;
  const int loc = ai - a.lv.a_off[lvl];
  const int p = loc / a.A, al = loc % a.A;
  const int hw = a.lv.hw[lvl];

  // ---- class logits: mean / population std over the T axis; first-max argmax or the given class
  const int cch = a.A * C;
  const float* cbase = a.lv.cls[lvl] + ((size_t)n * a.Tc * hw + p) * cch + al * C;
  const size_t cstride = (size_t)hw * cch;
  const float fT = (float)a.Tc;
  // park_all: slot (t * C + c), every logit parked up front (sample-major reads: the C logits of a sample
  // are contiguous); otherwise slot t, one class at a time (large T * C that would not fit LDS)
  float* pc = park + lane;
  const int cs = a.park_all ? C : 0;                        // slot of (t, c) = t * cs' + c' below
  if (a.Tc > 1 && a.park_all)
    for (int t = 0; t < a.Tc; ++t)
      for (int c = 0; c < C; ++c) pc[(t * C + c) * AGG_BLOCK] = cbase[t * cstride + c];
  float best = -INFINITY;
  int best_c = 0;
  for (int c = 0; c < C; ++c) {
    float m, sd = 0.f;
    if (a.Tc > 1) {
      const int c0 = a.park_all ? c : 0, ts = a.park_all ? cs : 1;
      if (!a.park_all)
        for (int t = 0; t < a.Tc; ++t) pc[t * AGG_BLOCK] = cbase[t * cstride + c];
      m = pc[c0 * AGG_BLOCK];
      for (int t = 1; t < a.Tc; ++t) m = m + pc[(t * ts + c0) * AGG_BLOCK];
      m = m / fT;
      if (a.u_cls && (fixed_c < 0 || fixed_c == c)) {
        float v = 0.f;
        for (int t = 0; t < a.Tc; ++t) {
          const float dlt = pc[(t * ts + c0) * AGG_BLOCK] - m;
          v = v + dlt * dlt;
        }
        sd = sqrtf(v / fT);
      }
    } else {
      m = cbase[c];
    }
    a.logits[(size_t)gid * C + c] = m;
    if (fixed_c < 0) {
      if (a.u_cls) a.u_cls[(size_t)gid * C + c] = sd;
      if (m > best) {
        best = m;
        best_c = c;
      }
    } else if (c == fixed_c) {
      if (a.u_cls) a.u_cls[gid] = sd;
      best = m;
      best_c = c;
    }
  }
  a.scores[gid] = (float)(1.0 / (1.0 + exp(-(double)best)));
  a.classes[gid] = best_c;

  // ---- boxes: per-sample decode, then mean / std over samples
  const int bch = a.A * (a.loss_att ? 8 : 4);
  const float* bbase = a.lv.box[lvl] + ((size_t)n * a.Tb * hw + p) * bch + al * 4;
  const size_t bstride = (size_t)hw * bch;
  const float an[4] = {a.anchors[ai * 4 + 0], a.anchors[ai * 4 + 1], a.anchors[ai * 4 + 2],
                       a.anchors[ai * 4 + 3]};
  Dec d;
  decode_one<SAMPLE>(a, bbase, a.A, an, d, (uint32_t)ai, a.row_base + (uint32_t)n * (uint32_t)a.Tb);
  if (a.Tb == 1) {
    for (int k = 0; k < 4; ++k) a.boxes[(size_t)gid * 4 + k] = d.box[k];
    if (a.u_al) for (int k = 0; k < 4; ++k) a.u_al[(size_t)gid * 4 + k] = d.sig[k];
    if (a.u_ep) for (int k = 0; k < 4; ++k) a.u_ep[(size_t)gid * 4 + k] = 0.f;
    return;
  }
  float* pb = park + (size_t)a.cls_slots * AGG_BLOCK + lane;   // slot (t * 4 + k)
  const float fTb = (float)a.Tb;
  float sb[4] = {d.box[0], d.box[1], d.box[2], d.box[3]};
  float ss[4] = {d.sig[0], d.sig[1], d.sig[2], d.sig[3]};
  for (int k = 0; k < 4; ++k) pb[k * AGG_BLOCK] = d.box[k];
  for (int t = 1; t < a.Tb; ++t) {
    decode_one<SAMPLE>(a, bbase + t * bstride, a.A, an, d, (uint32_t)ai, a.row_base + (uint32_t)n * (uint32_t)a.Tb + (uint32_t)t);
    for (int k = 0; k < 4; ++k) {
      sb[k] = sb[k] + d.box[k];
      ss[k] = ss[k] + d.sig[k];
      pb[(t * 4 + k) * AGG_BLOCK] = d.box[k];
    }
  }
  float mb[4];
  for (int k = 0; k < 4; ++k) {
    mb[k] = sb[k] / fTb;
    a.boxes[(size_t)gid * 4 + k] = mb[k];
    if (a.u_al) a.u_al[(size_t)gid * 4 + k] = ss[k] / fTb;
  }
  if (a.u_ep) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < a.Tb; ++t) {
      for (int k = 0; k < 4; ++k) {
        const float dlt = pb[(t * 4 + k) * AGG_BLOCK] - mb[k];
        v[k] = v[k] + dlt * dlt;
      }
    }
    for (int k = 0; k < 4; ++k) a.u_ep[(size_t)gid * 4 + k] = sqrtf(v[k] / fTb);
  }
}

// The same for the common small case (T samples of both heads, C classes, T * (C + 4) <= 110 values per candidate):
// the logits and decoded boxes of the candidate stay in REGISTERS between the mean pass and the deviation pass.  The
// LDS-parked version holds 28 KB per 64 threads (5 waves per CU: latency-bound, 2.3 ms); this one has no LDS, all
// T * C logit loads of a thread are in flight at once, and 16 waves fit a CU.  Same arithmetic order (bit-exact).
template <int T, int CT>     // CT = 0: any number of classes, one class at a time (T logits in registers per class)
__global__ __launch_bounds__(128) void aggregate_reg_kernel(AggArgs a) {
  const int C = CT ? CT : a.C;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)a.n_img * a.K) return;
  const int n = (int)(gid / a.K);
  int ai = (int)(gid % a.K), fixed_c = -1;
  if (a.cand_flat) {
    const int flat = a.cand_flat[gid];
    ai = flat / C;
    fixed_c = flat % C;
  }
  int lvl = 0;
  while (lvl + 1 < a.lv.num_levels && ai >= a.lv.a_off[lvl + 1]) ++lvl;
  const int loc = ai - a.lv.a_off[lvl];
  const int p = loc / a.A, al = loc % a.A;
  const int hw = a.lv.hw[lvl];
  const int cch = a.A * C;
  const float* cbase = a.lv.cls[lvl] + ((size_t)n * T * hw + p) * cch + al * C;
  const size_t cstride = (size_t)hw * cch;
  const float fT = (float)T;
  float best = -INFINITY;
  int best_c = 0;
  auto one_class = [&](int c, const float* x) {       // x[t] = logit of sample t
    float m = x[0], sd = 0.f;
#pragma unroll
    for (int t = 1; t < T; ++t) m = m + x[t];
    m = m / fT;
    if (a.u_cls && (fixed_c < 0 || fixed_c == c)) {
      float v = 0.f;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float dlt = x[t] - m;
        v = v + dlt * dlt;
      }
      sd = sqrtf(v / fT);
    }
    a.logits[(size_t)gid * C + c] = m;
    if (fixed_c < 0) {
      if (a.u_cls) a.u_cls[(size_t)gid * C + c] = sd;
      if (m > best) {
        best = m;
        best_c = c;
      }
    } else if (c == fixed_c) {
      if (a.u_cls) a.u_cls[gid] = sd;
      best = m;
      best_c = c;
    }
  };
  if constexpr (CT > 0) {
    float cl[T * (CT ? CT : 1)];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int c = 0; c < CT; ++c) cl[t * CT + c] = cbase[t * cstride + c];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      float x[T];
#pragma unroll
      for (int t = 0; t < T; ++t) x[t] = cl[t * CT + c];
      one_class(c, x);
    }
  } else {
    for (int c = 0; c < C; ++c) {
      float x[T];
#pragma unroll
      for (int t = 0; t < T; ++t) x[t] = cbase[t * cstride + c];
      one_class(c, x);
    }
  }
  a.scores[gid] = (float)(1.0 / (1.0 + exp(-(double)best)));
  a.classes[gid] = best_c;

  const int bch = a.A * (a.loss_att ? 8 : 4);
  const float* bbase = a.lv.box[lvl] + ((size_t)n * T * hw + p) * bch + al * 4;
  const size_t bstride = (size_t)hw * bch;
  const float an[4] = {a.anchors[ai * 4 + 0], a.anchors[ai * 4 + 1], a.anchors[ai * 4 + 2], a.anchors[ai * 4 + 3]};
  float bxs[T * 4];
  float sb[4], ss[4];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    Dec d;
    decode_one<false>(a, bbase + t * bstride, a.A, an, d);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sb[k] = t ? sb[k] + d.box[k] : d.box[k];
      ss[k] = t ? ss[k] + d.sig[k] : d.sig[k];
      bxs[t * 4 + k] = d.box[k];
    }
  }
  const float fTb = (float)T;
  float mb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    mb[k] = sb[k] / fTb;
    a.boxes[(size_t)gid * 4 + k] = mb[k];
    if (a.u_al) a.u_al[(size_t)gid * 4 + k] = ss[k] / fTb;
  }
  if (a.u_ep) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float dlt = bxs[t * 4 + k] - mb[k];
        v[k] = v[k] + dlt * dlt;
      }
#pragma unroll
    for (int k = 0; k < 4; ++k) a.u_ep[(size_t)gid * 4 + k] = sqrtf(v[k] / fTb);
  }
}

// The register kernel for the other common (T, C): the class statistics are computed in two STREAMING passes over the
// sample axis (sample-major: the C logits of an anchor are contiguous, so consecutive loads of a wave touch the same lines;
// the class-major loop of aggregate_reg_kernel<T, 0> re-fetched every line C times through a thrashing L1: 6.3 ms for
// T = 20 / C = 10 on 32 images) - pass 1 the sums, pass 2 the squared deviations - with 3 C registers instead of T C; the T
// decoded boxes stay in registers as before.  Same arithmetic order (bit-exact).
template <int T, int C>
__global__ __launch_bounds__(128) void aggregate_reg2_kernel(AggArgs a) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)a.n_img * a.K) return;
  const int n = (int)(gid / a.K);
  int ai = (int)(gid % a.K), fixed_c = -1;
  if (a.cand_flat) {
    const int flat = a.cand_flat[gid];
    ai = flat / C;
    fixed_c = flat % C;
  }
  int lvl = 0;
  while (lvl + 1 < a.lv.num_levels && ai >= a.lv.a_off[lvl + 1]) ++lvl;
  const int loc = ai - a.lv.a_off[lvl];
  const int p = loc / a.A, al = loc % a.A;
  const int hw = a.lv.hw[lvl];
  const int cch = a.A * C;
  const float* cbase = a.lv.cls[lvl] + ((size_t)n * T * hw + p) * cch + al * C;
  const size_t cstride = (size_t)hw * cch;
  const float fT = (float)T;
  float m[C], v[C];
#pragma unroll
  for (int c = 0; c < C; ++c) m[c] = cbase[c];
  for (int t = 1; t < T; ++t) {
    const float* x = cbase + t * cstride;
#pragma unroll
    for (int c = 0; c < C; ++c) m[c] = m[c] + x[c];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) { m[c] = m[c] / fT; v[c] = 0.f; }
  if (a.u_cls) {
    for (int t = 0; t < T; ++t) {
      const float* x = cbase + t * cstride;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float dlt = x[c] - m[c];
        v[c] = v[c] + dlt * dlt;
      }
    }
  }
  float best = -INFINITY;
  int best_c = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float sd = a.u_cls ? sqrtf(v[c] / fT) : 0.f;
    a.logits[(size_t)gid * C + c] = m[c];
    if (fixed_c < 0) {
      if (a.u_cls) a.u_cls[(size_t)gid * C + c] = sd;
      if (m[c] > best) { best = m[c]; best_c = c; }
    } else if (c == fixed_c) {
      if (a.u_cls) a.u_cls[gid] = sd;
      best = m[c];
      best_c = c;
    }
  }
  a.scores[gid] = (float)(1.0 / (1.0 + exp(-(double)best)));
  a.classes[gid] = best_c;

  const int bch = a.A * (a.loss_att ? 8 : 4);
  const float* bbase = a.lv.box[lvl] + ((size_t)n * T * hw + p) * bch + al * 4;
  const size_t bstride = (size_t)hw * bch;
  const float an[4] = {a.anchors[ai * 4 + 0], a.anchors[ai * 4 + 1], a.anchors[ai * 4 + 2], a.anchors[ai * 4 + 3]};
  float bxs[T * 4];
  float sb[4], ss[4];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    Dec d;
    decode_one<false>(a, bbase + t * bstride, a.A, an, d);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sb[k] = t ? sb[k] + d.box[k] : d.box[k];
      ss[k] = t ? ss[k] + d.sig[k] : d.sig[k];
      bxs[t * 4 + k] = d.box[k];
    }
  }
  float mb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    mb[k] = sb[k] / fT;
    a.boxes[(size_t)gid * 4 + k] = mb[k];
    if (a.u_al) a.u_al[(size_t)gid * 4 + k] = ss[k] / fT;
  }
  if (a.u_ep) {
    float vv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float dlt = bxs[t * 4 + k] - mb[k];
        vv[k] = vv[k] + dlt * dlt;
      }
#pragma unroll
    for (int k = 0; k < 4; ++k) a.u_ep[(size_t)gid * 4 + k] = sqrtf(vv[k] / fT);
  }
}

void launch_aggregate(const AggArgs& a0, hipStream_t s) {
  AggArgs a = a0;
  static const int regs = uda_env_int("UDA_AGG_REG", 1);
  const bool sample = a.loss_att && a.decode == UDA_DECODE_SAMPLE;      // the (slow, optional) sampling decode: LDS-parking kernel only
  if (regs && !sample && a.Tc == a.Tb && (a.Tc == 10 || a.Tc == 20)) {
    const int64_t tot = (int64_t)a.n_img * a.K;
    const dim3 grid((unsigned)((tot + 127) / 128)), block(128);
    if (a.Tc == 10 && a.C == 7) hipLaunchKernelGGL((aggregate_reg_kernel<10, 7>), grid, block, 0, s, a);
    else if (a.Tc == 10 && a.C == 10) hipLaunchKernelGGL((aggregate_reg2_kernel<10, 10>), grid, block, 0, s, a);
    else if (a.Tc == 20 && a.C == 7) hipLaunchKernelGGL((aggregate_reg2_kernel<20, 7>), grid, block, 0, s, a);
    else if (a.Tc == 20 && a.C == 10) hipLaunchKernelGGL((aggregate_reg2_kernel<20, 10>), grid, block, 0, s, a);
    else if (a.Tc == 10) hipLaunchKernelGGL((aggregate_reg_kernel<10, 0>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((aggregate_reg_kernel<20, 0>), grid, block, 0, s, a);
    return;
  }
  if (regs && !sample && a.Tc == a.Tb && a.Tc == 30 && (a.C == 7 || a.C == 10)) {      // configs[4]: T = 30
    const int64_t tot = (int64_t)a.n_img * a.K;
    const dim3 grid((unsigned)((tot + 127) / 128)), block(128);
    if (a.C == 7) hipLaunchKernelGGL((aggregate_reg2_kernel<30, 7>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((aggregate_reg2_kernel<30, 10>), grid, block, 0, s, a);
    return;
  }
  const int64_t total = (int64_t)a.n_img * a.K;
  const int box_slots = a.Tb > 1 ? a.Tb * 4 : 0;
  a.park_all = (a.Tc * a.C + box_slots) * AGG_BLOCK * (int)sizeof(float) <= 48 * 1024;   // >= 3 blocks per CU
  a.cls_slots = a.Tc > 1 ? (a.park_all ? a.Tc * a.C : a.Tc) : 0;
  const size_t lds = (size_t)(a.cls_slots + box_slots) * AGG_BLOCK * sizeof(float);
  static size_t attr_lds[2] = {64 * 1024, 64 * 1024};
  if (lds > attr_lds[sample]) {
    if (sample) hipFuncSetAttribute((const void*)aggregate_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    else hipFuncSetAttribute((const void*)aggregate_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_lds[sample] = lds;
  }
  const dim3 grid((unsigned)((total + AGG_BLOCK - 1) / AGG_BLOCK));
  if (sample) hipLaunchKernelGGL(aggregate_kernel<true>, grid, dim3(AGG_BLOCK), lds, s, a);
  else hipLaunchKernelGGL(aggregate_kernel<false>, grid, dim3(AGG_BLOCK), lds, s, a);
}

// ------------------------------------------------------------------------------------ top-k pre-selection
// postprocess.topk_class_boxes with max_nms_inputs > 0 (postprocess.py:96-121): the k largest mean
// logits over anchors*classes.  TF leaves the order of sorted=False open; the build fixes it to
// value descending, ties -> lower flat index, identically in oracle and kernel.
__global__ __launch_bounds__(256) void class_mean_kernel(AggArgs a, float* out) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (n, anchor, class)
  const int64_t per = (int64_t)a.A_tot * a.C;
  if (gid >= (int64_t)a.n_img * per) return;
  const int n = (int)(gid / per);
  const int r = (int)(gid % per);
  const int ai = r / a.C, c = r % a.C;
  int lvl = 0;
  while (lvl + 1 < a.lv.num_levels && ai >= a.lv.a_off[lvl + 1]) ++lvl;
  const int loc = ai - a.lv.a_off[lvl];
  const int p = loc / a.A, al = loc % a.A;
  const int hw = a.lv.hw[lvl], cch = a.A * a.C;
  const float* cbase = a.lv.cls[lvl] + ((size_t)n * a.Tc * hw + p) * cch + al * a.C + c;
  const size_t cstride = (size_t)hw * cch;
  float m = cbase[0];
  if (a.Tc > 1) {
    for (int t = 1; t < a.Tc; ++t) m = m + cbase[t * cstride];
    m = m / (float)a.Tc;
  }
  out[gid] = m;
}

void launch_class_mean(const AggArgs& a, float* out, hipStream_t s) {
  const int64_t total = (int64_t)a.n_img * a.A_tot * a.C;
  hipLaunchKernelGGL(class_mean_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, out);
}

constexpr int TOPK_THREADS = 1024;      // (block_excl_scan of post_common.h scans exactly this many threads)
constexpr int TOPK_MAX = 8192;

// radix-select step: among elements whose key matches `prefix` on the bits above `shift+bits`,
// histogram the next `bits` bits; pick the bin (from the top) where the running count reaches `need`.
__device__ __forceinline__ void topk_select_digit(const float* v, int L, uint32_t prefix, int hi_shift, int shift,
                                                  int bits, unsigned* hist, int* need, uint32_t* out_prefix) {
  const int nb = 1 << bits;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) hist[i] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < L; i += blockDim.x) {
    const uint32_t key = ord32(v[i]);
    if (hi_shift >= 32 || (key >> hi_shift) == prefix) atomicAdd(&hist[(key >> shift) & (nb - 1)], 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int rem = *need;
    int b = nb - 1;
    for (; b > 0; --b) {
      if ((int)hist[b] >= rem) break;
      rem -= (int)hist[b];
    }
    *need = rem;                                   // still to take inside bin b
    *out_prefix = (hi_shift >= 32 ? 0u : (prefix << bits)) | (uint32_t)b;
  }
  __syncthreads();
}

__global__ __launch_bounds__(TOPK_THREADS) void topk_kernel(const float* vals, int L, int k, int32_t* out_idx) {
  __shared__ unsigned long long keys[TOPK_MAX];
  __shared__ unsigned hist[2048];
  __shared__ int wsum[17];
  __shared__ int need;
  __shared__ uint32_t prefix;
  __shared__ int n_gt, n_eq_taken;
  const float* v = vals + (size_t)blockIdx.x * L;
  int32_t* out = out_idx + (size_t)blockIdx.x * k;
  if (threadIdx.x == 0) { need = k; prefix = 0; n_gt = 0; n_eq_taken = 0; }
  __syncthreads();
  topk_select_digit(v, L, 0u, 32, 21, 11, hist, &need, &prefix);
  topk_select_digit(v, L, prefix, 21, 10, 11, hist, &need, &prefix);
  topk_select_digit(v, L, prefix, 10, 0, 10, hist, &need, &prefix);
  const uint32_t T = prefix;            // key of the k-th largest value; `need` of the elements equal to it are taken
  const int take_eq = need;
  int P = 1;
  while (P < k) P <<= 1;
  for (int i = threadIdx.x; i < P; i += blockDim.x) keys[i] = 0ull;
  __syncthreads();
  // collect in index order: everything above T, and the first `take_eq` elements equal to T
  for (int base = 0; base < L; base += TOPK_THREADS) {
    const int i = base + threadIdx.x;
    uint32_t key = 0;
    int gt = 0, eq = 0;
    if (i < L) {
      key = ord32(v[i]);
      gt = key > T;
      eq = key == T;
    }
    int tot_gt, tot_eq;
    const int pg = block_excl_scan(gt, wsum, &tot_gt);
    const int pe = block_excl_scan(eq, wsum, &tot_eq);
    const int base_gt = n_gt, base_eq = n_eq_taken;
    const unsigned long long full = ((unsigned long long)key << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
    if (gt) keys[base_gt + pg] = full;
    if (eq && base_eq + pe < take_eq) keys[(k - take_eq) + base_eq + pe] = full;
    __syncthreads();
    if (threadIdx.x == 0) { n_gt = base_gt + tot_gt; n_eq_taken = min(take_eq, base_eq + tot_eq); }
    __syncthreads();
  }
  // bitonic sort, descending (padding keys are 0 = smallest)
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < P / 2; t += blockDim.x) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool desc = ((lo & size) == 0);
        const unsigned long long x = keys[lo], y = keys[hi];
        if ((x < y) == desc) { keys[lo] = y; keys[hi] = x; }
      }
      __syncthreads();
    }
  }
  for (int j = threadIdx.x; j < k; j += blockDim.x) out[j] = (int32_t)(0xFFFFFFFFu - (uint32_t)keys[j]);
}

// ---- the same selection spread over the device (an image of D2 at 1024 x 1024 has 1.37 M (anchor, class) values and a
// batch share of 2 images: one block per image left 254 CUs idle for 4.4 ms).  Every value gets a DISTINCT 53-bit composite
// key (order-preserving value bits << 21 | 2^21 - 1 - index): the k largest composites are exactly "value descending, ties ->
// lower index".  Radix select, 5 digits (11, 11, 11, 10, 10 bits): per digit one grid-wide histogram pass (LDS histogram per
// block, merged with atomics) - every block first re-derives the digits chosen so far from the previous histograms, so there
// is no separate pick launch; then one compaction pass (everything >= the k-th composite, appended in any order) and the
// bitonic sort of the k keys, one block per image.
constexpr int TK2_LEVELS = 5;
__device__ __constant__ int TK2_BITS[TK2_LEVELS] = {11, 11, 11, 10, 10};
__device__ __forceinline__ unsigned long long topk_comp(float v, int i) {
  return ((unsigned long long)ord32(v) << 21) | (unsigned long long)(0x1FFFFFu - (uint32_t)i);
}
// digits chosen on levels < level (deterministic, identical in every block): prefix of the k-th largest composite and how many
// elements of the current prefix class are still to be taken
__device__ __forceinline__ void topk2_resolve(const unsigned* hist_img /*[levels][2048]*/, int level, int k, unsigned long long* prefix, int* need,
                                              unsigned* sh /*[2048] scratch*/) {
  unsigned long long pre = 0;
  int rem = k;
  for (int l = 0; l < level; ++l) {
    const int nb = 1 << TK2_BITS[l];
    for (int i = threadIdx.x; i < nb; i += blockDim.x) sh[i] = hist_img[l * 2048 + i];
    __syncthreads();
    int b = nb - 1;                      // every thread walks the (<= 2048) bins itself: no broadcast, no extra barrier
    for (; b > 0; --b) {
      const int c = (int)sh[b];
      if (c >= rem) break;
      rem -= c;
    }
    pre = (pre << TK2_BITS[l]) | (unsigned long long)b;
    __syncthreads();
  }
  *prefix = pre;
  *need = rem;
}

__global__ __launch_bounds__(256) void topk2_hist_kernel(const float* vals, int L, int k, unsigned* hist /*[n_img][levels][2048]*/, int level) {
  __shared__ unsigned sh[2048];
  const int img = blockIdx.y;
  const float* v = vals + (size_t)img * L;
  unsigned* hist_img = hist + (size_t)img * TK2_LEVELS * 2048;
  unsigned long long prefix;
  int need;
  topk2_resolve(hist_img, level, k, &prefix, &need, sh);
  int used = 0;
  for (int l = 0; l < level; ++l) used += TK2_BITS[l];
  const int bits = TK2_BITS[level], shift = 53 - used - bits, nb = 1 << bits;
  for (int i = threadIdx.x; i < nb; i += 256) sh[i] = 0;
  __syncthreads();
  const int per = (L + gridDim.x - 1) / gridDim.x;
  const int lo = blockIdx.x * per, hi = min(L, lo + per);
  for (int i = lo + threadIdx.x; i < hi; i += 256) {
    const unsigned long long key = topk_comp(v[i], i);
    if (level == 0 || (key >> (shift + bits)) == prefix) atomicAdd(&sh[(unsigned)(key >> shift) & (nb - 1)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += 256)
    if (sh[i]) atomicAdd(&hist_img[level * 2048 + i], sh[i]);
}

__global__ __launch_bounds__(256) void topk2_collect_kernel(const float* vals, int L, int k, const unsigned* hist, unsigned long long* keys /*[n_img][P]*/,
                                                            int* count /*[n_img]*/, int P) {
  __shared__ unsigned sh[2048];
  const int img = blockIdx.y;
  const float* v = vals + (size_t)img * L;
  unsigned long long kth;
  int need;
  topk2_resolve(hist + (size_t)img * TK2_LEVELS * 2048, TK2_LEVELS, k, &kth, &need, sh);   // all 53 bits: the k-th largest composite itself
  const int per = (L + gridDim.x - 1) / gridDim.x;
  const int lo = blockIdx.x * per, hi = min(L, lo + per);
  for (int i = lo + threadIdx.x; i < hi; i += 256) {
    const unsigned long long key = topk_comp(v[i], i);
    if (key >= kth) {
      const int pos = atomicAdd(&count[img], 1);
      if (pos < P) keys[(size_t)img * P + pos] = key;
    }
  }
}

__global__ __launch_bounds__(TOPK_THREADS) void topk2_sort_kernel(const unsigned long long* keys_in, const int* count, int k, int P, int32_t* out_idx) {
  __shared__ unsigned long long keys[TOPK_MAX];
  const int img = blockIdx.x;
  const int n = min(count[img], P);
  for (int i = threadIdx.x; i < P; i += blockDim.x) keys[i] = i < n ? keys_in[(size_t)img * P + i] : 0ull;
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < P / 2; t += blockDim.x) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool desc = ((lo & size) == 0);
        const unsigned long long x = keys[lo], y = keys[hi];
        if ((x < y) == desc) { keys[lo] = y; keys[hi] = x; }
      }
      __syncthreads();
    }
  }
  int32_t* out = out_idx + (size_t)img * k;
  for (int j = threadIdx.x; j < k; j += blockDim.x) out[j] = (int32_t)(0x1FFFFFu - (uint32_t)(keys[j] & 0x1FFFFFull));
}

size_t topk_workspace_bytes(int n_img, int k) {
  int P = 1;
  while (P < k) P <<= 1;
  return (size_t)n_img * (TK2_LEVELS * 2048 * sizeof(unsigned) + sizeof(int) * 4 + (size_t)P * sizeof(unsigned long long)) + 256;
}

void launch_topk(const float* vals, int n_img, int L, int k, int32_t* out_idx, void* ws, hipStream_t s) {
  static const int multi = uda_env_int("UDA_TOPK_MULTI", 1);
  // few images per launch and a long value list: spread each image over the device; many images: one block each is enough
  // (UDA_TOPK_MULTI=2: also for short lists - test hook; 0: never)
  if (!multi || !ws || L > (1 << 21) || (L < (1 << 16) && multi != 2) || n_img > 64 || k > TOPK_MAX) {
    hipLaunchKernelGGL(topk_kernel, dim3(n_img), dim3(TOPK_THREADS), 0, s, vals, L, k, out_idx);
    return;
  }
  int P = 1;
  while (P < k) P <<= 1;
  unsigned* hist = (unsigned*)ws;
  int* count = (int*)(hist + (size_t)n_img * TK2_LEVELS * 2048);
  unsigned long long* keys = (unsigned long long*)(((uintptr_t)(count + 4 * n_img) + 255) & ~(uintptr_t)255);
  hipMemsetAsync(ws, 0, (size_t)n_img * (TK2_LEVELS * 2048 * sizeof(unsigned) + sizeof(int) * 4), s);
  int nblk = (1024 + n_img - 1) / n_img;            // about 1024 blocks in all
  if (nblk > (L + 4095) / 4096) nblk = (L + 4095) / 4096;
  if (nblk < 1) nblk = 1;
  for (int level = 0; level < TK2_LEVELS; ++level)
    hipLaunchKernelGGL(topk2_hist_kernel, dim3(nblk, n_img), dim3(256), 0, s, vals, L, k, hist, level);
  hipLaunchKernelGGL(topk2_collect_kernel, dim3(nblk, n_img), dim3(256), 0, s, vals, L, k, hist, keys, count, P);
  hipLaunchKernelGGL(topk2_sort_kernel, dim3(n_img), dim3(TOPK_THREADS), 0, s, keys, count, k, P, out_idx);
}

// ------------------------------------------------------------------------------------ gather / pack
__global__ __launch_bounds__(128) void gather_kernel(GatherArgs a) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.n_img * a.M) return;
  const int n = gid / a.M, i = gid % a.M;
  const int valid = a.nsel[n];
  if (i == 0) a.out_valid[n] = valid;
  const int idx = (i < valid) ? a.sel_idx[gid] : 0;   // padded slots replicate candidate 0
  const size_t src = (size_t)n * a.K + idx;
  const float sc = a.scales ? a.scales[n] : 1.0f;
  float* ob = a.out_boxes + (size_t)gid * a.box_cols;
  const float hi[4] = {a.clip_h, a.clip_w, a.clip_h, a.clip_w};
  for (int k = 0; k < 4; ++k) {
    float v = a.boxes[src * 4 + k];
    if (a.clip) v = fminf(fmaxf(v, 0.0f), hi[k]);
    ob[k] = a.scales ? v * sc : v;
  }
  int col = 4;
  if (a.u_al) {
    for (int k = 0; k < 4; ++k) ob[col + k] = a.scales ? a.u_al[src * 4 + k] * sc : a.u_al[src * 4 + k];
    col += 4;
  }
  if (a.u_ep) {
    for (int k = 0; k < 4; ++k) ob[col + k] = a.scales ? a.u_ep[src * 4 + k] * sc : a.u_ep[src * 4 + k];
    col += 4;
  }
  a.out_scores[gid] = (i < valid) ? a.sel_score[gid] : 0.0f;
  float* oc = a.out_classes + (size_t)gid * a.cls_cols;
  oc[0] = (float)(a.classes[src] + 1);
  if (a.u_cls)
    for (int c = 0; c < a.ucls_cols; ++c) oc[1 + c] = a.u_cls[src * a.ucls_cols + c];
  if (a.out_logits)
    for (int c = 0; c < a.C; ++c) a.out_logits[(size_t)gid * a.C + c] = a.logits[src * a.C + c];
}

// per-class mode (postprocess.per_class_nms, :676-698): concatenate the per-class selections in
// class order, append M zero rows, take the top M by score (ties -> lower position), scale; no clip.
__global__ __launch_bounds__(256) void merge_per_class_kernel(MergeArgs a) {
  __shared__ unsigned long long wbest[4];
  __shared__ int offs[130];
  const int n = blockIdx.x;
  const int E_max = a.C * a.M + a.M;
  unsigned long long* keys = a.keys + (size_t)n * E_max;
  if (threadIdx.x == 0) {
    int run = 0;
    for (int c = 0; c < a.C; ++c) {
      if (c < 128) offs[c] = run;
      run += a.nsel[(size_t)n * a.C + c];
    }
    offs[128] = run;                         // number of real detections
  }
  __syncthreads();
  const int total_valid = offs[128];
  const int E = total_valid + a.M;
  // position e of entry (class c, rank j) in the concatenation; key = (score, earlier position first)
  for (int c = 0; c < a.C; ++c) {
    const size_t seg = (size_t)n * a.C + c;
    int start = 0;
    for (int cc = 0; cc < c; ++cc) start += a.nsel[(size_t)n * a.C + cc];
    for (int j = threadIdx.x; j < a.nsel[seg]; j += blockDim.x) {
      const int e = start + j;
      keys[e] = nms_key(a.sel_score[seg * a.M + j], e);
    }
  }
  for (int j = threadIdx.x; j < a.M; j += blockDim.x) {
    const int e = total_valid + j;
    keys[e] = nms_key(0.0f, e);
  }
  __syncthreads();
  const float sc = a.scales ? a.scales[n] : 1.0f;
  for (int r = 0; r < a.M; ++r) {
    unsigned long long best = 0ull;
    for (int e = threadIdx.x; e < E; e += blockDim.x) best = keys[e] > best ? keys[e] : best;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(best, off, 64);
      best = o > best ? o : best;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
    __syncthreads();
    best = wbest[0];
    for (int w = 1; w < 4; ++w) best = wbest[w] > best ? wbest[w] : best;
    const int e = (int)(0xFFFFFFFFu - (uint32_t)best);
    if (threadIdx.x == 0) {
      keys[e] = 0ull;                                   // taken
      const size_t o = (size_t)n * a.M + r;
      if (e < total_valid) {
        int c = 0, start = 0;
        while (c + 1 < a.C && e >= start + a.nsel[(size_t)n * a.C + c]) { start += a.nsel[(size_t)n * a.C + c]; ++c; }
        const size_t seg = (size_t)n * a.C + c;
        const int j = e - start;
        const int idx = a.sel_idx[seg * a.M + j];
        const float* bx = a.boxes + ((size_t)n * a.K + idx) * 4;
        for (int q = 0; q < 4; ++q) a.out_boxes[o * 4 + q] = a.scales ? bx[q] * sc : bx[q];
        a.out_scores[o] = a.sel_score[seg * a.M + j];
        a.out_classes[o] = (float)(c + 1);
      } else {
        for (int q = 0; q < 4; ++q) a.out_boxes[o * 4 + q] = a.scales ? 0.0f * sc : 0.0f;
        a.out_scores[o] = 0.0f;
        a.out_classes[o] = 0.0f;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) a.out_valid[n] = total_valid < a.M ? total_valid : a.M;
}

void launch_merge_per_class(const MergeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(merge_per_class_kernel, dim3(a.n_img), dim3(256), 0, s, a);
}

void launch_gather(const GatherArgs& a, hipStream_t s) {
  const int total = a.n_img * a.M;
  hipLaunchKernelGGL(gather_kernel, dim3((total + 127) / 128), dim3(128), 0, s, a);
}

// ------------------------------------------------------------------------------------ class probabilities
// What every caller does right after serve() (validate_model.py:159-166, infer_model.py:585-600,
// utils_class.py:36-41): p = stable_softmax(logits) and the entropy -sum p * log2(max(p, 1e-7)), float32.
__global__ __launch_bounds__(128) void probs_kernel(const float* logits, float* probs, float* entropy, int rows, int C) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const float* x = logits + (size_t)r * C;
  float mx = x[0];
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, x[c]);
  float sum = 0.f;
  for (int c = 0; c < C; ++c) sum += expf(x[c] - mx);
  float h = 0.f;
  for (int c = 0; c < C; ++c) {
    const float pc = expf(x[c] - mx) / sum;
    probs[(size_t)r * C + c] = pc;
    h += pc * log2f(fmaxf(pc, 1e-7f));
  }
  entropy[r] = -h;
}

void launch_probs(const float* logits, float* probs, float* entropy, int rows, int C, hipStream_t s) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(probs_kernel, dim3((rows + 127) / 128), dim3(128), 0, s, logits, probs, entropy, rows, C);
}

// ------------------------------------------------------------------------------------ packed detection records
// One float32 row per (image, detection): [boxes (bc) | score | classes (cc) | logits (C, optional) | valid_len] - the record
// the multi-GPU layer gathers (dist.pack_detections builds the same row on the host).  Rows of images >= n are zero: padding
// of a ragged shard up to the collective's common size.  The gather then reads this buffer in place: the detections never
// cross PCIe before they have been collected.
__global__ __launch_bounds__(256) void pack_det_kernel(PackDetArgs a) {
  const int64_t total = (int64_t)a.rows_out * a.M * a.cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int col = (int)(i % a.cols);
    const int64_t r = i / a.cols;               // image * M + detection
    const int img = (int)(r / a.M);
    float v = 0.f;
    if (img < a.n) {
      if (col < a.bc) v = a.boxes[r * a.bc + col];
      else if (col == a.bc) v = a.scores[r];
      else if (col < a.bc + 1 + a.cc) v = a.classes[r * a.cc + (col - a.bc - 1)];
      else if (col < a.bc + 1 + a.cc + a.C) v = a.logits[r * a.C + (col - a.bc - 1 - a.cc)];
      else v = (float)a.valid[img];
    }
    a.out[i] = v;
  }
}

void launch_pack_det(const PackDetArgs& a, hipStream_t s) {
  const int64_t total = (int64_t)a.rows_out * a.M * a.cols;
  if (total <= 0) return;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(pack_det_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------------------------ box-uncertainty calibration
// CalibrateBoxUncert.calibrate_boxuncert (utils_box.py:404-524) on the selected rows: temperature scaling
// (uncert / T) or isotonic regression tables (sklearn IsotonicRegression(out_of_bounds="clip").predict = linear
// interpolation between the fitted thresholds in float64, clipped to their range), one table for all values,
// one per box coordinate, or one per (class, coordinate); the relative variant divides by the box height /
// width in float16 first (the reference passes dtype=np.float16) and multiplies back afterwards.
__device__ __forceinline__ float iso_predict(const double* xs, const double* ys, int m, float v) {
  if (m <= 0) return 0.f;
  double x = (double)v;
  if (x <= xs[0]) return (float)ys[0];
  if (x >= xs[m - 1]) return (float)ys[m - 1];
  int lo = 0, hi = m - 1;                  // xs[lo] <= x < xs[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (xs[mid] <= x) lo = mid; else hi = mid;
  }
  const double slope = (ys[hi] - ys[lo]) / (xs[hi] - xs[lo]);
  return (float)(ys[lo] + slope * (x - xs[lo]));
}

__global__ __launch_bounds__(128) void calib_kernel(CalibArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.rows) return;
  const float* row = a.boxes + (size_t)r * a.box_cols;
  const int cls = (int)a.classes[(size_t)r * a.cls_cols];
  const float hgt = row[2] - row[0], wid = row[3] - row[1];
  for (int j = 0; j < 4; ++j) {
    float u = row[a.col0 + j];
    if (isnan(u)) u = 0.f;                 // np.nan_to_num
    else if (isinf(u)) u = u > 0 ? 3.4028234663852886e38f : -3.4028234663852886e38f;
    float o;
    if (a.mode == UDA_CALIB_TS_ALL) {
      o = u / a.temps[0];
    } else if (a.mode == UDA_CALIB_TS_PERCOO) {
      o = u / a.temps[j];
    } else {
      int t = 0;
      if (a.mode == UDA_CALIB_ISO_PERCOO) t = j;
      else if (a.mode == UDA_CALIB_ISO_PERCLSCOO) t = (cls - 1) * 4 + j;
      if (a.mode == UDA_CALIB_ISO_PERCLSCOO && (cls < 1 || cls > a.n_tables / 4)) {
        o = 0.f;                           // rows of no calibrated class stay zero (np.zeros_like)
      } else {
        const double* xs = a.xs + a.tab_off[t];
        const double* ys = a.ys + a.tab_off[t];
        const int m = a.tab_off[t + 1] - a.tab_off[t];
        if (a.relative) {
          const float norm = (j & 1) ? wid : hgt;
          float rel = 0.f;
          if (norm != 0.f) rel = __half2float(__float2half(__half2float(__float2half(u)) / __half2float(__float2half(norm))));
          o = iso_predict(xs, ys, m, rel) * norm;
        } else {
          o = iso_predict(xs, ys, m, u);
        }
      }
    }
    a.out[(size_t)r * 4 + j] = o;
  }
}

void launch_calib(const CalibArgs& a, hipStream_t s) {
  if (a.rows <= 0) return;
  hipLaunchKernelGGL(calib_kernel, dim3((a.rows + 127) / 128), dim3(128), 0, s, a);
}

// ------------------------------------------------------------------------------------ class calibration (row f2)
// CalibrateClass._perform_class_calib (utils_class.py:109-187) on the selected rows: temperature scaling of the logits
// (one temperature or one per class) followed by the stable softmax, or isotonic regression of the softmax
// probabilities (one table or one per class) followed by re-normalisation to sum 1; entropy -sum p log2(max(p, 1e-7)).
// With MC class uncertainty the reference draws 10 logit vectors from Normal(mean logits, MC std), calibrates each,
// and returns mean / population std of the calibrated probabilities and the entropy of the mean; the draws come from
// the build's Philox stream (philox_normal: counter (class, row, draw), tag 0x5A) instead of TFP's.
__device__ __forceinline__ void class_calib_one(const ClsCalibArgs& a, const float* z, float* p) {
  const int C = a.C;
  if (a.mode == UDA_CLS_TS) {
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) { p[c] = z[c] / a.temps[c]; mx = fmaxf(mx, p[c]); }
    float s = 0.f;
    for (int c = 0; c < C; ++c) { p[c] = expf(p[c] - mx); s = s + p[c]; }
    for (int c = 0; c < C; ++c) p[c] = p[c] / s;
    return;
  }
  float mx = -INFINITY;
  for (int c = 0; c < C; ++c) mx = fmaxf(mx, z[c]);
  float s = 0.f;
  for (int c = 0; c < C; ++c) { p[c] = expf(z[c] - mx); s = s + p[c]; }
  float t = 0.f;
  for (int c = 0; c < C; ++c) {
    const int tb = a.mode == UDA_CLS_ISO_ALL ? 0 : c;
    const int m = a.tab_off[tb + 1] - a.tab_off[tb];
    p[c] = iso_predict(a.xs + a.tab_off[tb], a.ys + a.tab_off[tb], m, p[c] / s);
    t = t + p[c];
  }
  for (int c = 0; c < C; ++c) p[c] = p[c] / t;
}

constexpr int CLS_MAX = 128;
__global__ __launch_bounds__(64) void class_calib_kernel(ClsCalibArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.rows) return;
  const int C = a.C;
  const float* lg = a.logits + (size_t)r * C;
  float z[CLS_MAX], p[CLS_MAX];
  float* out = a.probs + (size_t)r * C;
  if (a.draws <= 0) {
    for (int c = 0; c < C; ++c) z[c] = lg[c];
    class_calib_one(a, z, p);
    for (int c = 0; c < C; ++c) out[c] = p[c];
  } else {
    const float* sg = a.classes + (size_t)r * a.cls_cols + 1;
    float mean[CLS_MAX], sq[CLS_MAX];
    for (int c = 0; c < C; ++c) { mean[c] = 0.f; sq[c] = 0.f; }
    for (int d = 0; d < a.draws; ++d) {
      for (int c = 0; c < C; ++c) z[c] = lg[c] + sg[c] * (float)philox_normal(a.seed, (uint32_t)c, (uint32_t)r, (uint32_t)d, 0x5Au);
      class_calib_one(a, z, p);
      for (int c = 0; c < C; ++c) mean[c] = mean[c] + p[c];
    }
    for (int c = 0; c < C; ++c) mean[c] = mean[c] / (float)a.draws;
    for (int d = 0; d < a.draws; ++d) {           // second pass over the same draws: population std around the mean
      for (int c = 0; c < C; ++c) z[c] = lg[c] + sg[c] * (float)philox_normal(a.seed, (uint32_t)c, (uint32_t)r, (uint32_t)d, 0x5Au);
      class_calib_one(a, z, p);
      for (int c = 0; c < C; ++c) { const float dl = p[c] - mean[c]; sq[c] = sq[c] + dl * dl; }
    }
    for (int c = 0; c < C; ++c) {
      out[c] = mean[c];
      if (a.uncert) a.uncert[(size_t)r * C + c] = sqrtf(sq[c] / (float)a.draws);
      p[c] = mean[c];
    }
  }
  float h = 0.f;
  for (int c = 0; c < C; ++c) h = h + p[c] * log2f(fmaxf(p[c], 1e-7f));
  a.entropy[r] = -h;
}

void launch_class_calib(const ClsCalibArgs& a, hipStream_t s) {
  if (a.rows <= 0) return;
  hipLaunchKernelGGL(class_calib_kernel, dim3((a.rows + 63) / 64), dim3(64), 0, s, a);
}

// ------------------------------------------------------------------------------------ numpy NMS family (row a18)
// nms_np.hard_nms / diou_nms / soft_nms (reference src/nms_np.py:30-192): boxes x1,y1,x2,y2 with the +1 pixel
// convention.  One block per problem (a class of an image); T = double for the float64 arrays the family functions
// are called with directly, float for per_class_nms (float32 boxes / scores make every intermediate float32).
// hard / diou: the dets arrive sorted by score (descending, host side = argsort()[::-1]); box i is kept iff no kept
// box before it suppresses it - n greedy steps, the suppression test of a step spread over the block.
// soft (gaussian / linear): every step takes the arg-max of the current scores, emits it, rescales the others
// (exp(-iou^2 / sigma) or 1 - iou above the threshold) and drops those that fall below score_thresh.
template <typename T>
__device__ __forceinline__ T np_iou(const T* a, T area_a, const T* b, T area_b) {
  const T w = max((T)0, min(a[2], b[2]) - max(a[0], b[0]) + (T)1);
  const T h = max((T)0, min(a[3], b[3]) - max(a[1], b[1]) + (T)1);
  const T inter = w * h;
  return inter / (area_a + area_b - inter);
}

template <typename T>
__global__ __launch_bounds__(256) void nmsnp_kernel(NmsNpArgs<T> a) {
  __shared__ T red_v[256];
  __shared__ int red_i[256];
  __shared__ int s_cur, s_nout;
  const int pb = blockIdx.x;
  const int off = a.off[pb], n = a.off[pb + 1] - off;
  const T* d = a.dets + (size_t)off * 5;
  T* sc = a.score + off;          // working scores (soft) 
  int* st = a.state + off;        // 0 alive, 1 removed / emitted
  T* out = a.out + (size_t)off * 5;
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += 256) { sc[i] = d[i * 5 + 4]; st[i] = 0; }
  if (tid == 0) s_nout = 0;
  __syncthreads();
  if (a.method <= 1) {            // hard (0) / diou (1): input sorted by score, descending
    for (int i = 0; i < n; ++i) {
      if (st[i]) continue;        // uniform: st[] is only written before a barrier
      const T* bi = d + i * 5;
      const T ai = (bi[2] - bi[0] + (T)1) * (bi[3] - bi[1] + (T)1);
      for (int j = i + 1 + tid; j < n; j += 256) {
        if (st[j]) continue;
        const T* bj = d + j * 5;
        const T aj = (bj[2] - bj[0] + (T)1) * (bj[3] - bj[1] + (T)1);
        T v = np_iou(bi, ai, bj, aj);
        if (a.method == 1) {
          const T ex1 = min(bi[0], bj[0]), ex2 = max(bi[2], bj[2]), ey1 = min(bi[1], bj[1]), ey2 = max(bi[3], bj[3]);
          const T diag = (ex2 - ex1) * (ex2 - ex1) + (ey2 - ey1) * (ey2 - ey1);
          const T cxi = (bi[0] + bi[2]) / (T)2, cyi = (bi[1] + bi[3]) / (T)2;
          const T cxj = (bj[0] + bj[2]) / (T)2, cyj = (bj[1] + bj[3]) / (T)2;
          const T dist = (cxi - cxj) * (cxi - cxj) + (cyi - cyj) * (cyi - cyj);
          v = v - dist / (diag + (T)1e-10);
        }
        if (!(v <= a.iou_thr)) st[j] = 1;
      }
      if (tid == 0) {
        T* o = out + (size_t)s_nout * 5;
        for (int k = 0; k < 5; ++k) o[k] = bi[k];
        s_nout = s_nout + 1;
      }
      __syncthreads();
    }
  } else {                         // soft: gaussian (2) / linear (3)
    for (int step = 0; step < n; ++step) {
      T bv = -INFINITY;
      int bidx = -1;
      for (int i = tid; i < n; i += 256)
        if (!st[i] && (sc[i] > bv || bidx < 0)) { bv = sc[i]; bidx = i; }     // first maximum of this thread's stride
      red_v[tid] = bv; red_i[tid] = bidx;
      __syncthreads();
      for (int s2 = 128; s2 > 0; s2 >>= 1) {
        if (tid < s2) {
          const int oi = red_i[tid + s2];
          const T ov = red_v[tid + s2];
          const int mi = red_i[tid];
          if (oi >= 0 && (mi < 0 || ov > red_v[tid] || (ov == red_v[tid] && oi < mi))) { red_v[tid] = ov; red_i[tid] = oi; }
        }
        __syncthreads();
      }
      if (tid == 0) s_cur = red_i[0];
      __syncthreads();
      const int m = s_cur;
      if (m < 0) break;
      const T* bm = d + m * 5;
      const T am = (bm[2] - bm[0] + (T)1) * (bm[3] - bm[1] + (T)1);
      if (tid == 0) {
        T* o = out + (size_t)s_nout * 5;
        for (int k = 0; k < 4; ++k) o[k] = bm[k];
        o[4] = sc[m];
        s_nout = s_nout + 1;
        st[m] = 1;
      }
      __syncthreads();
      for (int j = tid; j < n; j += 256) {
        if (st[j]) continue;
        const T* bj = d + j * 5;
        const T aj = (bj[2] - bj[0] + (T)1) * (bj[3] - bj[1] + (T)1);
        const T v = np_iou(bm, am, bj, aj);
        T wgt;
        if (a.method == 2) wgt = (T)exp(-(v * v) / a.sigma);
        else wgt = (v > a.iou_thr) ? (T)1 - v : (T)1;
        const T ns = sc[j] * wgt;
        sc[j] = ns;
        if (!(ns >= a.score_thr)) st[j] = 1;
      }
      __syncthreads();
    }
  }
  if (tid == 0) a.n_out[pb] = s_nout;
}

template <typename T>
void launch_nmsnp(const NmsNpArgs<T>& a, int n_problems, hipStream_t s) {
  if (n_problems > 0) hipLaunchKernelGGL(nmsnp_kernel<T>, dim3(n_problems), dim3(256), 0, s, a);
}
template void launch_nmsnp<float>(const NmsNpArgs<float>&, int, hipStream_t);
template void launch_nmsnp<double>(const NmsNpArgs<double>&, int, hipStream_t);

}  // namespace uda
