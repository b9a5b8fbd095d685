// Validation uncertainty report: the tallies behind the reference's judgement of a box sigma - the header numbers and the ECE of
// ValidUncertPlot.__init__ (utils_extra.py:378-445), the line of RegressionCalib._conf_all (calibrate_regression.py:231-349) and
// calc_ece / calc_nll / calc_rmse (utils_box.py:17-102) - for B ragged segments of matched rows and K sigma columns in one call:
// uda_uncert_report_np (include/uda_hip.h).  Built without FMA contraction (csrc/Makefile): every product and sum below is rounded
// on its own, so that the sums equal the stated tree bit for bit and the level comparison is the one numpy evaluates.
//
//   uncert_report_kernel        one block of REPORT_ROWS threads per (run of REPORT_ROWS rows of a segment, sigma column); a lane
//                               holds one row.  Blocks of column 0 also do what belongs to the segment alone.
//   uncert_report_tree_kernel   one block per (segment, sum): folds the segment's run roots in place
//
// Counts.  A predicate is balloted over the wave and the popcount kept by ONE lane: lane i % 64 owns level i, so the 4 L ECE
// counters of a wave live in eight registers a lane and reach LDS once, the block's reach global memory once (integer atomics
// only - every count is exact however rows are dealt out).  The level test is `fabs(pred - gt) <= fabs(sigma * z[i])`, level by
// level: sigma = 0 with z = -inf gives NaN and false, an infinite sigma with z = 0 likewise - nothing is inferred from the order
// of the levels.
// Sums.  The zero-padded pairwise tree of DESIGN §21, in the statements of wave_fold.h: a row's term is fold4 of its four
// coordinates' terms, the wave folds its 64 rows (wave_tree_sum), the block its four wave roots (fold4), and the tree kernel the
// runs' roots in their power of two of slots (fold_slots_in_place), whatever REPORT_ROWS is.  A lane past the segment's end
// contributes +0.0, the padding.
#include "box_iou.h"
#include "uda_internal.h"
#include "wave_fold.h"

namespace uda {

#define REPORT_WAVES (REPORT_ROWS / 64)
#define REPORT_HALF_LOG_2PI 0.9189385332046727
static_assert(REPORT_WAVES == 4, "the block folds four wave roots: (w0 + w1) + (w2 + w3)");

__global__ __launch_bounds__(REPORT_ROWS) void uncert_report_kernel(ReportArgs a) {
  __shared__ double z_s[REPORT_MAX_L];
  __shared__ unsigned int ece_s[4 * REPORT_MAX_L];
  __shared__ unsigned int cnt_s[6];                         // covered | res nonzero | degenerate | iou zero | misclassified | gt nonzero
  __shared__ double sum_s[REPORT_SEG_SUMS + REPORT_COL_SUMS][REPORT_WAVES];
  const ReportItem it = a.items[blockIdx.x];
  const int k = blockIdx.y, K = a.K, L = a.L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t s0 = a.off[it.seg];
  const int n = (int)(a.off[it.seg + 1] - s0);
  for (int e = tid; e < L; e += REPORT_ROWS) z_s[e] = a.z[e];
  for (int e = tid; e < 4 * L; e += REPORT_ROWS) ece_s[e] = 0u;
  if (tid < 6) cnt_s[tid] = 0u;
  __syncthreads();

  // the lane's row; a lane past the end reads the run's first row (it exists) and counts for nothing
  const bool valid = it.row0 + tid < n;
  const size_t row = (size_t)(s0 + it.row0 + (valid ? tid : 0));
  double gt[4], pred[4], sg[4], res[4];
  for (int c = 0; c < 4; ++c) {
    gt[c] = a.gt[row * 4 + c];
    pred[c] = a.pred[row * 4 + c];
    sg[c] = a.sigma[((size_t)k * (size_t)a.rows + row) * 4 + c];
    res[c] = fabs(gt[c] - pred[c]);
  }

  // ---- per (segment, column)
  bool covered = valid;
  double t_s2[4], t_ue[4], t_nll[4];
  for (int c = 0; c < 4; ++c) {
    const double s = sg[c];
    covered = covered && (pred[c] - s <= gt[c]) && (gt[c] <= pred[c] + s);
    const bool nz = res[c] != 0.0, bad = s == 0.0 || !(s - s == 0.0);   // (s - s is 0 for a finite s only)
    const double u = s - res[c], y = res[c] / s;
    t_s2[c] = s * s;
    t_ue[c] = nz ? u * u : 0.0;
    t_nll[c] = bad ? 0.0 : (y * y / 2.0 + log(s)) + REPORT_HALF_LOG_2PI;
  }
  double v[REPORT_COL_SUMS + REPORT_SEG_SUMS];
  v[0] = valid ? fold4(t_s2) : 0.0;
  v[1] = valid ? fold4(t_ue) : 0.0;
  v[2] = valid ? fold4(t_nll) : 0.0;
  const unsigned int w_cov = wave_count(covered);
  // (4 elements a row: the element counts go through the wave as four ballots of one bit each)
  unsigned int w_res = 0, w_deg = 0;
  for (int c = 0; c < 4; ++c) {
    w_res += wave_count(valid && res[c] != 0.0);
    w_deg += wave_count(valid && (sg[c] == 0.0 || !(sg[c] - sg[c] == 0.0)));
  }

  // ---- per segment: column 0's blocks only (k is uniform over the block)
  int n_sums = REPORT_COL_SUMS;
  unsigned int w_iou0 = 0, w_mis = 0, w_gnz = 0;
  if (k == 0) {
    const double iou = glc_iou(gt, pred);
    double t_sq[4];
    for (int c = 0; c < 4; ++c) {
      const double d = pred[c] - gt[c];
      t_sq[c] = gt[c] != 0.0 ? d * d : 0.0;
      w_gnz += wave_count(valid && gt[c] != 0.0);
    }
    v[3] = valid ? iou : 0.0;
    v[4] = valid ? fold4(t_sq) : 0.0;
    w_iou0 = wave_count(valid && iou == 0.0);
    w_mis = wave_count(valid && a.gt_class[row] != a.cls[row]);
    n_sums += REPORT_SEG_SUMS;
  }
  for (int j = 0; j < n_sums; ++j) {
    const double root = wave_tree_sum(v[j]);
    if (lane == 0) sum_s[j][wave] = root;
  }
  if (lane == 0) {
    atomicAdd(&cnt_s[0], w_cov); atomicAdd(&cnt_s[1], w_res); atomicAdd(&cnt_s[2], w_deg);
    if (k == 0) { atomicAdd(&cnt_s[3], w_iou0); atomicAdd(&cnt_s[4], w_mis); atomicAdd(&cnt_s[5], w_gnz); }
  }

  // ---- the level counts: every lane takes every step (the ballot sees all 64 lanes)
  for (int c = 0; c < 4; ++c) {
    const double r = res[c], s = sg[c];
    unsigned int lo = 0, hi = 0;                            // the counts of levels `lane` and `64 + lane`
    const int L0 = L < 64 ? L : 64;
    for (int i = 0; i < L0; ++i) {
      const unsigned int pc = wave_count(valid && r <= fabs(s * z_s[i]));
      lo += lane == i ? pc : 0u;
    }
    for (int i = 64; i < L; ++i) {
      const unsigned int pc = wave_count(valid && r <= fabs(s * z_s[i]));
      hi += lane == i - 64 ? pc : 0u;
    }
    if (lane < L && lo) atomicAdd(&ece_s[c * L + lane], lo);
    if (64 + lane < L && hi) atomicAdd(&ece_s[c * L + 64 + lane], hi);
  }
  __syncthreads();

  // ---- the block's share: run roots to the partials, counts to global memory
  if (tid < n_sums) {
    const double root = fold4(sum_s[tid]);
    const int sum_id = tid < REPORT_COL_SUMS ? REPORT_SEG_SUMS + REPORT_COL_SUMS * k + tid : tid - REPORT_COL_SUMS;
    a.partials[(size_t)sum_id * (size_t)a.slots + it.slot] = root;
  }
  if (tid < 3) {
    if (cnt_s[tid]) atomicAdd(a.col_counts + ((size_t)it.seg * K + k) * 3 + tid, (unsigned long long)cnt_s[tid]);
  } else if (tid < 6 && k == 0) {
    if (cnt_s[tid]) atomicAdd(a.seg_counts + (size_t)it.seg * 4 + (tid - 2), (unsigned long long)cnt_s[tid]);
  }
  unsigned long long* ece = a.ece_count + ((size_t)it.seg * K + k) * 4 * (size_t)L;
  for (int e = tid; e < 4 * L; e += REPORT_ROWS)
    if (ece_s[e]) atomicAdd(ece + e, (unsigned long long)ece_s[e]);
}

// folds the slots of one (segment, sum) in place, the whole block on one sum.  P is a power of two (0: the segment is empty,
// its sums stay 0) and uniform over the block: so are the barriers.
__global__ __launch_bounds__(256) void uncert_report_tree_kernel(ReportArgs a) {
  const int b = blockIdx.x, sum_id = blockIdx.y;
  const int P = (int)(a.pbase[b + 1] - a.pbase[b]);
  double* buf = a.partials + (size_t)sum_id * (size_t)a.slots + a.pbase[b];
  fold_slots_in_place(buf, P, (int)threadIdx.x, 256, true);
  if (threadIdx.x == 0 && P > 0) {
    if (sum_id < REPORT_SEG_SUMS) a.seg_sums[(size_t)b * REPORT_SEG_SUMS + sum_id] = buf[0];
    else a.col_sums[(size_t)b * a.K * REPORT_COL_SUMS + (sum_id - REPORT_SEG_SUMS)] = buf[0];
  }
}

void launch_uncert_report(const ReportArgs& a, hipStream_t s) {
  if (a.n_items > 0) hipLaunchKernelGGL(uncert_report_kernel, dim3((unsigned)a.n_items, (unsigned)a.K), dim3(REPORT_ROWS), 0, s, a);
  hipLaunchKernelGGL(uncert_report_tree_kernel, dim3((unsigned)a.B, (unsigned)(REPORT_SEG_SUMS + REPORT_COL_SUMS * a.K)), dim3(256), 0, s, a);
}

}  // namespace uda
