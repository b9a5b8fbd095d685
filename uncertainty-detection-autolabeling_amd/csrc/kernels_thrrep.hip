// Thresholding report: what the reference's judgement of a failure-recognition score needs beside the ROC curve
// (MainUncertViz._save_thr_performance / _collect_thresh_results, uncertainty_analysis.py:517-749, with calc_jsd,
// utils_extra.py:25-36) for B row segments x S score columns x K IoU thresholds: uda_thr_report_np (include/uda_hip.h).  The curves
// themselves are the objective's kernels (kernels_post.hip) on the segment's rows.  Built without FMA contraction (csrc/Makefile):
// every difference, product and sum below is rounded on its own, so that the sums equal the stated tree bit for bit.
//
//   thr_report_fill_kernel   (+inf, NaN, NaN) into every slot of roc: what a segment too short for a curve keeps
//   thr_report_kernel        one block of THRREP_ROWS threads per (threshold, column, segment), two passes over the segment's rows,
//                            THRREP_UNROLL runs of THRREP_ROWS rows between two barriers
//
// Counts.  A predicate is balloted over the wave and the popcount added to a wave-uniform register; the four waves meet in LDS
// once.  No atomics at all: a block owns its outputs.
// Sums.  -0.0 counts as 0.0 (as in the curve), a row outside the subset or past the segment's end contributes +0.0.  A run of
// THRREP_ROWS rows, counted from the segment's first row, is folded over the wave (wave_tree_sum) and over its four wave roots
// (fold4); the run roots are folded by the binary counter (run_tree_push, run_tree_root), all in one block.  That is the
// zero-padded pairwise tree of DESIGN §21 as wave_fold.h states it; no term is -0.0, so it does not matter how far the padding goes.
#include "uda_internal.h"
#include "wave_fold.h"

namespace uda {

static_assert(THRREP_ROWS == 256, "the block folds four wave roots: (w0 + w1) + (w2 + w3)");
static_assert((UDA_THR_MAX_N + THRREP_ROWS - 1) / THRREP_ROWS <= (1 << (RUN_TREE_LEVELS - 1)), "levels of the run tree");

__global__ __launch_bounds__(256) void thr_report_fill_kernel(double* roc, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  roc[3 * i] = __longlong_as_double(0x7ff0000000000000ll);
  roc[3 * i + 1] = roc[3 * i + 2] = __longlong_as_double(0x7ff8000000000000ll);
}

// one pass over the segment's rows for threads 0 and 1's trees: THRREP_UNROLL runs between two barriers, their loads in flight
// together.  SECOND: the terms are (u - mean)^2 about the subset's mean; else u itself, and the four counts are taken
template <bool SECOND>
__device__ __forceinline__ void thrrep_pass(const double* u, const uint32_t* m, int n, int k, double thr, double mean0, double mean1,
                                            double (*root_s)[THRREP_UNROLL][THRREP_ROWS / 64], double (*stack_s)[RUN_TREE_LEVELS],
                                            unsigned long long* counts) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int runs = (n + THRREP_ROWS - 1) / THRREP_ROWS;
  for (int run0 = 0; run0 < runs; run0 += THRREP_UNROLL) {
    double v[THRREP_UNROLL];
    uint32_t bits[THRREP_UNROLL];
#pragma unroll
    for (int r = 0; r < THRREP_UNROLL; ++r) {
      const int i = (run0 + r) * THRREP_ROWS + tid;
      const bool valid = i < n;
      v[r] = valid ? u[i] : 0.0;
      bits[r] = valid ? ((m[i] >> k) & 1u) | 2u : 0u;       // bit 0: correct, bit 1: a row of the segment
    }
#pragma unroll
    for (int r = 0; r < THRREP_UNROLL; ++r) {
      if (v[r] == 0.0) v[r] = 0.0;
      const bool cor = bits[r] == 3u, wrong = bits[r] == 2u;
      double t0, t1;
      if (SECOND) {
        const double d0 = __dsub_rn(v[r], mean0), d1 = __dsub_rn(v[r], mean1);
        t0 = __dmul_rn(d0, d0);
        t1 = __dmul_rn(d1, d1);
      } else {
        t0 = t1 = v[r];
        counts[0] += wave_count(cor);
        counts[1] += wave_count(wrong && v[r] >= thr);
        counts[2] += wave_count(cor && v[r] >= thr);
        counts[3] += wave_count(wrong && v[r] < thr);
      }
      const double r0 = wave_tree_sum(cor ? t0 : 0.0), r1 = wave_tree_sum(wrong ? t1 : 0.0);
      if (lane == 0) { root_s[0][r][wave] = r0; root_s[1][r][wave] = r1; }
    }
    __syncthreads();
    if (tid < 2)
      for (int r = 0; r < THRREP_UNROLL && run0 + r < runs; ++r) run_tree_push(stack_s[tid], run0 + r, fold4(root_s[tid][r]));
    __syncthreads();
  }
}

__global__ __launch_bounds__(THRREP_ROWS) void thr_report_kernel(ThrRepArgs a) {
  __shared__ double root_s[2][THRREP_UNROLL][THRREP_ROWS / 64];
  __shared__ double stack_s[2][RUN_TREE_LEVELS];
  __shared__ double mean_s[2];
  __shared__ unsigned long long cnt_s[THRREP_ROWS / 64][4];
  const int k = blockIdx.x, s = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lo = a.seg_lo[b], n = a.seg_hi[b] - lo;
  if (n <= 0) return;                                       // (uniform; the outputs were zeroed)
  const size_t slot = ((size_t)b * a.S + s) * a.K + k;
  const double thr = a.roc[slot * 3];
  const double* u = a.scores + (size_t)s * a.N + lo;
  const uint32_t* m = a.mask + lo;
  const int runs = (n + THRREP_ROWS - 1) / THRREP_ROWS;

  // ---- pass 1: counts (this wave's rows: correct | correctly removed | falsely removed | falsely remaining), the two sums
  unsigned long long c[4] = {0, 0, 0, 0};
  thrrep_pass<false>(u, m, n, k, thr, 0.0, 0.0, root_s, stack_s, c);
  if (lane == 0)
    for (int j = 0; j < 4; ++j) cnt_s[wave][j] = c[j];
  __syncthreads();
  const unsigned long long n_cor = fold4(&cnt_s[0][0], 4);  // (the waves' counts of one kind lie 4 apart)
  const unsigned long long n_sub = tid == 0 ? n_cor : (unsigned long long)n - n_cor;      // read by threads 0 and 1
  if (tid < 2) {
    const double sum = n_sub ? run_tree_root(stack_s[tid], runs) : 0.0;
    mean_s[tid] = n_sub ? sum / (double)n_sub : 0.0;
    a.moments[slot * 4 + 2 * tid] = sum;
  } else if (tid < 5) {
    const int j = tid - 1;
    a.removed[slot * 3 + (j - 1)] = (long long)fold4(&cnt_s[0][j], 4);
  } else if (tid < 7 && s == 0) {
    a.n_label[((size_t)b * a.K + k) * 2 + (tid - 5)] = (long long)(tid == 5 ? n_cor : (unsigned long long)n - n_cor);
  }
  __syncthreads();

  // ---- pass 2: the sums of (u - mean)^2, each subset about its own mean
  thrrep_pass<true>(u, m, n, k, thr, mean_s[0], mean_s[1], root_s, stack_s, c);
  if (tid < 2) a.moments[slot * 4 + 2 * tid + 1] = n_sub ? run_tree_root(stack_s[tid], runs) : 0.0;
}

void launch_thr_report_fill(const ThrRepArgs& a, hipStream_t s) {
  const long long n = (long long)a.B * a.S * a.K;
  hipLaunchKernelGGL(thr_report_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.roc, n);
}

void launch_thr_report(const ThrRepArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(thr_report_kernel, dim3((unsigned)a.K, (unsigned)a.S, (unsigned)a.B), dim3(THRREP_ROWS), 0, s, a);
}

}  // namespace uda
