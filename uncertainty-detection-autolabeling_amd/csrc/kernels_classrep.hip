// Classification calibration report: the tallies behind the reliability diagrams of the reference's ClassificationCalib
// (calibrate_classification.py:97-143 `_calibr_bins`, 250-440 `_calibr_plot`) - per class and over the arg-max class, for B ragged
// segments of rows and M probability tables in one call: uda_class_report_np (include/uda_hip.h).  Built without FMA contraction
// (csrc/Makefile): every difference, product and sum below is rounded on its own, so that the sums equal the stated tree bit for bit.
//
//   class_report_kernel        one block of CLASSREP_ROWS threads per (run of CLASSREP_ROWS rows of a segment, table); a lane holds
//                              one row and the block walks the C + 1 targets.  A probability is read once: the walk over the classes
//                              also keeps the row's sum (left to right), its arg-max, its non-finite flag and the label's entry,
//                              from which target C and the NLL term follow
//   class_report_tree_kernel   one wave per (segment of more than one run, sum): folds the segment's run roots in place
//
// Bin id.  The edges of the target sit in LDS; the id is the number of edges e with !(x < e) - np.digitize for ascending edges, a
// NaN lands in id n_edges.
// Counts.  `id == k` is balloted over the wave, the popcounts of the ballot and of `id == k && ytrue` go to the wave's LDS slot and
// the block's total reaches global memory by one integer atomic a (target, bin): every count is exact however rows are dealt out.
// Sums.  The zero-padded pairwise tree of DESIGN §21, in the statements of wave_fold.h: the wave folds its 64 terms
// (wave_tree_sum), the block its four wave roots (fold4) and the tree kernel the runs' roots (fold_slots_in_place).  The term of
// a row outside the bin is +0.0.  A bin no row of the wave falls into is skipped (its root is the +0.0 the tree of zeros gives).
// A segment of ONE run needs no second fold: its block writes the outputs itself.
#include "uda_internal.h"
#include "wave_fold.h"

namespace uda {

#define CLASSREP_WAVES (CLASSREP_ROWS / 64)
#define CLASSREP_SLOTS (CLASSREP_MAX_E + 1)
static_assert(CLASSREP_WAVES == 4, "the block folds four wave roots: (w0 + w1) + (w2 + w3)");
static_assert(CLASSREP_SLOTS + 1 <= CLASSREP_ROWS, "one finishing thread a bin slot and one for the Brier sum");

// where sum r of (segment, table) goes: r < (C + 1) * (E + 1) a bin sum, then the C Brier sums, then the NLL sum
__device__ __forceinline__ double* classrep_out(const ClassRepArgs& a, int seg, int m, int r) {
  const int n_bins = (a.C + 1) * (a.E + 1);
  const size_t sm = (size_t)seg * a.M + m;
  if (r < n_bins) return a.bin_sum + sm * n_bins + r;
  if (r < n_bins + a.C) return a.brier_sum + sm * a.C + (r - n_bins);
  return a.nll_sum + sm;
}

__global__ __launch_bounds__(CLASSREP_ROWS) void class_report_kernel(ClassRepArgs a) {
  __shared__ double ed_s[CLASSREP_MAX_E];
  __shared__ double sum_s[2][CLASSREP_SLOTS + 1][CLASSREP_WAVES];      // (slot CLASSREP_SLOTS: the Brier term) two targets in flight
  __shared__ unsigned int cnt_s[2][CLASSREP_SLOTS][CLASSREP_WAVES], hit_s[2][CLASSREP_SLOTS][CLASSREP_WAVES];
  __shared__ double nll_s[CLASSREP_WAVES];
  __shared__ unsigned int tab_s[2][CLASSREP_WAVES];
  const ClassRepItem it = a.items[blockIdx.x];
  const int m = blockIdx.y, M = a.M, C = a.C, E = a.E;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t s0 = a.off[it.seg];
  const int n = (int)(a.off[it.seg + 1] - s0);
  const int S = (C + 1) * (E + 1) + C + 1;                             // float64 sums of a (segment, table)
  const size_t sm = (size_t)it.seg * M + m;

  // the lane's row; a lane past the end reads the run's first row (it exists) and counts for nothing
  const bool valid = it.row0 + tid < n;
  const size_t row = (size_t)(s0 + it.row0 + (valid ? tid : 0));
  const double* p_row = a.prob + ((size_t)m * (size_t)a.rows + row) * (size_t)C;
  const int label = a.label[row];

  // a sum's place: the output itself for a segment of one run, else the run's slot of the partials
  auto place = [&](int r) -> double* {
    return it.slot < 0 ? classrep_out(a, it.seg, m, r) : a.partials + ((size_t)m * S + r) * (size_t)a.slots + it.slot;
  };

  double rowsum = 0.0, best = 0.0, p_label = 0.0;
  int amax = 0;
  bool has_nan = false, non_finite = false;
  for (int t = 0; t <= C; ++t) {                                       // (t is uniform over the block: so are the barriers)
    const int g = a.G == 1 ? 0 : (int)(sm * (C + 1) + t);
    const int ne = a.n_edges[g];
    if (t == 0 || a.G != 1) {                                          // every thread left the last target's edges behind the barrier below
      for (int e = tid; e < ne; e += CLASSREP_ROWS) ed_s[e] = a.edges[(size_t)g * E + e];
      __syncthreads();
    }
    double x;
    bool y;
    if (t < C) {
      x = p_row[t];
      y = label == t;
      rowsum = rowsum + x;
      non_finite = non_finite || !(x - x == 0.0);                      // (x - x is 0 for a finite x only)
      if (t == label) p_label = x;
      if (!has_nan) {                                                  // numpy.argmax: the first NaN, else the first maximum
        if (x != x) { has_nan = true; amax = t; best = x; }
        else if (t == 0 || x > best) { amax = t; best = x; }
      }
    } else {
      x = best;
      y = label == amax;
    }
    int id = 0;
    for (int e = 0; e < ne; ++e) id += !(x < ed_s[e]) ? 1 : 0;
    const int buf = t & 1;
    for (int k = 0; k <= ne; ++k) {
      const bool in = valid && id == k;
      const unsigned long long mask = __ballot(in);
      unsigned int c = 0, h = 0;
      double root = 0.0;
      if (mask != 0ull) {                                              // (uniform over the wave)
        c = (unsigned int)__popcll(mask);
        h = wave_count(in && y);
        root = wave_tree_sum(in ? x : 0.0);
      }
      if (lane == 0) { sum_s[buf][k][wave] = root; cnt_s[buf][k][wave] = c; hit_s[buf][k][wave] = h; }
    }
    if (t < C) {
      const double d = x - (y ? 1.0 : 0.0);
      const double root = wave_tree_sum(valid ? d * d : 0.0);
      if (lane == 0) sum_s[buf][CLASSREP_SLOTS][wave] = root;
    }
    __syncthreads();
    // ---- the block's share of target t.  The next target fills the other half of the buffers and the one after it comes behind
    // the next barrier, which these threads reach only after they have read.
    if (tid <= ne) {
      *place(t * (E + 1) + tid) = fold4(sum_s[buf][tid]);
      const unsigned int c = fold4(cnt_s[buf][tid]), h = fold4(hit_s[buf][tid]);
      const size_t o = (sm * (C + 1) + t) * (size_t)(E + 1) + tid;
      if (c) atomicAdd(a.bin_count + o, (unsigned long long)c);
      if (h) atomicAdd(a.bin_hits + o, (unsigned long long)h);
    } else if (tid == CLASSREP_ROWS - 1 && t < C) {
      *place((C + 1) * (E + 1) + t) = fold4(sum_s[buf][CLASSREP_SLOTS]);
    }
  }

  // ---- the row's NLL term: -log(clip(prob[label] / rowsum)); a row with a non-finite entry or a zero sum is left out and counted
  const bool out = non_finite || rowsum == 0.0;
  const double q = p_label / rowsum;
  const bool clipped = valid && !out && (q < 1e-7 || q > 1.0 - 1e-7);
  const double qc = q < 1e-7 ? 1e-7 : (q > 1.0 - 1e-7 ? 1.0 - 1e-7 : q);
  const double term = (valid && !out) ? -log(qc) : 0.0;
  const double root = wave_tree_sum(term);
  const unsigned int w_clip = wave_count(clipped), w_out = wave_count(valid && out);
  if (lane == 0) { nll_s[wave] = root; tab_s[0][wave] = w_clip; tab_s[1][wave] = w_out; }
  __syncthreads();
  if (tid == 0) *place((C + 1) * (E + 1) + C) = fold4(nll_s);
  if (tid < 2) {
    const unsigned int c = fold4(tab_s[tid]);
    if (c) atomicAdd(a.tab_counts + sm * 2 + tid, (unsigned long long)c);
  }
}

// folds the slots of one (segment, sum) in place, a wave a sum.  P is a power of two, at least 2, and the same for the four sums
// of a block (they belong to one segment): so are the barriers, which a wave without a sum takes too.
__global__ __launch_bounds__(256) void class_report_tree_kernel(ClassRepArgs a) {
  const int seg = a.tree_segs[blockIdx.y];
  const int S = (a.C + 1) * (a.E + 1) + a.C + 1;
  const int sum_id = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  const bool mine = sum_id < a.M * S;
  const int P = (int)(a.pbase[seg + 1] - a.pbase[seg]);
  double* buf = a.partials + (size_t)(mine ? sum_id : 0) * (size_t)a.slots + a.pbase[seg];
  fold_slots_in_place(buf, P, lane, 64, mine);
  if (mine && lane == 0) *classrep_out(a, seg, sum_id / S, sum_id % S) = buf[0];
}

void launch_class_report(const ClassRepArgs& a, hipStream_t s) {
  if (a.n_items > 0) hipLaunchKernelGGL(class_report_kernel, dim3((unsigned)a.n_items, (unsigned)a.M), dim3(CLASSREP_ROWS), 0, s, a);
  const int S = (a.C + 1) * (a.E + 1) + a.C + 1;
  if (a.n_tree > 0)
    hipLaunchKernelGGL(class_report_tree_kernel, dim3((unsigned)((a.M * S + 3) / 4), (unsigned)a.n_tree), dim3(256), 0, s, a);
}

}  // namespace uda
