// Nearest-neighbour kernels (gfx950): the squared distance from every query point to its nearest reference point, in float64,
// for a batch of ragged problems in one launch - the neighbour search of the set-similarity analysis (reference
// active_learning_eval.py:481-487, four KD-trees per (class, method); see DESIGN.md "Set similarity").
//
//   knn_fill_kernel     d2[i] = the bits of +inf
//   knn_min_kernel<D>   per work item (problem, row block, column span): every thread's minimum over the span, combined into d2
//
// Tiling as in prune_walk_kernel: a block is KNN_ROWS query points, one per thread, the D coordinates in registers; it stages
// KNN_COLS reference points at a time in LDS, where all lanes read the same address (a broadcast), and walks the chunks of its
// column span.  d2(i, j) = ((x0-y0)^2 + (x1-y1)^2) + ..., coordinates ascending, every operation rounded on its own (the file is
// built without contraction).  A squared distance is never negative and never NaN for finite coordinates, so its bit pattern
// orders like its value: the spans of one query combine by a 64-bit integer atomicMin, which does not care who comes first.
// Nothing inside a launch reads what another block of that launch wrote; the host reads d2 after the launch has ended.
#include "uda_internal.h"

namespace uda {

__global__ __launch_bounds__(256) void knn_fill_kernel(unsigned long long* d2, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total) d2[i] = 0x7FF0000000000000ull;
}

// the chunk in LDS against the thread's point; SKIP: the chunk holds rows of the block itself (a self problem), column `own` is
// the thread's own point and is left out
template <int D, bool SKIP>
__device__ __forceinline__ double knn_chunk_min(const double (&x)[D], const double* tile, int nc, int own_col, double best) {
  for (int j = 0; j < nc; ++j) {
    const double* y = tile + j * D;
    const double e0 = x[0] - y[0];
    double d2 = e0 * e0;
#pragma unroll
    for (int k = 1; k < D; ++k) {
      const double e = x[k] - y[k];
      d2 = d2 + e * e;
    }
    if (SKIP && j == own_col) continue;
    best = fmin(d2, best);                                     // one v_min_f64; no NaN arises from finite coordinates
  }
  return best;
}

template <int D>
__global__ __launch_bounds__(KNN_ROWS) void knn_min_kernel(KnnArgs a) {
  __shared__ double tile[KNN_COLS * D];
  const KnnItem it = a.items[blockIdx.x];
  const int64_t q0 = a.q_off[it.problem], r0 = a.r_off[it.problem];
  const int n = (int)(a.q_off[it.problem + 1] - q0), m = (int)(a.r_off[it.problem + 1] - r0);
  const bool self = a.self != nullptr && a.self[it.problem] != 0;
  const int own = it.row0 + (int)threadIdx.x;                 // the query's index inside its problem
  const bool live = own < n;
  const int row = live ? own : n - 1;                         // the lanes past the end repeat the last point and write nothing
  double x[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = a.queries[(size_t)(q0 + row) * D + k];
  double best = __longlong_as_double(0x7FF0000000000000ll);
  for (int c = it.c0; c < it.c1; ++c) {
    const int j0 = c * KNN_COLS, nc = min((int)KNN_COLS, m - j0);
    const double* src = a.refs + (size_t)(r0 + j0) * D;
    __syncthreads();
    for (int t = threadIdx.x; t < nc * D; t += KNN_ROWS) tile[t] = src[t];
    __syncthreads();
    if (self && j0 < it.row0 + KNN_ROWS && j0 + nc > it.row0)  // block-uniform
      best = knn_chunk_min<D, true>(x, tile, nc, row - j0, best);
    else
      best = knn_chunk_min<D, false>(x, tile, nc, 0, best);
  }
  if (live) atomicMin(a.d2_bits + q0 + own, (unsigned long long)__double_as_longlong(best));
}

void launch_knn_min(const KnnArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(knn_fill_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, s, a.d2_bits, a.total);
  const dim3 grid(a.n_items), block(KNN_ROWS);
  switch (a.D) {
    case 1: hipLaunchKernelGGL(knn_min_kernel<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(knn_min_kernel<2>, grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL(knn_min_kernel<3>, grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL(knn_min_kernel<4>, grid, block, 0, s, a); break;
    default: abort();                                          // the entry point refuses every other D
  }
}

}  // namespace uda
