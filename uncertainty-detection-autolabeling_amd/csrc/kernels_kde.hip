// Gaussian KDE kernels (gfx950): for a batch of ragged problems, the sum over a problem's whitened data rows of
// w_i * exp(-|p - d_i|^2 / 2) at every whitened evaluation point, in float64 - scipy.stats.gaussian_kde evaluated on a mesh, the
// one expensive step of the epistemic-vs-aleatoric comparison (reference uncertainty_ep_vs_al.py:361-375; see DESIGN.md
// "Epistemic vs aleatoric").  Whitening and the normalisation are the caller's.
//
//   kde_eval_kernel<D, W>   per work item (problem, point tile, span of runs): every thread's sequential sum over each run of the
//                           span, stored to run_sums [runs, points]
//   kde_tree_kernel         per point: folds its run sums in place as the zero-padded pairwise tree, the root to sum
//
// Tiling as in knn_min_kernel: a block is KDE_POINTS evaluation points, one per thread, the D coordinates in registers; it stages
// one run of KDE_RUN data rows and their weights in LDS, where all lanes read the same address (a broadcast), and walks the runs of
// its span.  arg = ((p0-d0)^2 + (p1-d1)^2) + ..., coordinates ascending, every operation rounded on its own (the file is built
// without contraction); the term is w * exp(arg * -0.5), exp being the float64 library function.  A run is summed row by row from
// 0.0, so its sum depends on the run's rows alone; which block sums it, and beside which other points, changes nothing.  There is
// no atomic: every element of run_sums has one writer, the tree launch starts after the first has ended, and a thread of the tree
// launch reads and writes its own point's column only.
#include "uda_internal.h"

namespace uda {

template <int D, bool W>
__global__ __launch_bounds__(KDE_POINTS) void kde_eval_kernel(KdeArgs a) {
  __shared__ double tile[KDE_RUN * D];
  __shared__ double wt[W ? KDE_RUN : 1];
  const KdeItem it = a.items[blockIdx.x];
  const int64_t d0 = a.d_off[it.problem], p0 = a.p_off[it.problem];
  const int n = (int)(a.d_off[it.problem + 1] - d0), m = (int)(a.p_off[it.problem + 1] - p0);
  const int own = it.point0 + (int)threadIdx.x;               // the point's index inside its problem
  const bool live = own < m;
  const int row = live ? own : m - 1;                         // the lanes past the end repeat the last point and write nothing
  double x[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = a.points[(size_t)(p0 + row) * D + k];
  double* out = a.run_sums + a.s_off[it.problem] + own;       // run r of this point: out[r * m]
  for (int r = it.r0; r < it.r1; ++r) {
    const int i0 = r * KDE_RUN, nc = min((int)KDE_RUN, n - i0);
    const double* src = a.data + (size_t)(d0 + i0) * D;
    __syncthreads();
    for (int t = threadIdx.x; t < nc * D; t += KDE_POINTS) tile[t] = src[t];
    if (W && (int)threadIdx.x < nc) wt[threadIdx.x] = a.weight[d0 + i0 + threadIdx.x];   // KDE_RUN <= KDE_POINTS
    __syncthreads();
    double acc = 0.0;
#pragma unroll 4
    for (int j = 0; j < nc; ++j) {
      const double* y = tile + j * D;
      const double e0 = x[0] - y[0];
      double arg = e0 * e0;
#pragma unroll
      for (int k = 1; k < D; ++k) {
        const double e = x[k] - y[k];
        arg = arg + e * e;
      }
      double t = exp(arg * -0.5);
      if (W) t = wt[j] * t;
      acc = acc + t;
    }
    if (live) out[(size_t)r * m] = acc;
  }
}

// folds the point's R run sums, column `own` of the problem's [R, m] block: at stride s run j (a multiple of 2 s) takes run
// j + s, or 0.0 where the zero padding begins - b = b[0::2] + b[1::2] over the terms padded to a power of two
__global__ __launch_bounds__(KDE_POINTS) void kde_tree_kernel(KdeArgs a) {
  const KdeTile tl = a.tiles[blockIdx.x];
  const int64_t d0 = a.d_off[tl.problem], p0 = a.p_off[tl.problem];
  const int n = (int)(a.d_off[tl.problem + 1] - d0), m = (int)(a.p_off[tl.problem + 1] - p0);
  const int own = tl.point0 + (int)threadIdx.x;
  if (own >= m) return;
  const int R = (n + KDE_RUN - 1) / KDE_RUN;
  double* col = a.run_sums + a.s_off[tl.problem] + own;
  for (int s = 1; s < R; s <<= 1)
    for (int j = 0; j < R; j += 2 * s) col[(size_t)j * m] = col[(size_t)j * m] + (j + s < R ? col[(size_t)(j + s) * m] : 0.0);
  a.sum[p0 + own] = col[0];
}

template <int D>
static void launch_kde_eval_d(const KdeArgs& a, hipStream_t s) {
  const dim3 grid(a.n_items), block(KDE_POINTS);
  if (a.weight) hipLaunchKernelGGL((kde_eval_kernel<D, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((kde_eval_kernel<D, false>), grid, block, 0, s, a);
}

void launch_kde_eval(const KdeArgs& a, hipStream_t s) {
  static_assert(KDE_RUN <= KDE_POINTS, "one thread stages one weight of a run");
  if (a.n_items < 1) return;                                   // no problem has a point
  switch (a.D) {
    case 1: launch_kde_eval_d<1>(a, s); break;
    case 2: launch_kde_eval_d<2>(a, s); break;
    case 3: launch_kde_eval_d<3>(a, s); break;
    case 4: launch_kde_eval_d<4>(a, s); break;
    default: abort();                                          // the entry point refuses every other D
  }
  hipLaunchKernelGGL(kde_tree_kernel, dim3(a.n_tiles), dim3(KDE_POINTS), 0, s, a);
}

}  // namespace uda
