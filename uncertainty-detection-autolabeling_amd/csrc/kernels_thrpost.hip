// Post-thresholding analysis: where in the image and on which images the failure-recognition threshold acts
// (MainUncertViz._plot_validheat, _plot_metricsspider, _collect_postthresholding, uncertainty_analysis.py:838-880, :920-1068):
// uda_heat_maps_np and uda_thr_post_np (include/uda_hip.h).  Built without FMA contraction (csrc/Makefile): every addition and the
// one division below are rounded on their own.
//
//   heat_maps_kernel   one block of HEAT_CHUNK threads per (tile of HEAT_TILE_H x HEAT_TILE_W pixels, map); a thread owns HEAT_PX
//                      pixels of one column of the tile and keeps their float64 sums and int counts in registers
//   thr_post_kernel    one block of THRPOST_ROWS threads per IoU threshold, THRPOST_UNROLL runs of rows between two barriers
//
// Heat maps.  numpy's `mask[r0:r1, c0:c1] += v[i]` once per row i adds, at every pixel, the values of the rows that cover it in row
// order, each addition rounded.  The block therefore walks the rows in order, HEAT_CHUNK at a time: thread t takes row chunk + t,
// tests its rectangle (and its selector byte) against the TILE, the survivors are written to LDS in row order - position = the
// survivors of the earlier waves (LDS, one barrier) + popcount of the wave's ballot below the lane - and all threads walk that list
// from its start and add where their pixels are covered.  The list holds at most the chunk, so it cannot overflow; a chunk that
// misses the tile costs one ballot and one barrier.  No atomics, and no pixel's sum depends on the tile size or the chunk.
// The list is single (every thread has left the walk when it reaches the next chunk's barrier); the wave counts are double-buffered,
// because a chunk without survivors has only that one barrier.
//
// Tallies.  Counts are ballots and popcounts added to wave-uniform registers; the waves meet in LDS once.  The IoU sums are the
// zero-padded pairwise tree of DESIGN §21 over all N rows from row 0, in the statements of wave_fold.h and in one block, as in
// kernels_thrrep.hip; a row of the other side contributes +0.0 and -0.0 counts as 0.0.  The per-image
// outputs use integer atomicAdd / atomicMin only, so they do not depend on the order of arrival either.
#include "uda_internal.h"
#include "wave_fold.h"

namespace uda {

static_assert(HEAT_CHUNK == 256 && HEAT_CHUNK % HEAT_TILE_W == 0 && (HEAT_TILE_H * HEAT_TILE_W) % HEAT_CHUNK == 0,
              "a thread owns HEAT_PX pixels of one column, HEAT_YSTEP rows apart");
static_assert(THRPOST_ROWS == 256, "the block folds four wave roots: (w0 + w1) + (w2 + w3)");
static_assert((UDA_THR_MAX_N + THRPOST_ROWS - 1) / THRPOST_ROWS <= (1 << (RUN_TREE_LEVELS - 1)), "levels of the run tree");

constexpr int HEAT_PX = HEAT_TILE_H * HEAT_TILE_W / HEAT_CHUNK;
constexpr int HEAT_YSTEP = HEAT_CHUNK / HEAT_TILE_W;
constexpr int HEAT_WAVES = HEAT_CHUNK / 64;

__global__ __launch_bounds__(HEAT_CHUNK) void heat_maps_kernel(HeatArgs a) {
  __shared__ int4 rect_s[HEAT_CHUNK];
  __shared__ double val_s[HEAT_CHUNK];
  __shared__ int wcnt_s[2][HEAT_WAVES];
  const int m = blockIdx.y, tile = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, H = a.H, W = a.W;
  const int ty0 = (tile / a.tiles_x) * HEAT_TILE_H, tx0 = (tile % a.tiles_x) * HEAT_TILE_W;
  const int ty1 = min(ty0 + HEAT_TILE_H, H), tx1 = min(tx0 + HEAT_TILE_W, W);
  const int x = tx0 + tid % HEAT_TILE_W, y_first = ty0 + tid / HEAT_TILE_W;
  const int4* rects = a.rects + (size_t)a.map_rect[m] * N;
  const double* values = a.map_value[m] >= 0 ? a.values + (size_t)a.map_value[m] * N : nullptr;
  const uint8_t* sel = a.map_sel[m] >= 0 ? a.sel + (size_t)a.map_sel[m] * N : nullptr;

  double s[HEAT_PX];
  int c[HEAT_PX];
#pragma unroll
  for (int j = 0; j < HEAT_PX; ++j) { s[j] = 0.0; c[j] = 0; }

  // the next chunk's rectangle and selector are in flight while this chunk is walked
  int4 nxt = make_int4(0, 0, 0, 0);
  bool nxt_on = tid < N;
  if (nxt_on) {
    nxt = rects[tid];
    if (sel) nxt_on = sel[tid] != 0;
  }
  int buf = 0;
  for (int chunk = 0; chunk < N; chunk += HEAT_CHUNK, buf ^= 1) {
    const int i = chunk + tid;
    const int4 cur = nxt;                                   // r0, r1, c0, c1
    const bool on = nxt_on;
    nxt_on = i + HEAT_CHUNK < N;                            // (N <= UDA_THR_MAX_N: no overflow)
    if (nxt_on) {
      nxt = rects[i + HEAT_CHUNK];
      if (sel) nxt_on = sel[i + HEAT_CHUNK] != 0;
    }
    const bool hit = on && cur.x < cur.y && cur.z < cur.w && cur.x < ty1 && cur.y > ty0 && cur.z < tx1 && cur.w > tx0;
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) wcnt_s[buf][wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < HEAT_WAVES; ++w) {
      const int n = wcnt_s[buf][w];
      before += w < wave ? n : 0;
      total += n;
    }
    if (total == 0) continue;                               // (uniform: every thread read the same counts)
    if (hit) {
      const int p = before + __popcll(mask & ((1ull << lane) - 1ull));
      rect_s[p] = cur;
      val_s[p] = values ? values[i] : 1.0;
    }
    __syncthreads();
    for (int e = 0; e < total; ++e) {
      const int4 q = rect_s[e];
      const double v = val_s[e];
      if (x >= q.z && x < q.w) {
#pragma unroll
        for (int j = 0; j < HEAT_PX; ++j) {
          const int y = y_first + j * HEAT_YSTEP;
          if (y >= q.x && y < q.y) {
            s[j] = s[j] + v;
            ++c[j];
          }
        }
      }
    }
  }

  if (x >= W) return;
  const bool mean = a.map_mean[m] != 0;
#pragma unroll
  for (int j = 0; j < HEAT_PX; ++j) {
    const int y = y_first + j * HEAT_YSTEP;
    if (y >= H) break;
    const size_t o = ((size_t)m * H + y) * W + x;
    a.heat[o] = mean ? (c[j] ? s[j] / (double)c[j] : 0.0) : s[j];
    if (a.count) a.count[o] = c[j];
  }
}

void launch_heat_maps(const HeatArgs& a, int tiles, int M, hipStream_t s) {
  hipLaunchKernelGGL(heat_maps_kernel, dim3((unsigned)tiles, (unsigned)M), dim3(HEAT_CHUNK), 0, s, a);
}

// ---------------------------------------------------------------------------------------------------------------- tallies
__global__ __launch_bounds__(THRPOST_ROWS) void thr_post_kernel(ThrPostArgs a) {
  __shared__ double root_s[2][THRPOST_UNROLL][THRPOST_ROWS / 64];
  __shared__ double stack_s[2][RUN_TREE_LEVELS];
  __shared__ long long cnt_s[THRPOST_ROWS / 64][8];
  const int k = blockIdx.x, N = a.N;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double iou_thr = a.iou_thr[k], thr = a.thr[k];
  const bool images = k == a.k_img;
  const int runs = (N + THRPOST_ROWS - 1) / THRPOST_ROWS;
  long long cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};              // side 0 | side 1: rows, tp_class rows, correct, wrong
  for (int run0 = 0; run0 < runs; run0 += THRPOST_UNROLL) {
    double u[THRPOST_UNROLL], iou[THRPOST_UNROLL];
    int tp[THRPOST_UNROLL];
#pragma unroll
    for (int r = 0; r < THRPOST_UNROLL; ++r) {
      const int i = (run0 + r) * THRPOST_ROWS + tid;
      const bool valid = i < N;
      u[r] = valid ? a.u[i] : 0.0;
      iou[r] = valid ? a.ious[i] : 0.0;
      tp[r] = valid ? (a.tp[i] != 0 ? 3 : 2) : 0;           // bit 1: a row, bit 0: its class is right
    }
#pragma unroll
    for (int r = 0; r < THRPOST_UNROLL; ++r) {
      if (iou[r] == 0.0) iou[r] = 0.0;
      const bool valid = tp[r] != 0, hit = tp[r] == 3, correct = hit && iou[r] >= iou_thr;
      const bool side0 = valid && u[r] >= thr, side1 = valid && u[r] < thr;
      cnt[0] += wave_count(side0);
      cnt[1] += wave_count(side0 && hit);
      cnt[2] += wave_count(side0 && correct);
      cnt[3] += wave_count(side0 && !correct);
      cnt[4] += wave_count(side1);
      cnt[5] += wave_count(side1 && hit);
      cnt[6] += wave_count(side1 && correct);
      cnt[7] += wave_count(side1 && !correct);
      const double r0 = wave_tree_sum(side0 ? iou[r] : 0.0), r1 = wave_tree_sum(side1 ? iou[r] : 0.0);
      if (lane == 0) { root_s[0][r][wave] = r0; root_s[1][r][wave] = r1; }
      if (images && valid) {
        const int i = (run0 + r) * THRPOST_ROWS + tid, img = a.image[i];
        const int kind = side0 ? (correct ? 1 : 0) : (correct ? -1 : 2);   // correctly removed, falsely removed, falsely remaining
        if (kind >= 0) {
          atomicAdd(&a.img_count[4 * img + kind], 1);
          atomicMin(&a.img_first[3 * img + kind], i);
        }
        if (side0) atomicAdd(&a.img_count[4 * img + 3], 1);
      }
    }
    __syncthreads();
    if (tid < 2)
      for (int r = 0; r < THRPOST_UNROLL && run0 + r < runs; ++r) run_tree_push(stack_s[tid], run0 + r, fold4(root_s[tid][r]));
    __syncthreads();
  }
  if (lane == 0)
    for (int j = 0; j < 8; ++j) cnt_s[wave][j] = cnt[j];
  __syncthreads();
  if (tid < 8) a.counts[8 * k + tid] = fold4(&cnt_s[0][tid], 8);   // (the waves' counts of one kind lie 8 apart)
  if (tid < 2) a.iou_sum[2 * k + tid] = run_tree_root(stack_s[tid], runs);
}

void launch_thr_post(const ThrPostArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(thr_post_kernel, dim3((unsigned)a.K), dim3(THRPOST_ROWS), 0, s, a);
}

}  // namespace uda
