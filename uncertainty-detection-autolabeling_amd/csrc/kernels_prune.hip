// Dataset pruning kernels (gfx950): the neighbour rows of ActiveLearning.extract_hash_matrix (reference
// active_learning_loop.py:240-270) without its N x N matrix of Hamming distances (see DESIGN.md "Dataset pruning").
// Integer arithmetic only; the one floating-point operation is the reference's own compare, (double)d <= limit.
//
//   prune_max_kernel<W>          the matrix maximum: one atomicMax per block, read by the host after the launch has ended
//   prune_walk_kernel<W, false>  per (row, column span) the number of columns within the limit
//   prune_scan_*_kernel          exclusive scan of those counts in (row, span) order -> a cursor per (row, span), row_off, total
//   prune_walk_kernel<W, true>   the same walk again: every thread writes its own hits from its own cursor, columns ascending
//
// Tiling: a block is PRUNE_ROWS rows, one per thread, the row's W words in registers; it stages PRUNE_COLS column hashes at a
// time in LDS, where all lanes read the same address (a broadcast), and walks the chunks of its column span.  Every hand-off
// between passes is a launch boundary; nothing inside a launch reads what another block of that launch wrote.  How the columns
// are cut into chunks and spans changes which thread counts a hit, never whether it is one or where it lands: a row's hits
// are written in ascending column order behind the cursor the scan gave its (row, span).
#include "uda_internal.h"

namespace uda {

template <int W>
__device__ __forceinline__ void prune_load_row(const uint64_t* hashes, int row, uint64_t (&r)[W]) {
#pragma unroll
  for (int w = 0; w < W; ++w) r[w] = hashes[(size_t)row * W + w];
}

// columns [j0, j0 + nc) into LDS: nc * W consecutive words, read coalesced
template <int W>
__device__ __forceinline__ void prune_stage(const uint64_t* hashes, int j0, int nc, uint64_t* tile) {
  const uint64_t* src = hashes + (size_t)j0 * W;
  for (int t = threadIdx.x; t < nc * W; t += PRUNE_ROWS) tile[t] = src[t];
}

template <int W>
__device__ __forceinline__ int prune_distance(const uint64_t (&r)[W], const uint64_t* col) {
  int d = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) d += __popcll(r[w] ^ col[w]);
  return d;
}

// d(i, j) = d(j, i): a chunk that lies wholly below the block's first row holds only pairs that another block sees mirrored
template <int W>
__global__ __launch_bounds__(PRUNE_ROWS) void prune_max_kernel(PruneArgs a) {
  __shared__ uint64_t tile[PRUNE_COLS * W];
  __shared__ int block_max;
  if (threadIdx.x == 0) block_max = 0;
  const int row0 = blockIdx.x * PRUNE_ROWS;
  const int row = min(row0 + (int)threadIdx.x, a.N - 1);      // the lanes past the end repeat the last row: same maximum
  uint64_t r[W];
  prune_load_row<W>(a.hashes, row, r);
  const int c0 = blockIdx.y * a.chunks_per_span, c1 = min(a.n_chunks, c0 + a.chunks_per_span);
  int m = 0;
  for (int c = c0; c < c1; ++c) {
    const int j0 = c * PRUNE_COLS, nc = min((int)PRUNE_COLS, a.N - j0);
    if (j0 + nc <= row0) continue;                            // block-uniform
    __syncthreads();
    prune_stage<W>(a.hashes, j0, nc, tile);
    __syncthreads();
    for (int j = 0; j < nc; ++j) m = max(m, prune_distance<W>(r, tile + j * W));
  }
  __syncthreads();
  atomicMax(&block_max, m);
  __syncthreads();
  if (threadIdx.x == 0 && block_max > 0) atomicMax(a.max_dist, block_max);
}

template <int W, bool FILL>
__global__ __launch_bounds__(PRUNE_ROWS) void prune_walk_kernel(PruneArgs a) {
  __shared__ uint64_t tile[PRUNE_COLS * W];
  const int own = blockIdx.x * PRUNE_ROWS + (int)threadIdx.x;
  const bool live = own < a.N;
  const int row = live ? own : a.N - 1;
  uint64_t r[W];
  prune_load_row<W>(a.hashes, row, r);
  const int c0 = blockIdx.y * a.chunks_per_span, c1 = min(a.n_chunks, c0 + a.chunks_per_span);
  const size_t slot = (size_t)row * a.spans + blockIdx.y;
  int64_t cursor = FILL ? a.cursor[slot] : 0;
  int count = 0;
  for (int c = c0; c < c1; ++c) {
    const int j0 = c * PRUNE_COLS, nc = min((int)PRUNE_COLS, a.N - j0);
    __syncthreads();
    prune_stage<W>(a.hashes, j0, nc, tile);
    __syncthreads();
    for (int j = 0; j < nc; ++j) {
      const bool hit = (double)prune_distance<W>(r, tile + j * W) <= a.limit;
      if (FILL) {
        if (hit && live) a.idx[cursor++] = j0 + j;
      } else {
        count += hit;
      }
    }
  }
  if (!FILL && live) a.counts[slot] = count;
}

// ---- exclusive scan of counts [n_slots] (int32) into cursor [n_slots] (int64), PRUNE_SCAN_TILE slots per block
__global__ __launch_bounds__(256) void prune_scan_sums_kernel(PruneArgs a) {
  __shared__ int64_t part[256];
  const int64_t base = (int64_t)blockIdx.x * PRUNE_SCAN_TILE;
  int64_t s = 0;
  for (int t = threadIdx.x; t < PRUNE_SCAN_TILE; t += 256)
    if (base + t < a.n_slots) s += a.counts[base + t];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) part[threadIdx.x] += part[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.tile_sums[blockIdx.x] = part[0];
}

// one block: tile sums -> tile bases (exclusive), the grand total behind them and into row_off[N]
__global__ __launch_bounds__(256) void prune_scan_bases_kernel(PruneArgs a) {
  __shared__ int64_t sums[PRUNE_SCAN_MAX_TILES];
  for (int t = threadIdx.x; t < a.n_tiles; t += 256) sums[t] = a.tile_sums[t];
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int t = 0; t < a.n_tiles; ++t) {
      const int64_t v = sums[t];
      sums[t] = run;
      run += v;
    }
    a.tile_sums[a.n_tiles] = run;
    a.row_off[a.N] = run;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < a.n_tiles; t += 256) a.tile_sums[t] = sums[t];
}

__global__ __launch_bounds__(256) void prune_scan_tile_kernel(PruneArgs a) {
  constexpr int ITEMS = PRUNE_SCAN_TILE / 256;
  __shared__ int64_t part[256];
  const int64_t first = (int64_t)blockIdx.x * PRUNE_SCAN_TILE + (int64_t)threadIdx.x * ITEMS;
  int v[ITEMS];
  int64_t s = 0;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    v[k] = first + k < a.n_slots ? a.counts[first + k] : 0;
    s += v[k];
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int k = 1; k < 256; k <<= 1) {                        // inclusive scan of the 256 thread sums
    const int64_t add = (int)threadIdx.x >= k ? part[threadIdx.x - k] : 0;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  int64_t run = a.tile_sums[blockIdx.x] + part[threadIdx.x] - s;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const int64_t i = first + k;
    if (i < a.n_slots) {
      a.cursor[i] = run;
      if (i % a.spans == 0) a.row_off[i / a.spans] = run;
    }
    run += v[k];
  }
}

template <int W>
static void prune_launch_w(const PruneArgs& a, int pass, hipStream_t s) {
  const dim3 grid((a.N + PRUNE_ROWS - 1) / PRUNE_ROWS, a.spans), block(PRUNE_ROWS);
  if (pass == 0)
    hipLaunchKernelGGL(prune_max_kernel<W>, grid, block, 0, s, a);
  else if (pass == 1)
    hipLaunchKernelGGL((prune_walk_kernel<W, false>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((prune_walk_kernel<W, true>), grid, block, 0, s, a);
}

static void prune_launch(const PruneArgs& a, int pass, hipStream_t s) {
  switch (a.W) {
    case 1: prune_launch_w<1>(a, pass, s); break;
    case 2: prune_launch_w<2>(a, pass, s); break;
    case 3: prune_launch_w<3>(a, pass, s); break;
    case 4: prune_launch_w<4>(a, pass, s); break;
    default: abort();                                          // the entry point refuses every other W
  }
}

void launch_prune_max(const PruneArgs& a, hipStream_t s) { prune_launch(a, 0, s); }
void launch_prune_count(const PruneArgs& a, hipStream_t s) { prune_launch(a, 1, s); }
void launch_prune_fill(const PruneArgs& a, hipStream_t s) { prune_launch(a, 2, s); }

void launch_prune_scan(const PruneArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(prune_scan_sums_kernel, dim3(a.n_tiles), dim3(256), 0, s, a);
  hipLaunchKernelGGL(prune_scan_bases_kernel, dim3(1), dim3(256), 0, s, a);
  hipLaunchKernelGGL(prune_scan_tile_kernel, dim3(a.n_tiles), dim3(256), 0, s, a);
}

}  // namespace uda
