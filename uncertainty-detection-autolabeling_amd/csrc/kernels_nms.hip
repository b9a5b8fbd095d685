// NMS kernels (gfx950): tf.raw_ops.NonMaxSuppressionV5 as an epoch-synchronous data-parallel algorithm
// (reference postprocess.py:342-420; see DESIGN.md "NMS").  Compiled with -ffp-contract=off like kernels_post.hip:
// selections and scores agree with the CPU oracle bit for bit.  Five paths execute the same epoch rule:
//
//   nms_init / bound / eval / commit_kernel   the grid version, two launches per epoch (fallback and test reference)
//   nms_solo_kernel                           one block per problem, state in memory, all epochs in one launch
//   nms_reg_kernel<IPT>                       the same with the state in registers, problems of up to 8192 candidates
//   nms_coop_kernel<IPT>                      the whole anchor set in one launch of a co-resident grid
//   prefix_select / prefix_check_kernel       NMS on a score prefix: the sub-problem handed to nms_reg_kernel and the
//                                             test that it stands in for the full one
//
// The weight of one link of a pending chain is stated once (nms_link_weight); ord32, nms_key and block_excl_scan are
// shared with kernels_post.hip through post_common.h.
#include "post_common.h"

namespace uda {

// ------------------------------------------------------------------------------------ NMS (NonMaxSuppressionV5)
// Epoch k (k boxes already selected) of the reference's lazy max-heap algorithm is exactly:
//   winner_k  = argmax over live candidates of the UPDATED priority (score after the pending
//               suppression chain j = k-1 .. begin, ties -> smaller index)
//   commit    = every candidate whose STALE priority outranks winner_k is popped once in this
//               epoch: its score becomes the updated one (dropped if <= threshold / hard-suppressed)
//               and its begin index becomes k.  Nothing else is touched.
// (proof sketch in DESIGN.md).  Three data-parallel passes per epoch:
//   A bound : each 2048-candidate chunk evaluates its stale-best candidate -> lower bound on the winner
//   B eval  : evaluate every candidate whose stale priority >= bound; global max -> winner
//   C commit: apply the commit rule, record the winner.
#ifndef UDA_NMS_ITEMS
#define UDA_NMS_ITEMS 8
#endif
constexpr int NMS_ITEMS = UDA_NMS_ITEMS;
constexpr int NMS_CHUNK = 256 * NMS_ITEMS;

__device__ __forceinline__ float nms_iou(const float* a, const float* b) {
  const float ymin_i = fminf(a[0], a[2]), xmin_i = fminf(a[1], a[3]);
  const float ymax_i = fmaxf(a[0], a[2]), xmax_i = fmaxf(a[1], a[3]);
  const float ymin_j = fminf(b[0], b[2]), xmin_j = fminf(b[1], b[3]);
  const float ymax_j = fmaxf(b[0], b[2]), xmax_j = fmaxf(b[1], b[3]);
  const float area_i = (ymax_i - ymin_i) * (xmax_i - xmin_i);
  const float area_j = (ymax_j - ymin_j) * (xmax_j - xmin_j);
  if (area_i <= 0.f || area_j <= 0.f) return 0.0f;
  const float iy0 = fmaxf(ymin_i, ymin_j), ix0 = fmaxf(xmin_i, xmin_j);
  const float iy1 = fminf(ymax_i, ymax_j), ix1 = fminf(xmax_i, xmax_j);
  const float inter = fmaxf(iy1 - iy0, 0.0f) * fmaxf(ix1 - ix0, 0.0f);
  return inter / (area_i + area_j - inter);
}

// LDS of the epoch kernels: the image's selected boxes + the block's compacted work list
struct NmsLds {
  float sel[4 * 128];        // up to 128 selected boxes (max_output_size <= 128 on this path)
  int list[NMS_CHUNK];       // candidates of this chunk whose pending chain must be evaluated
  float wgt[4][128];         // per wave: the chain's weights, computed 64 links at a time by the wave's lanes
  int count;
};

// first box of the image of this block's problem (grid kernels: blockIdx.y = problem; boxes are per image, state per problem)
__device__ __forceinline__ size_t nms_grid_bbase(const NmsArgs& a) { return (size_t)(blockIdx.y / a.segs) * a.K; }

__device__ __forceinline__ void nms_load_sel(const NmsArgs& a, NmsLds& L, int n, int k) {
  for (int t = threadIdx.x; t < 4 * k; t += blockDim.x) L.sel[t] = a.sel_box[(size_t)n * a.M * 4 + t];
  if (threadIdx.x == 0) L.count = 0;
  __syncthreads();
}

// Weight of one link of a pending chain, the reference's suppression rule: exp(scale * IoU^2) in float64, rounded once,
// for a soft NMS or an IoU within the hard threshold; 0 above it.  Every path multiplies this into the score.
__device__ __forceinline__ float nms_link_weight(const NmsArgs& a, float sim) {
  if (a.soft || sim <= a.iou_thr) {
    const float e = a.scale * sim * sim;
    return (e == 0.0f) ? 1.0f : (float)exp((double)e);
  }
  return 0.0f;
}

// The same for the chains that compute their weights ahead of the product (64 links at a time, one per lane): a link that
// hard-suppresses the candidate carries NMS_HARD, where the serial chain returns at once (a weight is never negative).
constexpr float NMS_HARD = -2.0f;
__device__ __forceinline__ float nms_link_weight_staged(const NmsArgs& a, float sim) {
  const float w = nms_link_weight(a, sim);
  return (!a.soft && sim > a.iou_thr) ? NMS_HARD : w;
}

// exact updated score in epoch k of the candidate with state index si and box index bi (state is per problem, boxes are
// per image): the reference's pending chain as written (j = k-1 .. begin, newest selected box first, with its early
// exits) against the selected boxes `sel`; -inf when dropped.
__device__ __forceinline__ float nms_chain_serial(const NmsArgs& a, const float* sel, size_t si, size_t bi, int k) {
  float score = a.stale[si];
  const int begin = a.begin[si];
  const float4 b4 = *(const float4*)(a.boxes + bi * 4);
  const float bx[4] = {b4.x, b4.y, b4.z, b4.w};
  for (int j = k - 1; j >= begin; --j) {
    const float sim = nms_iou(bx, sel + 4 * j);
    const float w = nms_link_weight(a, sim);
    score *= w;
    if (!a.soft && sim > a.iou_thr) return -INFINITY;
    if (score <= a.score_thr) return -INFINITY;
  }
  return score;
}

// The same chain for ONE candidate evaluated by a whole wave (the bound candidate of a chunk in the grid kernels and of an
// epoch in nms_solo_kernel, which used to be a serial chain on one thread): the expensive part of a link (IoU + the
// float64 exp of the soft weight) does not depend on the running score, so the 64 lanes compute 64 links at a time;
// lane 0 then multiplies them into the score in exactly the reference's order with its early exits (bit-identical).
// All lanes of the wave must call it with the same arguments; every lane returns the score.  `wg` holds the wave's
// weights (128 floats of LDS: max_output_size <= 128 on these paths).
__device__ __forceinline__ float nms_chain_staged(const NmsArgs& a, const float* sel, float* wg, size_t si, size_t bi, int k) {
  const int lane = threadIdx.x & 63;
  const int begin = a.begin[si];
  const float4 b4 = *(const float4*)(a.boxes + bi * 4);
  const float bx[4] = {b4.x, b4.y, b4.z, b4.w};
  const int n = k - begin;                   // links j = k-1 .. begin -> slot s = k-1-j
  for (int s0 = 0; s0 < n; s0 += 64) {
    const int sl = s0 + lane;
    if (sl < n) {
      const int j = k - 1 - sl;
      const float sim = nms_iou(bx, sel + 4 * j);
      wg[sl] = nms_link_weight_staged(a, sim);
    }
  }
  __builtin_amdgcn_wave_barrier();
  float score = a.stale[si];
  if (lane == 0) {
    for (int sl = 0; sl < n; ++sl) {
      const float w = wg[sl];
      if (w == NMS_HARD) { score = -INFINITY; break; }   // reference: score *= 0, then the hard-suppression return
      score *= w;
      if (score <= a.score_thr) { score = -INFINITY; break; }
    }
  }
  __builtin_amdgcn_wave_barrier();
  return __shfl(score, 0, 64);
}

// Evaluate the block's work list, one candidate per thread round-robin (the flagged candidates
// of a chunk are spatial neighbours, so without the compaction a few waves would carry all the
// chains; lists are long and chains short, so a thread per candidate beats a wave per candidate: measured 5x).
// Records tent / ub / ev; returns the best key among the entries this thread evaluated.
__device__ __forceinline__ unsigned long long nms_run_list(const NmsArgs& a, NmsLds& L, size_t base, int k) {
  __syncthreads();
  unsigned long long best = 0ull;
  const int cnt = L.count;
  for (int e = threadIdx.x; e < cnt; e += blockDim.x) {
    const int i = L.list[e];
    const float s = nms_chain_serial(a, L.sel, base + i, nms_grid_bbase(a) + i, k);
    a.tent[base + i] = s;
    a.ub[base + i] = s;       // weights are <= 1: no later epoch can score this candidate higher
    a.ev[base + i] = k;
    if (s != -INFINITY) {
      const unsigned long long key = nms_key(s, i);
      best = key > best ? key : best;
    }
  }
  __syncthreads();
  return best;
}

__device__ __forceinline__ unsigned long long block_max_key(unsigned long long v) {
  __shared__ unsigned long long wmax[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long r = wmax[0];
#pragma unroll
  for (int i = 1; i < 4; ++i) r = wmax[i] > r ? wmax[i] : r;
  return r;
}

__global__ __launch_bounds__(256) void nms_init_kernel(NmsArgs a, const float* scores) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)a.n_img * a.K;
  if (gid < total) {
    const int seg = (int)(gid / a.K), i = (int)(gid % a.K);
    const size_t src = (size_t)(seg / a.segs) * a.K + i;
    const float s = scores[src];
    const bool member = (a.segs == 1) || (a.classes[src] == seg % a.segs);
    const float v = (member && s > a.score_thr) ? s : -INFINITY;
    a.stale[gid] = v;
    a.ub[gid] = v;
    a.ev[gid] = -1;
    a.begin[gid] = 0;
  }
  if (gid < (int64_t)a.n_img * a.M) {
    a.bound_key[gid] = 0ull;
    a.win_key[gid] = 0ull;
    a.sel_idx[gid] = 0;
    a.sel_score[gid] = 0.f;
  }
  if (gid < a.n_img) {
    a.nsel[gid] = 0;
    a.done[gid] = 0;
  }
}

// A bound: every chunk evaluates its best candidate by cached upper bound -> lower bound on the winner
__global__ __launch_bounds__(256) void nms_bound_kernel(NmsArgs a, int k) {
  __shared__ NmsLds L;
  const int n = blockIdx.y;
  if (a.done[n]) return;
  nms_load_sel(a, L, n, k);
  const size_t base = (size_t)n * a.K;
  const int i0 = blockIdx.x * NMS_CHUNK;
  unsigned long long best = 0ull;
#pragma unroll
  for (int it = 0; it < NMS_ITEMS; ++it) {
    const int i = i0 + it * 256 + threadIdx.x;
    if (i < a.K) {
      const float u = a.ub[base + i];
      if (u != -INFINITY && a.stale[base + i] != -INFINITY) {
        const unsigned long long key = nms_key(u, i);
        best = key > best ? key : best;
      }
    }
  }
  best = block_max_key(best);
  if (threadIdx.x < 64 && best != 0ull) {       // wave 0, cooperatively
    const int idx = (int)(0xFFFFFFFFu - (uint32_t)best);
    const float s = nms_chain_staged(a, L.sel, L.wgt[threadIdx.x >> 6], base + idx, nms_grid_bbase(a) + idx, k);
    if (threadIdx.x == 0) {
      a.tent[base + idx] = s;
      a.ub[base + idx] = s;
      a.ev[base + idx] = k;
      if (s != -INFINITY) atomicMax(&a.bound_key[(size_t)n * a.M + k], nms_key(s, idx));
    }
  }
}

// B eval: exact scores for every candidate whose upper bound can still reach the bound -> winner
__global__ __launch_bounds__(256) void nms_eval_kernel(NmsArgs a, int k) {
  __shared__ NmsLds L;
  const int n = blockIdx.y;
  if (a.done[n]) return;
  nms_load_sel(a, L, n, k);
  const size_t base = (size_t)n * a.K;
  const unsigned long long bound = a.bound_key[(size_t)n * a.M + k];
  const int i0 = blockIdx.x * NMS_CHUNK;
  unsigned long long best = 0ull;
#pragma unroll
  for (int it = 0; it < NMS_ITEMS; ++it) {
    const int i = i0 + it * 256 + threadIdx.x;
    if (i < a.K) {
      const float u = a.ub[base + i];
      if (u != -INFINITY && a.stale[base + i] != -INFINITY && nms_key(u, i) >= bound) {
        if (a.ev[base + i] == k) {                 // already exact (the chunk's bound candidate)
          const unsigned long long key = nms_key(a.tent[base + i], i);
          best = key > best ? key : best;
        } else {
          L.list[atomicAdd(&L.count, 1)] = i;
        }
      }
    }
  }
  const unsigned long long b2 = nms_run_list(a, L, base, k);
  best = b2 > best ? b2 : best;
  best = block_max_key(best);
  if (threadIdx.x == 0 && best != 0ull) atomicMax(&a.win_key[(size_t)n * a.M + k], best);
}

// C commit: the winner is selected; every candidate whose STALE priority outranks it is popped
// once in this epoch (score <- updated score, begin <- k), exactly the reference's heap traffic.
// The same pass then does the bound step of epoch k+1 (its chunk's best candidate by upper bound,
// evaluated against the k+1 selected boxes), so an epoch costs two launches instead of three.
__global__ __launch_bounds__(256) void nms_commit_kernel(NmsArgs a, int k) {
  __shared__ NmsLds L;
  const int n = blockIdx.y;
  if (a.done[n]) return;
  const size_t base = (size_t)n * a.K;
  const unsigned long long wk = a.win_key[(size_t)n * a.M + k];
  if (wk == 0ull) {
    if (blockIdx.x == 0 && threadIdx.x == 0) a.done[n] = 1;
    return;
  }
  nms_load_sel(a, L, n, k);
  const int widx = (int)(0xFFFFFFFFu - (uint32_t)wk);
  const int i0 = blockIdx.x * NMS_CHUNK;
  bool pop[NMS_ITEMS];
#pragma unroll
  for (int it = 0; it < NMS_ITEMS; ++it) {
    const int i = i0 + it * 256 + threadIdx.x;
    pop[it] = false;
    if (i < a.K && i != widx) {
      const float s = a.stale[base + i];
      if (s != -INFINITY && nms_key(s, i) > wk) {
        pop[it] = true;
        if (a.ev[base + i] != k) L.list[atomicAdd(&L.count, 1)] = i;   // popped without having been scored this epoch
      }
    }
  }
  nms_run_list(a, L, base, k);      // (ends with a barrier: tent[] of this chunk is visible below)
  unsigned long long best = 0ull;   // best upper bound left in this chunk, for the next epoch's bound
#pragma unroll
  for (int it = 0; it < NMS_ITEMS; ++it) {
    const int i = i0 + it * 256 + threadIdx.x;
    if (i >= a.K) continue;
    float u = a.ub[base + i];
    bool alive = a.stale[base + i] != -INFINITY;
    if (pop[it]) {
      u = a.tent[base + i];
      a.stale[base + i] = u;
      a.begin[base + i] = k;
      alive = (u != -INFINITY);
    }
    if (i == widx) {
      const size_t o = (size_t)n * a.M + k;
      a.sel_idx[o] = i;
      a.sel_score[o] = a.tent[base + i];
      const float* bx = a.boxes + ((size_t)(n / a.segs) * a.K + i) * 4;
      a.sel_box[o * 4 + 0] = bx[0];
      a.sel_box[o * 4 + 1] = bx[1];
      a.sel_box[o * 4 + 2] = bx[2];
      a.sel_box[o * 4 + 3] = bx[3];
      a.stale[base + i] = -INFINITY;
      a.nsel[n] = k + 1;
      alive = false;
    }
    if (alive && u != -INFINITY) {
      const unsigned long long key = nms_key(u, i);
      best = key > best ? key : best;
    }
  }
  if (k + 1 >= a.M) return;
  best = block_max_key(best);
  // bound of epoch k+1: selected box k is the winner's box (read from the candidate table: the
  // sel_box row may be written by another block of this launch)
  if (threadIdx.x < 4) L.sel[4 * k + threadIdx.x] = a.boxes[((size_t)(n / a.segs) * a.K + widx) * 4 + threadIdx.x];
  __syncthreads();
  if (threadIdx.x < 64 && best != 0ull) {       // wave 0, cooperatively
    const int idx = (int)(0xFFFFFFFFu - (uint32_t)best);
    const float s = nms_chain_staged(a, L.sel, L.wgt[threadIdx.x >> 6], base + idx, nms_grid_bbase(a) + idx, k + 1);
    if (threadIdx.x == 0) {
      a.tent[base + idx] = s;
      a.ub[base + idx] = s;
      a.ev[base + idx] = k + 1;
      if (s != -INFINITY) atomicMax(&a.bound_key[(size_t)n * a.M + k + 1], nms_key(s, idx));
    }
  }
}

void launch_nms_init(const NmsArgs& a, const float* scores, hipStream_t s) {
  int64_t total = (int64_t)a.n_img * a.K;
  const int64_t t2 = (int64_t)a.n_img * a.M;
  if (t2 > total) total = t2;
  hipLaunchKernelGGL(nms_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, scores);
}

void launch_nms_epoch(const NmsArgs& a, int epoch, hipStream_t s) {
  const dim3 grid((a.K + NMS_CHUNK - 1) / NMS_CHUNK, a.n_img), block(256);
  if (epoch == 0) hipLaunchKernelGGL(nms_bound_kernel, grid, block, 0, s, a, epoch);   // later bounds ride on the commit pass
  hipLaunchKernelGGL(nms_eval_kernel, grid, block, 0, s, a, epoch);
  hipLaunchKernelGGL(nms_commit_kernel, grid, block, 0, s, a, epoch);
}

// ------------------------------------------------------------------------------------ NMS, one launch
// The same epoch rule executed by ONE block per problem (image, or image x class) for all epochs: problems are
// independent, so nothing but __syncthreads is needed and the 2 x max_output_size dependent launches of the grid
// version become one.  The candidates are cut into chunks of 1024 (one per thread); the block keeps, per chunk,
//   cub[ch] = max key over alive candidates of the cached upper bound ub (<= stale: drives the search for the winner)
//   cst[ch] = max key over alive candidates of the stale score          (drives the pops)
// in LDS, so an epoch only visits chunks that can matter:
//   search: repeatedly take the unvisited chunk with the largest cub > L, evaluate the exact score of every
//           candidate in it with key(ub) > L (one thread each), L = max(L, best exact key) - until no chunk beats L;
//   pops  : every chunk with cst > key(winner) (and the winner's chunk): candidates whose STALE priority outranks
//           the winner take their exact score (begin = k), the winner is recorded and removed; cub / cst of the
//           chunk are recomputed.
// Identical selections and scores to the grid version (and to the heap of the reference) bit for bit.
constexpr int SOLO_T = 1024;
constexpr int SOLO_MAXCH = 512;

struct SoloLds {
  float sel[4 * 128];
  unsigned long long cub[SOLO_MAXCH], cst[SOLO_MAXCH];
  unsigned long long r0[SOLO_T / 64], r1[SOLO_T / 64];
  unsigned char visited[SOLO_MAXCH];
  float wgt[128];            // link weights of the epoch's first bound candidate (computed by wave 0, 64 links at a time)
  unsigned long long L;
  int pick;
};

// max of two keys over the block; results valid in every thread
__device__ __forceinline__ void solo_max2(SoloLds& S, unsigned long long& v0, unsigned long long& v1) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o0 = __shfl_xor(v0, off, 64), o1 = __shfl_xor(v1, off, 64);
    v0 = o0 > v0 ? o0 : v0;
    v1 = o1 > v1 ? o1 : v1;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { S.r0[threadIdx.x >> 6] = v0; S.r1[threadIdx.x >> 6] = v1; }
  __syncthreads();
  v0 = S.r0[0]; v1 = S.r1[0];
#pragma unroll
  for (int w = 1; w < SOLO_T / 64; ++w) {
    v0 = S.r0[w] > v0 ? S.r0[w] : v0;
    v1 = S.r1[w] > v1 ? S.r1[w] : v1;
  }
}

__global__ __launch_bounds__(SOLO_T) void nms_solo_kernel(NmsArgs a, const float* scores) {
  __shared__ SoloLds S;
  const int n = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)n * a.K;
  const int img = n / a.segs;
  const size_t bbase = (size_t)img * a.K;
  const int NCH = (a.K + SOLO_T - 1) / SOLO_T;
  // ---- initial state and chunk maxima
  for (int ch = 0; ch < NCH; ++ch) {
    const int i = ch * SOLO_T + tid;
    unsigned long long key = 0ull, dummy = 0ull;
    if (i < a.K) {
      const float s = scores[bbase + i];
      const bool member = (a.segs == 1) || (a.classes[bbase + i] == n % a.segs);
      const float v = (member && s > a.score_thr) ? s : -INFINITY;
      a.stale[base + i] = v;
      a.ub[base + i] = v;
      a.ev[base + i] = -1;
      a.begin[base + i] = 0;
      if (v != -INFINITY) key = nms_key(v, i);
    }
    solo_max2(S, key, dummy);
    if (tid == 0) { S.cub[ch] = key; S.cst[ch] = key; }
  }
  if (tid < a.M) {
    a.sel_idx[(size_t)n * a.M + tid] = 0;
    a.sel_score[(size_t)n * a.M + tid] = 0.f;
  }
  if (tid == 0) a.nsel[n] = 0;
  __syncthreads();

  for (int k = 0; k < a.M; ++k) {
    // ---- search for the winner of epoch k
    for (int ch = tid; ch < NCH; ch += SOLO_T) S.visited[ch] = 0;
    if (tid == 0) S.L = 0ull;
    __syncthreads();
    // a first lower bound: the exact score of the candidate with the largest upper bound of all (its index is in the
    // key), evaluated by wave 0 with the links spread over the lanes - otherwise the first visited chunk would have to
    // evaluate every one of its candidates
    if (tid < 64) {
      unsigned long long bk = 0ull;
      for (int ch = tid; ch < NCH; ch += 64) bk = S.cub[ch] > bk ? S.cub[ch] : bk;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long ok = __shfl_xor(bk, off, 64);
        bk = ok > bk ? ok : bk;
      }
      if (bk != 0ull) {
        const int i = (int)(0xFFFFFFFFu - (uint32_t)bk);
        const float score = nms_chain_staged(a, S.sel, S.wgt, base + i, bbase + i, k);
        if (tid == 0) {
          a.tent[base + i] = score;
          a.ub[base + i] = score;
          a.ev[base + i] = k;
          if (score != -INFINITY) S.L = nms_key(score, i) - 1ull;   // "- 1": the candidate itself must still pass the > L tests below
        }
      }
    }
    __syncthreads();
    while (true) {
      if (tid < 64) {            // wave 0 picks the unvisited chunk with the largest upper bound above L
        const unsigned long long L = S.L;
        unsigned long long bk = 0ull;
        int bc = -1;
        for (int ch = tid; ch < NCH; ch += 64) {
          const unsigned long long v = S.cub[ch];
          if (!S.visited[ch] && v > L && v > bk) { bk = v; bc = ch; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const unsigned long long ok = __shfl_xor(bk, off, 64);
          const int oc = __shfl_xor(bc, off, 64);
          if (ok > bk || (ok == bk && oc >= 0 && (bc < 0 || oc < bc))) { bk = ok; bc = oc; }
        }
        if (tid == 0) S.pick = bc;
      }
      __syncthreads();
      const int ch = S.pick;
      if (ch < 0) break;
      const unsigned long long L = S.L;
      const int i = ch * SOLO_T + tid;
      unsigned long long ke = 0ull, ku = 0ull;
      if (i < a.K) {
        float u = a.ub[base + i];
        if (u != -INFINITY && a.stale[base + i] != -INFINITY) {
          if (nms_key(u, i) > L) {
            float sc;
            if (a.ev[base + i] == k) {
              sc = a.tent[base + i];             // already exact in this epoch (the first bound candidate)
            } else {
              sc = nms_chain_serial(a, S.sel, base + i, bbase + i, k);
              a.tent[base + i] = sc;
              a.ub[base + i] = sc;
              a.ev[base + i] = k;
            }
            u = sc;
            if (sc != -INFINITY) ke = nms_key(sc, i);
          }
          if (u != -INFINITY) ku = nms_key(u, i);
        }
      }
      solo_max2(S, ke, ku);
      if (tid == 0) {
        S.cub[ch] = ku;
        S.visited[ch] = 1;
        if (ke > S.L) S.L = ke;
      }
      __syncthreads();
    }
    const unsigned long long wk = S.L;
    if (wk == 0ull) break;                       // no live candidate left: the remaining slots stay padded
    const int widx = (int)(0xFFFFFFFFu - (uint32_t)wk);
    const int wch = widx / SOLO_T;
    // ---- pops and the winner
    for (int ch = 0; ch < NCH; ++ch) {
      if (!(S.cst[ch] > wk || ch == wch)) continue;     // uniform: LDS values written before the last barrier
      const int i = ch * SOLO_T + tid;
      unsigned long long ks = 0ull, ku = 0ull;
      if (i < a.K) {
        float st = a.stale[base + i];
        if (st != -INFINITY) {
          if (i == widx) {
            const size_t o = (size_t)n * a.M + k;
            const float ws = a.tent[base + i];
            a.sel_idx[o] = i;
            a.sel_score[o] = ws;
            const float4 b4 = *(const float4*)(a.boxes + (bbase + i) * 4);
            *(float4*)(a.sel_box + o * 4) = b4;
            S.sel[4 * k + 0] = b4.x; S.sel[4 * k + 1] = b4.y; S.sel[4 * k + 2] = b4.z; S.sel[4 * k + 3] = b4.w;
            a.stale[base + i] = -INFINITY;
            a.nsel[n] = k + 1;
            st = -INFINITY;
          } else if (nms_key(st, i) > wk) {
            float e;
            if (a.ev[base + i] == k) {
              e = a.tent[base + i];
            } else {
              e = nms_chain_serial(a, S.sel, base + i, bbase + i, k);
              a.tent[base + i] = e;
              a.ub[base + i] = e;
              a.ev[base + i] = k;
            }
            a.stale[base + i] = e;
            a.begin[base + i] = k;
            st = e;
          }
          if (st != -INFINITY) {
            ks = nms_key(st, i);
            const float u = a.ub[base + i];
            if (u != -INFINITY) ku = nms_key(u, i);
          }
        }
      }
      solo_max2(S, ks, ku);
      if (tid == 0) { S.cst[ch] = ks; S.cub[ch] = ku; }
      __syncthreads();
    }
    __syncthreads();
  }
}

bool nms_solo_supported(const NmsArgs& a) { return a.K <= SOLO_T * SOLO_MAXCH && a.M <= 128; }

void launch_nms_solo(const NmsArgs& a, const float* scores, hipStream_t s) {
  if (a.n_img <= 0) return;
  hipLaunchKernelGGL(nms_solo_kernel, dim3(a.n_img), dim3(SOLO_T), 0, s, a, scores);
}

// ------------------------------------------------------------------------------------ NMS, one launch, state in registers
// Problems of up to 8192 candidates (top-k / per-class paths, score prefixes): the same epoch rule with the whole
// per-candidate state (stale score, cached exact score = upper bound, begin, epoch of the cached score, box) in the
// registers of the thread that owns the candidate (candidate i = j * 1024 + tid), the selected boxes in LDS.  Nothing
// is read from memory inside the epoch loop; an epoch costs three block reductions:
//   1. the candidate with the largest upper bound takes its exact score (links spread over the lanes of wave 0)
//      -> lower bound L on the winner;
//   2. every candidate whose upper bound beats L takes its exact score (one thread each, in parallel); max -> winner;
//   3. pops: every candidate whose STALE priority outranks the winner becomes exact (begin = k); the winner is recorded.
// Bit-identical selections and scores to the grid version and to the reference's heap.
struct RegLds {
  alignas(16) float sel[4 * 128];
  unsigned long long red2[2][SOLO_T / 64];     // reg_max2: alternating halves
  float wgt[128];
  unsigned long long L;
  float pbox[4];
  float pscore;
  int pbegin;
};

// Maximum of a 64-bit key over the 64 lanes of a wave, in every lane: two 32-bit DPP reductions (row_shr 1 / 2 / 4 / 8, row_bcast
// 15 / 31 - seven instructions each, no LDS traffic; a __shfl_xor ladder is six dependent ds_bpermute round trips per word):
// the high word (ordered score) first, then the low word (~index) among the lanes that hold the maximal high word.
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
  unsigned t;
  t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false); v = t > v ? t : v;   // row_shr:1
  t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false); v = t > v ? t : v;   // row_shr:2
  t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xe, false); v = t > v ? t : v;   // row_shr:4, banks 1-3
  t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xc, false); v = t > v ? t : v;   // row_shr:8, banks 2-3
  t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); v = t > v ? t : v;   // row_bcast:15, rows 1 and 3
  t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); v = t > v ? t : v;   // row_bcast:31, rows 2 and 3
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long k) {
  const unsigned hi = (unsigned)(k >> 32), lo = (unsigned)k;
  const unsigned mh = wave_max_u32(hi);
  const unsigned ml = wave_max_u32(hi == mh ? lo : 0u);
  return ((unsigned long long)mh << 32) | ml;
}

// Block-wide maximum of a 64-bit key with ONE barrier: per wave by DPP (wave_max_key: 14 instructions; a __shfl_xor ladder was 12
// dependent ds_bpermute round trips), the waves' maxima to alternating halves of red2 (par = 0, 1, 0, ... - uniform over the block),
// so a call never overwrites what a slower wave may still be reading from the call before (it read that before it arrived at THIS
// call's barrier).  The caller must not rely on a barrier in front of the reduction.
__device__ __forceinline__ unsigned long long reg_max2(RegLds& S, unsigned long long v, int& par) {
  v = wave_max_key(v);
  unsigned long long* red = S.red2[par];
  par ^= 1;
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = red[0];
#pragma unroll
  for (int w = 1; w < SOLO_T / 64; ++w) v = red[w] > v ? red[w] : v;
  return v;
}


// Pending chain of one candidate: links k-1 .. begin, newest first.  Most links are no-ops - a selected box that does not
// strictly overlap the candidate has IoU 0, weight exactly 1.0f - so the chain runs in two passes: a cheap interval test
// over all links that leaves a bit mask of the overlapping ones, then IoU + exp + multiply (the reference's order and
// early exits) over the set bits only.  Lanes of a wave then diverge over a handful of expensive links instead of
// paying the double-precision exp at nearly every one of up to 100 links.
// pass 1: bit mask of the links begin .. k-1 whose selected box strictly overlaps the candidate
__device__ __forceinline__ void chain_mask(const NmsArgs& a, const RegLds& S, int begin, const float* bx, int k, unsigned long long* m) {
  m[0] = 0ull; m[1] = 0ull;                      // links 0..63 / 64..127
  if (a.soft || a.iou_thr >= 0.f) {
    const float y0 = fminf(bx[0], bx[2]), x0 = fminf(bx[1], bx[3]), y1 = fmaxf(bx[0], bx[2]), x1 = fmaxf(bx[1], bx[3]);
    auto test = [&](const float4& sb, int j) {       // strict overlap, copy 1 of 3 (chain_wave, coop_strict_overlap): a shared form costs these kernels registers
      const float sy0 = fminf(sb.x, sb.z), sx0 = fminf(sb.y, sb.w), sy1 = fmaxf(sb.x, sb.z), sx1 = fmaxf(sb.y, sb.w);
      const bool ov = (fminf(y1, sy1) > fmaxf(y0, sy0)) && (fminf(x1, sx1) > fmaxf(x0, sx0));
      if (ov) m[j >> 6] |= 1ull << (j & 63);
    };
    int j = begin;
    // four selected boxes on their way at a time: one LDS round trip per link otherwise (up to 100 in a row for a candidate that was
    // never evaluated - the longest single-thread stretch of an epoch of the one-block kernel)
    for (; j + 4 <= k; j += 4) {
      const float4 s0 = *(const float4*)(S.sel + 4 * j), s1 = *(const float4*)(S.sel + 4 * j + 4);
      const float4 s2 = *(const float4*)(S.sel + 4 * j + 8), s3 = *(const float4*)(S.sel + 4 * j + 12);
      test(s0, j); test(s1, j + 1); test(s2, j + 2); test(s3, j + 3);
    }
    for (; j < k; ++j) test(*(const float4*)(S.sel + 4 * j), j);
  } else {                                        // (negative hard threshold: IoU 0 suppresses too - no link can be skipped)
    for (int j = begin; j < k; ++j) m[j >> 6] |= 1ull << (j & 63);
  }
}

// pass 2: IoU + exp + multiply over the set bits, newest first, with the reference's early exits
__device__ __forceinline__ float chain_product(const NmsArgs& a, const RegLds& S, float score, const float* bx, const unsigned long long* m) {
#pragma unroll
  for (int h = 1; h >= 0; --h) {
    unsigned long long mm = m[h];
    while (mm) {
      const int bit = 63 - __clzll((long long)mm);
      mm &= ~(1ull << bit);
      const int j = h * 64 + bit;
      const float sim = nms_iou(bx, S.sel + 4 * j);
      const float w = nms_link_weight(a, sim);
      score *= w;
      if (!a.soft && sim > a.iou_thr) return -INFINITY;
      if (score <= a.score_thr) return -INFINITY;
    }
  }
  return score;
}

// the two passes together
__device__ __forceinline__ float reg_chain(const NmsArgs& a, const RegLds& S, float score, int begin, const float* bx, int k) {
  unsigned long long m[2];
  chain_mask(a, S, begin, bx, k, m);
  return chain_product(a, S, score, bx, m);
}

// The same chain evaluated by a whole wave (all 64 lanes call it with the same arguments): links spread over the lanes,
// 64 at a time, newest first; only the lanes whose selected box strictly overlaps the candidate compute a weight, and
// the product runs over those lanes in link order with the weights read out of the lanes' registers.  Every lane
// returns the same score.
__device__ __forceinline__ float chain_wave(const NmsArgs& a, const RegLds& S, float score, int begin, const float* pb, int k) {
  const int lane = threadIdx.x & 63, nl = k - begin;
  const bool sparse = a.soft || a.iou_thr >= 0.f;
  const float y0 = fminf(pb[0], pb[2]), x0 = fminf(pb[1], pb[3]), y1 = fmaxf(pb[0], pb[2]), x1 = fmaxf(pb[1], pb[3]);
  for (int s0 = 0; s0 < nl && score != -INFINITY; s0 += 64) {
    const int sl = s0 + lane;
    bool ov = false;
    float w = 1.0f;
    if (sl < nl) {
      const float* sb = S.sel + 4 * (k - 1 - sl);     // strict overlap, copy 2 of 3 (chain_mask, coop_strict_overlap)
      const float sy0 = fminf(sb[0], sb[2]), sx0 = fminf(sb[1], sb[3]), sy1 = fmaxf(sb[0], sb[2]), sx1 = fmaxf(sb[1], sb[3]);
      ov = !sparse || ((fminf(y1, sy1) > fmaxf(y0, sy0)) && (fminf(x1, sx1) > fmaxf(x0, sx0)));
      if (ov) {
        w = nms_link_weight_staged(a, nms_iou(pb, sb));
      }
    }
    unsigned long long mm = __ballot(ov);
    while (mm) {
      const int ln = __ffsll((long long)mm) - 1;
      mm &= mm - 1ull;
      const float wl = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(w), ln));      // (ln is wave-uniform: v_readlane, not a ds_bpermute round trip per link)
      if (wl == NMS_HARD) { score = -INFINITY; break; }
      score *= wl;
      if (score <= a.score_thr) { score = -INFINITY; break; }
    }
  }
  return score;
}

template <int IPT>
__global__ __launch_bounds__(SOLO_T) void nms_reg_kernel(NmsArgs a, const float* scores) {
  // more than four candidates per thread: the boxes live in (dynamic) LDS instead of registers, 16 B per candidate
  constexpr bool BOXLDS = IPT > 4;
  constexpr int NBX = BOXLDS ? 1 : IPT;
  extern __shared__ float4 reg_boxes[];
  __shared__ RegLds S;
  const int n = blockIdx.x, tid = threadIdx.x;
  const int img = n / a.segs;
  const size_t bbase = (size_t)img * a.K;
  float st[IPT], ub[IPT], bx[NBX][4];
  int be[IPT];                  // begin | (epoch of the cached exact score + 1) << 8
#pragma unroll
  for (int j = 0; j < IPT; ++j) {
    const int i = j * SOLO_T + tid;
    float v = -INFINITY;
    float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < a.K) {
      const float s = scores[bbase + i];
      const bool member = (a.segs == 1) || (a.classes[bbase + i] == n % a.segs);
      if (member && s > a.score_thr) v = s;
      b4 = *(const float4*)(a.boxes + (bbase + i) * 4);
    }
    st[j] = v; ub[j] = v; be[j] = 0;
    if constexpr (BOXLDS) {
      reg_boxes[j * SOLO_T + tid] = b4;
    } else {
      bx[j][0] = b4.x; bx[j][1] = b4.y; bx[j][2] = b4.z; bx[j][3] = b4.w;
    }
  }
  auto box_of = [&](int j, float* o) {
    if constexpr (BOXLDS) {
      const float4 b4 = reg_boxes[j * SOLO_T + tid];
      o[0] = b4.x; o[1] = b4.y; o[2] = b4.z; o[3] = b4.w;
    } else {
      o[0] = bx[j][0]; o[1] = bx[j][1]; o[2] = bx[j][2]; o[3] = bx[j][3];
    }
  };
  if (tid < a.M) {
    a.sel_idx[(size_t)n * a.M + tid] = 0;
    a.sel_score[(size_t)n * a.M + tid] = 0.f;
  }
  int nsel = 0, rpar = 0;

  for (int k = 0; k < a.M; ++k) {
    // ---- 1. exact score of the candidate with the largest upper bound
    unsigned long long bk = 0ull;
#pragma unroll
    for (int j = 0; j < IPT; ++j)
      if (st[j] != -INFINITY && ub[j] != -INFINITY) {
        const unsigned long long key = nms_key(ub[j], j * SOLO_T + tid);
        bk = key > bk ? key : bk;
      }
    bk = reg_max2(S, bk, rpar);
    if (bk == 0ull) break;                 // nothing alive
    const int bi = (int)(0xFFFFFFFFu - (uint32_t)bk);
    const bool own = (bi % SOLO_T) == tid;
    const int oj = bi / SOLO_T;
#pragma unroll
    for (int j = 0; j < IPT; ++j)
      if (own && j == oj) {
        float b[4];
        box_of(j, b);
        S.pbox[0] = b[0]; S.pbox[1] = b[1]; S.pbox[2] = b[2]; S.pbox[3] = b[3];
        S.pscore = st[j];
        S.pbegin = be[j] & 255;
      }
    __syncthreads();
    if (tid < 64) {
      const float pb[4] = {S.pbox[0], S.pbox[1], S.pbox[2], S.pbox[3]};
      const float score = chain_wave(a, S, S.pscore, S.pbegin, pb, k);
      __builtin_amdgcn_wave_barrier();
      if (tid == 0) {
        S.pscore = score;
        S.L = (score != -INFINITY) ? nms_key(score, bi) - 1ull : 0ull;   // "- 1": the candidate itself passes the > L test
      }
    }
    __syncthreads();
    const unsigned long long L = S.L;
    const float pscore = S.pscore;
    // ---- 2. exact scores of everything that can still beat L
    unsigned long long ke = 0ull;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
      if (own && j == oj) { ub[j] = pscore; be[j] = (be[j] & 255) | ((k + 1) << 8); }
      if (st[j] != -INFINITY && ub[j] != -INFINITY && nms_key(ub[j], j * SOLO_T + tid) > L) {
        if ((be[j] >> 8) != k + 1) {
          float b[4];
          box_of(j, b);
          ub[j] = reg_chain(a, S, st[j], be[j] & 255, b, k);
          be[j] = (be[j] & 255) | ((k + 1) << 8);
        }
        if (ub[j] != -INFINITY) {
          const unsigned long long key = nms_key(ub[j], j * SOLO_T + tid);
          ke = key > ke ? key : ke;
        }
      }
    }
    const unsigned long long wk = reg_max2(S, ke, rpar);
    if (wk == 0ull) break;                 // no live candidate left: the remaining slots stay padded
    const int widx = (int)(0xFFFFFFFFu - (uint32_t)wk);
    // ---- 3. pops and the winner
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
      const int i = j * SOLO_T + tid;
      if (st[j] == -INFINITY) continue;
      if (i == widx) {
        const size_t o = (size_t)n * a.M + k;
        float b[4];
        box_of(j, b);
        a.sel_idx[o] = i;
        a.sel_score[o] = ub[j];
        *(float4*)(a.sel_box + o * 4) = make_float4(b[0], b[1], b[2], b[3]);
        S.sel[4 * k + 0] = b[0]; S.sel[4 * k + 1] = b[1]; S.sel[4 * k + 2] = b[2]; S.sel[4 * k + 3] = b[3];
        st[j] = -INFINITY;
      } else if (nms_key(st[j], i) > wk) {
        if ((be[j] >> 8) != k + 1) {
          float b[4];
          box_of(j, b);
          ub[j] = reg_chain(a, S, st[j], be[j] & 255, b, k);
        }
        st[j] = ub[j];
        be[j] = k | ((k + 1) << 8);
      }
    }
    nsel = k + 1;
    // (no barrier at the end of an epoch: the winner's S.sel entry and the per-epoch words of S are next touched behind the
    // barrier of the following block maximum; four block barriers per epoch instead of seven)
  }
  if (tid == 0) a.nsel[n] = nsel;
}

bool nms_reg_supported(const NmsArgs& a) { return a.K <= SOLO_T * 8 && a.M <= 128; }

template <int IPT>
static void launch_nms_reg_t(const NmsArgs& a, const float* scores, hipStream_t s) {
  const size_t lds = IPT > 4 ? (size_t)IPT * SOLO_T * sizeof(float4) : 0;
  if (lds > 48 * 1024) {
    static bool opted = false;     // above the default limit the kernel needs an explicit opt-in
    if (!opted) {
      hipFuncSetAttribute((const void*)nms_reg_kernel<IPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      opted = true;
    }
  }
  hipLaunchKernelGGL((nms_reg_kernel<IPT>), dim3(a.n_img), dim3(SOLO_T), lds, s, a, scores);
}

void launch_nms_reg(const NmsArgs& a, const float* scores, hipStream_t s) {
  if (a.n_img <= 0) return;
  if (a.K <= SOLO_T) launch_nms_reg_t<1>(a, scores, s);
  else if (a.K <= 2 * SOLO_T) launch_nms_reg_t<2>(a, scores, s);
  else if (a.K <= 3 * SOLO_T) launch_nms_reg_t<3>(a, scores, s);
  else if (a.K <= 4 * SOLO_T) launch_nms_reg_t<4>(a, scores, s);
  else if (a.K <= 6 * SOLO_T) launch_nms_reg_t<6>(a, scores, s);
  else launch_nms_reg_t<8>(a, scores, s);
}

// ------------------------------------------------------------------------------------ NMS, one cooperative launch
// The whole anchor set (184 k candidates per image) in ONE launch for all epochs: a problem is spread over `bpi`
// blocks of 1024 threads, each thread keeps the state of IPT candidates in registers (as in nms_reg_kernel; boxes are
// fetched from the candidate table when a chain is evaluated), and the two grid-wide dependencies of an epoch - the
// lower bound and the winner, both atomicMax on per-epoch slots - are crossed with a per-image barrier (a monotonic
// counter in memory) instead of a kernel boundary.  The grid version pays a chain of dependent global loads per
// launch (state re-read from memory, 2 launches x 100 epochs); here only the two barriers remain on the critical path.
// All blocks must be co-resident: the launcher refuses grids larger than the device holds (occupancy x CUs), and the
// spin is bounded (error flag -> every block falls through to the end), so the grid always drains.
//   A  every block: exact score of its best candidate by upper bound (wave 0) -> atomicMax(bound[k])   | barrier
//   B  every candidate whose upper bound reaches bound[k]: exact score -> atomicMax(win[k])            | barrier
//   C  pops (stale priority above the winner -> exact, begin = k); the winner's owner records it.
// Grid-wide step of a problem: every block contributes a 64-bit key, all blocks get the maximum.  Data and arrival are
// ONE word per block: slot[blk] = key (or 1 = "arrived with nothing"; slots start at 0, real keys are >= 2^63), written
// by one relaxed device-scope store; wave 0 polls the problem's slots, one per lane, until none is 0.  One store and
// one load round trip per step, no counter, no atomic read-modify-write on the critical path, and no fences: the
// blocks of a problem exchange nothing else (everything else a block reads was written by itself or is read-only;
// on a multi-XCD part a release / acquire pair writes back and invalidates the whole L2 - measured: every load
// after a fenced barrier missed).  The spin is bounded: a time-out raises *err and every later step falls through.
constexpr int COOP_MAX_BPI = 64;     // blocks per problem: one exchange slot per lane of the polling wave

#ifdef UDA_NMS_STATS      // the instrumentation build (tools/build_nmsstats.sh): counters of nms_coop_kernel, printed by launch_nms_coop
__device__ unsigned long long g_nms_dbg[8];
__device__ unsigned long long g_nms_dbg2[2];
__device__ unsigned long long g_nms_dbg3[8];
__device__ unsigned long long g_nms_hist[16];
__device__ unsigned long long g_nms_win[10];     // steps that settled 1, 2, ... winners
__device__ unsigned long long g_nms_stepmax[128][4];   // per grid-wide step: the slowest block's A / B / C+D compute, ticks
#define NMS_STAT(slot, v) atomicAdd(&g_nms_dbg[slot], (unsigned long long)(v))
#else
#define NMS_STAT(slot, v)
#endif

__device__ __forceinline__ float coop_chain(const NmsArgs& a, const RegLds& S, float score, int begin, size_t bidx, int k) {
  NMS_STAT(0, 1); NMS_STAT(1, k - begin); if (k - begin >= 16) NMS_STAT(2, 1); if (k - begin >= 48) NMS_STAT(3, 1);
  if (k <= begin) return score;
  const float4 b4 = *(const float4*)(a.boxes + bidx * 4);
  const float bx[4] = {b4.x, b4.y, b4.z, b4.w};
  return reg_chain(a, S, score, begin, bx, k);
}

#ifndef UDA_NMS_LDS_STATE_IPT
#define UDA_NMS_LDS_STATE_IPT 4
#endif
constexpr bool coop_lds_state(int ipt) { return ipt <= UDA_NMS_LDS_STATE_IPT; }     // per-candidate state of the block in LDS (nms_coop_kernel)
constexpr int COOP_LIST = 3072;      // entries of the block-wide work list
constexpr int COOP_HEAVY = 1024;     // entries of the list of chains handed to whole waves
constexpr int COOP_HEAVY_LINKS = 6;  // overlapping links above which a chain is evaluated by a wave
constexpr int COOP_W = 8;            // winners one grid-wide step can settle, at most (round 5)
constexpr int COOP_KL = 512;         // exact keys >= the step's bound a block can rank for its contribution
constexpr unsigned long long COOP_OVF = 2ull;    // exchange word: "more keys than I could rank" (keys are >= 2^63, 1 = nothing)

// Several winners per grid-wide step (tests/test_nms_multiwinner_model.py states the rule on the CPU):
//   A  every block offers the exact score of its best candidate by upper bound; the step's bound is the W-th largest of
//      those keys - at least W candidates are then KNOWN to have an exact key >= bound;
//   B  every candidate whose upper bound reaches the bound takes its exact score; every block contributes its W best exact
//      keys; the W best of the problem, e_1 >= e_2 >= ..., are all >= bound, i.e. above everything that was not evaluated;
//   C  e_1 is the winner of epoch k; e_j is the winner of epoch k + j - 1 as long as its box does not strictly overlap
//      e_1 .. e_{j-1} (its own score is unchanged - IoU 0, weight exactly 1 - and no other score can have grown);
//   D  the pops of those epochs, per candidate and in epoch order: while its stale key outranks e_{t+1} it is popped in
//      epoch k + t (links begin .. k + t - 1, newest first; begin = k + t) - the reference's pops, hence its products.
// One pair of exchanges settles up to W selections instead of one.
struct CoopLds {
  unsigned long long mine[COOP_W];   // this block's words for the next exchange
  unsigned long long top[COOP_W];    // result of an exchange: the largest keys of the problem, descending, 0-padded
  int ovf;                           // a block could not rank its keys: only top[0] is usable
  int nwin;                          // winners this step settles
  int kcount;                        // entries of the key list
};

// Grid-wide step of a problem with `nm` words per block (X.mine[0 .. nm): keys, 0 = none, COOP_OVF): data and arrival are
// one word each, as in coop_exchange; wave 0 polls the problem's bpi x nm words (bpi <= 64: at most COOP_W per lane) and
// leaves the nt largest keys in X.top[0 .. nt) (keys are unique: the candidate index is part of them), 0 behind them.
__device__ __forceinline__ void coop_exchange_top(unsigned long long* slots, int blk, int bpi, int nm, int nt, CoopLds& X, int* err, unsigned spin_max) {
  // (no barrier in front: X.mine is written by wave 0 and sent by wave 0; everybody else waits at the barrier behind the poll)
  __builtin_amdgcn_wave_barrier();
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    if (lane < nm) {
      const unsigned long long v = X.mine[lane];
      __hip_atomic_store(&slots[blk * nm + lane], v ? v : 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const int total = bpi * nm;
    unsigned long long loc[COOP_W];
    bool ovf = false, dead = false;
#pragma unroll
    for (int q = 0; q < COOP_W; ++q) {
      unsigned long long v = 1ull;
      const int w = lane + 64 * q;
      if (w < total && !dead) {
        unsigned spins = 0;
        while ((v = __hip_atomic_load(&slots[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0ull) {
          ++spins;
          if ((spins & 4095u) == 0u || spins > spin_max) {
            if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) { dead = true; break; }
            if (spins > spin_max) { __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); dead = true; break; }
          }
        }
      }
      if (v == COOP_OVF) ovf = true;
      loc[q] = v <= COOP_OVF ? 0ull : v;
    }
    for (int r = 0; r < COOP_W; ++r) {        // the nt largest (the rest of X.top: 0)
      unsigned long long m = 0ull;
      if (r < nt) {
        m = loc[0];
#pragma unroll
        for (int q = 1; q < COOP_W; ++q) m = loc[q] > m ? loc[q] : m;
        m = wave_max_key(m);
#pragma unroll
        for (int q = 0; q < COOP_W; ++q)
          if (loc[q] == m) loc[q] = 0ull;
      }
      if (lane == 0) X.top[r] = m;
    }
    const bool any = __ballot(ovf) != 0ull;
    if (lane == 0) X.ovf = any ? 1 : 0;
  }
  __syncthreads();
}

__device__ __forceinline__ bool coop_strict_overlap(const float* p, const float* q) {      // strict overlap, copy 3 of 3 (chain_mask, chain_wave)
  const float y0 = fminf(p[0], p[2]), x0 = fminf(p[1], p[3]), y1 = fmaxf(p[0], p[2]), x1 = fmaxf(p[1], p[3]);
  const float sy0 = fminf(q[0], q[2]), sx0 = fminf(q[1], q[3]), sy1 = fmaxf(q[0], q[2]), sx1 = fmaxf(q[1], q[3]);
  return (fminf(y1, sy1) > fmaxf(y0, sy0)) && (fminf(x1, sx1) > fmaxf(x0, sx0));
}

template <int IPT>
__global__ __launch_bounds__(SOLO_T) void nms_coop_kernel(NmsArgs a, const float* scores, unsigned long long* slots_all, int* err, int bpi, int n0, unsigned spin_max,
                                                           int wcfg) {
  // Per candidate: the stale score in a register of its thread (scanned every epoch, candidate i0 + j * 1024 of its thread), the
  // cached exact score / upper bound in LDS (scanned every epoch, 128 KB), begin / epoch / a copy of the stale score in
  // the workspace arrays in memory (touched only when a chain is evaluated, together with the candidate's box).
  extern __shared__ float U[];                    // [IPT * 1024] | work list [COOP_LIST] | heavy list | "exact this epoch" bits | key list
  int* wlist = (int*)(U + IPT * SOLO_T);
  int* hlist = wlist + COOP_LIST;
  unsigned* ebits = (unsigned*)(hlist + COOP_HEAVY);  // [IPT * 1024 / 32]
  unsigned long long* klist = (unsigned long long*)(ebits + IPT * 32);     // [COOP_KL] (8-byte aligned: every part above is a multiple of 8 bytes)
  // Small batches (IPT <= 4: tens of blocks per problem, 4096 candidates per block): box, stale score and begin of the block's
  // candidates live in LDS (24 B each, 96 KB) instead of the workspace arrays in memory - a chain evaluation then starts without
  // a memory round trip, in each of the three phases of an epoch.
  constexpr bool LST = coop_lds_state(IPT);
  float4* lbox = (float4*)(klist + COOP_KL);                               // [IPT * 1024] (16-byte aligned: 16 K + 12 K + 4 K + 128 IPT + 4 K bytes above)
  float* lstale = (float*)(lbox + (LST ? IPT * SOLO_T : 0));
  int* lbegin = (int*)(lstale + (LST ? IPT * SOLO_T : 0));
  auto st_begin = [&](int rel, size_t g) -> int { if constexpr (LST) return lbegin[rel]; else return a.begin[g]; };
  auto st_stale = [&](int rel, size_t g) -> float { if constexpr (LST) return lstale[rel]; else return a.stale[g]; };
  auto st_box = [&](int rel, size_t g) -> float4 { if constexpr (LST) return lbox[rel]; else return *(const float4*)(a.boxes + g * 4); };
  __shared__ RegLds S;
  __shared__ CoopLds X;
  __shared__ int wcount, hcount;
  const int n = n0 + blockIdx.x / bpi, blk = blockIdx.x % bpi, tid = threadIdx.x;   // n0: first problem of this launch
  const size_t bbase = (size_t)n * a.K;           // one problem per image (segs == 1)
  // Candidate <-> (block, slot rel = j * 1024 + tid).  Large batches (IPT > 8, a few blocks per problem): one contiguous range of
  // IPT * 1024 candidates per block.  Small batches (IPT <= 8: tens of blocks per problem): stripes of 64 candidates (one wave)
  // dealt round-robin to the blocks of the problem, so that the spatial neighbours of a winner - the candidates that take
  // exact scores in phase B and are popped in phase D - are spread over all blocks and every block finishes its entries in
  // one eight-lane pass (run_balanced).  Measured, round 5: batch 1 / 45 blocks 1.47 -> 1.36 ms with stripes; batch 32 / 8 blocks
  // 3.5 -> 4.3 ms (every block then has entries in every phase), hence the switch on IPT.
#ifndef UDA_NMS_STRIPE_IPT
#define UDA_NMS_STRIPE_IPT 8
#endif
  constexpr bool STRIPE = IPT <= UDA_NMS_STRIPE_IPT;
  const int istride = STRIPE ? SOLO_T * bpi : SOLO_T;
  const int cbase = STRIPE ? 0 : blk * IPT * SOLO_T;
  auto gidx = [&](int rel) {
    if constexpr (STRIPE) { const int t = rel & (SOLO_T - 1); return (rel >> 10) * istride + ((t >> 6) * bpi + blk) * 64 + (t & 63); }
    else return cbase + rel;
  };
  auto rel_of = [&](int i) {                    // (STRIPE: -1 = not this block's candidate)
    if constexpr (STRIPE) {
      const int st = i >> 6, q = st / bpi;
      if (st - q * bpi != blk) return -1;
      return (q >> 4) * SOLO_T + (q & 15) * 64 + (i & 63);
    } else {
      return i - cbase;
    }
  };
  static_assert(SOLO_T == 1024, "the stripe mapping is written for 16 waves per block");
  const int i0 = gidx(tid);                     // this thread's first candidate; slot j: i0 + j * istride
  unsigned long long* slots = slots_all + (size_t)n * a.M * (1 + COOP_W) * bpi;      // [step][bound: bpi | winners: bpi x COOP_W]
  float st[IPT];
#pragma unroll
  for (int j = 0; j < IPT; ++j) {
    const int i = i0 + j * istride;
    float v = -INFINITY;
    if (i < a.K) {
      const float s = scores[bbase + i];
      if (s > a.score_thr) v = s;
      if constexpr (LST) lbox[j * SOLO_T + tid] = *(const float4*)(a.boxes + (bbase + i) * 4);
      else { a.stale[bbase + i] = v; a.begin[bbase + i] = 0; }
    }
    if constexpr (LST) { lstale[j * SOLO_T + tid] = v; lbegin[j * SOLO_T + tid] = 0; }
    st[j] = v;
    U[j * SOLO_T + tid] = v;
  }
  // (the padded form of the outputs - index 0 / score 0 in the slots that stay empty - is written by the launcher's
  // memsets: a slot must have ONE writer inside the kernel, the L2s of different XCDs are not coherent with each other)
  int nsel = 0;
  if (tid == 0) { wcount = 0; hcount = 0; X.kcount = 0; X.nwin = 1; }
  for (int f = tid; f < IPT * 32; f += SOLO_T) ebits[f] = 0u;
  __syncthreads();

  // Exact scores of the candidates flagged in the threads' bit masks.  These are spatial neighbours, so a few threads
  // would carry all the chains: they go through a block-wide list and every thread takes entries round-robin (entries
  // beyond the capacity stay with their owners).  A thread runs the cheap mask pass of its entry; chains with few
  // overlapping links it finishes itself, the others - big boxes overlap most of the selected ones, up to 100 IoU + exp
  // in a row - go to a second list that whole waves work off (chain_wave).  stale / begin / box come from memory in one
  // round trip; "already exact in this epoch" is a bit per candidate in LDS.
  //   pops == false (phase B): exact score in epoch k (links begin .. k-1); `fn(rel, v)` receives every candidate once.
  //   pops == true  (phase D): the candidate's pops of the epochs k .. k + nw - 1 (X.top[0 .. nw) are their winners'
  //                 keys): first pop in the first epoch k + t whose winner its stale key outranks (the long chain: this
  //                 is what goes through the lists), later ones - one new link each - by the same thread; stale / begin
  //                 in memory and U[] receive the final state.
  auto run_balanced = [&](unsigned mask, int k, int nw, auto pops_tag, auto&& fn) {
    constexpr bool POPS = decltype(pops_tag)::value;
    // (wcount / hcount are 0 here: reset at the end of the previous call, with block barriers in between)
    unsigned left = 0u;
    {
      unsigned m = mask;
      while (m) {
        const int j = __ffs((int)m) - 1;
        m &= m - 1u;
        const int pos = atomicAdd(&wcount, 1);
        if (pos < COOP_LIST) wlist[pos] = j * SOLO_T + tid;
        else left |= 1u << j;
      }
    }
    __syncthreads();
    const int cnt = wcount < COOP_LIST ? wcount : COOP_LIST;
#ifdef UDA_NMS_STATS
    const unsigned long long tb0 = wall_clock64();
    if (tid == 0) { atomicAdd(&g_nms_dbg3[0], (unsigned long long)wcount); atomicMax(&g_nms_dbg3[1], (unsigned long long)wcount); }
#endif
    // epoch of the candidate's first pop: the first winner its stale key outranks (the mask guarantees there is one)
    auto first_pop = [&](float stale, int gi) {
      const unsigned long long key = nms_key(stale, gi);
      int t = 0;
      while (t < nw - 1 && !(key > X.top[t])) ++t;
      return t;
    };
    // the candidate's later pops after a first pop in epoch k + t: one epoch at a time, each over the links that are new
    auto later_pops = [&](int rel, size_t g, float v, int t, const float* bx) {
      int b = k + t;
      if (POPS) {
        for (int u = t + 1; u < nw && v != -INFINITY; ++u) {
          if (nms_key(v, gidx(rel)) > X.top[u]) {
            v = reg_chain(a, S, v, b, bx, k + u);
            b = k + u;
          }
        }
        if constexpr (LST) { lstale[rel] = v; lbegin[rel] = b; }
        else { a.stale[g] = v; a.begin[g] = b; }
      }
      U[rel] = v;
      return v;
    };
    auto one = [&](int rel) {
      const bool cached = (ebits[rel >> 5] >> (rel & 31)) & 1u;
      if (!POPS && cached) { fn(rel, U[rel]); return; }
      const int gi = gidx(rel);
      const size_t g = bbase + gi;
      const int begin = st_begin(rel, g);
      const float stale = st_stale(rel, g);
      const float4 b4 = st_box(rel, g);
      const float bx[4] = {b4.x, b4.y, b4.z, b4.w};
      const int t = POPS ? first_pop(stale, gi) : 0;
      const int kk = k + t;
      float v = stale;
      if (POPS && t == 0 && cached) {
        v = U[rel];                          // exact in epoch k already (phase B): the same links in the same order
      } else if (kk > begin) {
        unsigned long long m[2];
        chain_mask(a, S, begin, bx, kk, m);
        if (__popcll(m[0]) + __popcll(m[1]) > COOP_HEAVY_LINKS) {
          const int pos = atomicAdd(&hcount, 1);
          if (pos < COOP_HEAVY) { hlist[pos] = rel; return; }
        }
        v = chain_product(a, S, stale, bx, m);
      }
      v = later_pops(rel, g, v, t, bx);
      if (!POPS) atomicOr(&ebits[rel >> 5], 1u << (rel & 31));
      fn(rel, v);
    };
    // Few entries (the usual case: a handful per block and phase): GL = SIXTEEN lanes per entry.  The interval test over the links
    // begin .. kk-1 - up to 100 LDS reads and compares in a row for a candidate that was never evaluated, the longest
    // single-thread stretch of an epoch (slowest block of a step 7-8 us in B and in D at batch 1, mean 3) - is spread over
    // the lanes of the group, GL links per pass; a wave ballot hands every group its GL overlap bits.  The rest of
    // the entry (product over the few overlapping links, stores) is done by the group's first lane, exactly as below.
    // (The product spread over the group's lanes as well - a weight per lane, then the product in link order, no heavy list -
    // was measured in the same job: batch 1 / 4 / 8 1.42 / 1.42 / 1.58 ms against 1.40 / 1.40 / 1.59 without; not kept.)
    // Many entries (pops with short chains): one thread per entry as before - the same arithmetic either way.
#ifndef UDA_NMS_GL
#define UDA_NMS_GL 16     // (A/B in one job, batch 1 / 4 / 8 NMS ms: 4 lanes 1.49 / 1.50 / 1.59, 8: 1.40 / 1.39 / 1.51, 16: 1.36 / 1.35 / 1.45, 32: 1.34 / 1.34 / 1.47)
#endif
    constexpr int GL = UDA_NMS_GL;          // lanes per entry (a power of two <= 32)
    if (cnt <= 2 * (SOLO_T / GL)) {
      const int lane = tid & 63, sub = tid & (GL - 1);
      const bool sparse = a.soft || a.iou_thr >= 0.f;
      for (int e0 = 0; e0 < cnt; e0 += SOLO_T / GL) {
        const int e = e0 + tid / GL;
        const bool valid = e < cnt;
        const int rel = valid ? wlist[e] : 0;
        bool cached = false, domask = false, plain = false;
        int gi = 0, begin = 0, t = 0, kk = 0;
        size_t g = 0;
        float stale = 0.f, bx[4] = {0.f, 0.f, 0.f, 0.f};
        if (valid) {
          cached = (ebits[rel >> 5] >> (rel & 31)) & 1u;
          plain = !POPS && cached;
          if (!plain) {
            gi = gidx(rel);
            g = bbase + gi;
            begin = st_begin(rel, g);
            stale = st_stale(rel, g);
            const float4 b4 = st_box(rel, g);
            bx[0] = b4.x; bx[1] = b4.y; bx[2] = b4.z; bx[3] = b4.w;
            t = POPS ? first_pop(stale, gi) : 0;
            kk = k + t;
            domask = !(POPS && t == 0 && cached) && kk > begin;
          }
        }
        unsigned long long m[2] = {0ull, 0ull};
        {
          const float y0 = fminf(bx[0], bx[2]), x0 = fminf(bx[1], bx[3]), y1 = fmaxf(bx[0], bx[2]), x1 = fmaxf(bx[1], bx[3]);
          const int npass = domask ? (kk - begin + GL - 1) / GL : 0;
          for (int it = 0; __ballot(it < npass) != 0ull; ++it) {       // (wave-uniform trip count: the longest chain of the wave)
            const int j = begin + it * GL + sub;
            bool ov = false;
            if (it < npass && j < kk) {
              if (sparse) {
                const float4 sb = *(const float4*)(S.sel + 4 * j);
                const float sy0 = fminf(sb.x, sb.z), sx0 = fminf(sb.y, sb.w), sy1 = fmaxf(sb.x, sb.z), sx1 = fmaxf(sb.y, sb.w);
                ov = (fminf(y1, sy1) > fmaxf(y0, sy0)) && (fminf(x1, sx1) > fmaxf(x0, sx0));
              } else {
                ov = true;
              }
            }
            const unsigned long long bal = __ballot(ov);
            const unsigned long long byte = (bal >> (lane & ~(GL - 1))) & ((1ull << GL) - 1ull);     // this group's links begin + GL it .. + GL - 1
            if (byte) {
              const int pos = begin + it * GL;                       // < 128 (M <= 128)
              if (pos < 64) {
                m[0] |= byte << pos;
                if (pos > 64 - GL) m[1] |= byte >> (64 - pos);
              } else {
                m[1] |= byte << (pos - 64);
              }
            }
          }
        }
        if (valid && sub == 0) {
          if (plain) {
            fn(rel, U[rel]);
          } else {
            float v = stale;
            bool heavy = false;
            if (POPS && t == 0 && cached) {
              v = U[rel];
            } else if (kk > begin) {
              if (__popcll(m[0]) + __popcll(m[1]) > COOP_HEAVY_LINKS) {
                const int pos = atomicAdd(&hcount, 1);
                if (pos < COOP_HEAVY) { hlist[pos] = rel; heavy = true; }
              }
              if (!heavy) v = chain_product(a, S, stale, bx, m);
            }
            if (!heavy) {
              v = later_pops(rel, g, v, t, bx);
              if (!POPS) atomicOr(&ebits[rel >> 5], 1u << (rel & 31));
              fn(rel, v);
            }
          }
        }
      }
    }
    // one thread per entry: long lists, and the entries that did not fit the list (they stay with their owners).  (ONE loop, so
    // that the entry code exists once per phase: the epoch loop is 50 KB of instructions as it is.)
    {
      int e = (cnt <= 2 * (SOLO_T / GL)) ? cnt : tid;
      for (;;) {
        int rel;
        if (e < cnt) { rel = wlist[e]; e += SOLO_T; }
        else if (left) { const int j = __ffs((int)left) - 1; left &= left - 1u; rel = j * SOLO_T + tid; }
        else break;
        one(rel);
      }
    }
    __syncthreads();
#ifdef UDA_NMS_STATS
    const unsigned long long tb1 = wall_clock64();
    if (tid == 0) { atomicAdd(&g_nms_dbg3[2], (unsigned long long)hcount); atomicMax(&g_nms_dbg3[3], (unsigned long long)hcount);
                    atomicAdd(&g_nms_dbg3[4], tb1 - tb0); atomicMax(&g_nms_dbg3[5], tb1 - tb0); }
#endif
    const int hc = hcount < COOP_HEAVY ? hcount : COOP_HEAVY;
    if (hc == 0) {                           // the common case: no heavy chain, one barrier less
      if (tid == 0) wcount = 0;
      return;
    }
    for (int e = tid >> 6; e < hc; e += SOLO_T / 64) {
      const int rel = hlist[e];
      const int gi = gidx(rel);
      const size_t g = bbase + gi;
      const float4 b4 = st_box(rel, g);
      const float bx[4] = {b4.x, b4.y, b4.z, b4.w};
      const float stale = st_stale(rel, g);
      const int t = POPS ? first_pop(stale, gi) : 0;
      float v = chain_wave(a, S, stale, st_begin(rel, g), bx, k + t);
      if ((tid & 63) == 0) {
        v = later_pops(rel, g, v, t, bx);
        if (!POPS) atomicOr(&ebits[rel >> 5], 1u << (rel & 31));
        fn(rel, v);
      }
    }
    __syncthreads();
#ifdef UDA_NMS_STATS
    if (tid == 0) { const unsigned long long tb2 = wall_clock64(); atomicAdd(&g_nms_dbg3[6], tb2 - tb1); atomicMax(&g_nms_dbg3[7], tb2 - tb1); }
#endif
    if (tid == 0) { wcount = 0; hcount = 0; }
  };

  int k = 0, rpar = 0;
  for (int step = 0; k < a.M; ++step) {
    // (the candidate index is rebuilt from an opaque base in every epoch: otherwise the per-candidate index words and
    // addresses of all IPT candidates are hoisted out of the epoch loop and spill)
    int ib = i0;
    asm volatile("" : "+v"(ib));
    unsigned long long* sslots = slots + (size_t)step * (1 + COOP_W) * bpi;
#ifdef UDA_NMS_STATS
    const unsigned long long t0 = wall_clock64();
#endif
    // ---- A. this block's best candidate by upper bound takes its exact score -> lower bound on the winner.  Scores
    // first, the index only for the best one: max over j of (ordered score, smaller j) is max over the keys
    unsigned long long bk = 0ull;
    {
      uint32_t bo = 0u;
      int bj = 0;
#pragma unroll
      for (int j = IPT - 1; j >= 0; --j) {
        const float u = U[j * SOLO_T + tid];
        if (st[j] != -INFINITY && u != -INFINITY) {
          const uint32_t o = ord32(u);
          if (o >= bo) { bo = o; bj = j; }      // descending j with >=: the smallest index wins a tie
        }
      }
      if (bo != 0u) bk = ((unsigned long long)bo << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(ib + bj * istride));
    }
    bk = reg_max2(S, bk, rpar);

    if (bk != 0ull && tid < 64) {
      const int bi = (int)(0xFFFFFFFFu - (uint32_t)bk);
      const size_t g = bbase + bi;
      const int br = rel_of(bi);
      const int begin = st_begin(br, g);
      const float stale0 = st_stale(br, g);
      const float4 b4 = st_box(br, g);
      const float pb[4] = {b4.x, b4.y, b4.z, b4.w};
      const float score = chain_wave(a, S, stale0, begin, pb, k);
      if (tid == 0) {
        U[br] = score;
        atomicOr(&ebits[br >> 5], 1u << (br & 31));
        X.mine[0] = (score != -INFINITY) ? nms_key(score, bi) : 0ull;
      }
    }
    if (tid == 0) {
      if (bk == 0ull) X.mine[0] = 0ull;
      X.kcount = 0;
    }
#ifdef UDA_NMS_STATS
    __syncthreads();
    const unsigned long long t1 = wall_clock64();
#endif
    coop_exchange_top(sslots, blk, bpi, 1, wcfg, X, err, spin_max);
    // the step's bound: the weff-th largest block key (fewer blocks alive: the smallest one; none: 0 = everything is evaluated)
    int nz = 0;
#pragma unroll
    for (int r = 0; r < COOP_W; ++r) nz += X.top[r] != 0ull ? 1 : 0;
    int weff = wcfg < nz ? wcfg : nz;
    if (weff > a.M - k) weff = a.M - k;
    if (weff < 1) weff = 1;
    const unsigned long long bd = nz ? X.top[weff - 1] : 0ull;
#ifdef UDA_NMS_STATS
    const unsigned long long t2 = wall_clock64();
#endif
    // ---- B. exact scores of everything that can still reach the bound (few: a loop over a bit mask)
    unsigned long long ke = 0ull;
    unsigned need = 0u;
    {
      // key(u, i) >= bd  <=>  ord(u) > ord(bd)  or  (ord(u) == ord(bd) and ~i >= low word of bd)
      const uint32_t bdo = (uint32_t)(bd >> 32), bdl = (uint32_t)bd;
#pragma unroll
      for (int j = 0; j < IPT; ++j) {
        const float u = U[j * SOLO_T + tid];
        if (st[j] != -INFINITY && u != -INFINITY) {
          const uint32_t o = ord32(u);
          if (o > bdo || (o == bdo && 0xFFFFFFFFu - (uint32_t)(ib + j * istride) >= bdl)) need |= 1u << j;
        }
      }
    }
    run_balanced(need, k, 1, std::false_type{}, [&](int rel, float v) {
      if (v != -INFINITY) {
        const unsigned long long key = nms_key(v, gidx(rel));
        ke = key > ke ? key : ke;
        if (weff > 1 && key >= bd) {         // ranked below for this block's contribution
          const int pos = atomicAdd(&X.kcount, 1);
          if (pos < COOP_KL) klist[pos] = key;
        }
      }
    });
    ke = reg_max2(S, ke, rpar);
    // this block's weff best exact keys (wave 0; the list is complete: run_balanced ends with a barrier)
    if (tid < 64) {
      const int cnt = X.kcount;
      if (weff == 1 || cnt > COOP_KL) {
        if (tid < COOP_W) X.mine[tid] = tid == 0 ? ke : ((tid == 1 && weff > 1) ? COOP_OVF : 0ull);      // (words behind weff are not sent)
      } else {
        unsigned long long loc[COOP_KL / 64];
#pragma unroll
        for (int q = 0; q < COOP_KL / 64; ++q) loc[q] = (tid + 64 * q < cnt) ? klist[tid + 64 * q] : 0ull;
        for (int r = 0; r < weff; ++r) {
          unsigned long long m = loc[0];
#pragma unroll
          for (int q = 1; q < COOP_KL / 64; ++q) m = loc[q] > m ? loc[q] : m;
          m = wave_max_key(m);
          if (tid == 0) X.mine[r] = m;
#pragma unroll
          for (int q = 0; q < COOP_KL / 64; ++q)
            if (loc[q] == m) loc[q] = 0ull;
        }
      }
    }
#ifdef UDA_NMS_STATS
    const unsigned long long t3 = wall_clock64();
#endif
    coop_exchange_top(sslots + bpi, blk, bpi, weff, weff, X, err, spin_max);
#ifdef UDA_NMS_STATS
    const unsigned long long t4 = wall_clock64();
#endif
    const unsigned long long wk = X.top[0];
    if (wk == 0ull) break;                  // no live candidate in the whole problem (uniform over its blocks)
    // ---- C. the winners this step settles: boxes of the weff best keys, then the prefix that does not overlap
    if (tid < 4 * COOP_W) {
      const int t = tid >> 2;
      const unsigned long long key = X.top[t];
      if (t < weff && key != 0ull) S.sel[4 * (k + t) + (tid & 3)] = a.boxes[(bbase + (size_t)(0xFFFFFFFFu - (uint32_t)key)) * 4 + (tid & 3)];
    }
    // (one winner per step, the default: nothing reads this epoch's S.sel before the barrier inside run_balanced below)
    int nw = 1;
    if (weff > 1) {                         // (uniform)
      __syncthreads();
      if (tid == 0) {
        int nw_ = 1;
        if (!X.ovf && (a.soft || a.iou_thr >= 0.f)) {
          for (; nw_ < weff; ++nw_) {
            const unsigned long long key = X.top[nw_];
            if (key == 0ull || key < bd) break;
            bool ov = false;
            for (int p = 0; p < nw_; ++p) ov = ov || coop_strict_overlap(S.sel + 4 * (k + nw_), S.sel + 4 * (k + p));
            if (ov) break;
          }
        }
        X.nwin = nw_;
      }
      __syncthreads();
      nw = X.nwin;
    }
#ifdef UDA_NMS_STATS
    if (tid == 0 && blk == 0) atomicAdd(&g_nms_win[nw < 9 ? nw : 9], 1ull);
#endif
    // ---- D. the winners' records and the pops of the epochs k .. k + nw - 1
    unsigned pops = 0u;
    {
      unsigned wmask = 0u;                  // this thread's candidates among the winners
      for (int t = 0; t < nw; ++t) {
        const int widx = (int)(0xFFFFFFFFu - (uint32_t)X.top[t]);
        const int rel = rel_of(widx);
        if (rel >= 0 && rel < IPT * SOLO_T && (rel % SOLO_T) == tid) {
          const size_t o = (size_t)n * a.M + k + t;
          a.sel_idx[o] = widx;
          a.sel_score[o] = U[rel];          // exact in epoch k = exact in epoch k + t (no link of the step touches it)
          *(float4*)(a.sel_box + o * 4) = st_box(rel, bbase + widx);
          if constexpr (LST) lstale[rel] = -INFINITY; else a.stale[bbase + widx] = -INFINITY;
          wmask |= 1u << (rel / SOLO_T);
        }
      }
      // key(st, i) > low  <=>  ord(st) > ord(low)  or  (equal and ~i > low word): low = the last winner's key
      const unsigned long long low = X.top[nw - 1];
      const uint32_t wo = (uint32_t)(low >> 32), wl = (uint32_t)low;
#pragma unroll
      for (int j = 0; j < IPT; ++j) {
        if ((wmask >> j) & 1u) st[j] = -INFINITY;
        if (st[j] != -INFINITY) {
          const uint32_t o = ord32(st[j]);
          if (o > wo || (o == wo && 0xFFFFFFFFu - (uint32_t)(ib + j * istride) > wl)) pops |= 1u << j;
        }
      }
    }
    run_balanced(pops, k, nw, std::true_type{}, [&](int, float) {});      // (ends with a barrier: U[] of the popped candidates is complete)
#pragma unroll
    for (int j = 0; j < IPT; ++j)
      if ((pops >> j) & 1u) st[j] = U[j * SOLO_T + tid];
    k += nw;
    nsel = k;
    for (int f = tid; f < IPT * 32; f += SOLO_T) ebits[f] = 0u;      // "exact in this epoch" bits of the next step
    // (no barrier here: the next step touches ebits, U[] and the list counters only behind the barrier of its first block maximum)
#ifdef UDA_NMS_STATS
    if (tid == 0) {
      const unsigned long long t5 = wall_clock64();
      NMS_STAT(4, t1 - t0); NMS_STAT(5, t2 - t1); NMS_STAT(6, t3 - t2); NMS_STAT(7, t4 - t3);
      atomicAdd(&g_nms_dbg2[0], t5 - t4); atomicAdd(&g_nms_dbg2[1], 1ull);
      if (step < 128) { atomicMax(&g_nms_stepmax[step][0], t1 - t0); atomicMax(&g_nms_stepmax[step][1], t3 - t2); atomicMax(&g_nms_stepmax[step][2], t5 - t4); }
      {
        const unsigned long long te = t5 - t0;        // whole step of this block, 10 ns ticks
        int bkt = 0;
        while (bkt < 7 && te >= (2000ull << bkt)) ++bkt;     // < 20, 40, 80, 160, 320, 640, 1280 us, more
        atomicAdd(&g_nms_hist[bkt], 1ull);
        atomicAdd(&g_nms_hist[8 + bkt], te);
      }
    }
#endif
  }
  if (blk == 0 && tid == 0) a.nsel[n] = nsel;
}

// 64-bit words of exchange slots per problem (the caller's scratch: n_img x this; a launch uses M x 2 x its blocks per problem)
size_t nms_coop_slot_words(int M) { return (size_t)M * (1 + COOP_W) * COOP_MAX_BPI; }

template <int IPT>
constexpr size_t coop_lds_bytes() {
  return (size_t)IPT * SOLO_T * sizeof(float) + (size_t)(COOP_LIST + COOP_HEAVY) * sizeof(int) + (size_t)IPT * 32 * sizeof(unsigned) +
         (size_t)COOP_KL * sizeof(unsigned long long) + (coop_lds_state(IPT) ? (size_t)IPT * SOLO_T * 24 : 0);
}

// co-resident blocks of nms_coop_kernel<IPT> on the current device (occupancy x CUs; 0 = cannot run), cached per HIP device
template <int IPT>
static int coop_capacity(int dev, int* n_cu) {
  static int capacity_of[64], cus_of[64];
  static bool known[64];
  if (!known[dev]) {
    (void)hipGetLastError();          // an error left behind by an unrelated earlier call must not be read as ours
    // Blocks of this kernel a CU holds, from the kernel's own resources: 16 waves of <= 128 registers (launch bounds) are one
    // block per CU by registers, two below 65; LDS and the 2048-thread limit likewise.  (Not
    // hipOccupancyMaxActiveBlocksPerMultiprocessor: on ROCm 7.2 it answered 0 for this kernel - same registers, same LDS -
    // depending on which other kernels the process had run before, and 1 otherwise.)
    int per_cu = 0, cap = 0, n_cus = 0, coop = 0, lds_cu = 0;
    const hipError_t e0 = hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev);
    const hipError_t e1 = hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, dev);
    if (hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess) lds_cu = 0;
    hipError_t e2 = hipSuccess, e3 = hipSuccess;
    hipFuncAttributes fa{};
    cus_of[dev] = e0 == hipSuccess ? n_cus : 0;
    if (e0 == hipSuccess && e1 == hipSuccess && coop) {
      e2 = hipFuncSetAttribute((const void*)nms_coop_kernel<IPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)coop_lds_bytes<IPT>());
      if (e2 == hipSuccess) e3 = hipFuncGetAttributes(&fa, (const void*)nms_coop_kernel<IPT>);
      if (e2 == hipSuccess && e3 == hipSuccess && fa.numRegs > 0 && fa.numRegs <= 128 && fa.maxThreadsPerBlock >= SOLO_T) {
        const size_t lds = fa.sharedSizeBytes + coop_lds_bytes<IPT>();       // the launch was accepted above: one block fits
        const int by_regs = (512 / ((fa.numRegs + 7) / 8 * 8)) * 4 / (SOLO_T / 64);
        const int by_lds = (size_t)lds_cu >= lds ? (int)((size_t)lds_cu / lds) : 1;
        per_cu = by_regs < by_lds ? by_regs : by_lds;
        if (per_cu > 2048 / SOLO_T) per_cu = 2048 / SOLO_T;
        if (per_cu < 1) per_cu = 1;
        cap = per_cu * n_cus;
      }
    }
    (void)hipGetLastError();
    if (getenv("UDA_NMS_DEBUG"))
      fprintf(stderr, "[uda] cooperative NMS capacity<%d> on device %d: %d CUs (%d B LDS each), cooperative %d, %d registers, %zu + %zu B LDS -> %d blocks per CU "
              "(%s / %s / %s / %s)\n", IPT, dev, n_cus, lds_cu, coop, fa.numRegs, fa.sharedSizeBytes, coop_lds_bytes<IPT>(), per_cu,
              hipGetErrorName(e0), hipGetErrorName(e1), hipGetErrorName(e2), hipGetErrorName(e3));
    const char* hook = getenv("UDA_NMS_COOP_CAP");     // test hook: a wrong capacity must end in the time-out path, not in a hang
    if (hook) cap = atoi(hook);
    capacity_of[dev] = cap;
    known[dev] = cap > 0 || hook != nullptr;          // a failed query is asked again next time
  }
  *n_cu = cus_of[dev];
  return capacity_of[dev];
}

template <int IPT>
static void coop_launch(const NmsArgs& a, const float* scores, unsigned long long* slots, int* err, int bpi, int per, unsigned spin_max, int wcfg, hipStream_t s) {
  for (int n0 = 0; n0 < a.n_img; n0 += per) {
    const int cnt = a.n_img - n0 < per ? a.n_img - n0 : per;
    hipLaunchKernelGGL((nms_coop_kernel<IPT>), dim3((unsigned)(bpi * cnt)), dim3(SOLO_T), coop_lds_bytes<IPT>(), s, a, scores, slots, err, bpi, n0, spin_max, wcfg);
  }
}

// 1 = launched; 0 = a problem outside this kernel's domain (segmented candidates, more than 128 outputs, nothing to do);
// -1 = wanted but NOT launched (the capacity query failed, the grid is not co-resident on this device, more candidates than
// COOP_MAX_BPI blocks hold, or the runtime refused): the caller falls back to the slower versions and counts it.
int launch_nms_coop(const NmsArgs& a, const float* scores, unsigned long long* slots, int* err, hipStream_t s) {
  if (a.segs != 1 || a.M > 128 || a.K < 1 || a.n_img <= 0) return 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
  // Candidates per thread (IPT).  An epoch is latency-bound - three scans of the block's candidates, two grid-wide steps -
  // so a small batch is spread over more, shorter blocks: the smallest IPT with which every block of the launch still has
  // a CU to itself; a batch that fills the device anyway takes 32 (fewest blocks per problem, most problems per launch).
  // UDA_NMS_COOP_IPT = 4 | 8 | 16 | 24 | 32 forces one.
  static const int force = uda_env_int("UDA_NMS_COOP_IPT", 0);
  const int ipts[5] = {4, 8, 16, 24, 32};
  int ipt = 0, bpi = 0, capacity = 0;
  for (int i = 0; i < 5 && !ipt; ++i) {
    const int t = ipts[i];
    if (force && t != force) continue;
    const int b = (a.K + t * SOLO_T - 1) / (t * SOLO_T);
    if (b > COOP_MAX_BPI) continue;
    int n_cu = 0;
    const int cap = t == 4 ? coop_capacity<4>(dev, &n_cu) : t == 8 ? coop_capacity<8>(dev, &n_cu) : t == 16 ? coop_capacity<16>(dev, &n_cu)
                  : t == 24 ? coop_capacity<24>(dev, &n_cu) : coop_capacity<32>(dev, &n_cu);
    if (force || t == 32 || ((long long)a.n_img * b <= n_cu && b <= cap)) { ipt = t; bpi = b; capacity = cap; }
  }
  // polls of an exchange slot before a block gives up (UDA_NMS_COOP_SPIN: debug knob, a tiny bound forces the time-out -> redo path)
  static long long spin_env = -1;
  if (spin_env < 0) { const char* e = getenv("UDA_NMS_COOP_SPIN"); spin_env = e ? atoll(e) : (1ll << 22); if (spin_env < 0) spin_env = 0; }
  const unsigned spin_max = (unsigned)(spin_env > 0xffffffffll ? 0xffffffffll : spin_env);
  static const bool dbg = getenv("UDA_NMS_DEBUG") != nullptr;
  if (!ipt || bpi > capacity) {
    if (dbg) fprintf(stderr, "[uda] cooperative NMS: %d blocks per problem > capacity %d\n", bpi, capacity);
    return -1;
  }
  const int per = capacity / bpi;          // problems per launch: more problems than the device holds run in consecutive grids
  // winners one grid-wide step may settle (UDA_NMS_WINNERS = 1 .. 8).  Default 1, measured: the second-best
  // candidate of an epoch overlaps the winner in 86 % of the steps under random-init weights (scores are spatially correlated:
  // the runners-up sit next to the maximum) and on every clustered score map, so extra winners are rarely certified while
  // the looser bound (the W-th largest of the blocks' offers) has every block evaluate more: 3.47 ms (1) / 3.66 (2) / 4.3 (4) /
  // 32 ms (8 of 8 blocks: the bound of the weakest block) per 32-image step
  static const int wenv = uda_env_int("UDA_NMS_WINNERS", 0);
  int wcfg = wenv > 0 ? wenv : 1;
  if (wcfg > COOP_W) wcfg = COOP_W;
  if (wcfg < 1) wcfg = 1;
  hipMemsetAsync(slots, 0, (size_t)a.n_img * a.M * (1 + COOP_W) * bpi * sizeof(unsigned long long), s);
  hipMemsetAsync(a.sel_idx, 0, (size_t)a.n_img * a.M * sizeof(int32_t), s);
  hipMemsetAsync(a.sel_score, 0, (size_t)a.n_img * a.M * sizeof(float), s);
  // An ordinary launch: the grid fits the device (checked above against the occupancy of this kernel), so every block
  // becomes resident as soon as whatever else runs on the device drains - other kernels never wait for this one - and the
  // bounded spin is the safety net.  (hipLaunchCooperativeKernel gives the same placement plus a formal check, but
  // rocprofv3's kernel tracing crashes at process exit after a cooperative launch, ROCm 7.2.)
  if (ipt == 4) coop_launch<4>(a, scores, slots, err, bpi, per, spin_max, wcfg, s);
  else if (ipt == 8) coop_launch<8>(a, scores, slots, err, bpi, per, spin_max, wcfg, s);
  else if (ipt == 16) coop_launch<16>(a, scores, slots, err, bpi, per, spin_max, wcfg, s);
  else if (ipt == 24) coop_launch<24>(a, scores, slots, err, bpi, per, spin_max, wcfg, s);
  else coop_launch<32>(a, scores, slots, err, bpi, per, spin_max, wcfg, s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    if (dbg) fprintf(stderr, "[uda] cooperative NMS: launch refused: %s\n", hipGetErrorString(e));
    return -1;
  }
  if (dbg) fprintf(stderr, "[uda] cooperative NMS: %d problems x %d blocks of %d candidates per thread (capacity %d), up to %d winners per step\n", a.n_img, bpi, ipt, capacity, wcfg);
#ifdef UDA_NMS_STATS
  {
    hipStreamSynchronize(s);
    unsigned long long h[8];
    hipMemcpyFromSymbol(h, HIP_SYMBOL(g_nms_dbg), sizeof(h));
    fprintf(stderr, "[uda] nms stats (cumulative): chains %llu links %llu chains>=16 %llu chains>=48 %llu\n", h[0], h[1], h[2], h[3]);
    unsigned long long h2[2];
    hipMemcpyFromSymbol(h2, HIP_SYMBOL(g_nms_dbg2), sizeof(h2));
    unsigned long long hh[16];
    hipMemcpyFromSymbol(hh, HIP_SYMBOL(g_nms_hist), sizeof(hh));
    fprintf(stderr, "[uda] nms epoch-time histogram (block-epochs : total ms) <20us %llu:%.1f <40 %llu:%.1f <80 %llu:%.1f <160 %llu:%.1f <320 %llu:%.1f <640 %llu:%.1f <1280 %llu:%.1f more %llu:%.1f\n",
            hh[0], hh[8] * 1e-5, hh[1], hh[9] * 1e-5, hh[2], hh[10] * 1e-5, hh[3], hh[11] * 1e-5, hh[4], hh[12] * 1e-5, hh[5], hh[13] * 1e-5, hh[6], hh[14] * 1e-5, hh[7], hh[15] * 1e-5);
    unsigned long long hw[10];
    hipMemcpyFromSymbol(hw, HIP_SYMBOL(g_nms_win), sizeof(hw));
    fprintf(stderr, "[uda] nms winners per grid-wide step (problems x steps, cumulative): 1:%llu 2:%llu 3:%llu 4:%llu 5:%llu 6:%llu 7:%llu 8:%llu\n",
            hw[1], hw[2], hw[3], hw[4], hw[5], hw[6], hw[7], hw[8]);
    unsigned long long h3[8];
    hipMemcpyFromSymbol(h3, HIP_SYMBOL(g_nms_dbg3), sizeof(h3));
    if (h2[1]) fprintf(stderr, "[uda] nms lists per block-phase: entries mean %.1f max %llu, heavy mean %.1f max %llu; stage1 mean %.1f max %llu, stage2 mean %.1f max %llu ticks\n",
                       (double)h3[0] / (2 * h2[1]), h3[1], (double)h3[2] / (2 * h2[1]), h3[3], (double)h3[4] / (2 * h2[1]), h3[5], (double)h3[6] / (2 * h2[1]), h3[7]);
    {
      static unsigned long long sm[128][4];
      hipMemcpyFromSymbol(sm, HIP_SYMBOL(g_nms_stepmax), sizeof(sm));
      double sa = 0, sb = 0, sc = 0; int ns = 0;
      for (int i = 0; i < 128; ++i) if (sm[i][0] | sm[i][1] | sm[i][2]) { sa += sm[i][0]; sb += sm[i][1]; sc += sm[i][2]; ++ns; }
      if (ns) fprintf(stderr, "[uda] nms slowest block per step (this launch and earlier ones, max), mean over %d steps in 10 ns ticks: A %.1f B %.1f C+D %.1f\n", ns, sa / ns, sb / ns, sc / ns);
      static unsigned long long zero[128][4];
      hipMemcpyToSymbol(HIP_SYMBOL(g_nms_stepmax), zero, sizeof(zero));
    }
    if (h2[1]) fprintf(stderr, "[uda] nms phases, mean per block-epoch in 10 ns ticks: A %.1f bar1 %.1f B %.1f bar2 %.1f C %.1f (%llu block-epochs)\n",
                       (double)h[4] / h2[1], (double)h[5] / h2[1], (double)h[6] / h2[1], (double)h[7] / h2[1], (double)h2[0] / h2[1], h2[1]);
  }
#endif
  return 1;
}

// ------------------------------------------------------------------------------------ NMS on a score prefix
// With the whole anchor set as candidates (184 k per image) almost none can ever be selected: a candidate is popped
// from the reference's heap only while its score is at least the score of the LAST box selected.  So the NMS is run
// (single-launch kernel above) on the candidates whose score is >= tau, tau chosen so that 2048..4096 candidates pass,
// kept in index order so that ties break exactly as in the full problem.  The result is the full problem's result iff
// no excluded candidate could have been popped before the loop ended:
//     max_out boxes selected : every excluded score <  the smallest selected (updated) score, or <= score_thresh
//     fewer selected         : every excluded score <= score_thresh (excluded candidates never enter the heap)
// prefix_check_kernel tests exactly that per image; images that fail are flagged and redone on the full set by the
// host (uda_api.hip finish_post), so the output is bit-identical either way.
constexpr int PFX_T = 1024;

struct PfxLds {
  unsigned hist[2048];
  int wsum[17];
  int bin, above, inbin;       // result of a digit selection
  int wcnt[PFX_T / 64];
  unsigned wex[PFX_T / 64];
};

// histogram of ((key >> shift) & (nb - 1)) over this block's candidates whose key matches `prefix` above hi_shift.
// Scores cluster (random-init: every score ~ 0.01), so a bin shared by >= 16 lanes of a wave is added once.
__device__ __forceinline__ void pfx_hist(const float* v, int K, uint32_t prefix, int hi_shift, int shift, int nb,
                                         unsigned* hist) {
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < nb; i += PFX_T) hist[i] = 0;
  __syncthreads();
  const int Kr = (K + 63) & ~63;
  for (int i = threadIdx.x; i < Kr; i += PFX_T) {
    uint32_t bin = 0xFFFFFFFFu;
    if (i < K) {
      const uint32_t key = ord32(v[i]);
      if (hi_shift >= 32 || (key >> hi_shift) == prefix) bin = (key >> shift) & (uint32_t)(nb - 1);
    }
    unsigned long long todo = __ballot(bin != 0xFFFFFFFFu);
    if (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const uint32_t b = (uint32_t)__shfl((int)bin, leader, 64);
      const unsigned long long same = __ballot(bin == b);
      const int ns = __popcll(same);
      if (ns >= 16) {
        if (lane == leader) atomicAdd(&hist[b], (unsigned)ns);
        if (bin == b) bin = 0xFFFFFFFFu;
      }
    }
    if (bin != 0xFFFFFFFFu) atomicAdd(&hist[bin], 1u);
  }
  __syncthreads();
}

// the bin (from the top) in which the running count reaches `need`; S.above = count in the bins above it
__device__ __forceinline__ void pfx_pick(PfxLds& S, int nb, int need) {
  // thread t owns bins nb-1-2t and nb-2-2t (descending order)
  const int hi = nb - 1 - 2 * (int)threadIdx.x, lo = hi - 1;
  const int ch = hi >= 0 ? (int)S.hist[hi] : 0, cl = lo >= 0 ? (int)S.hist[lo] : 0;
  int total;
  const int excl = block_excl_scan(ch + cl, S.wsum, &total);
  if (excl < need && need <= excl + ch + cl) {
    if (excl + ch >= need) { S.bin = hi; S.above = excl; S.inbin = ch; }
    else { S.bin = lo; S.above = excl + ch; S.inbin = cl; }
  }
  __syncthreads();
}

__global__ __launch_bounds__(PFX_T) void prefix_select_kernel(PrefixArgs a) {
  __shared__ PfxLds S;
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* v = a.scores + (size_t)n * a.K;
  const float* bx = a.boxes + (size_t)n * a.K * 4;
  int32_t* sidx = a.sub_idx + (size_t)n * a.Lcap;
  float* ssc = a.sub_scores + (size_t)n * a.Lcap;
  float4* sbx = (float4*)(a.sub_boxes + (size_t)n * a.Lcap * 4);

  // ---- tau: the coarsest key prefix with Lp <= #(key >= tau) <= Lcap
  uint32_t tau;
  bool ok = true;
  pfx_hist(v, a.K, 0u, 32, 21, 2048, S.hist);
  pfx_pick(S, 2048, a.Lp);
  const int b1 = S.bin, above1 = S.above;
  if (above1 + S.inbin <= a.Lcap) {
    tau = (uint32_t)b1 << 21;
  } else {
    __syncthreads();
    pfx_hist(v, a.K, (uint32_t)b1, 21, 10, 2048, S.hist);
    pfx_pick(S, 2048, a.Lp - above1);
    const int b2 = S.bin, above2 = above1 + S.above;
    if (above2 + S.inbin <= a.Lcap) {
      tau = ((uint32_t)b1 << 21) | ((uint32_t)b2 << 10);
    } else {
      __syncthreads();
      pfx_hist(v, a.K, ((uint32_t)b1 << 11) | (uint32_t)b2, 10, 0, 1024, S.hist);
      pfx_pick(S, 1024, a.Lp - above2);
      tau = ((uint32_t)b1 << 21) | ((uint32_t)b2 << 10) | (uint32_t)S.bin;
      ok = above2 + S.above + S.inbin <= a.Lcap;    // more exact ties than the prefix can hold: full problem
    }
  }
  __syncthreads();

  // ---- ordered compaction: wave w owns the contiguous slice [w * seg, (w + 1) * seg)
  const int seg = ((a.K + (PFX_T / 64) - 1) / (PFX_T / 64) + 63) & ~63;
  const int s0 = wave * seg, s1 = min(a.K, s0 + seg);
  int cnt = 0;
  uint32_t ex = 0u;                      // largest key among the excluded candidates (0 = none)
  if (ok) {
    for (int i = s0 + lane; i < s0 + seg; i += 64) {
      uint32_t key = 0u;
      if (i < s1) key = ord32(v[i]);
      const bool take = (i < s1) && key >= tau;
      cnt += __popcll(__ballot(take));
      if (i < s1 && !take) ex = key > ex ? key : ex;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)ex, off, 64);
    ex = o > ex ? o : ex;
  }
  if (lane == 0) { S.wcnt[wave] = cnt; S.wex[wave] = ex; }
  __syncthreads();
  int pos = 0, total = 0;
  uint32_t exall = 0u;
  for (int w = 0; w < PFX_T / 64; ++w) {
    if (w < wave) pos += S.wcnt[w];
    total += S.wcnt[w];
    exall = S.wex[w] > exall ? S.wex[w] : exall;
  }
  if (ok && total > 0) {
    for (int i = s0 + lane; i < s0 + seg; i += 64) {
      float sc = 0.f;
      bool take = false;
      if (i < s1) {
        sc = v[i];
        take = ord32(sc) >= tau;
      }
      const unsigned long long m = __ballot(take);
      if (m == 0ull) continue;
      if (take) {
        const int o = pos + __popcll(m & ((1ull << lane) - 1ull));
        sidx[o] = i;
        ssc[o] = sc;
        sbx[o] = *(const float4*)(bx + (size_t)i * 4);
      }
      pos += __popcll(m);
    }
  }
  if (!ok) total = 0;
  for (int o = total + tid; o < a.Lcap; o += PFX_T) {     // padding: dead candidates
    sidx[o] = 0;
    ssc[o] = -INFINITY;
    sbx[o] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (tid == 0) {
    a.excl_key[n] = exall;
    a.bad[n] = ok ? 0 : 1;
  }
}

void launch_prefix_select(const PrefixArgs& a, hipStream_t s) {
  if (a.n_img <= 0) return;
  hipLaunchKernelGGL(prefix_select_kernel, dim3(a.n_img), dim3(PFX_T), 0, s, a);
}

// maps the prefix problem's selections back to candidate indices and checks that the prefix was sufficient
__global__ __launch_bounds__(128) void prefix_check_kernel(PrefixCheckArgs a) {
  __shared__ uint32_t wmin[128];
  const int n = blockIdx.x, j = threadIdx.x;
  const int ns = a.sub_nsel[n];
  uint32_t key = 0xFFFFFFFFu;
  if (j < a.M) {
    const size_t o = (size_t)n * a.M + j;
    const float sc = a.sub_sel_score[o];
    a.sel_idx[o] = (j < ns) ? a.sub_idx[(size_t)n * a.Lcap + a.sub_sel_idx[o]] : 0;
    a.sel_score[o] = sc;
    if (j < ns) key = ord32(sc);
  }
  wmin[j] = key;
  __syncthreads();
  if (j == 0) {
    uint32_t m = 0xFFFFFFFFu;
    for (int t = 0; t < 128; ++t) m = wmin[t] < m ? wmin[t] : m;
    const uint32_t ek = a.excl_key[n];
    bool fine = true;
    if (ek != 0u) {                      // something was excluded
      const uint32_t eb = (ek & 0x80000000u) ? (ek ^ 0x80000000u) : ~ek;
      const float es = __uint_as_float(eb);
      fine = (es <= a.score_thr) || (ns == a.M && ek < m);
    }
    a.nsel[n] = ns;
    if (!fine) a.bad[n] = 1;
  }
}

void launch_prefix_check(const PrefixCheckArgs& a, hipStream_t s) {
  if (a.n_img <= 0) return;
  hipLaunchKernelGGL(prefix_check_kernel, dim3(a.n_img), dim3(128), 0, s, a);
}

}  // namespace uda
