// RCC's manual augmentations (reference ssl_utils/parent.py:261-315, Parent_SSL.apply_manual_augmentation) on the packed RGB
// uint8 planes of a collage call: uda_collage_np (include/uda_hip.h, which states the arithmetic).  Pillow's operations are
// integer and float32 arithmetic, so the result is Pillow's bit for bit.  Built without FMA contraction (csrc/Makefile), and the
// blend spells its roundings out with __fmul_rn / __fadd_rn: Pillow's x86 build rounds the product and the sum separately, and a
// fused blend truncates to another byte now and then.
//
//   augment_mean_kernel      the luma sum of a contrast job's whole source plane: AUG_MEAN_PIX pixels a block, summed in uint32 (at
//                            most 4096 * 255), one 64-bit integer atomic add a block into the job's slot.  Integer, so exact and
//                            independent of the order
//   augment_point_kernel     flip, blend (brightness, contrast), add bytes and the copy: a tile of AUG_TILE pixels x AUG_ROWS
//                            rows a block, a pixel a thread.  A contrast job reads its plane's sum from device memory (the mean
//                            kernel ran in the launch before it) and divides in double: no value goes to the host in between
//   blur_stage_kernel<VERT>  the three box passes of one axis of ImagingGaussianBlur.  A block takes AUG_TILE positions x
//                            BLUR_LINES lines (a line is a row along x, a column along y), stages them with a halo of 3 (r + 1)
//                            positions a side - cut at the line's true ends - channel by channel in LDS, and runs the passes
//                            between two LDS buffers, each pass rounded to uint8 as a pass over the whole plane would be: pass
//                            k needs (r + 1) positions more a side than it gives, so the valid range shrinks from 3 (r + 1) to
//                            0 around the tile.  Clamping refers to the line's true ends, which the staged range holds
//                            whenever the tile is that near them.  The sum is integral: a thread adds its 2 r + 1 taps
//                            directly, no running accumulator.  Only the tile is stored
//
// Blocks find their job by a binary search of the block index in the jobs' first tiles, as resample_pass_kernel does.  Stores are
// single bytes of the job's own rectangle; no atomics on pixels.
#include <math.h>

#include "uda_internal.h"

namespace uda {

static_assert(AUG_THREADS == 256 && AUG_TILE * AUG_ROWS == AUG_THREADS, "a pointwise tile is a pixel a thread");
static_assert(BLUR_EXT == AUG_TILE + 6 * (UDA_BLUR_MAX_BOX + 1) && BLUR_LDS <= 24576, "tile + halo of the largest box in 24 KiB, both buffers");

template <typename J>
__device__ __forceinline__ int find_job(const J* jobs, int n_jobs, int blk) {
  int lo = 0, hi = n_jobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].tile0 <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(AUG_THREADS) void augment_mean_kernel(const AugMeanJob* __restrict__ jobs, int n_jobs,
                                                                   unsigned long long* __restrict__ sums, const uint8_t* __restrict__ base) {
  __shared__ uint32_t s_sum[AUG_THREADS];
  const int tid = threadIdx.x;
  const AugMeanJob j = jobs[find_job(jobs, n_jobs, (int)blockIdx.x)];
  const int64_t p0 = (int64_t)((int)blockIdx.x - j.tile0) * AUG_MEAN_PIX;
  const uint8_t* src = base + j.src;
  uint32_t acc = 0;
  for (int i = 0; i < AUG_MEAN_PIX / AUG_THREADS; ++i) {
    const int64_t p = p0 + tid + (int64_t)i * AUG_THREADS;
    if (p < j.n_pix) {
      const uint8_t* px = src + p * 3;
      acc += ((uint32_t)px[0] * 19595u + (uint32_t)px[1] * 38470u + (uint32_t)px[2] * 7471u + 0x8000u) >> 16;
    }
  }
  s_sum[tid] = acc;
  __syncthreads();
  for (int step = AUG_THREADS / 2; step > 0; step >>= 1) {
    if (tid < step) s_sum[tid] += s_sum[tid + step];
    __syncthreads();
  }
  if (tid == 0) atomicAdd(sums + j.slot, (unsigned long long)s_sum[0]);
}

__global__ __launch_bounds__(AUG_THREADS) void augment_point_kernel(const AugJob* __restrict__ jobs, int n_jobs,
                                                                    const unsigned long long* __restrict__ sums,
                                                                    const uint8_t* __restrict__ noise, uint8_t* __restrict__ base) {
  const int tid = threadIdx.x;
  const AugJob j = jobs[find_job(jobs, n_jobs, (int)blockIdx.x)];
  const int tile = (int)blockIdx.x - j.tile0;
  const int x = (tile % j.tiles_x) * AUG_TILE + tid % AUG_TILE, y = (tile / j.tiles_x) * AUG_ROWS + tid / AUG_TILE;
  if (x >= j.cw || y >= j.ch) return;
  const int sx = j.kind == AUG_FLIP ? j.w - 1 - x : x;
  const uint8_t* px = base + j.src + (int64_t)y * j.src_stride + (int64_t)sx * 3;
  uint8_t* to = base + j.dst + (int64_t)y * j.dst_stride + (int64_t)x * 3;
  if (j.kind == AUG_BLEND || j.kind == AUG_BLEND_CLIP) {
    int deg = 0;
    if (j.mean >= 0) deg = (int)((double)sums[j.mean] / (double)j.n_pix + 0.5);
    const float d = (float)deg;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float t = __fadd_rn(d, __fmul_rn(j.a, __fsub_rn((float)px[c], d)));
      int v = (int)t;                                                  // (truncation toward zero)
      if (j.kind == AUG_BLEND_CLIP) v = t <= 0.0f ? 0 : (t >= 255.0f ? 255 : v);
      to[c] = (uint8_t)v;
    }
  } else if (j.kind == AUG_ADD) {
    const uint8_t* nz = noise + j.noise + ((int64_t)y * j.w + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) to[c] = (uint8_t)((uint32_t)px[c] + (uint32_t)nz[c]);
  } else {
    to[0] = px[0];
    to[1] = px[1];
    to[2] = px[2];
  }
}

template <bool VERT>
__global__ __launch_bounds__(AUG_THREADS) void blur_stage_kernel(const BlurPass* __restrict__ passes, int n_pass, uint8_t* __restrict__ base) {
  __shared__ uint8_t s_buf[2][BLUR_LINES * 3 * BLUR_EXT];              // [line * 3 + channel][position - lo3]
  const int tid = threadIdx.x;
  const BlurPass p = passes[find_job(passes, n_pass, (int)blockIdx.x)];
  const int tile = (int)blockIdx.x - p.tile0, tp = tile % p.tiles_pos, tl = tile / p.tiles_pos;
  const int o0 = tp * AUG_TILE, l0 = tl * BLUR_LINES;
  const int no = min((int)AUG_TILE, p.n_out - o0), nl = min((int)BLUR_LINES, p.n_lines - l0);
  if (no < 1 || nl < 1) return;                                        // (block-uniform; the host launches no such tile)
  const int r = p.r, r1 = r + 1, n = p.n;
  const int lo3 = max(0, o0 - 3 * r1), hi3 = min(n, o0 + no + 3 * r1), span = hi3 - lo3;
  if (span > BLUR_EXT) return;                                         // (never: the host refuses a box above UDA_BLUR_MAX_BOX)
  // stage: global bytes in their own order (runs of span * 3 bytes a row along x, of nl * 3 bytes a row along y)
  {
    const uint8_t* src = base + p.src;
    const int run = VERT ? nl * 3 : span * 3, outer = VERT ? span : nl;
    const uint8_t* from = src + (VERT ? (int64_t)lo3 * p.src_stride + (int64_t)l0 * 3 : (int64_t)l0 * p.src_stride + (int64_t)lo3 * 3);
    for (int i = tid; i < run * outer; i += AUG_THREADS) {
      const int o = i / run, b = i - o * run, q = b / 3, c = b - q * 3;
      const int line = VERT ? q : o, pos = VERT ? o : q;
      s_buf[0][(line * 3 + c) * BLUR_EXT + pos] = from[(int64_t)o * p.src_stride + b];
    }
  }
  __syncthreads();
  int cur = 0;
  for (int k = 2; k >= 0; --k) {
    const int lo = max(0, o0 - k * r1), hi = min(n, o0 + no + k * r1), cnt = hi - lo;
    const uint8_t* in = s_buf[cur];
    uint8_t* out = s_buf[cur ^ 1];
    for (int i = tid; i < nl * 3 * cnt; i += AUG_THREADS) {
      const int lc = i / cnt, pos = lo + (i - lc * cnt);
      const uint8_t* line = in + lc * BLUR_EXT - lo3;                   // indexed by the position in the whole line
      uint32_t sum = 0;
      for (int d = -r; d <= r; ++d) sum += line[min(max(pos + d, 0), n - 1)];
      const uint32_t edge = (uint32_t)line[min(max(pos - r1, 0), n - 1)] + (uint32_t)line[min(max(pos + r1, 0), n - 1)];
      out[lc * BLUR_EXT + pos - lo3] = (uint8_t)((p.ww * sum + p.fw * edge + (1u << 23)) >> 24);
    }
    __syncthreads();
    cur ^= 1;
  }
  // store the tile, bytes in their own order
  {
    const int run = VERT ? nl * 3 : no * 3, outer = VERT ? no : nl;
    uint8_t* to = base + p.dst + (VERT ? (int64_t)o0 * p.dst_stride + (int64_t)l0 * 3 : (int64_t)l0 * p.dst_stride + (int64_t)o0 * 3);
    for (int i = tid; i < run * outer; i += AUG_THREADS) {
      const int o = i / run, b = i - o * run, q = b / 3, c = b - q * 3;
      const int line = VERT ? q : o, pos = VERT ? o : q;
      to[(int64_t)o * p.dst_stride + b] = s_buf[cur][(line * 3 + c) * BLUR_EXT + (o0 + pos - lo3)];
    }
  }
}

void launch_augment_means(const AugMeanJob* jobs, int n_jobs, int n_tiles, unsigned long long* sums, const uint8_t* base, hipStream_t s) {
  if (n_jobs < 1 || n_tiles < 1) return;
  hipLaunchKernelGGL(augment_mean_kernel, dim3(n_tiles), dim3(AUG_THREADS), 0, s, jobs, n_jobs, sums, base);
}

void launch_augment_points(const AugJob* jobs, int n_jobs, int n_tiles, const unsigned long long* sums, const uint8_t* noise, uint8_t* base,
                           hipStream_t s) {
  if (n_jobs < 1 || n_tiles < 1) return;
  hipLaunchKernelGGL(augment_point_kernel, dim3(n_tiles), dim3(AUG_THREADS), 0, s, jobs, n_jobs, sums, noise, base);
}

void launch_blur_stages(const BlurPass* passes, int n_pass, int n_tiles, bool vertical, uint8_t* base, hipStream_t s) {
  if (n_pass < 1 || n_tiles < 1) return;
  if (vertical) hipLaunchKernelGGL(blur_stage_kernel<true>, dim3(n_tiles), dim3(AUG_THREADS), 0, s, passes, n_pass, base);
  else hipLaunchKernelGGL(blur_stage_kernel<false>, dim3(n_tiles), dim3(AUG_THREADS), 0, s, passes, n_pass, base);
}

// ---- host: ImagingGaussianBlur's box radius (_gaussian_blur_radius, 3 passes) and ImagingLineBoxBlur's weights.  The C source
// computes in float where it says float and lets sqrt and floor work in double; every assignment below is one such step.
void gauss_box(double radius, float* fr_out, uint32_t* ww_out, uint32_t* fw_out) {
  const float rad = (float)radius;
  const float s2 = rad * rad / 3.0f;
  const float L = (float)sqrt(12.0 * (double)s2 + 1.0);
  const float l = (float)floor(((double)L - 1.0) / 2.0);
  float a = (2.0f * l + 1.0f) * (l * (l + 1.0f) - 3.0f * s2);
  a = a / (6.0f * (s2 - (l + 1.0f) * (l + 1.0f)));
  const float fr = l + a;
  const int r = (int)fr;
  const uint32_t ww = (uint32_t)((float)(1u << 24) / (fr * 2.0f + 1.0f));
  *fr_out = fr;
  *ww_out = ww;
  *fw_out = (uint32_t)(((1 << 24) - (int64_t)(2 * r + 1) * ww) / 2);
}

}  // namespace uda
