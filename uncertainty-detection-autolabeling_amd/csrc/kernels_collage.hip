// RCC collages (reference ssl_utils/parent.py:317-686, Parent_SSL.crop_collage): Pillow's two-pass 8-bit Lanczos resample on
// packed RGB uint8 planes, many jobs per call: uda_resample_np (include/uda_hip.h).  The same passes with bicubic tables are
// the first step of the perceptual hash (uda_phash_np; kernels_phash.hip has the rest): the kernel does not know the filter.  Pillow's arithmetic (src/libImaging/Resample.c,
// precompute_coeffs / normalize_coeffs_8bpc / ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc) is integer
// arithmetic on coefficient tables, so the result is Pillow's bit for bit.  Built without FMA contraction (csrc/Makefile): the
// tables are made by resample_coeffs below, host code, every operation in double and rounded on its own, with the C library's sin.
//
//   resample_pass_kernel<false>   one axis of one job: along x.  A line is a row, a position a column
//   resample_pass_kernel<true>    the same along y.  A line is a column, a position a row
//
// Which passes a job takes and in which order is the host's decision (uda_services.hip): along x first with the result rounded to
// uint8 in scratch, a pass skipped where its axis keeps its length, and along y first where Image.resize itself goes that way.
//
// A block takes one tile of one pass: tw output positions x 256 / tw lines (tw a power of two <= RESAMPLE_TW, chosen by the host
// so that the tile's source span fits the LDS buffer), found by a binary search of the block index in the passes' first tiles.
// The window of an output position (ksize coefficients, of which the first xmax count) is walked in chunks of RESAMPLE_KCH: per
// chunk the block stages the chunk of the tile's coefficient rows and the source span those need - first xmin of the tile plus
// the chunk's offset up to the last xmin plus the chunk's end, cut at the plane's end - in LDS; xmin ascends with the output
// position, so every live thread finds its taps there.  ksize is 7 when enlarging and unbounded when shrinking; the chunks
// make the LDS need independent of it.  An accumulator starts at 2^21, adds pixel * coefficient in int32, is shifted right
// arithmetically by 22 and clamped to 0..255, as Pillow's clip8 does.
//
// Stores are three single bytes per thread: a job writes the bytes of its own rectangle and no others, whatever its x offset.
// No atomics.  A job that keeps its source's size is one pass over the identity table (one coefficient of 2^22: the accumulator
// gives the pixel back), so a copy takes the same path as everything else.
#include <math.h>

#include "uda_internal.h"

namespace uda {

static_assert(RESAMPLE_THREADS == 256 && RESAMPLE_TW * RESAMPLE_SPAN_PER_POS * 3 * (RESAMPLE_THREADS / RESAMPLE_TW) == RESAMPLE_LDS,
              "a tile of tw positions holds a span of RESAMPLE_SPAN_PER_POS * tw pixels for each of its 256 / tw lines");

template <bool VERT>
__global__ __launch_bounds__(RESAMPLE_THREADS) void resample_pass_kernel(const ResamplePass* __restrict__ passes, int n_pass,
                                                                        const int32_t* __restrict__ pool, uint8_t* __restrict__ base) {
  __shared__ uint8_t s_src[RESAMPLE_LDS];
  __shared__ int32_t s_k[RESAMPLE_TW * RESAMPLE_KCH];
  __shared__ int32_t s_b[RESAMPLE_TW * 2];
  const int blk = blockIdx.x, tid = threadIdx.x;
  int lo = 0, hi = n_pass - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (passes[mid].tile0 <= blk) lo = mid; else hi = mid - 1;
  }
  const ResamplePass p = passes[lo];
  const int tw = p.tw, lines = RESAMPLE_THREADS / tw;
  const int tile = blk - p.tile0, tp = tile % p.tiles_pos, tl = tile / p.tiles_pos;
  const int o0 = tp * tw, l0 = tl * lines;
  const int no = min(tw, p.n_out - o0), nl = min(lines, p.n_lines - l0);
  if (no < 1 || nl < 1) return;                                        // (block-uniform; the host launches no such tile)
  // along y neighbouring threads take neighbouring columns, along x neighbouring output columns: either way neighbouring bytes
  const int t = VERT ? tid / lines : tid % tw, l = VERT ? tid % lines : tid / tw;
  const int32_t* bounds = pool + p.coef_off;
  const int32_t* kk = bounds + 2 * (int64_t)p.out_full;
  if (tid < 2 * no) s_b[tid] = bounds[2 * o0 + tid];
  __syncthreads();
  const int first = s_b[0], last = s_b[2 * (no - 1)];
  const bool live = t < no && l < nl;
  const int xmin = live ? s_b[2 * t] : 0, xmax = live ? s_b[2 * t + 1] : 0;
  int a0 = 1 << (RESAMPLE_BITS - 1), a1 = a0, a2 = a0;
  const uint8_t* src = base + p.src;
  for (int k0 = 0; k0 < p.ksize; k0 += RESAMPLE_KCH) {
    const int s0 = first + k0, span = min(last + k0 + RESAMPLE_KCH, p.in_size) - s0;
    if (span <= 0) break;                                              // every window of the tile has ended (block-uniform)
    const int run = VERT ? nl * 3 : span * 3, outer = VERT ? span : nl;
    if (run * outer > RESAMPLE_LDS) return;                            // (never: the host fits tw to the span)
    if (k0) __syncthreads();                                           // the previous chunk has been read
    for (int i = tid; i < no * RESAMPLE_KCH; i += RESAMPLE_THREADS) {
      const int k = k0 + i % RESAMPLE_KCH;
      s_k[i] = k < p.ksize ? kk[(int64_t)(o0 + i / RESAMPLE_KCH) * p.ksize + k] : 0;
    }
    const uint8_t* from = src + (VERT ? (int64_t)s0 * p.src_stride + (int64_t)l0 * 3 : (int64_t)l0 * p.src_stride + (int64_t)s0 * 3);
    for (int i = tid; i < run * outer; i += RESAMPLE_THREADS) {
      const int o = i / run;
      s_src[i] = from[(int64_t)o * p.src_stride + (i - o * run)];
    }
    __syncthreads();
    const int ke = min(xmax, k0 + RESAMPLE_KCH);
    const uint8_t* px = s_src + (VERT ? (xmin + k0 - s0) * run + l * 3 : l * run + (xmin + k0 - s0) * 3);
    const int step = VERT ? run : 3;
    for (int k = k0; k < ke; ++k, px += step) {
      const int c = s_k[t * RESAMPLE_KCH + k - k0];
      a0 += (int)px[0] * c;
      a1 += (int)px[1] * c;
      a2 += (int)px[2] * c;
    }
  }
  if (!live) return;
  uint8_t* to = base + p.dst + (VERT ? (int64_t)(o0 + t) * p.dst_stride + (int64_t)(l0 + l) * 3 : (int64_t)(l0 + l) * p.dst_stride + (int64_t)(o0 + t) * 3);
  to[0] = (uint8_t)min(max(a0 >> RESAMPLE_BITS, 0), 255);
  to[1] = (uint8_t)min(max(a1 >> RESAMPLE_BITS, 0), 255);
  to[2] = (uint8_t)min(max(a2 >> RESAMPLE_BITS, 0), 255);
}

void launch_resample_passes(const ResamplePass* passes, int n_pass, int n_tiles, bool vertical, const int32_t* pool, uint8_t* base,
                            hipStream_t s) {
  if (n_pass < 1 || n_tiles < 1) return;
  if (vertical) hipLaunchKernelGGL(resample_pass_kernel<true>, dim3(n_tiles), dim3(RESAMPLE_THREADS), 0, s, passes, n_pass, pool, base);
  else hipLaunchKernelGGL(resample_pass_kernel<false>, dim3(n_tiles), dim3(RESAMPLE_THREADS), 0, s, passes, n_pass, pool, base);
}

// ---- host: Pillow's coefficient tables
static double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
static double lanczos_filter(double x) {                                // truncated sinc
  if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
  return 0.0;
}
static double bicubic_filter(double x) {                                // Keys' cubic with a = -0.5, Pillow's BICUBIC
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
static double filter_support(int filter) { return filter == UDA_FILTER_BICUBIC ? 2.0 : 3.0; }

int resample_ksize(int in_size, int out_size, int filter) {
  double filterscale = (double)in_size / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  return (int)ceil(filter_support(filter) * filterscale) * 2 + 1;
}

// precompute_coeffs and normalize_coeffs_8bpc for the whole axis [0, in_size) with the filter UDA_FILTER_LANCZOS or
// UDA_FILTER_BICUBIC: bounds [out_size, 2] = (xmin, xmax), kk [out_size, ksize], zero past xmax
void resample_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk) {
  double filterscale, scale;
  filterscale = scale = (double)in_size / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = filter_support(filter) * filterscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  std::vector<double> pre(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale, ss = 1.0 / filterscale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    for (int x = 0; x < xmax; ++x) {
      const double at = (x + xmin - center + 0.5) * ss;
      const double w = filter == UDA_FILTER_BICUBIC ? bicubic_filter(at) : lanczos_filter(at);
      pre[x] = w;
      ww = ww + w;
    }
    int32_t* k = kk + (size_t)xx * ksize;
    for (int x = 0; x < xmax; ++x) {
      if (ww != 0.0) pre[x] = pre[x] / ww;
      k[x] = pre[x] < 0 ? (int)(-0.5 + pre[x] * (1 << RESAMPLE_BITS)) : (int)(0.5 + pre[x] * (1 << RESAMPLE_BITS));
    }
    for (int x = xmax; x < ksize; ++x) k[x] = 0;
    bounds[xx * 2] = xmin;
    bounds[xx * 2 + 1] = xmax;
  }
}

}  // namespace uda
