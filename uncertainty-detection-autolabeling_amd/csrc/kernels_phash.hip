// The perceptual hash of the pruning step (reference active_learning_loop.py:215-224: imagehash.phash of every pool image after
// Image.resize((512, 256))), from the 512 x 256 RGB plane on: uda_phash_np (include/uda_hip.h).  The resize to 512 x 256 itself is
// the bicubic passes of kernels_collage.hip; this file has what follows it.
//
//   phash_tail_kernel   one block an image: grey, Lanczos 512 -> 32 along x, Lanczos 256 -> 32 along y (the thumbnail), the 8 x 8
//                       low corner of the two-axis DCT-II in float64, its median, the 64 bits and the margin
//
// Grey is Pillow's L = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16.  The two Lanczos passes are Pillow's 8-bit resample on one
// channel with the tables of resample_coeffs(512, 32) and (256, 32): the accumulator starts at 2^21, adds pixel * coefficient in
// int32, is shifted right arithmetically by 22 and clamped to 0..255; the x pass is rounded to uint8 before the y pass reads it.
// A wave takes two neighbouring rows at a time - 3072 contiguous bytes, 48 a lane - turns them into 1024 grey bytes in LDS and
// reduces them to 2 x 32 bytes, a half wave a row and a lane an output column: the 128 KB grey plane never exists.
//
// The DCT is a direct sum against T[k][i] = 2 cos(pi k (2 i + 1) / 64), built on the host (phash_dct_table, every operation in
// double and rounded on its own, the C library's cos): a[k][j] = sum_i T[k][i] x[i][j] with i ascending from 0.0, then
// low[k][l] = sum_j a[k][j] T[l][j] with j ascending; every product is rounded, then every sum (built without FMA contraction,
// csrc/Makefile), so the result is bit-equal to a numpy loop that adds in the same order.  Wave 0 then holds low[k][l] in lane
// 8 k + l: a lane's rank is the count of values below its own, ties broken by the lane index; the lanes of rank 31 and 32 give
// med = (a + b) / 2 (numpy's median of 64 values), the hash word is the wave's ballot of low > med bit-reversed (lane 0 is bit
// 63: the first bit is the most significant), and margin = min over the lanes of |low - med|.
//
// LDS: the tables 21 248 bytes (T 2048, bounds 512, x coefficients 12 416, y coefficients 6272), the x pass's result 8192, the
// waves' grey rows 4096, the thumbnail 1024, a 2048, low, |low - med| and the two middle values 1040: 37 648 bytes a block,
// four blocks a CU.  Plain vector stores, no atomics.
#include <math.h>

#include "uda_internal.h"

namespace uda {

static_assert(PHASH_THREADS == 256 && PHASH_W == 512 && PHASH_H == 256 && PHASH_SIDE == 32 && PHASH_LOW == 8,
              "a lane takes 16 pixels of a pair of rows, a half wave the 32 columns of a row, a thread one a[k][j], a wave the 64 bits");
static_assert(PHASH_H % (2 * PHASH_WAVES) == 0 && sizeof(PhashTables) % 4 == 0, "every wave walks the same number of row pairs");

__device__ __forceinline__ uint32_t phash_byte(const uint32_t* w, int b) { return (w[b >> 2] >> ((b & 3) * 8)) & 255u; }

__global__ __launch_bounds__(PHASH_THREADS) void phash_tail_kernel(const uint8_t* __restrict__ pre, const PhashTables* __restrict__ tab,
                                                                   unsigned long long* __restrict__ words, double* __restrict__ margin,
                                                                   uint8_t* __restrict__ thumb, double* __restrict__ low) {
  __shared__ PhashTables s_t;
  __shared__ __attribute__((aligned(16))) uint8_t s_grey[PHASH_WAVES][2 * PHASH_W];
  __shared__ uint8_t s_h[PHASH_H * PHASH_SIDE];
  __shared__ uint8_t s_thumb[PHASH_SIDE * PHASH_SIDE];
  __shared__ double s_a[PHASH_LOW * PHASH_SIDE];
  __shared__ double s_low[64], s_dev[64], s_med[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t img = blockIdx.x;
  {
    const int32_t* from = (const int32_t*)tab;
    int32_t* to = (int32_t*)&s_t;
    for (int i = tid; i < (int)(sizeof(PhashTables) / 4); i += PHASH_THREADS) to[i] = from[i];
  }
  __syncthreads();
  const uint8_t* plane = pre + img * (PHASH_H * PHASH_W * 3);

  // grey and the pass along x: rows r and r + 1 of the wave, the row's half wave, column x
  {
    const int half = lane >> 5, x = lane & 31;
    const int xmin = s_t.bx[2 * x], xmax = s_t.bx[2 * x + 1];
    const int32_t* k = s_t.kx + x * PHASH_KX;
    for (int r0 = 0; r0 < PHASH_H; r0 += 2 * PHASH_WAVES) {
      const int r = r0 + 2 * wave;
      const uint4* src = (const uint4*)(plane + (int64_t)r * (PHASH_W * 3)) + lane * 3;   // 16-byte aligned: planes are, rows are 1536
      const uint4 v0 = src[0], v1 = src[1], v2 = src[2];
      const uint32_t w[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
      uint32_t g[4] = {0, 0, 0, 0};
#pragma unroll
      for (int p = 0; p < 16; ++p) {
        const uint32_t l = (phash_byte(w, 3 * p) * 19595u + phash_byte(w, 3 * p + 1) * 38470u + phash_byte(w, 3 * p + 2) * 7471u + 0x8000u) >> 16;
        g[p >> 2] |= l << ((p & 3) * 8);
      }
      *((uint4*)(&s_grey[wave][0]) + lane) = make_uint4(g[0], g[1], g[2], g[3]);
      __syncthreads();
      const uint8_t* px = &s_grey[wave][half * PHASH_W + xmin];
      int acc = 1 << (RESAMPLE_BITS - 1);
      for (int i = 0; i < xmax; ++i) acc += (int)px[i] * k[i];
      s_h[(r + half) * PHASH_SIDE + x] = (uint8_t)min(max(acc >> RESAMPLE_BITS, 0), 255);
      __syncthreads();                                                   // the rows have been read; s_h is whole after the last
    }
  }
  // the pass along y: the thumbnail
  for (int o = tid; o < PHASH_SIDE * PHASH_SIDE; o += PHASH_THREADS) {
    const int y = o / PHASH_SIDE, x = o % PHASH_SIDE;
    const int ymin = s_t.by[2 * y], ymax = s_t.by[2 * y + 1];
    const int32_t* k = s_t.ky + y * PHASH_KY;
    int acc = 1 << (RESAMPLE_BITS - 1);
    for (int i = 0; i < ymax; ++i) acc += (int)s_h[(ymin + i) * PHASH_SIDE + x] * k[i];
    const uint8_t v = (uint8_t)min(max(acc >> RESAMPLE_BITS, 0), 255);
    s_thumb[o] = v;
    thumb[img * (PHASH_SIDE * PHASH_SIDE) + o] = v;
  }
  __syncthreads();
  // the DCT along axis 0, rows 0..7 of it: one a[k][j] a thread
  {
    const int k = tid / PHASH_SIDE, j = tid % PHASH_SIDE;
    double s = 0.0;
    for (int i = 0; i < PHASH_SIDE; ++i) s = s + s_t.T[k * PHASH_SIDE + i] * (double)s_thumb[i * PHASH_SIDE + j];
    s_a[tid] = s;
  }
  __syncthreads();
  // along axis 1, columns 0..7: wave 0, lane 8 k + l
  double v = 0.0;
  if (tid < 64) {
    const int k = tid / PHASH_LOW, l = tid % PHASH_LOW;
    for (int j = 0; j < PHASH_SIDE; ++j) v = v + s_a[k * PHASH_SIDE + j] * s_t.T[l * PHASH_SIDE + j];
    s_low[tid] = v;
    low[img * 64 + tid] = v;
  }
  __syncthreads();
  if (tid < 64) {
    int rank = 0;
    for (int j = 0; j < 64; ++j) {
      const double u = s_low[j];
      rank += (u < v || (u == v && j < tid)) ? 1 : 0;
    }
    if (rank == 31) s_med[0] = v;
    if (rank == 32) s_med[1] = v;
  }
  __syncthreads();
  if (tid < 64) {
    const double med = (s_med[0] + s_med[1]) / 2.0;
    const unsigned long long bits = __ballot(v > med);
    s_dev[tid] = fabs(v - med);
    if (tid == 0) words[img] = __brevll(bits);
  }
  __syncthreads();
  if (tid == 0) {
    double m = s_dev[0];
    for (int j = 1; j < 64; ++j) m = fmin(m, s_dev[j]);
    margin[img] = m;
  }
}

void launch_phash_tail(const uint8_t* pre, int n, const PhashTables* tab, unsigned long long* words, double* margin, uint8_t* thumb,
                       double* low, hipStream_t s) {
  if (n < 1) return;
  hipLaunchKernelGGL(phash_tail_kernel, dim3(n), dim3(PHASH_THREADS), 0, s, pre, tab, words, margin, thumb, low);
}

// ---- host: the DCT-II table of scipy.fftpack.dct (type 2, unnormalised), rows 0..7 of 32
void phash_dct_table(double* T) {
  for (int k = 0; k < PHASH_LOW; ++k)
    for (int i = 0; i < PHASH_SIDE; ++i) T[k * PHASH_SIDE + i] = 2.0 * cos(M_PI * k * (2 * i + 1) / 64.0);
}

}  // namespace uda
