// Device helpers shared by the post-processing kernels (kernels_post.hip: top-k pre-selection, per-class merge) and the
// NMS kernels (kernels_nms.hip): the order-preserving key of a score, the 64-bit priority key built on it and the
// block-wide scan of the radix selections.  Both files are compiled with -ffp-contract=off (see the Makefile).
#pragma once
#include "uda_internal.h"

namespace uda {

// order-preserving bits of a float; -0.0 takes +0.0's key: the reference compares floats, to which the two zeros are a tie
// (broken by the index), so no selection may rank one above the other
__device__ __forceinline__ uint32_t ord32(float v) {
  uint32_t b = __float_as_uint(v);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// priority of (score, position): the larger score first, among equal scores the smaller position
__device__ __forceinline__ unsigned long long nms_key(float s, int idx) {
  const uint32_t o = ord32(s);          // (-0.0 ties with +0.0 as in the reference's heap: the smaller index first)
  return ((unsigned long long)o << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)idx);
}

// block-wide exclusive scan of one int per thread (1024 threads = 16 waves); *total gets the sum
__device__ __forceinline__ int block_excl_scan(int v, int* wsum /*[17]*/, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  __syncthreads();
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int w = 0; w < 16; ++w) {
      const int t = wsum[w];
      wsum[w] = run;
      run += t;
    }
    wsum[16] = run;
  }
  __syncthreads();
  *total = wsum[16];
  return wsum[wave] + incl - v;
}

}  // namespace uda
