// The device idioms the services share, each stated once: the float64 zero-padded pairwise tree sum of DESIGN §21
// (`b = b[0::2] + b[1::2]` over the zero-padded terms until one value is left; tests/tree_ref.py is its numpy statement), the
// wave's ballot count and the wave's lexicographic arg-max.  No state; a wave is 64 lanes.  The files that promise the tree bit
// for bit are built without FMA contraction (csrc/Makefile).
#pragma once
#include <hip/hip_runtime.h>

namespace uda {

// The tree over the wave's 64 values, lane l holding term l.  The offsets ASCEND: at offset 1 a lane adds its neighbour, which
// is the tree's first level `b[0::2] + b[1::2]`, at offset 2 the neighbouring pair's sum, and so on - after offset o a lane holds
// the node over its aligned group of 2 o lanes.  Descending offsets would sum the same terms in another tree.  Both lanes of a
// pair compute left + right, one as v + other and one as other + v; addition commutes, so they agree bit for bit and every lane
// ends with the root.
__device__ __forceinline__ double wave_tree_sum(double v) {
  for (int o = 1; o < 64; o <<= 1) v = v + __shfl_xor(v, o);
  return v;
}

// the lanes of the wave with p; every lane takes the step (the ballot sees all 64), a lane that is off counts for nothing
__device__ __forceinline__ unsigned int wave_count(bool p) { return (unsigned int)__popcll(__ballot(p)); }

// The tree over four values `stride` apart: a block's fold of its four wave roots or counts (the kernels that rely on a block
// being four waves assert it), or a row's four coordinate terms.  Never ((w0 + w1) + w2) + w3.
template <typename T>
__device__ __forceinline__ T fold4(const T* w, int stride = 1) {
  return (w[0] + w[stride]) + (w[2 * stride] + w[3 * stride]);
}

// The tree over run roots that arrive one by one, as a binary counter: root number `index` (from 0) joins the tree held in
// stack[level] - it waits at level l until the next root of that level arrives, the earlier one on the left.  A caller asserts
// that its largest number of runs fits 2^(RUN_TREE_LEVELS - 1).
constexpr int RUN_TREE_LEVELS = 16;
__device__ __forceinline__ void run_tree_push(double* stack, int index, double r) {
  int l = 0;
  for (int c = index; c & 1; c >>= 1, ++l) r = stack[l] + r;
  stack[l] = r;
}
// after `runs` >= 1 pushes: zero roots up to a power of two, then the root
__device__ __forceinline__ double run_tree_root(double* stack, int runs) {
  int P = 1, top = 0;
  while (P < runs) { P <<= 1; ++top; }
  for (int z = runs; z < P; ++z) run_tree_push(stack, z, 0.0);
  return stack[top];
}

// The tree over P slots (a power of two, or 0: nothing to fold), in place, the root to buf[0]; thread t of T cooperating
// threads.  At stride s slot j (a multiple of 2 s) takes slot j + s, so no slot is read by one thread and written by another
// between two barriers.  There is a __syncthreads() per stride: P must be uniform over the BLOCK, and every thread of the block
// calls - one whose buf is not to be folded with mine == false, which takes the barriers only.
__device__ __forceinline__ void fold_slots_in_place(double* buf, int P, int t, int T, bool mine) {
  for (int s = 1; s < P; s <<= 1) {
    if (mine)
      for (int j = t * 2 * s; j < P; j += T * 2 * s) buf[j] = buf[j] + buf[j + s];
    __syncthreads();
  }
}

// the wave's lexicographic best of (higher key, lower index); every lane ends with it (the callers keep NaN
// out of the keys: no comparison with one holds)
__device__ __forceinline__ void wave_best_max(double& key, int& best) {
  for (int o = 32; o > 0; o >>= 1) {
    const double ok = __shfl_xor(key, o);
    const int ob = __shfl_xor(best, o);
    if (ok > key || (ok == key && ob < best)) { key = ok; best = ob; }
  }
}

}  // namespace uda
