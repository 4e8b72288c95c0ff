// The fixed-order reductions every deterministic operator shares ("no float atomics, two calls give identical bits").
// One order, stated here and nowhere else:
//   1. each thread accumulates its own strided elements sequentially (the caller's loop);
//   2. the 64 lanes of a wave combine by the xor tree  v = v op v[lane ^ o],  o = 32, 16, 8, 4, 2, 1;
//   3. lane 0 of wave w stores its N values to the caller's LDS array sh[w][0..N);
//   4. after a barrier the waves are left-folded in wave order:  ((w0 op w1) op w2) op ... ;
//   5. per-block partials are summed by one workgroup the same way: thread t takes partials t, t + threads, ... sequentially,
//      then steps 2-4.
// The barrier that guards the LDS array against the previous reduction's readers is INSIDE nm_block_reduce: reducing twice
// through one array needs nothing from the caller.  Every loop over N is fully unrolled, so accumulator arrays stay in registers.
#pragma once
#include <hip/hip_runtime.h>

// An operator is apply(j, a, b): j is the accumulator's index, so that one reduction can carry accumulators of different kinds.
struct NmSum {
  template <typename T>
  __device__ __forceinline__ static T apply(int, T a, T b) { return a + b; }
};
struct NmMin {
  __device__ __forceinline__ static float apply(int, float a, float b) { return fminf(a, b); }
  __device__ __forceinline__ static double apply(int, double a, double b) { return fmin(a, b); }
};
struct NmMax {
  __device__ __forceinline__ static float apply(int, float a, float b) { return fmaxf(a, b); }
  __device__ __forceinline__ static double apply(int, double a, double b) { return fmax(a, b); }
};
// a bounding box in one reduction: accumulators [0, H) by min, the others by max
template <int H>
struct NmMinMax {
  template <typename T>
  __device__ __forceinline__ static T apply(int j, T a, T b) { return j < H ? NmMin::apply(j, a, b) : NmMax::apply(j, a, b); }
};

// step 2 for accumulator j; the result is valid in every lane.  (x by reference on purpose: by value, hipcc optimises the
// CALLER's accumulation loop along another path and k_classical_bwd / k_regist_bwd contract other products into fmas, which
// moves their results by an ulp.  tests cannot see that; a byte comparison of outputs against the previous build does.)
template <class Op, typename T>
__device__ __forceinline__ T nm_wave_reduce(const T& x, int j = 0) {
  T v = x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = Op::apply(j, v, __shfl_xor(v, o, 64));
  return v;
}

// What nm_block_reduce leaves behind: tot[j] is step 4 for accumulator j (j < N, may differ per thread), readable by any
// thread until the next reduction through the same LDS array.
template <int NW, int N, class Op, typename T>
struct NmBlockTotals {
  const T* sh;
  __device__ __forceinline__ T operator[](int j) const {
    T v = sh[j];
#pragma unroll
    for (int w = 1; w < NW; ++w) v = Op::apply(j, v, sh[w * N + j]);
    return v;
  }
};

// steps 2-4 for a workgroup of NW waves; every thread of the workgroup must call it.  sh: LDS, NW * N elements.
template <int NW, class Op, int N, typename T>
__device__ __forceinline__ NmBlockTotals<NW, N, Op, T> nm_block_reduce(const T (&acc)[N], T* sh) {
  T v[N];
#pragma unroll
  for (int j = 0; j < N; ++j) v[j] = nm_wave_reduce<Op>(acc[j], j);
  __syncthreads();      // sh may still be read as the previous reduction's totals
  if ((threadIdx.x & 63) == 0) {
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < N; ++j) sh[wave * N + j] = v[j];
  }
  __syncthreads();
  return {sh};
}

// one accumulator, its total in every thread
template <int NW, class Op, typename T>
__device__ __forceinline__ T nm_block_reduce(T v, T* sh) {
  const T acc[1] = {v};
  return nm_block_reduce<NW, Op>(acc, sh)[0];
}

// step 5: the sums of nb per-block partial sets, element j of set b at part[b * stride + j]
template <int NW, int N, typename T>
__device__ __forceinline__ NmBlockTotals<NW, N, NmSum, T> nm_block_sum_partials(const T* __restrict__ part, int nb, int stride, T* sh) {
  T acc[N];
#pragma unroll
  for (int j = 0; j < N; ++j) acc[j] = T(0);
  for (int b = threadIdx.x; b < nb; b += NW * 64) {
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] += part[(size_t)b * stride + j];
  }
  return nm_block_reduce<NW, NmSum>(acc, sh);
}
