// scan_dev.h -- the prefix scan over a wave and over a workgroup, written once (device only; every
// scan of the built-in kernels comes from here, the per-pattern kernels of jit.cpp have none).
// lane / wid: the thread's lane in its wave and its wave in the workgroup (threadIdx.x & 63, >> 6).
#pragma once
#include <hip/hip_runtime.h>

namespace kcep {

struct ScanAdd {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct ScanMax {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; }
};

// Inclusive scan of x over the wave's 64 lanes by shuffle-up: lane i gets op over lanes 0..i
template <class T, class Op = ScanAdd>
__device__ __forceinline__ T wave_scan_incl(T x, int lane, Op op = {}) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T y = __shfl_up(x, d, 64);
    if (lane >= d) x = op(x, y);
  }
  return x;
}
// x of the lane below; lane 0 gets `first` (an inclusive wave scan made exclusive)
template <class T>
__device__ __forceinline__ T wave_prev(T x, int lane, T first) {
  const T y = __shfl_up(x, 1, 64);
  return lane == 0 ? first : y;
}

// Exclusive prefix sum of x over the workgroup's threads (whole waves, at most 16): the wave scan, then
// the wave sums through s_w (one barrier; the caller keeps s_w free until it)
template <class T, class W>
__device__ __forceinline__ T block_scan_excl(T x, W* s_w, int lane, int wid) {
  const T incl = wave_scan_incl(x, lane);
  if (lane == 63) s_w[wid] = incl;
  __syncthreads();
  T run = incl - x;
  for (int w = 0; w < wid; w++) run += T(s_w[w]);
  return run;
}

// The same over a workgroup of exactly NW waves, with the workgroup's sum in total (every thread's)
template <int NW, class T, class W>
__device__ __forceinline__ T block_scan_total(T x, W* s_w, int lane, int wid, T& total) {
  const T incl = wave_scan_incl(x, lane);
  if (lane == 63) s_w[wid] = incl;
  __syncthreads();
  T run = incl - x;
  total = 0;
#pragma unroll
  for (int w = 0; w < NW; w++) {
    const T s = T(s_w[w]);
    if (w < wid) run += s;
    total += s;
  }
  return run;
}

}  // namespace kcep
