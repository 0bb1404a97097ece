// scan.hip -- the device utilities every path shares: exclusive scans of int64 arrays, the key segments
// of a grouped batch, and the small word kernels that carry a batch's scalars between device and host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "launch.h"
#include "scan_dev.h"

namespace kcep {

// ---- key segments ----
// Key segments of a grouped batch in three passes over 1024-record blocks (256 threads x 4): boundaries
// per block, the blocks' exclusive prefix (scan_sums_reg), then every boundary's segment start.  flag /
// idx (optional: the runs carry build reads them) get the per-record boundary flag and its exclusive
// prefix.
__global__ __launch_bounds__(256) void seg_count(const int32_t* __restrict__ key, int64_t n, int64_t* __restrict__ bsum) {
  __shared__ int64_t s_w[4];
  const int64_t b0 = int64_t(blockIdx.x) * 1024 + threadIdx.x * 4;
  int64_t acc = 0, tot;
  for (int k = 0; k < 4; k++) {
    const int64_t i = b0 + k;
    if (i < n) acc += (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
  }
  block_scan_total<4>(acc, s_w, threadIdx.x & 63, threadIdx.x >> 6, tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(256) void seg_write(const int32_t* __restrict__ key, int64_t n, const int64_t* __restrict__ boff,
                                                 const int64_t* __restrict__ nseg, int64_t* __restrict__ seg_start,
                                                 int64_t* __restrict__ flag, int64_t* __restrict__ idx) {
  __shared__ int s_w[4];
  const int64_t b0 = int64_t(blockIdx.x) * 1024 + threadIdx.x * 4;
  int f[4], acc = 0;
  for (int k = 0; k < 4; k++) {
    const int64_t i = b0 + k;
    f[k] = i < n && (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
    acc += f[k];
  }
  int64_t run = boff[blockIdx.x] + block_scan_excl(acc, s_w, threadIdx.x & 63, threadIdx.x >> 6);
  for (int k = 0; k < 4; k++) {
    const int64_t i = b0 + k;
    if (i >= n) break;
    if (f[k]) seg_start[run] = i;
    if (flag) { flag[i] = f[k]; idx[i] = run; }
    run += f[k];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) seg_start[*nseg] = n;
}

// ---- exclusive scans ----
// 1024 elements per block: (1) block sums, (2) scan of block sums in one block, (3) per-block scan +
// offset.  Two arrays of one length at once (blockIdx.y / the block of pass 2 picks the array; tmp
// holds 2 x the block count); n_dev (optional): the length on the device, at most n (the grid is sized
// by n).
struct ScanPair {
  const int64_t* in[2];
  int64_t* out[2];
  int64_t* total[2];
  int64_t n;
  const int64_t* n_dev;
  int64_t nb;                     // blocks of the grid (from n)
};
__device__ __forceinline__ int64_t scan_len(const ScanPair& S) {
  return S.n_dev ? (*S.n_dev < S.n ? *S.n_dev : S.n) : S.n;
}
__global__ void scan_blocks(ScanPair S, int64_t* __restrict__ bsum) {
  __shared__ int64_t s[256];
  const int64_t n = scan_len(S);
  const int64_t* __restrict__ in = S.in[blockIdx.y];
  const int64_t b0 = int64_t(blockIdx.x) * 1024;
  // loads at clamped indices, masked after (a load under `i < n` is a branch waited on inside it)
  const int64_t last = n > 0 ? n - 1 : 0;
  int64_t v[4], acc = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int64_t i = b0 + threadIdx.x * 4 + k;
    v[k] = in[i < n ? i : last];
  }
#pragma unroll
  for (int k = 0; k < 4; k++) acc += b0 + threadIdx.x * 4 + k < n ? v[k] : 0;
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (threadIdx.x < unsigned(d)) s[threadIdx.x] += s[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) bsum[blockIdx.y * S.nb + blockIdx.x] = s[0];
}
// the fallback of pass 2 for more than SCAN_REG x 1024 block sums: 256 at a time with a carry
__global__ __launch_bounds__(256) void scan_sums(int64_t* __restrict__ bsum, int64_t nb, int64_t* __restrict__ total) {
  __shared__ int64_t s_w[4];
  int64_t carry = 0;
  for (int64_t base = 0; base < nb; base += 256) {
    const int64_t i = base + threadIdx.x;
    int64_t tot;
    const int64_t ex = block_scan_total<4>(i < nb ? bsum[i] : 0, s_w, threadIdx.x & 63, threadIdx.x >> 6, tot);
    if (i < nb) bsum[i] = carry + ex;
    carry += tot;
    __syncthreads();                               // (s_w is rewritten by the next step)
  }
  if (threadIdx.x == 0) *total = carry;
}
// the same scan of up to 16 x 1024 block sums (batches of <= 16 M elements) in one pass: every
// thread holds its 16 consecutive sums in registers, one block scan of the threads' sums (the loop
// above walks the sums 256 at a time: 44 us for 10 M elements when it took two barriers per scan step)
constexpr int SCAN_REG = 16;
__device__ __forceinline__ void scan_sums_reg_body(int64_t* __restrict__ bsum, int64_t nb, int64_t* __restrict__ total) {
  __shared__ int64_t s_w[16];
  const int tid = threadIdx.x;
  const int64_t per = (nb + 1023) / 1024, a = tid * per;
  int64_t v[SCAN_REG], sum = 0;
  const int64_t lastb = nb > 0 ? nb - 1 : 0;
#pragma unroll
  for (int i = 0; i < SCAN_REG; i++) v[i] = bsum[i < per && a + i < nb ? a + i : lastb];   // (clamped, masked below)
#pragma unroll
  for (int i = 0; i < SCAN_REG; i++) {
    if (!(i < per && a + i < nb)) v[i] = 0;
    sum += v[i];
  }
  int64_t run = block_scan_excl(sum, s_w, tid & 63, tid >> 6);
#pragma unroll
  for (int i = 0; i < SCAN_REG; i++)
    if (i < per && a + i < nb) { bsum[a + i] = run; run += v[i]; }
  if (tid == 1023) *total = run;
}
__global__ __launch_bounds__(1024) void scan_sums_reg(int64_t* __restrict__ bsum, int64_t nb, int64_t* __restrict__ total) {
  scan_sums_reg_body(bsum, nb, total);
}
__global__ __launch_bounds__(1024) void scan_sums_pair(ScanPair S, int64_t* __restrict__ bsum) {
  const int64_t nb = (scan_len(S) + 1023) / 1024;
  scan_sums_reg_body(bsum + blockIdx.x * S.nb, nb, S.total[blockIdx.x]);
}
__global__ __launch_bounds__(256) void scan_final(ScanPair S, const int64_t* __restrict__ bsum) {
  __shared__ int64_t s_w[4];
  const int64_t n = scan_len(S);
  const int64_t* __restrict__ in = S.in[blockIdx.y];
  int64_t* __restrict__ out = S.out[blockIdx.y];
  const int64_t b0 = int64_t(blockIdx.x) * 1024;
  if (b0 >= n) return;                             // (whole block: the barrier below stays uniform)
  int64_t v[4], acc = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int64_t i = b0 + threadIdx.x * 4 + k;
    v[k] = in[i < n ? i : n - 1];                  // (clamped, masked below; n > b0 >= 0 here)
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (b0 + threadIdx.x * 4 + k >= n) v[k] = 0;
    acc += v[k];
  }
  int64_t run = bsum[blockIdx.y * S.nb + blockIdx.x] + block_scan_excl(acc, s_w, threadIdx.x & 63, threadIdx.x >> 6);
  for (int k = 0; k < 4; k++) {
    const int64_t i = b0 + threadIdx.x * 4 + k;
    if (i < n) out[i] = run;
    run += v[k];
  }
}

// pass 2 over nb block sums of one array
static void scan_sums_launch(int64_t* bsum, int64_t nb, int64_t* total, hipStream_t st) {
  if (nb <= int64_t(SCAN_REG) * 1024) hipLaunchKernelGGL(scan_sums_reg, dim3(1), dim3(1024), 0, st, bsum, nb, total);
  else hipLaunchKernelGGL(scan_sums, dim3(1), dim3(256), 0, st, bsum, nb, total);
}

hipError_t exclusive_scan(const int64_t* in, int64_t n, int64_t* out, int64_t* total, int64_t* tmp,
                          hipStream_t st) {
  if (n <= 0) return hipMemsetAsync(total, 0, sizeof(int64_t), st);
  const int64_t nb = (n + 1023) / 1024;
  const ScanPair S{{in, in}, {out, out}, {total, total}, n, nullptr, nb};
  hipLaunchKernelGGL(scan_blocks, dim3(unsigned(nb)), dim3(256), 0, st, S, tmp);
  scan_sums_launch(tmp, nb, total, st);
  hipLaunchKernelGGL(scan_final, dim3(unsigned(nb)), dim3(256), 0, st, S, tmp);
  return hipGetLastError();
}

// Two exclusive scans of one length n (or *n_dev <= n, read on the device) in one set of launches;
// tmp: 2 x ceil(n / 1024) words.
hipError_t exclusive_scan_pair(const int64_t* in0, const int64_t* in1, int64_t n, const int64_t* n_dev, int64_t* out0,
                               int64_t* out1, int64_t* total0, int64_t* total1, int64_t* tmp, hipStream_t st) {
  const int64_t nb = (std::max<int64_t>(n, 1) + 1023) / 1024;
  const ScanPair S{{in0, in1}, {out0, out1}, {total0, total1}, std::max<int64_t>(n, 0), n_dev, nb};
  hipLaunchKernelGGL(scan_blocks, dim3(unsigned(nb), 2), dim3(256), 0, st, S, tmp);
  if (nb <= int64_t(SCAN_REG) * 1024) {
    hipLaunchKernelGGL(scan_sums_pair, dim3(2), dim3(1024), 0, st, S, tmp);
  } else {                                         // (blocks past *n_dev summed to 0 in scan_blocks)
    hipLaunchKernelGGL(scan_sums, dim3(1), dim3(256), 0, st, tmp, nb, total0);
    hipLaunchKernelGGL(scan_sums, dim3(1), dim3(256), 0, st, tmp + nb, nb, total1);
  }
  hipLaunchKernelGGL(scan_final, dim3(unsigned(nb), 2), dim3(256), 0, st, S, tmp);
  return hipGetLastError();
}

// flag / idx: nullptr, or n words each (the runs carry build's per-record boundary flags); tmp:
// ceil(n / 1024) + 1 words.  *nseg: the segment count (device).
hipError_t nfa_segments(const int32_t* key, int64_t n, int64_t* flag, int64_t* idx, int64_t* seg_start, int64_t* nseg,
                        int64_t* tmp, hipStream_t st) {
  if (n <= 0) return hipMemsetAsync(nseg, 0, sizeof(int64_t), st);
  const int64_t nb = (n + 1023) / 1024;
  hipLaunchKernelGGL(seg_count, dim3(unsigned(nb)), dim3(256), 0, st, key, n, tmp);
  scan_sums_launch(tmp, nb, nseg, st);
  hipLaunchKernelGGL(seg_write, dim3(unsigned(nb)), dim3(256), 0, st, key, n, tmp, nseg, seg_start, flag, idx);
  return hipGetLastError();
}

// ---- a batch's scalar words ----
// w[0..n) = 0 except w[at] = v
__global__ void set_words(int64_t* __restrict__ w, int n, int at, int64_t v) {
  const int t = threadIdx.x;
  if (t < n) w[t] = t == at ? v : 0;
}
hipError_t set_words_launch(int64_t* w, int n, int at, int64_t v, hipStream_t st) {
  if (n > 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(set_words, dim3(1), dim3(64), 0, st, w, n, at, v);
  return hipGetLastError();
}
// a[0..na) then b[0..nb) into h (pinned host memory mapped for the device): the host's view of a batch
__global__ void gather_words(const int64_t* __restrict__ a, int na, const int64_t* __restrict__ b, int nb,
                             int64_t* __restrict__ h) {
  const int t = threadIdx.x;
  if (t < na) h[t] = a[t];
  else if (t < na + nb) h[t] = b[t - na];
}
hipError_t gather_words_launch(const int64_t* a, int na, const int64_t* b, int nb, int64_t* h, hipStream_t st) {
  if (na + nb > 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gather_words, dim3(1), dim3(64), 0, st, a, na, b, nb, h);
  return hipGetLastError();
}

}  // namespace kcep
