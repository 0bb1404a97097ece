// filter.hip -- CEP_BATCH_FILTER: the two rules CEPProcessor.process applies to a record before it
// evaluates the NFA, on the device, for the sessions that carry records instead of NFA state (stencil,
// chain, runs):
//   - a record with a null key or value is dropped (CEPProcessor.java:136-138);
//   - a record whose offset is below its key's per-topic high-water mark is dropped (:140, :152-160); an
//     admitted one moves the mark to offset + 1 (:144-145).
// A dropped record has offset + 1 <= mark, so the mark record i sees is
//   max(carried mark, max over the earlier valid records j of its key and topic in the batch of offset_j + 1):
// an exclusive prefix maximum, segmented by key, per topic -- no sequential dependency.  The batch is
// key-grouped (the caller's, or group.hip's output), so a key is one segment, of any length.
//
//   filter_tiles    per tile of FILTER_TF records: its summary (a segment starts in it; per topic the
//                   maximum of offset + 1 since that start, or over the whole tile)
//   filter_scan     one workgroup: the exclusive segmented scan of the tile summaries
//   filter_apply    per tile again, from its prefix: the admission of every record, its rank among the
//                   tile's admitted ones, the tile's count; the thread holding a key's last record stages
//                   the key's new marks (the inclusive maximum there)
//   filter_offsets  one workgroup: the tiles' counts scanned; the admitted count (and the topic-range
//                   flag) to a pinned host word, stamped -- the host sizes the path's launches by it
//   filter_gather   per record: every column of an admitted record to tile offset + rank, with its
//                   stream position
//   filter_commit   after the path accepted the batch: staged marks into the table (one thread per key)
// No workgroup waits for another; every pass is linear in n whatever the key distribution.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "scan_dev.h"

namespace kcep {

namespace {

constexpr int64_t FM_NONE = INT64_MIN;           // no valid record of the topic since the segment's start
constexpr uint16_t FS_DROPPED = 0xFFFF;          // slot of a dropped record (ranks are < FILTER_TF)
constexpr int FPT = FILTER_TF / 256;             // consecutive records per thread

// the scan's element: per topic the maximum of offset + 1, and whether a key segment starts inside
template <int NT>
struct Seg {
  int64_t v[NT];
  int f;
};
template <int NT>
__device__ __forceinline__ Seg<NT> seg_none() {
  Seg<NT> s;
#pragma unroll
  for (int t = 0; t < NT; t++) s.v[t] = FM_NONE;
  s.f = 0;
  return s;
}
// b = a (+) b, a the earlier: a segment start inside b cuts a off
template <int NT>
__device__ __forceinline__ void seg_after(Seg<NT>& b, const Seg<NT>& a) {
#pragma unroll
  for (int t = 0; t < NT; t++) b.v[t] = b.f || a.v[t] < b.v[t] ? b.v[t] : a.v[t];
  b.f |= a.f;
}
template <int NT>
__device__ __forceinline__ Seg<NT> seg_shfl_up(const Seg<NT>& x, int d) {
  Seg<NT> y;
#pragma unroll
  for (int t = 0; t < NT; t++) y.v[t] = __shfl_up(x.v[t], d, 64);
  y.f = __shfl_up(x.f, d, 64);
  return y;
}
// exclusive scan over the workgroup's 256 threads (s_w: 4 elements of LDS); total: all of them
template <int NT>
__device__ __forceinline__ Seg<NT> seg_block_excl(const Seg<NT>& x, Seg<NT>* s_w, Seg<NT>& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  Seg<NT> incl = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const Seg<NT> y = seg_shfl_up(incl, d);
    if (lane >= d) seg_after(incl, y);
  }
  Seg<NT> ex = seg_shfl_up(incl, 1);
  if (lane == 0) ex = seg_none<NT>();
  if (lane == 63) s_w[wid] = incl;
  __syncthreads();
  Seg<NT> pre = seg_none<NT>();
  total = seg_none<NT>();
#pragma unroll
  for (int w = 0; w < 4; w++) {
    if (w == wid) pre = total;
    Seg<NT> a = s_w[w];
    seg_after(a, total);
    total = a;
  }
  seg_after(ex, pre);
  __syncthreads();                                 // (s_w may be written again)
  return ex;
}

// a thread's FPT consecutive records, every load issued at a clamped index before any is used
template <int NT>
struct Recs {
  int32_t key[FPT + 2];                            // [0] the record before, [FPT + 1] the record after
  int32_t tp[FPT];
  int64_t off[FPT];
  uint8_t vl[FPT];
};
template <int NT>
__device__ __forceinline__ void recs_load(const FilterArgs& A, int64_t b0, int64_t n, Recs<NT>& R) {
  const int64_t last = n - 1;
#pragma unroll
  for (int j = 0; j < FPT + 2; j++) {
    const int64_t i = b0 - 1 + j;
    R.key[j] = A.key[i < 0 ? 0 : i > last ? last : i];
  }
#pragma unroll
  for (int j = 0; j < FPT; j++) {
    const int64_t i = b0 + j > last ? last : b0 + j;
    R.vl[j] = A.valid ? A.valid[i] : uint8_t(1);
    R.tp[j] = NT > 1 ? A.topic[i] : 0;
    R.off[j] = A.offset[i];
  }
}
// record j's own contribution, its topic in range
template <int NT>
__device__ __forceinline__ void seg_take(Seg<NT>& S, bool ok, int32_t tp, int64_t off) {
#pragma unroll
  for (int t = 0; t < NT; t++)
    if (ok && t == tp && S.v[t] < off + 1) S.v[t] = off + 1;
}
// the thread's records folded from an empty element
template <int NT>
__device__ __forceinline__ Seg<NT> recs_fold(const Recs<NT>& R, int64_t b0, int64_t n) {
  Seg<NT> S = seg_none<NT>();
#pragma unroll
  for (int j = 0; j < FPT; j++) {
    const int64_t i = b0 + j;
    if (i >= n) break;
    if (i == 0 || R.key[j + 1] != R.key[j]) {
      S = seg_none<NT>();
      S.f = 1;
    }
    seg_take(S, R.vl[j] && uint32_t(R.tp[j]) < uint32_t(NT), R.tp[j], R.off[j]);
  }
  return S;
}

template <int NT>
__global__ __launch_bounds__(256) void filter_tiles(FilterArgs A, int64_t n) {
  __shared__ Seg<NT> s_w[4];
  const int64_t b0 = int64_t(blockIdx.x) * FILTER_TF + threadIdx.x * FPT;
  Recs<NT> R;
  recs_load<NT>(A, b0, n, R);
  const Seg<NT> S = recs_fold<NT>(R, b0, n);
  Seg<NT> tot;
  seg_block_excl<NT>(S, s_w, tot);
  if (threadIdx.x == 0) {
    A.tile_f[blockIdx.x] = tot.f;
#pragma unroll
    for (int t = 0; t < NT; t++) A.tile_v[int64_t(blockIdx.x) * NT + t] = tot.v[t];
  }
}

// tile summaries -> what each tile's first record sees from the tiles before it (in place); zeroes the
// batch's topic-range flag, which filter_apply sets
template <int NT>
__global__ __launch_bounds__(256) void filter_scan(FilterArgs A, int64_t nt) {
  __shared__ Seg<NT> s_w[4];
  if (threadIdx.x == 0) *A.bad = 0;
  Seg<NT> carry = seg_none<NT>();
  for (int64_t base = 0; base < nt; base += 256) {
    const int64_t i = base + threadIdx.x, c = i < nt ? i : nt - 1;
    Seg<NT> x;
    x.f = A.tile_f[c];
#pragma unroll
    for (int t = 0; t < NT; t++) x.v[t] = A.tile_v[c * NT + t];
    if (i >= nt) x = seg_none<NT>();
    Seg<NT> tot;
    Seg<NT> ex = seg_block_excl<NT>(x, s_w, tot);
    seg_after(ex, carry);
    seg_after(tot, carry);
    carry = tot;
    if (i < nt) {
#pragma unroll
      for (int t = 0; t < NT; t++) A.tile_v[i * NT + t] = ex.v[t];
    }
  }
}

// the admitted records of the thread ranked within the tile: slots (one 8-byte store per thread: the slot
// array is padded to whole tiles) and the tile's count
__device__ __forceinline__ void filter_emit(const FilterArgs& A, const bool (&adm)[FPT], int64_t b0, int64_t n,
                                            int* s_c) {
  static_assert(FPT == 4, "a thread's slots are one 8-byte store");
  int c = 0, tot;
#pragma unroll
  for (int j = 0; j < FPT; j++) c += adm[j] ? 1 : 0;
  int run = block_scan_total<4>(c, s_c, threadIdx.x & 63, threadIdx.x >> 6, tot);
  uint64_t word = 0;
#pragma unroll
  for (int j = 0; j < FPT; j++) {
    const uint16_t sl = adm[j] ? uint16_t(run) : FS_DROPPED;
    run += adm[j] ? 1 : 0;
    word |= uint64_t(sl) << (16 * j);
  }
  if (b0 < n) *reinterpret_cast<uint64_t*>(A.slot + b0) = word;
  if (threadIdx.x == 0) A.tile_cnt[blockIdx.x] = tot;
}

template <int NT>
__global__ __launch_bounds__(256) void filter_apply(FilterArgs A, int64_t n) {
  __shared__ Seg<NT> s_w[4];
  __shared__ int s_c[4];
  __shared__ int s_bad;
  const int64_t b0 = int64_t(blockIdx.x) * FILTER_TF + threadIdx.x * FPT;
  if (threadIdx.x == 0) s_bad = 0;
  Recs<NT> R;
  recs_load<NT>(A, b0, n, R);
  // the carried marks of the thread's records (key ids out of range: none; the path fails the batch)
  int64_t mk[FPT];
  bool ok[FPT], kin[FPT + 1];
#pragma unroll
  for (int j = 0; j < FPT; j++) {
    kin[j] = R.key[j + 1] >= 0 && R.key[j + 1] < A.max_keys;
    ok[j] = R.vl[j] && uint32_t(R.tp[j]) < uint32_t(NT);
    mk[j] = A.marks[(kin[j] ? int64_t(R.key[j + 1]) : 0) * FILTER_MAX_TOPICS + (ok[j] ? R.tp[j] : 0)];
  }
  Seg<NT> pre;                                     // what the tile's first record sees
  pre.f = 0;
#pragma unroll
  for (int t = 0; t < NT; t++) pre.v[t] = A.tile_v[int64_t(blockIdx.x) * NT + t];
  Seg<NT> tot;
  Seg<NT> S = seg_block_excl<NT>(recs_fold<NT>(R, b0, n), s_w, tot);
  seg_after(S, pre);
  bool adm[FPT], bad = false;
#pragma unroll
  for (int j = 0; j < FPT; j++) {
    const int64_t i = b0 + j;
    adm[j] = false;
    if (i >= n) continue;
    if (i == 0 || R.key[j + 1] != R.key[j]) S = seg_none<NT>();
    int64_t seen = kin[j] && ok[j] ? mk[j] : -1;   // a mark never set: -1 (the reference's -1L)
#pragma unroll
    for (int t = 0; t < NT; t++)
      if (t == R.tp[j] && seen < S.v[t]) seen = S.v[t];
    adm[j] = ok[j] && !(R.off[j] < seen);
    bad = bad || (R.vl[j] && !ok[j]);
    seg_take(S, ok[j], R.tp[j], R.off[j]);
    if ((i == n - 1 || R.key[j + 2] != R.key[j + 1]) && kin[j]) {   // the key's last record: its new marks
#pragma unroll
      for (int t = 0; t < NT; t++) A.stage[int64_t(R.key[j + 1]) * FILTER_MAX_TOPICS + t] = S.v[t];
    }
  }
  __syncthreads();                                 // (s_bad zeroed)
  if (bad) s_bad = 1;
  filter_emit(A, adm, b0, n, s_c);                 // (its barrier orders s_bad)
  if (threadIdx.x == 0 && s_bad) *A.bad = 1;       // a valid record's topic id out of [0, FILTER_MAX_TOPICS)
}

// without marks (CEP_MODE_NFA, or a batch without offsets): only the null rule
__global__ __launch_bounds__(256) void filter_valid(FilterArgs A, int64_t n) {
  __shared__ int s_c[4];
  const int64_t b0 = int64_t(blockIdx.x) * FILTER_TF + threadIdx.x * FPT;
  const int64_t last = n - 1;
  uint8_t vl[FPT];
#pragma unroll
  for (int j = 0; j < FPT; j++) vl[j] = A.valid ? A.valid[b0 + j > last ? last : b0 + j] : uint8_t(1);
  bool adm[FPT];
#pragma unroll
  for (int j = 0; j < FPT; j++) adm[j] = b0 + j < n && vl[j];
  if (blockIdx.x == 0 && threadIdx.x == 0) *A.bad = 0;
  filter_emit(A, adm, b0, n, s_c);
}

// the tiles' counts scanned into their offsets; the batch's admitted count to the device word and, with
// the topic-range flag, to the pinned host words, stamped last
__global__ __launch_bounds__(256) void filter_offsets(FilterArgs A, int64_t nt) {
  __shared__ int64_t s_w[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int64_t carry = 0;
  for (int64_t base = 0; base < nt; base += 256) {
    const int64_t i = base + threadIdx.x;
    const int64_t c = A.tile_cnt[i < nt ? i : nt - 1];
    int64_t tot;
    const int64_t run = carry + block_scan_total<4>(i < nt ? c : 0, s_w, lane, wid, tot);
    if (i < nt) A.tile_off[i] = run;
    carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *A.n_dev = carry;
    A.host[0] = carry;
    A.host[1] = *A.bad;
    __threadfence_system();
    *reinterpret_cast<volatile int64_t*>(A.host + 2) = A.stamp;
  }
}

__device__ __forceinline__ void put_col(const void* src, void* dst, int type, int64_t from, int64_t to) {
  if (type == T_I32) static_cast<int32_t*>(dst)[to] = static_cast<const int32_t*>(src)[from];
  else static_cast<int64_t*>(dst)[to] = static_cast<const int64_t*>(src)[from];
}

// admitted record i -> tile offset + rank: every column, and its stream position (the batch's own:
// dropped records keep theirs)
__global__ __launch_bounds__(256) void filter_gather(FilterArgs A, int64_t n) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int64_t c = i < n ? i : n - 1;
  const uint16_t sl = A.slot[c];
  const int64_t off = A.tile_off[c / FILTER_TF];
  const int32_t k = A.key[c];
  const int32_t tp = A.topic ? A.topic[c] : 0;
  const int32_t pt = A.partition ? A.partition[c] : 0;
  const int64_t of = A.offset ? A.offset[c] : 0;
  const int64_t ts = A.ts ? A.ts[c] : 0;
  const int64_t ps = A.pos ? A.pos[c] : A.base + c;
  if (i >= n || sl == FS_DROPPED) return;
  const int64_t d = off + sl;
  A.o_key[d] = k;
  if (A.topic) A.o_topic[d] = tp;
  if (A.partition) A.o_partition[d] = pt;
  if (A.offset) A.o_offset[d] = of;
  if (A.ts) A.o_ts[d] = ts;
  A.o_pos[d] = ps;
  for (int q = 0; q < A.ncols; q++) put_col(A.cols[q], A.o_cols[q], A.coltype[q], i, d);
}

// the staged marks of the batch's keys into the table: the thread at a key's last record, one per key
__global__ __launch_bounds__(256) void filter_commit(FilterArgs A, int64_t n, int ntopics) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int64_t last = n - 1;
  const int32_t k = A.key[i < last ? i : last], k1 = A.key[i + 1 < last ? i + 1 : last];
  if (i >= n || !(i == last || k1 != k) || k < 0 || k >= A.max_keys) return;
  for (int t = 0; t < ntopics; t++) {
    const int64_t v = A.stage[int64_t(k) * FILTER_MAX_TOPICS + t];
    int64_t* m = A.marks + int64_t(k) * FILTER_MAX_TOPICS + t;
    if (v != FM_NONE && *m < v) *m = v;
  }
}

}  // namespace

// the batch (A's input columns, n > 0 records, key-grouped, on the device) -> its admitted records in A's
// output columns and their count in A.n_dev and A.host; A.tile_f: a word per tile, A.tile_v:
// FILTER_MAX_TOPICS per tile, A.tile_cnt / A.tile_off: one per tile, A.slot: FILTER_TF per tile
hipError_t filter_launch(const FilterArgs& A, int64_t n, hipStream_t st) {
  if (n <= 0) return hipErrorInvalidValue;
  const int64_t nt = (n + FILTER_TF - 1) / FILTER_TF;
  const dim3 grid(static_cast<unsigned>(nt)), wg(256);
  if (!A.use_marks) {
    hipLaunchKernelGGL(filter_valid, grid, wg, 0, st, A, n);
  } else if (A.topic) {
    hipLaunchKernelGGL(filter_tiles<FILTER_MAX_TOPICS>, grid, wg, 0, st, A, n);
    hipLaunchKernelGGL(filter_scan<FILTER_MAX_TOPICS>, dim3(1), wg, 0, st, A, nt);
    hipLaunchKernelGGL(filter_apply<FILTER_MAX_TOPICS>, grid, wg, 0, st, A, n);
  } else {                                         // no topic column: every record on topic 0
    hipLaunchKernelGGL(filter_tiles<1>, grid, wg, 0, st, A, n);
    hipLaunchKernelGGL(filter_scan<1>, dim3(1), wg, 0, st, A, nt);
    hipLaunchKernelGGL(filter_apply<1>, grid, wg, 0, st, A, n);
  }
  hipLaunchKernelGGL(filter_offsets, dim3(1), wg, 0, st, A, nt);
  hipLaunchKernelGGL(filter_gather, dim3(blocks256(n)), wg, 0, st, A, n);
  return hipGetLastError();
}

// the marks filter_launch staged for the same A and n, into the table
hipError_t filter_commit_launch(const FilterArgs& A, int64_t n, hipStream_t st) {
  if (n <= 0 || !A.use_marks) return hipSuccess;
  hipLaunchKernelGGL(filter_commit, dim3(blocks256(n)), dim3(256), 0, st, A, n, A.topic ? FILTER_MAX_TOPICS : 1);
  return hipGetLastError();
}

}  // namespace kcep
