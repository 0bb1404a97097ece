// follow.hip -- the follow path (CEP_PATH_FOLLOW): patterns of strict and skip-till-next stages of
// cardinality ONE / times(n) (compile.cpp analyse_follow), sessions without carry.
//
// Every run of such a pattern is one deterministic walk from its start record j0 (slot 0 holds at j0):
// a strict slot takes the key's next record or the walk dies, a skip-till-next slot takes the key's
// next record that satisfies it.  A completed walk is one match, emitted at its last record; matches
// come out by (last record, start).  Phases, each its own launch (no workgroup waits on another):
//   follow_bits   streaming: key + value column [+ topic], 8 B per record, the stage masks computed as
//                 the stencil kernels compute them; out: one bitmap per slot (bit p: record p satisfies
//                 the slot), one of key starts (key[p] != key[p - 1]), a second level over each (bit w:
//                 word w is not zero) and per tile the number of starts -- (K + 1) / 8 B per record
//   follow_count  a wave per word of slot 0's bitmap, a lane per set bit: walks, counts the completed
//   (scan)        exclusive_scan over the words' counts (scan.hip)
//   follow_write  the same walks again (the bitmaps of a flush-sized batch sit in L2): the completed
//                 ones compacted in start order as (end << 31) | start, the form runs_order / runs_sort
//                 (runs.hip) put into (end, start) order
//   follow_rows   a thread per ordered match walks once more and writes its K-int row, the finished
//                 batch of a stencil session without carry (stencil_post, cep_collect, cep_checksum)
// A strict hop is one bit test; a skip-till-next hop and the end of the start's key segment are a
// find-next-set-bit: the rest of the current word, then second-level words, then one first-level word,
// <= 2 + gap / 4096 word reads.
#include "stencil_kernel.h"

namespace kcep {

static_assert(FOLLOW_TILE == ST_TILE, "follow_bits takes the stencil kernels' tile: one chunk per thread");
static_assert(FOLLOW_TILE == 64 * 64, "a tile is 64 bitmap words: one second-level word");

typedef unsigned long long u64;

int64_t follow_tiles(int64_t n) { return (std::max<int64_t>(n, 1) + FOLLOW_TILE - 1) / FOLLOW_TILE; }

// ---- the bitmaps as the walks read them: plane s at s * wpl words (s = k: key starts), its second level at
// s * nt words; bits of records >= n are zero ----
struct FollowMaps {
  const u64* bits;
  const u64* sum;
  int64_t wpl;                    // words per plane: 64 per tile
  int64_t nt;                     // tiles: second-level words per plane
  int64_t n;
  int32_t k;
  uint32_t next;                  // bit s: slot s is skip-till-next
};

// the first set bit of the plane at or after `from` and before `limit` (<= n); none: a value >= limit
__device__ __forceinline__ int64_t next_set(const u64* __restrict__ plane, const u64* __restrict__ sum, int64_t from,
                                            int64_t limit) {
  if (from >= limit) return limit;
  int64_t w = from >> 6;
  const u64 x = plane[w] & (~0ull << (from & 63));
  if (x) return w * 64 + __builtin_ctzll(x);
  int64_t sw = w >> 6;
  const int b = int(w & 63);
  u64 sx = b == 63 ? 0ull : sum[sw] & (~0ull << (b + 1));
  while (!sx) {                                    // (sw * 4096 < limit <= n: sw is a tile of the batch)
    sw++;
    if ((sw << 12) >= limit) return limit;
    sx = sum[sw];
  }
  w = sw * 64 + __builtin_ctzll(sx);
  return w * 64 + __builtin_ctzll(plane[w]);       // (not zero: its second-level bit is set)
}

// the walk from start j0: its last record, or -1 if it dies or does not complete in the batch; row: its
// records, slot by slot (or null)
__device__ __forceinline__ int64_t follow_walk(const FollowMaps& M, int64_t j0, int32_t* __restrict__ row) {
  const int64_t E = next_set(M.bits + M.k * M.wpl, M.sum + M.k * M.nt, j0 + 1, M.n);   // the key segment's end
  const int64_t end = E < M.n ? E : M.n;
  int64_t p = j0;
  if (row) row[0] = int32_t(j0);
  for (int s = 1; s < M.k; s++) {
    const u64* plane = M.bits + s * M.wpl;
    p++;
    if (M.next >> s & 1) {
      p = next_set(plane, M.sum + s * M.nt, p, end);
      if (p >= end) return -1;
    } else if (p >= end || !(plane[p >> 6] >> (p & 63) & 1)) {
      return -1;
    }
    if (row) row[s] = int32_t(p);
  }
  return p;
}

// ---- follow_bits: one tile per workgroup ----
template <class VT, bool TOPIC>
__global__ __launch_bounds__(ST_THREADS) void follow_bits(const int32_t* __restrict__ key, const VT* __restrict__ val,
                                                         const int32_t* __restrict__ topic, int64_t n,
                                                         const StencilProgram* __restrict__ P, int k,
                                                         u64* __restrict__ bits, u64* __restrict__ sum, int64_t wpl,
                                                         int64_t nt, int64_t* __restrict__ tile_starts) {
  __shared__ __attribute__((aligned(16))) uint8_t s_mask[ST_TILE];   // the records' stage masks
  __shared__ __attribute__((aligned(16))) uint8_t s_ks[ST_TILE];     // 1: the record starts a key segment
  __shared__ MaskTables<VT> s_mt;
  __shared__ uint32_t s_part[STENCIL_MAX_K + 1][ST_THREADS / 64];    // per plane and wave: its 16 words' not-zero bits
  __shared__ int32_t s_cnt[ST_THREADS / 64];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  load_tables<VT>(s_mt, P, tid);
  const MaskUni<VT> U = load_uni<VT>(P);
  const int64_t tile = blockIdx.x;
  const int64_t base = tile * ST_TILE;

  Chunk<VT, TOPIC> cur;
  load_chunk<VT, TOPIC>(cur, key, val, topic, base, n, tid);
  // the record before each wave's first, per vector: the lane before has it, lane 0 reads it
  int32_t before[ST_EPT / 4];
#pragma unroll
  for (int q = 0; q < ST_EPT / 4; q++) {
    const int64_t g = base + q * (ST_THREADS * 4) + tid * 4;
    before[q] = 0;
    if (lane == 0 && g > 0 && g < n) before[q] = key[g - 1];
  }
  __syncthreads();                                // the tables
  uint32_t packed[4];
  masks_of_chunk<VT, TOPIC>(cur, P, s_mt, U, packed);
#pragma unroll
  for (int q = 0; q < ST_EPT / 4; q++) {
    const int local = q * (ST_THREADS * 4) + tid * 4;
    const int64_t g = base + local;
    const v4i kv = cur.k[q];
    int32_t kp = __shfl_up(kv[3], 1);
    if (lane == 0) kp = before[q];
    uint32_t ks = uint32_t(g == 0 || kp != kv[0]) | (uint32_t(kv[1] != kv[0]) << 8) | (uint32_t(kv[2] != kv[1]) << 16) |
                  (uint32_t(kv[3] != kv[2]) << 24);
    uint32_t w = packed[q];
    const int64_t left = n - g;                   // records >= n: zero bits
    if (left < 4) {
      const uint32_t keep = left <= 0 ? 0u : (0xFFFFFFFFu >> (8 * (4 - left)));
      w &= keep;
      ks &= keep;
    }
    *reinterpret_cast<uint32_t*>(&s_mask[local]) = w;
    *reinterpret_cast<uint32_t*>(&s_ks[local]) = ks;
  }
  __syncthreads();
  // bytes to bitmap words: wave wid has the tile's words 16 wid .. 16 wid + 15, a ballot per word and plane;
  // lane i keeps word i's, so that lanes 0..15 store each plane's 16 words as one 128-B run
  u64 mine[STENCIL_MAX_K + 1];
#pragma unroll
  for (int s = 0; s <= STENCIL_MAX_K; s++) mine[s] = 0;
  for (int i = 0; i < 16; i++) {
    const int r = (wid * 16 + i) * 64 + lane;
    const uint32_t m = s_mask[r];
    const u64 bk = __ballot(s_ks[r] != 0);
    if (lane == i) mine[STENCIL_MAX_K] = bk;
#pragma unroll
    for (int s = 0; s < STENCIL_MAX_K; s++) {
      if (s < k) {                                // uniform
        const u64 bs = __ballot((m >> s & 1) != 0);
        if (lane == i) mine[s] = bs;
      }
    }
  }
  const int64_t w0 = tile * 64 + wid * 16 + lane;
#pragma unroll
  for (int s = 0; s <= STENCIL_MAX_K; s++) {
    const int plane = s == STENCIL_MAX_K ? k : s;  // (the key starts' plane comes after the slots')
    if (s < k || s == STENCIL_MAX_K) {             // uniform
      if (lane < 16) bits[plane * wpl + w0] = mine[s];
      const u64 nz = __ballot(lane < 16 && mine[s] != 0);
      if (lane == 0) s_part[plane][wid] = uint32_t(nz);
    }
  }
  int c0 = lane < 16 ? __popcll(mine[0]) : 0;      // the tile's starts
#pragma unroll
  for (int d = 8; d >= 1; d >>= 1) c0 += __shfl_xor(c0, d);
  if (lane == 0) s_cnt[wid] = c0;
  __syncthreads();
  if (tid <= k) {
    const u64 sw = u64(s_part[tid][0]) | (u64(s_part[tid][1]) << 16) | (u64(s_part[tid][2]) << 32) |
                   (u64(s_part[tid][3]) << 48);
    sum[tid * nt + tile] = sw;
  }
  if (tid == 0) tile_starts[tile] = int64_t(s_cnt[0]) + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// ---- follow_count / follow_write: a workgroup per tile, each wave 16 words of slot 0's bitmap ----
template <bool WRITE>
__global__ __launch_bounds__(256) void follow_walks(FollowMaps M, const int64_t* __restrict__ tile_starts,
                                                   int64_t* __restrict__ wcnt, const int64_t* __restrict__ wpre,
                                                   u64* __restrict__ keys, u64* __restrict__ max_span) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t tile = blockIdx.x;
  if (tile_starts[tile] == 0) {                    // uniform
    if (!WRITE && threadIdx.x < 64) wcnt[tile * 64 + threadIdx.x] = 0;
    return;
  }
  int64_t span = 0;
  for (int i = 0; i < 16; i++) {
    const int64_t w = tile * 64 + wid * 16 + i;
    if (WRITE && wcnt[w] == 0) continue;           // uniform per wave
    const u64 x = M.bits[w];
    if (x == 0) {
      if (!WRITE && lane == 0) wcnt[w] = 0;
      continue;
    }
    const int64_t j0 = w * 64 + lane;
    int64_t e = -1;
    if (x >> lane & 1) e = follow_walk(M, j0, nullptr);
    const u64 done = __ballot(e >= 0);
    if (WRITE) {
      if (e >= 0) keys[wpre[w] + __popcll(done & ((1ull << lane) - 1))] = (u64(e) << 31) | u64(j0);
    } else {
      if (lane == 0) wcnt[w] = __popcll(done);
      if (e >= 0 && e - j0 > span) span = e - j0;
    }
  }
  if (!WRITE) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const int64_t o = __shfl_xor(span, d);
      span = o > span ? o : span;
    }
    // (one address for the whole grid: only a wave that would raise the value it sees sends its atomic)
    if (lane == 0 && u64(span) > *static_cast<volatile u64*>(max_span)) atomicMax(max_span, u64(span));
  }
}

// ---- follow_rows: the ordered matches' rows ----
__global__ __launch_bounds__(256) void follow_rows(FollowMaps M, const u64* __restrict__ sorted, int64_t nm,
                                                  int32_t* __restrict__ out, int64_t* __restrict__ total) {
  const int64_t m = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (m == 0) *total = nm;
  if (m >= nm) return;
  (void)follow_walk(M, int64_t(sorted[m] & 0x7FFFFFFFull), out + m * M.k);
}

static FollowMaps follow_maps(const FollowArgs& A) {
  const int64_t nt = follow_tiles(A.n);
  return FollowMaps{A.bits, A.sum, nt * 64, nt, A.n, A.k, A.next_mask};
}

template <class VT>
static void bits_launch(const FollowArgs& A, hipStream_t st) {
  const int64_t nt = follow_tiles(A.n);
  if (A.use_topic)
    hipLaunchKernelGGL((follow_bits<VT, true>), dim3(unsigned(nt)), dim3(ST_THREADS), 0, st, A.key,
                       static_cast<const VT*>(A.val), A.topic, A.n, A.prog_dev, A.k, A.bits, A.sum, nt * 64, nt,
                       A.tile_starts);
  else
    hipLaunchKernelGGL((follow_bits<VT, false>), dim3(unsigned(nt)), dim3(ST_THREADS), 0, st, A.key,
                       static_cast<const VT*>(A.val), A.topic, A.n, A.prog_dev, A.k, A.bits, A.sum, nt * 64, nt,
                       A.tile_starts);
}

hipError_t follow_bits_launch(const FollowArgs& A, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st) {
  if (A.n <= 0 || A.k < 2 || A.k > STENCIL_MAX_K) return hipErrorInvalidValue;
  if (ev0) (void)hipEventRecord(ev0, st);
  if (A.coltype == T_I32) bits_launch<int32_t>(A, st);
  else if (A.coltype == T_I64) bits_launch<int64_t>(A, st);
  else bits_launch<double>(A, st);
  if (ev1) (void)hipEventRecord(ev1, st);
  return hipGetLastError();
}

// the completed walks counted per word of slot 0's bitmap, the counts' prefix, their number (*nm) and
// the longest span (*max_span)
hipError_t follow_count_launch(const FollowArgs& A, hipStream_t st) {
  const int64_t nt = follow_tiles(A.n);
  hipError_t e = hipMemsetAsync(A.max_span, 0, 8, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(follow_walks<false>, dim3(unsigned(nt)), dim3(256), 0, st, follow_maps(A), A.tile_starts, A.wcnt,
                     A.wpre, A.keys, A.max_span);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return exclusive_scan(A.wcnt, nt * 64, A.wpre, A.nm, A.scan_tmp, st);
}

hipError_t follow_write_launch(const FollowArgs& A, hipStream_t st) {
  hipLaunchKernelGGL(follow_walks<true>, dim3(unsigned(follow_tiles(A.n))), dim3(256), 0, st, follow_maps(A),
                     A.tile_starts, A.wcnt, A.wpre, A.keys, A.max_span);
  return hipGetLastError();
}

hipError_t follow_rows_launch(const FollowArgs& A, const unsigned long long* sorted, int64_t nm, int32_t* out,
                              int64_t* total, hipStream_t st) {
  hipLaunchKernelGGL(follow_rows, dim3(blocks256(nm)), dim3(256), 0, st, follow_maps(A), sorted, nm, out, total);
  return hipGetLastError();
}

}  // namespace kcep
