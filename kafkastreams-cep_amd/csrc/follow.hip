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
//   follow_eval_bits  the same planes where the predicates read several columns, arithmetic or metadata
//                 (the evaluated form, follow_bits_dev.h): the key and the columns they read, each slot
//                 evaluated per record; interpreted here, compiled per pattern by jit.cpp
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
// With oneOrMore stages (CEP_SESSION_FOLLOW_MANY, compile.cpp analyse_follow_many; sessions without carry) a
// match has a variable length: follow_many_walks count and write, follow_many_len and follow_many_rows leave
// the runs path's CSR instead of rows ("oneOrMore slots" below).
#include "follow_bits_dev.h"
#include "stencil_kernel.h"

namespace kcep {

static_assert(FOLLOW_TILE == ST_TILE, "follow_bits takes the stencil kernels' tile: one chunk per thread");
static_assert(FOLLOW_TILE == 64 * 64, "a tile is 64 bitmap words: one second-level word");
static_assert(FB_TILE == FOLLOW_TILE && FB_THREADS == ST_THREADS && FB_MAX_K == STENCIL_MAX_K,
              "follow_bits_dev.h's tile is follow_bits' tile");

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
  const int64_t* pos;             // carry sessions: the records' stream positions (null: base + index)
  int64_t base;
};

__device__ __forceinline__ int64_t pos_of(const FollowMaps& M, int64_t i) { return M.pos ? M.pos[i] : M.base + i; }

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

// A walk that does not complete either dies (a strict hop lands on a record of the key that does not
// satisfy the slot) or stays open (a hop reaches the end of the key's segment: on a carry session it
// goes on in the key's next batch); without carry both mean "no match".
constexpr int64_t FW_DEAD = -1, FW_OPEN = -2;

// a walk continued at slot s0 from record p (a strict slot tests p, a skip-till-next slot searches from
// p) within the key segment ending at `end`: its last record, FW_DEAD, or FW_OPEN with *reached = the
// slots taken.  row: the records taken, by slot (or null); prow: their stream positions, slot s at
// prow[s * pstride] (or null)
__device__ __forceinline__ int64_t follow_steps(const FollowMaps& M, int64_t p, int s0, int64_t end,
                                                int32_t* __restrict__ row, int64_t* __restrict__ prow, int pstride,
                                                int* reached) {
  int64_t last = p - 1;
  for (int s = s0; s < M.k; s++) {
    const u64* plane = M.bits + s * M.wpl;
    const bool next = M.next >> s & 1;
    if (next) p = next_set(plane, M.sum + s * M.nt, p, end);
    if (p >= end) {
      if (reached) *reached = s;
      return FW_OPEN;
    }
    if (!next && !(plane[p >> 6] >> (p & 63) & 1)) return FW_DEAD;
    if (row) row[s] = int32_t(p);
    if (prow) prow[s * pstride] = pos_of(M, p);
    last = p++;
  }
  return last;
}

// the end of the key segment that holds record j
__device__ __forceinline__ int64_t segment_end(const FollowMaps& M, int64_t j) {
  const int64_t E = next_set(M.bits + M.k * M.wpl, M.sum + M.k * M.nt, j + 1, M.n);
  return E < M.n ? E : M.n;
}

// the walk from start j0: its last record, or FW_DEAD / FW_OPEN (both < 0)
__device__ __forceinline__ int64_t follow_walk_open(const FollowMaps& M, int64_t j0) {
  return follow_steps(M, j0 + 1, 1, segment_end(M, j0), nullptr, nullptr, 0, nullptr);
}

// ... as the sessions without carry walk it, where dead and open are both "no match" (-1): the loop those
// kernels have always run, kept apart from follow_steps so that their code does not move with it; row: its
// records, slot by slot (or null)
__device__ __forceinline__ int64_t follow_walk(const FollowMaps& M, int64_t j0, int32_t* __restrict__ row) {
  const int64_t end = segment_end(M, j0);
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

// ---- follow_eval_bits: the evaluated form's streaming kernel (follow_bits_dev.h), the slots interpreted;
// jit.cpp compiles the same body per pattern (kcep_follow_bits) ----
__global__ __launch_bounds__(FB_THREADS) void follow_eval_bits(MaskArgs A, int k, u64* __restrict__ bits,
                                                              u64* __restrict__ sum, int64_t wpl, int64_t nt,
                                                              int64_t* __restrict__ tile_starts) {
  follow_eval_bits_body(FollowInterpTab{{A.P}}, A, k, bits, sum, wpl, nt, tile_starts);
}

// ---- follow_count / follow_write: a workgroup per tile, each wave 16 words of slot 0's bitmap ----
// CARRY (count pass of a carry session): also the starts whose walk is open at the batch end, as a bitmap
// plane (open) and per word a count (wopen)
template <bool WRITE, bool CARRY>
__global__ __launch_bounds__(256) void follow_walks(FollowMaps M, const int64_t* __restrict__ tile_starts,
                                                   int64_t* __restrict__ wcnt, const int64_t* __restrict__ wpre,
                                                   u64* __restrict__ keys, u64* __restrict__ max_span,
                                                   u64* __restrict__ open, int64_t* __restrict__ wopen) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t tile = blockIdx.x;
  if (tile_starts[tile] == 0) {                    // uniform
    if (!WRITE && threadIdx.x < 64) {
      wcnt[tile * 64 + threadIdx.x] = 0;
      if (CARRY) {
        wopen[tile * 64 + threadIdx.x] = 0;
        open[tile * 64 + threadIdx.x] = 0;
      }
    }
    return;
  }
  int64_t span = 0;
  for (int i = 0; i < 16; i++) {
    const int64_t w = tile * 64 + wid * 16 + i;
    if (WRITE && wcnt[w] == 0) continue;           // uniform per wave
    const u64 x = M.bits[w];
    if (x == 0) {
      if (!WRITE && lane == 0) {
        wcnt[w] = 0;
        if (CARRY) {
          wopen[w] = 0;
          open[w] = 0;
        }
      }
      continue;
    }
    const int64_t j0 = w * 64 + lane;
    int64_t e = FW_DEAD;
    if (x >> lane & 1) e = CARRY ? follow_walk_open(M, j0) : follow_walk(M, j0, nullptr);
    const u64 done = __ballot(e >= 0);
    if (WRITE) {
      if (e >= 0) keys[wpre[w] + __popcll(done & ((1ull << lane) - 1))] = (u64(e) << 31) | u64(j0);
    } else {
      if (lane == 0) wcnt[w] = __popcll(done);
      if (e >= 0 && e - j0 > span) span = e - j0;
      if (CARRY) {
        const u64 op = __ballot(e == FW_OPEN);
        if (lane == 0) {
          open[w] = op;
          wopen[w] = __popcll(op);
        }
      }
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
  return FollowMaps{A.bits, A.sum, nt * 64, nt, A.n, A.k, A.next_mask, A.pos, A.base};
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

// the evaluated form: M the columns the slots read (push.cpp), A the planes; jf: the per-pattern kernel, or null
hipError_t follow_eval_bits_launch(const MaskArgs& M, const FollowArgs& A, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st,
                                   hipFunction_t jf) {
  if (A.n <= 0 || M.n != A.n || A.k < 2 || A.k > STENCIL_MAX_K) return hipErrorInvalidValue;
  const int64_t nt = follow_tiles(A.n);
  if (ev0) (void)hipEventRecord(ev0, st);
  hipError_t e = hipSuccess;
  if (jf) {
    MaskArgs m = M;
    int k = A.k;
    u64 *bits = A.bits, *sum = A.sum;
    int64_t wpl = nt * 64, ntv = nt;
    int64_t* ts = A.tile_starts;
    void* args[] = {&m, &k, &bits, &sum, &wpl, &ntv, &ts};
    e = hipModuleLaunchKernel(jf, unsigned(nt), 1, 1, FB_THREADS, 1, 1, 0, st, args, nullptr);
  } else {
    hipLaunchKernelGGL(follow_eval_bits, dim3(unsigned(nt)), dim3(FB_THREADS), 0, st, M, A.k, A.bits, A.sum, nt * 64, nt,
                       A.tile_starts);
    e = hipGetLastError();
  }
  if (ev1) (void)hipEventRecord(ev1, st);
  return e;
}

// the completed walks counted per word of slot 0's bitmap, the counts' prefix, their number (*nm) and
// the longest span (*max_span)
hipError_t follow_count_launch(const FollowArgs& A, hipStream_t st) {
  const int64_t nt = follow_tiles(A.n);
  hipError_t e = hipMemsetAsync(A.max_span, 0, 8, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((follow_walks<false, false>), dim3(unsigned(nt)), dim3(256), 0, st, follow_maps(A), A.tile_starts,
                     A.wcnt, A.wpre, A.keys, A.max_span, nullptr, nullptr);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return exclusive_scan(A.wcnt, nt * 64, A.wpre, A.nm, A.scan_tmp, st);
}

hipError_t follow_write_launch(const FollowArgs& A, hipStream_t st) {
  hipLaunchKernelGGL((follow_walks<true, false>), dim3(unsigned(follow_tiles(A.n))), dim3(256), 0, st, follow_maps(A),
                     A.tile_starts, A.wcnt, A.wpre, A.keys, A.max_span, nullptr, nullptr);
  return hipGetLastError();
}

hipError_t follow_rows_launch(const FollowArgs& A, const unsigned long long* sorted, int64_t nm, int32_t* out,
                              int64_t* total, hipStream_t st) {
  hipLaunchKernelGGL(follow_rows, dim3(blocks256(nm)), dim3(256), 0, st, follow_maps(A), sorted, nm, out, total);
  return hipGetLastError();
}

// ---- oneOrMore slots (CEP_SESSION_FOLLOW_MANY): variable-length matches ----
// A oneOrMore stage is one slot flagged many (compile.cpp analyse_follow_many): its predicate excludes its
// successor's.  The hop out of a many slot B at record r into slot s scans the key's records after r: a B
// record is collected, the first slot-s record is taken, a record that is neither is skipped if B or s is
// skip-till-next and kills the walk if both are strict.  So the mixed hop is the find-next-set on plane s
// the other hops take, and the strict / strict hop a find-next-zero on plane B (word by word over inverted
// words: a second level says nothing about all-ones words) with one bit test on plane s.  The collected
// records are the set bits of plane B strictly between the two records: a match's length is K plus their
// popcounts, and its rows enumerate them from the plane's words.  The walk is a loop of its own, so that the
// kernels above keep their code.
namespace {

struct FollowManyMaps {
  FollowMaps M;
  uint32_t many;                  // bit s: slot s is a oneOrMore stage
};

// the first zero bit of the plane at or after `from` and before `limit` (<= n); none: limit
__device__ __forceinline__ int64_t next_zero(const u64* __restrict__ plane, int64_t from, int64_t limit) {
  if (from >= limit) return limit;
  int64_t w = from >> 6;
  const int64_t wl = (limit - 1) >> 6;             // (the last word read: limit <= n, inside the plane)
  u64 x = ~plane[w] & (~0ull << (from & 63));
  while (!x) {
    if (++w > wl) return limit;
    x = ~plane[w];
  }
  const int64_t q = w * 64 + __builtin_ctzll(x);
  return q < limit ? q : limit;
}

// the set bits of the plane in [lo, hi), hi <= n; tiles without a set bit are passed by their second-level word
__device__ __forceinline__ int64_t count_set(const u64* __restrict__ plane, const u64* __restrict__ sum, int64_t lo,
                                             int64_t hi) {
  if (lo >= hi) return 0;
  const int64_t w0 = lo >> 6, w1 = (hi - 1) >> 6;
  const u64 m0 = ~0ull << (lo & 63), m1 = ~0ull >> (63 - ((hi - 1) & 63));
  if (w0 == w1) return __popcll(plane[w0] & m0 & m1);
  int64_t c = __popcll(plane[w0] & m0) + __popcll(plane[w1] & m1);
  for (int64_t w = w0 + 1; w < w1;) {
    if ((w & 63) == 0 && w + 64 <= w1 && sum[w >> 6] == 0) {
      w += 64;
      continue;
    }
    c += __popcll(plane[w]);
    w++;
  }
  return c;
}

// the hop out of many slot s - 1 at record p into slot s within the key segment ending at `end`: the record
// taken, or -1 (the walk dies, or reaches the segment's end)
__device__ __forceinline__ int64_t many_hop(const FollowMaps& M, int s, int64_t p, int64_t end) {
  const u64* plane = M.bits + s * M.wpl;
  if ((M.next >> s | M.next >> (s - 1)) & 1) {
    const int64_t q = next_set(plane, M.sum + s * M.nt, p + 1, end);
    return q < end ? q : -1;
  }
  const int64_t q = next_zero(M.bits + (s - 1) * M.wpl, p + 1, end);
  return q < end && (plane[q >> 6] >> (q & 63) & 1) ? q : -1;
}

// the walk from start j0: its last record or -1; *len (or null): its entries, K + the collected records
__device__ __forceinline__ int64_t many_walk(const FollowManyMaps& F, int64_t j0, int64_t* len) {
  const FollowMaps& M = F.M;
  const int64_t end = segment_end(M, j0);
  int64_t p = j0, L = M.k;
  for (int s = 1; s < M.k; s++) {
    const u64* plane = M.bits + s * M.wpl;
    if (F.many >> (s - 1) & 1) {
      const int64_t q = many_hop(M, s, p, end);
      if (q < 0) return -1;
      if (len) {
        const bool both_strict = !((M.next >> s | M.next >> (s - 1)) & 1);   // (then every record between is one)
        L += both_strict ? q - p - 1 : count_set(M.bits + (s - 1) * M.wpl, M.sum + (s - 1) * M.nt, p + 1, q);
      }
      p = q;
      continue;
    }
    p++;
    if (M.next >> s & 1) {
      p = next_set(plane, M.sum + s * M.nt, p, end);
      if (p >= end) return -1;
    } else if (p >= end || !(plane[p >> 6] >> (p & 63) & 1)) {
      return -1;
    }
  }
  if (len) *len = L;
  return p;
}

// follow_walks for such a pattern; the count pass also sums the completed walks' lengths per word (wlen)
template <bool WRITE>
__global__ __launch_bounds__(256) void follow_many_walks(FollowManyMaps F, const int64_t* __restrict__ tile_starts,
                                                        int64_t* __restrict__ wcnt, int64_t* __restrict__ wlen,
                                                        const int64_t* __restrict__ wpre, u64* __restrict__ keys,
                                                        u64* __restrict__ max_span) {
  const FollowMaps& M = F.M;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t tile = blockIdx.x;
  if (tile_starts[tile] == 0) {                    // uniform
    if (!WRITE && threadIdx.x < 64) {
      wcnt[tile * 64 + threadIdx.x] = 0;
      wlen[tile * 64 + threadIdx.x] = 0;
    }
    return;
  }
  int64_t span = 0;
  for (int i = 0; i < 16; i++) {
    const int64_t w = tile * 64 + wid * 16 + i;
    if (WRITE && wcnt[w] == 0) continue;           // uniform per wave
    const u64 x = M.bits[w];
    if (x == 0) {
      if (!WRITE && lane == 0) {
        wcnt[w] = 0;
        wlen[w] = 0;
      }
      continue;
    }
    const int64_t j0 = w * 64 + lane;
    int64_t e = -1, len = 0;
    if (x >> lane & 1) e = many_walk(F, j0, WRITE ? nullptr : &len);
    const u64 done = __ballot(e >= 0);
    if (WRITE) {
      if (e >= 0) keys[wpre[w] + __popcll(done & ((1ull << lane) - 1))] = (u64(e) << 31) | u64(j0);
    } else {
      if (e < 0) len = 0;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) len += __shfl_xor(len, d);
      if (lane == 0) {
        wcnt[w] = __popcll(done);
        wlen[w] = len;
      }
      if (e >= 0 && e - j0 > span) span = e - j0;
    }
  }
  if (!WRITE) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const int64_t o = __shfl_xor(span, d);
      span = o > span ? o : span;
    }
    if (lane == 0 && u64(span) > *static_cast<volatile u64*>(max_span)) atomicMax(max_span, u64(span));
  }
}

// the ordered matches' lengths
__global__ __launch_bounds__(256) void follow_many_len(FollowManyMaps F, const u64* __restrict__ sorted, int64_t nm,
                                                      int64_t* __restrict__ len) {
  const int64_t m = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (m >= nm) return;
  int64_t L = 0;
  const int64_t e = many_walk(F, int64_t(sorted[m] & 0x7FFFFFFFull), &L);
  len[m] = e >= 0 ? L : 0;
}

// The CSR of the ordered matches, a lane per match: batch indices, entries final slot first, a many slot's
// collected records (descending) before the slot's own.  The walk runs forward, so its f-th record goes to
// entry off + L - 1 - f; a store past the length the scan was given is dropped.
__global__ __launch_bounds__(256) void follow_many_rows(FollowManyMaps F, const int32_t* __restrict__ key,
                                                       const StencilProgram* __restrict__ P,
                                                       const u64* __restrict__ sorted, int64_t nm,
                                                       const int64_t* __restrict__ len, int64_t* __restrict__ match_record,
                                                       int32_t* __restrict__ match_key, const int64_t* __restrict__ ent_off,
                                                       int32_t* __restrict__ ent_name, int64_t* __restrict__ ent_record,
                                                       int64_t* __restrict__ total) {
  const int64_t m = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (m == 0) *total = nm;
  if (m >= nm) return;
  const FollowMaps& M = F.M;
  const u64 v = sorted[m];
  const int64_t j0 = int64_t(v & 0x7FFFFFFFull);
  const int64_t L = len[m], top = ent_off[m] + L - 1;
  const int64_t end = segment_end(M, j0);
  match_record[m] = int64_t(v >> 31);
  match_key[m] = key[j0];
  int64_t f = 0, p = j0;
  auto put = [&](int s, int64_t r) {
    if (f < L) {
      ent_record[top - f] = r;
      ent_name[top - f] = P->name[s];
    }
    f++;
  };
  put(0, j0);
  for (int s = 1; s < M.k; s++) {
    const u64* plane = M.bits + s * M.wpl;
    if (F.many >> (s - 1) & 1) {
      const int64_t q = many_hop(M, s, p, end);
      if (q < 0) return;                           // (not a completed walk: never among the sorted)
      // the collected records: the set bits of plane s - 1 in (p, q), ascending
      const u64* prev = M.bits + (s - 1) * M.wpl;
      const u64* psum = M.sum + (s - 1) * M.nt;
      if (p + 1 < q) {
        const int64_t w0 = (p + 1) >> 6, w1 = (q - 1) >> 6;
        for (int64_t w = w0; w <= w1;) {
          if (w > w0 && (w & 63) == 0 && w + 64 <= w1 && psum[w >> 6] == 0) {
            w += 64;
            continue;
          }
          u64 x = prev[w];
          if (w == w0) x &= ~0ull << ((p + 1) & 63);
          if (w == w1) x &= ~0ull >> (63 - ((q - 1) & 63));
          while (x) {
            put(s - 1, w * 64 + __builtin_ctzll(x));
            x &= x - 1;
          }
          w++;
        }
      }
      p = q;
    } else {
      p++;
      if (M.next >> s & 1) {
        p = next_set(plane, M.sum + s * M.nt, p, end);
        if (p >= end) return;
      } else if (p >= end || !(plane[p >> 6] >> (p & 63) & 1)) {
        return;
      }
    }
    put(s, p);
  }
}

}  // namespace

hipError_t follow_many_count_launch(const FollowArgs& A, hipStream_t st) {
  const int64_t nt = follow_tiles(A.n);
  hipError_t e = hipMemsetAsync(A.max_span, 0, 8, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((follow_many_walks<false>), dim3(unsigned(nt)), dim3(256), 0, st,
                     FollowManyMaps{follow_maps(A), A.many_mask}, A.tile_starts, A.wcnt, A.wlen, A.wpre, A.keys, A.max_span);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return exclusive_scan_pair(A.wcnt, A.wlen, nt * 64, nullptr, A.wpre, A.wlpre, A.nm, A.ne, A.scan_tmp, st);
}

hipError_t follow_many_write_launch(const FollowArgs& A, hipStream_t st) {
  hipLaunchKernelGGL((follow_many_walks<true>), dim3(unsigned(follow_tiles(A.n))), dim3(256), 0, st,
                     FollowManyMaps{follow_maps(A), A.many_mask}, A.tile_starts, A.wcnt, A.wlen, A.wpre, A.keys, A.max_span);
  return hipGetLastError();
}

hipError_t follow_many_rows_launch(const FollowArgs& A, const unsigned long long* sorted, int64_t nm, int64_t* len,
                                   int64_t* len_total, int64_t* match_record, int32_t* match_key, int64_t* ent_off,
                                   int32_t* ent_name, int64_t* ent_record, int64_t* total, hipStream_t st) {
  const FollowManyMaps F{follow_maps(A), A.many_mask};
  if (nm > 0) {
    hipLaunchKernelGGL(follow_many_len, dim3(blocks256(nm)), dim3(256), 0, st, F, sorted, nm, len);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = exclusive_scan(len, nm, ent_off, len_total, A.scan_tmp, st)) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(follow_many_rows, dim3(blocks256(nm)), dim3(256), 0, st, F, A.key, A.prog_dev, sorted, nm, len,
                     match_record, match_key, ent_off, ent_name, ent_record, total);
  return hipGetLastError();
}

// ---- carry sessions (CEP_SESSION_FOLLOW_CARRY): carried walks ----
// A walk open at the end of a batch waits for its key's next records: it is carried as k int64 words (slots
// taken s, the stream positions of its s records, zeros), a key's walks contiguous in ascending start
// (launch.h FollowCarry).  Every waiting walk of a key at slot s takes the same records of the key's next
// segment, so a batch continues its keys' walks once per (segment, slot) -- follow_resume, k - 1 lanes per
// segment however many walks wait -- and each carried walk is a table lookup and a copy.  Matches come out
// by (completing record, start): carried walks start before every in-batch start of their key and equal
// completing records imply one key, so the sort input is the completed carried walks in (segment, list)
// order, marked above the sorted bits, then the in-batch ones in start order, and the sort is stable.
// A key's new list: its surviving carried walks in order, then its open in-batch walks in start order,
// appended at *rtop; placement is ordered (prefixes and ranks), no atomics.
namespace {

constexpr int32_t FR_DEAD = 0, FR_DONE = 1, FR_OPEN = 2;   // a continuation's outcome (open: | slots reached << 8)
constexpr u64 FC_MARK = 1ull << 63;                        // a sort key of a carried walk: its low bits number it

// the in-batch starts with an open walk before record j
struct OpenRank {
  const u64* open;
  const int64_t* wopre;
  const int64_t* nopen;
  int64_t n;
};
__device__ __forceinline__ int64_t open_rank(const OpenRank& R, int64_t j) {
  if (j >= R.n) return *R.nopen;
  return R.wopre[j >> 6] + __popcll(R.open[j >> 6] & ((1ull << (j & 63)) - 1));
}
// the carried walks that stay open among the first x of the enumeration
__device__ __forceinline__ int64_t open_before(const FollowCarry& C, int64_t x) {
  return x < *C.ncw && x < C.bound ? C.cw_opre[x] : *C.nco;
}
// the segment of the enumeration's x-th carried walk: the last whose walks start at or before x
__device__ __forceinline__ int64_t walk_segment(const FollowCarry& C, int64_t x) {
  int64_t lo = 0, hi = *C.nseg - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (C.toff[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ const int64_t* walk_words(const FollowCarry& C, const int32_t* __restrict__ key, int k,
                                                     int64_t sg, int64_t x, int32_t* kk) {
  *kk = key[C.seg_start[sg]];
  return C.rpool + (C.rtab[2 * int64_t(*kk)] + (x - C.toff[sg])) * k;
}

// one lane per (segment whose key has walks, slot 1..k-1): the walk continued from the segment's first record
__global__ __launch_bounds__(256) void follow_resume(FollowMaps M, FollowCarry C, int64_t items) {
  const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (t >= items) return;
  const int km1 = M.k - 1;
  const int64_t sg = t / km1;
  const int s = 1 + int(t % km1);
  if (sg >= *C.nseg || C.tlen[sg] == 0) return;
  int32_t* row = C.res + t * M.k;
  int reached = s;
  const int64_t e = follow_steps(M, C.seg_start[sg], s, C.seg_start[sg + 1], row, nullptr, 0, &reached);
  row[0] = e >= 0 ? FR_DONE : e == FW_OPEN ? (FR_OPEN | reached << 8) : FR_DEAD;
}

// per carried walk of the batch's keys: completed / still open (dead: neither)
__global__ __launch_bounds__(256) void follow_classify(FollowCarry C, const int32_t* __restrict__ key, int k) {
  const int64_t x = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (x >= C.bound || x >= *C.ncw) return;
  const int64_t sg = walk_segment(C, x);
  int32_t st = FR_DEAD;
  if (sg < C.nseg_cap) {                           // (past it: a batch the key check rejects)
    int32_t kk;
    const int64_t s = walk_words(C, key, k, sg, x, &kk)[0];
    if (s >= 1 && s < k) st = C.res[(sg * (k - 1) + s - 1) * k] & 3;
  }
  C.cw_done[x] = st == FR_DONE;
  C.cw_open[x] = st == FR_OPEN;
}

// the completed carried walks' sort keys; the surviving ones, extended by the records taken, into the pool
__global__ __launch_bounds__(256) void follow_carried_out(FollowMaps M, FollowCarry C, OpenRank R,
                                                         const int32_t* __restrict__ key, u64* __restrict__ keys) {
  const int64_t x = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (x >= C.bound || x >= *C.ncw) return;
  const bool done = C.cw_done[x] != 0, open = C.cw_open[x] != 0;
  if (!done && !open) return;
  const int k = M.k;
  const int64_t sg = walk_segment(C, x);
  int32_t kk;
  const int64_t* src = walk_words(C, key, k, sg, x, &kk);
  const int s = int(src[0]);
  const int32_t* row = C.res + (sg * (k - 1) + s - 1) * k;
  if (done) {
    const int64_t c = C.cw_dpre[x];
    keys[c] = FC_MARK | (u64(uint32_t(row[k - 1])) << 31) | u64(c);
    C.cd_x[c] = x;
    return;
  }
  const int reached = row[0] >> 8;
  int64_t* d = C.rpool + (*C.rtop + C.cw_opre[x] + open_rank(R, C.seg_start[sg])) * k;
  d[0] = reached;
  for (int t = 1; t < k; t++) d[t] = t <= s ? src[t] : t <= reached ? pos_of(M, row[t - 1]) : 0;
}

// the CSR of the ordered matches: entries final slot first, stream positions
__global__ __launch_bounds__(256) void follow_carry_rows(FollowMaps M, FollowCarry C, const int32_t* __restrict__ key,
                                                        const StencilProgram* __restrict__ P,
                                                        const u64* __restrict__ sorted, int64_t nm,
                                                        int64_t* __restrict__ match_record, int32_t* __restrict__ match_key,
                                                        int64_t* __restrict__ ent_off, int32_t* __restrict__ ent_name,
                                                        int64_t* __restrict__ ent_record, int64_t* __restrict__ total) {
  const int64_t m = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (m == 0) *total = nm;
  if (m >= nm) return;
  const int k = M.k;
  const u64 v = sorted[m];
  int64_t* er = ent_record + m * k;
  if (v & FC_MARK) {
    // a carried walk: its prefix from the pool, the rest from its continuation -- every load before the
    // row's stores (DESIGN 4.1 "the gather's loads")
    const int64_t x = C.cd_x[v & 0x7FFFFFFFull];
    const int64_t sg = walk_segment(C, x);
    int32_t kk;
    const int64_t* src = walk_words(C, key, k, sg, x, &kk);
    const int s = int(src[0]);
    const int32_t* row = C.res + (sg * (k - 1) + s - 1) * k;
    int64_t pv[STENCIL_MAX_K], last = 0;
#pragma unroll
    for (int t = 0; t < STENCIL_MAX_K; t++) {
      pv[t] = 0;
      if (t < k) pv[t] = t < s ? src[1 + t] : pos_of(M, row[t]);
      if (t == k - 1) last = pv[t];
    }
#pragma unroll
    for (int t = 0; t < STENCIL_MAX_K; t++)
      if (t < k) er[k - 1 - t] = pv[t];
    match_record[m] = last;
    match_key[m] = kk;
  } else {
    const int64_t j0 = int64_t(v & 0x7FFFFFFFull);
    er[k - 1] = pos_of(M, j0);
    const int64_t e = follow_steps(M, j0 + 1, 1, segment_end(M, j0), nullptr, er + k - 1, -1, nullptr);
    match_record[m] = pos_of(M, e);
    match_key[m] = key[j0];
  }
  ent_off[m] = m * k;
  for (int t = 0; t < k; t++) ent_name[m * k + k - 1 - t] = P->name[t];
}

// the open in-batch walks behind their key's surviving carried ones, in start order
__global__ __launch_bounds__(256) void follow_open_write(FollowMaps M, FollowCarry C, OpenRank R) {
  const int64_t j0 = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (j0 >= M.n || !(R.open[j0 >> 6] >> (j0 & 63) & 1)) return;
  const int k = M.k;
  const int64_t sg = C.seg_idx[j0] + C.seg_flag[j0] - 1;
  int64_t* d = C.rpool + (*C.rtop + open_before(C, C.toff[sg + 1]) + open_rank(R, j0)) * k;
  int reached = 1;
  d[1] = pos_of(M, j0);
  (void)follow_steps(M, j0 + 1, 1, segment_end(M, j0), nullptr, d + 1, 1, &reached);
  d[0] = reached;
  for (int t = reached + 1; t < k; t++) d[t] = 0;
}

// the table entries of the batch's keys (a key absent from the batch keeps its own)
__global__ __launch_bounds__(256) void follow_tab(FollowCarry C, OpenRank R, const int32_t* __restrict__ key, int64_t nmax) {
  const int64_t sg = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (sg >= nmax || sg >= *C.nseg) return;
  const int64_t kk = key[C.seg_start[sg]];
  const int64_t o0 = open_before(C, C.toff[sg]), o1 = open_before(C, C.toff[sg + 1]);
  const int64_t r0 = open_rank(R, C.seg_start[sg]), r1 = open_rank(R, C.seg_start[sg + 1]);
  const int64_t cnt = (o1 - o0) + (r1 - r0);
  if (cnt) C.rtab[2 * kk] = *C.rtop + o0 + r0;
  C.rtab[2 * kk + 1] = cnt;
}
__global__ void follow_top_add(int64_t* __restrict__ top, const int64_t* __restrict__ a, const int64_t* __restrict__ b) {
  *top += *a + *b;
}

OpenRank open_rank_args(const FollowArgs& A) { return OpenRank{A.open, A.wopre, A.nopen, A.n}; }

}  // namespace

hipError_t follow_carry_count_launch(const FollowArgs& A, const FollowCarry& C, hipStream_t st) {
  const int64_t nt = follow_tiles(A.n);
  hipError_t e = hipMemsetAsync(A.max_span, 0, 8, st);
  if (e != hipSuccess) return e;
  if (C.bound > 0) {
    const int64_t items = C.nseg_cap * (A.k - 1);
    hipLaunchKernelGGL(follow_resume, dim3(blocks256(items)), dim3(256), 0, st, follow_maps(A), C, items);
    hipLaunchKernelGGL(follow_classify, dim3(blocks256(C.bound)), dim3(256), 0, st, C, A.key, A.k);
    if ((e = exclusive_scan_pair(C.cw_done, C.cw_open, C.bound, C.ncw, C.cw_dpre, C.cw_opre, C.ncd, C.nco, C.scan_tmp,
                                 st)) != hipSuccess)
      return e;
  }
  hipLaunchKernelGGL((follow_walks<false, true>), dim3(unsigned(nt)), dim3(256), 0, st, follow_maps(A), A.tile_starts,
                     A.wcnt, A.wpre, A.keys, A.max_span, A.open, A.wopen);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return exclusive_scan_pair(A.wcnt, A.wopen, nt * 64, nullptr, A.wpre, A.wopre, A.nm, A.nopen, C.scan_tmp, st);
}

hipError_t follow_carry_keys_launch(const FollowArgs& A, const FollowCarry& C, int64_t ncd, hipStream_t st) {
  if (C.bound > 0)
    hipLaunchKernelGGL(follow_carried_out, dim3(blocks256(C.bound)), dim3(256), 0, st, follow_maps(A), C,
                       open_rank_args(A), A.key, A.keys);
  hipLaunchKernelGGL((follow_walks<true, false>), dim3(unsigned(follow_tiles(A.n))), dim3(256), 0, st, follow_maps(A),
                     A.tile_starts, A.wcnt, A.wpre, A.keys + ncd, A.max_span, nullptr, nullptr);
  return hipGetLastError();
}

hipError_t follow_carry_rows_launch(const FollowArgs& A, const FollowCarry& C, const unsigned long long* sorted,
                                    int64_t nm, int64_t* match_record, int32_t* match_key, int64_t* ent_off,
                                    int32_t* ent_name, int64_t* ent_record, int64_t* total, hipStream_t st) {
  hipLaunchKernelGGL(follow_carry_rows, dim3(blocks256(nm)), dim3(256), 0, st, follow_maps(A), C, A.key, A.prog_dev,
                     sorted, nm, match_record, match_key, ent_off, ent_name, ent_record, total);
  return hipGetLastError();
}

hipError_t follow_carry_state_launch(const FollowArgs& A, const FollowCarry& C, hipStream_t st) {
  hipLaunchKernelGGL(follow_open_write, dim3(blocks256(A.n)), dim3(256), 0, st, follow_maps(A), C, open_rank_args(A));
  hipLaunchKernelGGL(follow_tab, dim3(blocks256(A.n)), dim3(256), 0, st, C, open_rank_args(A), A.key, A.n);
  hipLaunchKernelGGL(follow_top_add, dim3(1), dim3(1), 0, st, C.rtop, C.nco, A.nopen);
  return hipGetLastError();
}

}  // namespace kcep
