// follow_bits_dev.h -- device bodies of the follow path's streaming kernels (follow.hip), also compiled per
// pattern by hiprtc (jit.cpp):
//   follow_planes_out      the back half of a bitmap kernel: a tile's mask and key-start bytes in LDS -> the
//                          slots' bit planes, their second level and the tile's starts.  The text of
//                          follow_bits' back half (follow.hip), which keeps its own copy: called from here
//                          its instructions came out in another order
//   follow_eval_bits_body  the evaluated form (CEP_SESSION_MASK_PASS with a follow flag, compile.cpp
//                          analyse_follow_mask): the slots' predicates evaluated per record from the columns
//                          they read, straight into those bytes -- no mask column in between.  Templated on
//                          the program table as masks_body is: MaskInterpTab (built-in, interpreted) or the
//                          MaskJitTab jit.cpp generates.
// One 4096-record tile per 256-thread workgroup; a thread owns the records follow_bits gives it: groups of 4
// at q * 1024 + tid * 4, q = 0..3.  No atomics; no workgroup waits on another.
#pragma once
#include "masks_dev.h"

namespace kcep {

constexpr int FB_TILE = 4096;                     // records per workgroup: 64 bitmap words, one second-level word
constexpr int FB_THREADS = 256;
constexpr int FB_MAX_K = MASK_SLOTS;              // slots: planes 0..k-1, then the key starts' plane

typedef unsigned long long u64;

// s_mask / s_ks: the tile's stage masks and key-start flags, a byte per record, zero for records >= n (written
// by every thread, a barrier since).  Wave wid has the tile's words 16 wid .. 16 wid + 15, a ballot per word
// and plane; lane i keeps word i's, so that lanes 0..15 store each plane's 16 words as one 128-B run.
__device__ __forceinline__ void follow_planes_out(const uint8_t* s_mask, const uint8_t* s_ks,
                                                  uint32_t (*s_part)[FB_THREADS / 64], int32_t* s_cnt, int k, int64_t tile,
                                                  u64* __restrict__ bits, u64* __restrict__ sum, int64_t wpl,
                                                  int64_t nt, int64_t* __restrict__ tile_starts) {
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  u64 mine[FB_MAX_K + 1];
#pragma unroll
  for (int s = 0; s <= FB_MAX_K; s++) mine[s] = 0;
  for (int i = 0; i < 16; i++) {
    const int r = (wid * 16 + i) * 64 + lane;
    const uint32_t m = s_mask[r];
    const u64 bk = __ballot(s_ks[r] != 0);
    if (lane == i) mine[FB_MAX_K] = bk;
#pragma unroll
    for (int s = 0; s < FB_MAX_K; s++) {
      if (s < k) {                                // uniform
        const u64 bs = __ballot((m >> s & 1) != 0);
        if (lane == i) mine[s] = bs;
      }
    }
  }
  const int64_t w0 = tile * 64 + wid * 16 + lane;
#pragma unroll
  for (int s = 0; s <= FB_MAX_K; s++) {
    const int plane = s == FB_MAX_K ? k : s;       // (the key starts' plane comes after the slots')
    if (s < k || s == FB_MAX_K) {                  // uniform
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

// ---- the evaluated form ----
// four consecutive records as the slots read them: the first NC value columns, the metadata (MaskEnv's
// defaults), the key
template <int NC>
struct FbGroup {
  int64_t cv[4][NC], ts4[4], off4[4], part4[4], key4[4], top4[4];
};

// records g..g+3: 16-B non-temporal loads of the key and of every column and metadata array the program
// reads.  FULL: the tile lies inside the batch, so nothing here branches per lane (a lane's branch around
// a load makes the compiler wait for every load in flight where the lanes meet again).  Else (the batch's
// last tile) the group that reaches past n reads by clamped elements, a group at or past n nothing.
template <int NC, bool FULL, class Prog>
__device__ __forceinline__ void fb_load(const Prog& P, const MaskArgs& A, int64_t g, FbGroup<NC>& G) {
  const int64_t n = A.n;
  const int32_t used = P.used, meta = P.meta, ncols = P.ncols;
  int64_t pos4[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    G.ts4[i] = G.off4[i] = G.part4[i] = G.key4[i] = G.top4[i] = 0;
    pos4[i] = A.base + g + i;
#pragma unroll
    for (int c = 0; c < NC; c++) G.cv[i][c] = 0;
  }
  if (!FULL && g >= n) return;
  const bool full = FULL || g + 3 < n;
  const bool need_pos = ((meta & MASK_META_TS) && !A.ts) || ((meta & MASK_META_OFFSET) && !A.offset);
  mk_load32(A.key, g, n, full, G.key4);
#pragma unroll
  for (int c = 0; c < NC; c++) {
    if (c < ncols && (used >> c & 1)) {            // uniform
      int64_t o[4];
      if (P.coltype[c] == T_I32) mk_load32(static_cast<const int32_t*>(A.cols[c]), g, n, full, o);
      else mk_load64(static_cast<const int64_t*>(A.cols[c]), g, n, full, o);
#pragma unroll
      for (int i = 0; i < 4; i++) G.cv[i][c] = o[i];
    }
  }
  if (need_pos && A.pos) mk_load64(A.pos, g, n, full, pos4);
  if (meta & MASK_META_TS) {
    if (A.ts) mk_load64(A.ts, g, n, full, G.ts4);
    else {
#pragma unroll
      for (int i = 0; i < 4; i++) G.ts4[i] = pos4[i];
    }
  }
  if (meta & MASK_META_OFFSET) {
    if (A.offset) mk_load64(A.offset, g, n, full, G.off4);
    else {
#pragma unroll
      for (int i = 0; i < 4; i++) G.off4[i] = pos4[i];
    }
  }
  if ((meta & MASK_META_PARTITION) && A.partition) mk_load32(A.partition, g, n, full, G.part4);
  if ((meta & MASK_META_TOPIC) && A.topic) mk_load32(A.topic, g, n, full, G.top4);
}

// the four records' mask bytes, record g + i in byte i.  As in masks_body record 0 of the registers is
// evaluated, then the four shift down (every index a constant); the group is used up.  A slot that shares
// its code offset with the slot before it -- the n slots of a times(n) stage -- takes that slot's value.
template <class Tab, class Prog>
__device__ __forceinline__ uint32_t fb_eval(const Tab& T, const Prog& P, const MaskArgs& A, int64_t g,
                                            FbGroup<Tab::NC>& G) {
  constexpr int NC = Tab::NC;
  const int32_t pslots = P.pslots;
  uint32_t out = 0;
  KCEP_UNROLL
  for (int i = 0; i < 4; i++) {
    const int64_t gi = g + i < A.n ? g + i : A.n - 1;
    MaskEnv<NC> env{A, gi, G.cv[0], G.ts4[0], G.off4[0], G.part4[0], G.key4[0], int32_t(G.top4[0]), false, 0, 0};
    uint32_t m = 0, hit = 0;
    KCEP_UNROLL
    for (int p = 0; p < MASK_SLOTS; p++) {
      if (pslots >> p & 1) {                       // uniform
        if (p == 0 || P.pc[p] != P.pc[p - 1]) {    // uniform
          int64_t v = 0;
          const bool ok = T.eval(P.pc[p], env, v);
          hit = uint32_t(ok && v != 0);
        }
        m |= hit << p;
      }
    }
    out = (out >> 8) | (m << 24);
#pragma unroll
    for (int r = 0; r < 3; r++) {
      G.ts4[r] = G.ts4[r + 1]; G.off4[r] = G.off4[r + 1]; G.part4[r] = G.part4[r + 1]; G.key4[r] = G.key4[r + 1];
      G.top4[r] = G.top4[r + 1];
#pragma unroll
      for (int c = 0; c < NC; c++) G.cv[r][c] = G.cv[r + 1][c];
    }
  }
  return out;
}

// Tab::AHEAD of a thread's four groups are loaded before the first of them is evaluated: four or two where
// the slots are straight-line code over the columns they name (the per-pattern build: jit.cpp chooses by
// the registers the loads take), one at a time where the interpreter's NC columns and five metadata words
// per record would not fit the registers four times over.
template <class Tab>
__device__ __forceinline__ void follow_eval_bits_body(const Tab& T, const MaskArgs& A, int k, u64* __restrict__ bits,
                                                      u64* __restrict__ sum, int64_t wpl, int64_t nt,
                                                      int64_t* __restrict__ tile_starts) {
  constexpr int NC = Tab::NC, AH = Tab::AHEAD;
  static_assert(AH == 1 || AH == 2 || AH == 4, "the groups loaded ahead divide a thread's four");
  __shared__ __attribute__((aligned(16))) uint8_t s_mask[FB_TILE];   // the records' stage masks
  __shared__ __attribute__((aligned(16))) uint8_t s_ks[FB_TILE];     // 1: the record starts a key segment
  __shared__ uint32_t s_part[FB_MAX_K + 1][FB_THREADS / 64];         // per plane and wave: its 16 words' not-zero bits
  __shared__ int32_t s_cnt[FB_THREADS / 64];
  const auto& P = T.prog();                       // uniform: scalar reads (a constant in the per-pattern build)
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int64_t tile = blockIdx.x;
  const int64_t base = tile * FB_TILE;
  const int64_t n = A.n;
  KCEP_UNROLL
  for (int q0 = 0; q0 < 4; q0 += AH) {
    FbGroup<NC> G[AH];
    int32_t before[AH];                            // the record before each wave's first: lane 0 reads it
    const int64_t g0 = base + q0 * (FB_THREADS * 4) + tid * 4;
    if (base + FB_TILE <= n) {                     // uniform
#pragma unroll
      for (int a = 0; a < AH; a++) fb_load<NC, true>(P, A, g0 + a * (FB_THREADS * 4), G[a]);
    } else {
#pragma unroll
      for (int a = 0; a < AH; a++) fb_load<NC, false>(P, A, g0 + a * (FB_THREADS * 4), G[a]);
    }
#pragma unroll
    for (int a = 0; a < AH; a++) {
      const int64_t g = g0 + a * (FB_THREADS * 4);
      before[a] = 0;
      if (lane == 0 && g > 0 && g < n) before[a] = A.key[g - 1];
    }
#pragma unroll
    for (int a = 0; a < AH; a++) {
      const int local = (q0 + a) * (FB_THREADS * 4) + tid * 4;
      const int64_t g = base + local;
      const int32_t k0 = int32_t(G[a].key4[0]), k1 = int32_t(G[a].key4[1]), k2 = int32_t(G[a].key4[2]),
                    k3 = int32_t(G[a].key4[3]);
      uint32_t w = fb_eval(T, P, A, g, G[a]);
      int32_t kp = __shfl_up(k3, 1);               // the lane before has the record before this group
      if (lane == 0) kp = before[a];
      uint32_t ks = uint32_t(g == 0 || kp != k0) | (uint32_t(k1 != k0) << 8) | (uint32_t(k2 != k1) << 16) |
                    (uint32_t(k3 != k2) << 24);
      const int64_t left = n - g;                  // records >= n: zero bits
      if (left < 4) {
        const uint32_t keep = left <= 0 ? 0u : (0xFFFFFFFFu >> (8 * (4 - left)));
        w &= keep;
        ks &= keep;
      }
      *reinterpret_cast<uint32_t*>(&s_mask[local]) = w;
      *reinterpret_cast<uint32_t*>(&s_ks[local]) = ks;
    }
  }
  __syncthreads();
  follow_planes_out(s_mask, s_ks, s_part, s_cnt, k, tile, bits, sum, wpl, nt, tile_starts);
}

// the built-in kernel's table: the interpreter over the MaskProgram in device memory, the first NC value
// columns in registers, one group at a time
struct FollowInterpTab : MaskInterpTab {
  static constexpr int AHEAD = 1;
};

}  // namespace kcep
