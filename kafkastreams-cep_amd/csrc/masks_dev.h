// masks_dev.h — device body of the mask pre-pass (CEP_SESSION_MASK_PASS; see masks.hip).  Templated on
// the program table Tab, as runs_dev.h is:
//   MaskInterpTab (below)  the MaskProgram in device memory, slots interpreted (libkcep.so's built-in kernel)
//   MaskJitTab (jit.cpp)   the MaskProgram as a compile-time constant and the slots as straight-line code
//
// A streaming element-wise kernel: each thread takes 4 consecutive records per step (16-B loads of the
// i32 columns, 2 x 16 B of the i64 / f64 ones, one 16-B store of the 4 masks), the grid is capped and
// strides.  No LDS, no atomics.  The last, partial group reads with clamped element accesses and stores
// element-wise: nothing at or past n is read or written.
#pragma once
#include "interp.h"

#ifndef KCEP_UNROLL
#ifdef KCEP_JIT
#define KCEP_UNROLL _Pragma("unroll")
#else
#define KCEP_UNROLL
#endif
#endif

namespace kcep {

constexpr int MK_THREADS = 256;
constexpr int MK_MAX_BLOCKS = 2048;                // 256 CUs x 8 workgroups; the rest by grid stride

typedef int mk_v4i __attribute__((ext_vector_type(4)));
typedef long long mk_v2l __attribute__((ext_vector_type(2)));
typedef const MaskProgram __attribute__((address_space(4))) cMaskProgram;

// records g..g+3 of a column (streamed once: non-temporal); !full: the group reaches past n
__device__ __forceinline__ void mk_load32(const int32_t* __restrict__ p, int64_t g, int64_t n, bool full, int64_t (&o)[4]) {
  if (full) {
    const mk_v4i v = __builtin_nontemporal_load(reinterpret_cast<const mk_v4i*>(p + g));
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = p[g + i < n ? g + i : n - 1];
  }
}
__device__ __forceinline__ void mk_load64(const int64_t* __restrict__ p, int64_t g, int64_t n, bool full, int64_t (&o)[4]) {
  if (full) {
    const mk_v2l a = __builtin_nontemporal_load(reinterpret_cast<const mk_v2l*>(p + g));
    const mk_v2l b = __builtin_nontemporal_load(reinterpret_cast<const mk_v2l*>(p + g + 2));
    o[0] = a[0]; o[1] = a[1]; o[2] = b[0]; o[3] = b[1];
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = p[g + i < n ? g + i : n - 1];
  }
}

// one record: its first NC columns and its metadata in registers.  Field and metadata defaults are
// runs_dev.h RunEnv's: ts / offset default to the stream position, partition and topic to 0; doubles
// are read as their bits.  A slot is event-only by construction (compile.cpp analyse_mask_pass):
// state, fold and sequence reads fail.
template <int NC>
struct MaskEnv {
  const MaskArgs& A;
  int64_t g;
  const int64_t* cv;
  int64_t v_ts, v_off, v_part, v_key;
  int32_t v_topic;
  bool in_fold;
  int32_t curr_tag;
  int64_t curr;
  __device__ __forceinline__ int64_t field(int col, int t) {
    if (col < NC) {
      int64_t v = 0;
#pragma unroll
      for (int i = 0; i < NC; i++)
        if (i == col) v = cv[i];
      return v;
    }
    const void* c = A.cols[col];
    if (t == T_I32) return static_cast<const int32_t*>(c)[g];
    return static_cast<const int64_t*>(c)[g];
  }
  __device__ __forceinline__ int64_t key() { return v_key; }
  __device__ __forceinline__ int64_t ts() { return v_ts; }
  __device__ __forceinline__ int64_t off() { return v_off; }
  __device__ __forceinline__ int64_t part() { return v_part; }
  __device__ __forceinline__ int32_t topic() { return v_topic; }
  __device__ __forceinline__ bool state(int, int32_t& tag, int64_t& v) { tag = 0; v = 0; return false; }
  __device__ __forceinline__ bool seq_avg(int, int64_t&) { return false; }
  __device__ __forceinline__ bool seq_agg(int, int, int, int64_t&) { return false; }
  __device__ __forceinline__ void fail(int) {}
};

template <class Tab>
__device__ __forceinline__ void masks_body(const Tab& T, const MaskArgs& A) {
  constexpr int NC = Tab::NC;
  const auto& P = T.prog();                       // uniform: scalar reads (a constant in the per-pattern build)
  const int64_t n = A.n;
  const int64_t ngroups = (n + 3) >> 2;
  const int32_t pslots = P.pslots, used = P.used, meta = P.meta, ncols = P.ncols;
  const bool need_pos = ((meta & MASK_META_TS) && !A.ts) || ((meta & MASK_META_OFFSET) && !A.offset);
  for (int64_t q = int64_t(blockIdx.x) * MK_THREADS + threadIdx.x; q < ngroups; q += int64_t(gridDim.x) * MK_THREADS) {
    const int64_t g = q << 2;
    const bool full = g + 3 < n;
    int64_t cv[4][NC], ts4[4], off4[4], part4[4], key4[4], top4[4], pos4[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      ts4[i] = off4[i] = part4[i] = key4[i] = top4[i] = 0;
      pos4[i] = A.base + g + i;
#pragma unroll
      for (int c = 0; c < NC; c++) cv[i][c] = 0;
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
      if (c < ncols && (used >> c & 1)) {          // uniform
        int64_t o[4];
        if (P.coltype[c] == T_I32) mk_load32(static_cast<const int32_t*>(A.cols[c]), g, n, full, o);
        else mk_load64(static_cast<const int64_t*>(A.cols[c]), g, n, full, o);
#pragma unroll
        for (int i = 0; i < 4; i++) cv[i][c] = o[i];
      }
    }
    if (need_pos && A.pos) mk_load64(A.pos, g, n, full, pos4);
    if (meta & MASK_META_TS) {
      if (A.ts) mk_load64(A.ts, g, n, full, ts4);
      else {
#pragma unroll
        for (int i = 0; i < 4; i++) ts4[i] = pos4[i];
      }
    }
    if (meta & MASK_META_OFFSET) {
      if (A.offset) mk_load64(A.offset, g, n, full, off4);
      else {
#pragma unroll
        for (int i = 0; i < 4; i++) off4[i] = pos4[i];
      }
    }
    if ((meta & MASK_META_PARTITION) && A.partition) mk_load32(A.partition, g, n, full, part4);
    if ((meta & MASK_META_TOPIC) && A.topic) mk_load32(A.topic, g, n, full, top4);
    if (meta & MASK_META_KEY) mk_load32(A.key, g, n, full, key4);

    // record 0 of the registers is evaluated, then the four shift down: every index is a constant
    mk_v4i out = {0, 0, 0, 0};
    KCEP_UNROLL
    for (int i = 0; i < 4; i++) {
      const int64_t gi = g + i < n ? g + i : n - 1;
      MaskEnv<NC> env{A, gi, cv[0], ts4[0], off4[0], part4[0], key4[0], int32_t(top4[0]), false, 0, 0};
      uint32_t m = 0;
      KCEP_UNROLL
      for (int p = 0; p < MASK_SLOTS; p++) {
        if (pslots >> p & 1) {                     // uniform
          int64_t v = 0;
          const bool ok = T.eval(P.pc[p], env, v);
          m |= uint32_t(ok && v != 0) << p;
        }
      }
      out = mk_v4i{out[1], out[2], out[3], int(m)};
#pragma unroll
      for (int r = 0; r < 3; r++) {
        ts4[r] = ts4[r + 1]; off4[r] = off4[r + 1]; part4[r] = part4[r + 1]; key4[r] = key4[r + 1]; top4[r] = top4[r + 1];
#pragma unroll
        for (int c = 0; c < NC; c++) cv[r][c] = cv[r + 1][c];
      }
    }
    if (full) {
      *reinterpret_cast<mk_v4i*>(A.mask + g) = out;
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (g + i < n) A.mask[g + i] = out[i];
    }
  }
}

// the built-in kernel's table: the first 4 value columns are held in registers (vector loads), later
// ones are read by element at each use
struct MaskInterpTab {
  static constexpr int NC = 4;
  const MaskProgram* raw;
  __device__ __forceinline__ const cMaskProgram& prog() const { return *(const cMaskProgram*)raw; }
  template <class Env>
  __device__ __forceinline__ bool eval(int pc, Env& env, int64_t& v) const {
    return interp_ls(raw->code, pc, env, true, v);
  }
};

}  // namespace kcep
