// session.h -- what abi.cpp, push.cpp and state.cpp share: the session and pattern structs, the owning
// resource types their members are made of, error reporting, and the helpers that cross a unit boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <type_traits>
#include <utility>

#include "../../include/kcep.h"
#include "launch.h"

namespace kcep {

int set_error(int code, const std::string& msg);   // abi.cpp: the thread's cep_last_error() message
inline int fail(int code, const std::string& msg) { return set_error(code, msg); }

#define HIPCHECK(x)                                                                                \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) return fail(CEP_E_HIP, std::string(#x ": ") + hipGetErrorString(e_));    \
  } while (0)

inline size_t type_size(int t) { return t == T_I32 ? 4 : 8; }

// device buffer that only grows; owns its allocation (move-only)
struct DBuf {
  void* p = nullptr;
  size_t cap = 0;
  DBuf() = default;
  DBuf(DBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}   // (no copies)
  DBuf& operator=(DBuf&& o) noexcept {             // takes o's allocation; o frees what this held
    std::swap(p, o.p);
    std::swap(cap, o.cap);
    return *this;
  }
  ~DBuf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
    if (e == hipSuccess) cap = bytes ? bytes : 16;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};
static_assert(!std::is_copy_constructible_v<DBuf>, "a DBuf has one owner");

// an event, destroyed with its owner (created where it is first needed: hipEventCreate*(&ev.e, ...))
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { if (e) (void)hipEventDestroy(e); }
  operator hipEvent_t() const { return e; }
};

// a pinned host allocation (hipHostMalloc), freed with its owner
template <class T>
struct Pinned {
  T* p = nullptr;
  size_t cap = 0;
  Pinned() = default;
  Pinned(const Pinned&) = delete;
  Pinned& operator=(const Pinned&) = delete;
  ~Pinned() { if (p) (void)hipHostFree(p); }
  hipError_t alloc(size_t bytes, unsigned flags) {   // replaces what it held
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), bytes, flags);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  operator T*() const { return p; }
};

// first allocation of a key's workspace on the general path (grown on demand from the pool)
constexpr NfaCaps kCaps{16, 64, 32, 32, 8, 16};
constexpr int kMaxRetry = 24;                      // pool regrowths (each toward free HBM) before CEP_E_RUN_CAPACITY
constexpr int kPoolQuiet = 4;                      // batches within the estimate before a grown pool is given back
constexpr int64_t kRunsErrCap = int64_t(1) << 20;  // runs path: failing runs listed per batch (cep_batch_errors)

}  // namespace kcep

struct cep_pattern {
  kcep::Program prog;
};

// Destruction: ~cep_session (abi.cpp) waits for the ring slots and deliveries, then the members go in reverse order.
struct cep_session {
  using DBuf = kcep::DBuf;
  using Event = kcep::Event;
  using JitModule = kcep::JitModule;
  template <class T>
  using Pinned = kcep::Pinned<T>;
  ~cep_session();
  const cep_pattern* pat = nullptr;
  cep_opts opts{};
  int path = 0;                 // preferred path
  // the stencil program the session's stencil / chain batches run: the pattern's direct
  // lowering, or on a CEP_SESSION_MASK_PASS session of an eligible pattern its mask-pass form
  const kcep::StencilProgram* sp = nullptr;
  bool mask_pass = false;       // stencil / chain batches run the pre-pass (masks.hip) first
  // a follow session in the evaluated form (Program::follow_mask_ok, CEP_SESSION_MASK_PASS with a follow flag):
  // sp = &follow_mask, the bitmaps come from follow_eval_bits over the columns the predicates read (mprog);
  // follow_split (KCEP_FOLLOW_MASK_SPLIT=1 at open): from the pre-pass into mcol and follow_bits over it
  bool follow_eval = false, follow_split = false;
  uint32_t follow_next = 0;     // a follow session's skip-till-next slots
  // a follow session of a pattern with oneOrMore stages (Program::follow_many_ok, CEP_SESSION_FOLLOW_MANY):
  // sp = &follow_many, its batches leave the runs path's CSR (variable-length matches); follow_many_mask: its
  // oneOrMore slots
  bool follow_many = false;
  uint32_t follow_many_mask = 0;
  int last_path = 0;            // path of the last batch
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t n = 0;
  bool pending = false;
  Event ev0, ev1, eb0, eb1;
  bool timing = true;                      // cep_session_set_timing: stencil/chain batches record events
  // ---- stencil workspace ----
  DBuf prog, out, status, counter, total, sum, mkey, slots;   // status: tile counts + prefixes; counter: scan scratch
  int64_t out_cap = 0;
  const int32_t* d_key = nullptr;
  DBuf mprog, mcol;             // mask pass: the MaskProgram; the mask column (max_events rounded up to 4 int32)
  // ---- follow path (follow.hip; prog, out, total, sum as above): the slots' bitmaps and their second level,
  // the tiles' starts, the completed walks per bitmap word and their prefix, sized from max_events at open;
  // the walks' keys, their order and the sort's scratch are the runs workspace's rk, rk_sorted, r_len, rk_tmp ----
  DBuf fw_bits, fw_sum, fw_tile, fw_cnt, fw_pre;
  // ... on a carry session (CEP_SESSION_FOLLOW_CARRY; the walks are carried in the runs path's tail pool below,
  // records of k words): the open starts' plane, their count per word and its prefix; the continuations per
  // (segment, slot); per carried walk of the batch's keys its outcome flags, their prefixes, the completed ones
  DBuf fw_open, fw_ocnt, fw_opre, fw_res, fw_cdone, fw_copen, fw_cdpre, fw_copre, fw_cdx;
  // ... of a pattern with oneOrMore stages (CEP_SESSION_FOLLOW_MANY): the completed walks' entries per word and
  // their prefix
  DBuf fw_len, fw_lpre;
  // ---- staging of host-resident batches (stage_host): a pinned ring the caller's columns are copied
  // into in chunks, each chunk moved by one async copy into one packed device image; caller memory
  // that is itself pinned is copied from directly and the push waits for that copy ----
  DBuf dstage, h_topic;
  Pinned<void> ring[2];
  Event ring_ev[2];
  int ring_next = 0;
  Event h2d_ev;
  // ---- CEP_BATCH_DELIVER (carry stencil / chain sessions): the matches handed to pinned host memory by
  // the device during the push; cep_collect then only waits ----
  Pinned<void> dl[2];                 // dl_layout: header, host_cap keys, host_cap * k positions; by stamp parity
  int64_t dl_pid[2] = {-1, -1};       // the batch (push number) each holds: a host pushes batch i + 1 before it
                                      // collects batch i (cep_collect_batch)
  int64_t push_id = 0;                // cep_push_batch calls so far (cep_batch_id)
  int64_t dl_cap = 0;
  DBuf dl_ticket;                 // device: workgroups of the delivery kernel done
  int64_t dl_stamp = 0;           // the last delivery's number
  bool delivered = false;
  bool h2d_wait = false;          // the push copied from pinned caller memory: wait for h2d_ev
  int zc_slot = -1;               // the push's kernels read ring slot zc_slot in place (zero copy)
  // ---- general workspace ----
  DBuf dprog, flag, idx, seg, scan_tmp, scal, ctl, pool, r_matches, r_words, r_out, r_ent, r_err, r_errrec, r_carry,
      moff, eoff, o_record, o_key, o_entoff, o_name, o_entrec, ord, ord_bucket, ord_cnt;
  int64_t pool_words = 0;       // pool capacity this batch uses
  int64_t pool_est = 0;         // the batches' estimated pool (largest so far)
  int64_t pool_learned = 0;     // what the last overflowing batch grew the pool to (0: none): later batches start
                                // there, without re-running, until kPoolQuiet batches in a row fit the estimate
  int pool_quiet = 0;
  int last_attempts = 0;        // general path: kernel attempts of the last batch (1 + pool regrowths)
  // CEP_BATCH_STOP_AT_ERROR (cep_batch_stopped): key segments the last general batch's early-out stopped or
  // skipped, and their records left unevaluated
  int64_t stopped_keys = 0, stopped_records = 0;
  // records of the stopped batches since the last committed one: their positions stay used (base), but a
  // state export still names the position the committed state stands at -- it is byte for byte the
  // checkpoint before them
  int64_t stop_uncommitted = 0;
  int64_t nseg = 0, g_matches = 0, g_entries = 0;
  int64_t nseg_hint = 0;        // the last general batch's segment count (pool estimate of the next)
  // ---- carried per-key state (CEP_SESSION_CARRY): NFAStore equivalent ----
  bool carry = false;
  int64_t base = 0;             // stream position of the next batch's record 0
  DBuf ctab, cpool;             // per key id: blob offset (-1 none); blobs (int32 words)
  DBuf kstamp;                  // per key id: number of the last batch that had a segment of it
  int32_t batch_no = 0;
  // ---- carried halos of the stencil path (CEP_SESSION_CARRY, kcep_internal.h HaloHdr) ----
  DBuf halo, hpos, hflags, opos;
  int32_t halo_stamp = 0;
  int64_t halo_base = 0;        // stream position of the last stencil batch's record 0
  int64_t cpool_words = 0, cpool_used = 0;
  // ---- deterministic runs workspace ----
  DBuf rk, rk_sorted, rk_tmp, r_len, r_entoff, r_errcode, r_endof, r_segs, r_blk, r_errlist;
  // kernels compiled for the pattern (jit.cpp); null: the built-in interpreting kernels run
  bool jit_on = false;                     // allowed (not CEP_SESSION_INTERPRET / KCEP_JIT=0)
  std::shared_ptr<const JitModule> jit;    // runs path
  std::shared_ptr<const JitModule> jitm;   // mask pass: the pre-pass kernel; evaluated follow form: its streaming kernel
  std::shared_ptr<const JitModule> jitg;   // general path (built at open, or at the first general batch)
  bool jitg_tried = false;
  std::shared_ptr<const JitModule> jitg_stop;   // its CEP_BATCH_STOP_AT_ERROR build (at the first flagged batch)
  bool jitg_stop_tried = false;
  int64_t live_hwm = 0;                    // general path: most live runs any key held in the last batch
  bool wave = false;                       // general path: one key per wave (nfa_wave.h) for this pattern
  DBuf wscratch;                           // the wave kernel's recycled per-workgroup workspace regions
  bool g_any_err = false;                  // general path: some key of the last batch raised
  DBuf r_prof;                             // CEP_SESSION_PROFILE: per key segment {live max, evaluations, cycles}
  std::string jit_why;
  int32_t g_err = CEP_OK;
  int64_t g_err_rec = -1;
  std::vector<int64_t> e_rec;              // every failing key's (record, code) of the last batch
  std::vector<int32_t> e_code;
  // ---- host CSR of the last collect ----
  std::vector<int64_t> match_record, ent_off, ent_record;
  std::vector<int32_t> match_key, ent_name, out_host;
  // ---- carried tails of the runs path (CEP_SESSION_CARRY, runs.hip) ----
  DBuf rtab, rpool, rpool2, rtop, e_key, e_topic, e_part, e_seg, e_off, e_ts, e_pos, rc_a, rc_b, rc_c, rc_d, gc_len, gc_off;
  DBuf e_cols[16];
  int64_t rpool_cap = 0, rpool_used = 0;   // tail records (5 + ncols int64 words each)
  Pinned<int64_t> h_res;                   // runs / general paths: the batch's counts, written by the device into
                                           // pinned memory (16 words)
  // ---- CEP_BATCH_ARRIVAL_ORDER (group.hip): the batch grouped by key on the device ----
  DBuf g_key, g_arr, g_pos, g_valid, g_topic, g_part, g_off, g_ts, g_head, g_top, g_nodes, g_start, a_cnt,
      a_ecnt, a_head, a_moff, a_moffe, a_tmp, a_record, a_key, a_entoff, a_name, a_entrec;
  uint32_t group_stamp = 0;                // the groupings so far (epoch of the per-key list heads)
  DBuf g_cols[16];
  const int64_t* cur_pos = nullptr;        // the batch being pushed: stream position per grouped record (else null)
  const int64_t* last_gpos = nullptr;      // ... of the last stencil / chain batch (carry_args)
  int64_t arrival_n = 0;                   // ... its records if it came in arrival order (CEP_BATCH_ARRIVAL_ORDER), else 0:
                                           // arrival indices run over them, also where a filter dropped some
  // ---- CEP_BATCH_FILTER (filter.hip): the high-water marks of stencil / chain / runs carry sessions, per
  // (key id, topic id), allocated at the first filtered push; the batch's staged marks; the admitted batch ----
  DBuf f_marks, f_stage, f_tile_f, f_tile_v, f_tile_cnt, f_tile_off, f_slot, f_scal;
  DBuf f_key, f_topic, f_part, f_off, f_ts, f_pos;
  DBuf f_cols[16];
  Pinned<int64_t> f_host;                  // {admitted count, topic-range flag, stamp}, written by the device
  int64_t f_stamp = 0;                     // the filtered pushes so far
  kcep::FilterArgs f_args{};               // the last filtered push's (its staged marks are committed by them)
  bool collected = false;                  // the CSR above is the last batch's: a second collect re-uses it
  cep_matches last{};
  std::vector<uint8_t> evict_buf;          // cep_state_evict's blobs
};

namespace kcep {

// an environment switch for A/B runs ("1" on)
inline bool getenv_flag(const char* name) {
  const char* v = getenv(name);
  return v && v[0] == '1';
}
// an on-by-default path switched off by NAME=0
inline bool getenv_flag_off(const char* name) {
  const char* v = getenv(name);
  return v && v[0] == '0' && v[1] == 0;
}

inline int32_t max_keys32(const cep_session* s) { return int32_t(std::min<int64_t>(s->opts.max_keys, INT32_MAX)); }

// the halo arguments of the last stencil batch (its stamp and stream position)
inline StencilCarry carry_args(const cep_session* s) {
  return StencilCarry{s->halo.as<HaloHdr>(), s->hpos.as<int64_t>(), s->sp->k - 1, s->halo_stamp,
                      max_keys32(s), s->halo_base,
                      s->hflags.as<unsigned long long>() + (s->halo_stamp & 1), s->last_gpos};
}

// Host-resident batch columns -> one packed device image (s->dstage), 256-B aligned per column.  The
// caller's memory is borrowed only for the call (kcep.h cep_push_batch):
//  - pageable memory (a JVM heap array, a numpy buffer) is copied into the session's pinned ring in
//    chunks of 2 MB, each chunk moved by one async copy while the next one is filled; the
//    call returns once the last chunk is in the ring;
//  - memory that is itself pinned is copied from directly, and the call waits for that copy (the
//    kernels are already enqueued behind it).
struct HostArr {
  const void* src;
  size_t bytes;
  const void** dst;               // receives the device address (null src: left null)
};
// zero copy only pays for small batches: the kernel then reads the batch over the link itself, which
// for an 8 MB batch (1 M records) cost 706 us per flush against ~280 us by DMA (r04 bench)
constexpr size_t kZeroCopyMax = size_t(1) << 20;

// the tail pool's sessions: runs carry sessions (records of 5 + ncols words) and follow carry sessions
// (walks of k words)
inline bool walk_session(const cep_session* s) { return s->carry && s->path == CEP_PATH_FOLLOW; }
inline int tail_rw(const cep_session* s) {
  return walk_session(s) ? s->sp->k : 5 + int(s->pat->prog.coltypes.size());
}
inline bool tail_session(const cep_session* s) { return s->carry && (s->path == CEP_PATH_RUNS || s->path == CEP_PATH_FOLLOW); }
// the last batch left the general / runs CSR on the device (o_record ...; its match count in scal[3])
inline bool csr_batch(const cep_session* s) {
  return s->last_path == CEP_PATH_GENERAL || s->last_path == CEP_PATH_RUNS ||
         (s->last_path == CEP_PATH_FOLLOW && (s->carry || s->follow_many));
}
inline bool halo_session(const cep_session* s) { return s->carry && (s->path == CEP_PATH_STENCIL || s->path == CEP_PATH_CHAIN); }

// ---- helpers that cross a unit boundary (push.cpp) ----
void dl_layout(const cep_session* s, int slot, int64_t*& hdr, int32_t*& hkey, int64_t*& hpos);
int push_stencil(cep_session* s, const cep_batch* b, hipStream_t st);
int push_runs(cep_session* s, const cep_batch* b, hipStream_t st);
int push_follow(cep_session* s, const cep_batch* b, hipStream_t st);
int push_general(cep_session* s, const cep_batch* b, hipStream_t st);
int group_batch(cep_session* s, const cep_batch* b, hipStream_t st, cep_batch& gb, const void** gcols);
int arrival_csr(cep_session* s, int64_t base, int64_t n, hipStream_t st);
int filter_batch(cep_session* s, const cep_batch* b, hipStream_t st, cep_batch& fb, const void** fcols);
int marks_ensure(cep_session* s, hipStream_t st);
int carry_gc(cep_session* s, int64_t min_words, hipStream_t st);
int tail_reserve(cep_session* s, int64_t more, hipStream_t st);

}  // namespace kcep
