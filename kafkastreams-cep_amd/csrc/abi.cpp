// abi.cpp — the extern "C" surface of include/kcep.h: patterns, sessions, cep_push_batch and its dispatch,
// timing, collection, the getters.  push.cpp: the push paths; state.cpp: cep_state_*; session.h: shared.
//
// A session plays the role of one CEPProcessor (processor/CEPProcessor.java:45-171)
// bound to one GPU: it owns the device workspace, receives whole batches of
// records (struct-of-arrays, grouped by key) instead of one process(K,V) call
// per record, launches the HIP kernels on the caller's stream and hands back
// the emitted sequences as a CSR.  There is no CPU evaluation path: if a
// pattern or batch cannot be lowered to a device path, the call fails with a
// status code.
//
// Device paths:
//   stencil  (stencil.hip)  strict single-cardinality patterns, SURVEY Q9
//   runs     (runs.hip)     deterministic strict runs
//   follow   (follow.hip)   strict and skip-till-next stages: one deterministic walk per start (opt-in;
//                           carry sessions carry the waiting walks per key; with CEP_SESSION_FOLLOW_MANY
//                           oneOrMore stages too, their matches of variable length)
//   general  (nfa.hip)      every pattern the IR expresses: one lane (or wave) per key
//                           running the reference NFA over an HBM arena
#include <dlfcn.h>
#include <string.h>

#include <atomic>
#include <chrono>

#include "build_id.h"   // KCEP_BUILD_ID (Makefile: hash of the library sources)
#include "jit.h"
#include "session.h"

using namespace kcep;

static thread_local std::string g_err;
int kcep::set_error(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

cep_session::~cep_session() {
  for (auto& ev : ring_ev)                         // a ring slot's last copy or zero-copy read has finished
    if (ev) (void)hipEventSynchronize(ev);
  if (dl[0] || dl[1]) (void)hipDeviceSynchronize();   // a delivery may still be writing into them
}

namespace {

uint64_t mix64(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
  return x;
}

// roctx ranges around the C-ABI calls (SURVEY §5 tracing), for rocprofv3 --marker-trace: on with
// KCEP_ROCTX=1, the roctx library loaded at the first call (no link-time dependency, no cost when off)
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    const char* on = getenv("KCEP_ROCTX");
    if (!on || on[0] != '1') return;
    void* h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_LOCAL);
    if (!h) return;
    push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
    pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
    if (!push || !pop) push = nullptr;
  }
};
const Roctx& roctx() {
  static const Roctx r;
  return r;
}
struct RoctxRange {
  bool on;
  explicit RoctxRange(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
  ~RoctxRange() { if (on) roctx().pop(); }
};

}  // namespace

extern "C" {

const char* cep_last_error(void) { return g_err.c_str(); }
const char* cep_version(void) { return "kcep 0.1 (gfx950) build " KCEP_BUILD_ID; }

int cep_compile(const uint8_t* ir, size_t len, cep_pattern** out) {
  if (!ir || !out) return fail(CEP_E_ARG, "null argument");
  *out = nullptr;
  auto* p = new cep_pattern();
  std::string err;
  int rc = compile_ir(ir, len, p->prog, err);
  if (rc) {
    delete p;
    return fail(rc, err);
  }
  *out = p;
  return CEP_OK;
}

void cep_pattern_free(cep_pattern* p) { delete p; }

int cep_pattern_get_info(const cep_pattern* p, cep_pattern_info* o) {
  if (!p || !o) return fail(CEP_E_ARG, "null argument");
  const Program& P = p->prog;
  o->n_stages = int32_t(P.stages.size());
  o->n_names = int32_t(P.names.size());
  o->n_patterns = int32_t(P.pats.size());
  o->n_cols = int32_t(P.coltypes.size());
  o->stencil_ok = P.stencil_ok && !P.stencil.chain ? 1 : 0;
  o->stencil_k = P.stencil_ok ? P.stencil.k : 0;
  o->chain_ok = P.stencil_ok && P.stencil.chain ? 1 : 0;
  o->runs_ok = P.runs_ok ? 1 : 0;
  return CEP_OK;
}

const char* cep_pattern_name(const cep_pattern* p, int32_t id) {
  if (!p || id < 0 || id >= int32_t(p->prog.names.size())) return nullptr;
  return p->prog.names[id].c_str();
}

int cep_pattern_check(const cep_pattern* p, int32_t session_flags) {
  if (!p) return fail(CEP_E_ARG, "null argument");
  const Program& P = p->prog;
  // a carry session keeps its keys' full NFA state on the general path whenever a batch needs it
  if ((session_flags & CEP_SESSION_CARRY) && !P.general_ok)
    return fail(CEP_E_UNSUPPORTED, "pattern cannot be lowered to the device NFA: " + P.general_why);
  // (CEP_SESSION_FOLLOW_MANY: a pattern with oneOrMore stages the follow path takes, as cep_session_open decides)
  const bool many = (session_flags & CEP_SESSION_FOLLOW_MANY) && !(session_flags & CEP_SESSION_CARRY) && P.follow_many_ok &&
                    (!P.follow_many_eval || (session_flags & CEP_SESSION_MASK_PASS));
  if (!P.stencil_ok && !P.runs_ok && !P.general_ok && !many)
    return fail(CEP_E_UNSUPPORTED, "no device path: " + P.general_why);
  return CEP_OK;
}

int32_t cep_pattern_stage(const cep_pattern* p, int32_t sid, int32_t* name_id, int32_t* type, int64_t* window_ms,
                          int32_t* ops, int32_t* targets, int32_t cap) {
  if (!p || sid < 0 || sid >= int32_t(p->prog.stages.size())) return -1;
  const StageDef& st = p->prog.stages[sid];
  if (name_id) *name_id = st.name;
  if (type) *type = st.type;
  if (window_ms) *window_ms = st.window_ms;
  const int32_t ne = int32_t(st.edges.size());
  for (int32_t i = 0; i < ne && i < cap; i++) {
    if (ops) ops[i] = st.edges[i].op;
    if (targets) targets[i] = st.edges[i].target;
  }
  return ne;
}

int cep_session_open(const cep_pattern* p, const cep_opts* opts, cep_session** out) {
  if (!p || !opts || !out) return fail(CEP_E_ARG, "null argument");
  *out = nullptr;
  if (opts->mode != CEP_MODE_NFA && opts->mode != CEP_MODE_PROCESSOR) return fail(CEP_E_ARG, "bad mode");
  const Program& P = p->prog;
  int path = opts->force_path;
  // CEP_SESSION_MASK_PASS: where the direct lowering does not apply, the eligible pattern's mask-pass form
  const bool mask_flag = (opts->flags & CEP_SESSION_MASK_PASS) && !P.stencil_ok;
  const bool masked = mask_flag && P.mask_ok;
  const StencilProgram* sp = P.stencil_ok ? &P.stencil : masked ? &P.mask_stencil : nullptr;
  const int fast = sp && sp->chain ? CEP_PATH_CHAIN : CEP_PATH_STENCIL;   // the streaming kernel's flavour
  const bool carry = opts->flags & CEP_SESSION_CARRY;
  // CEP_SESSION_FOLLOW: an eligible pattern's skip-till-next walks, on sessions without carry;
  // CEP_SESSION_FOLLOW_CARRY: on carry sessions too (the waiting walks carried per key), and implies the former
  const bool follow_carry = (opts->flags & CEP_SESSION_FOLLOW_CARRY) != 0;
  // ... with CEP_SESSION_MASK_PASS also a pattern of the follow shape whose predicates the direct lowering does
  // not take (cep_pattern_follow_mask), in the evaluated form
  const bool follow_eval = (opts->flags & CEP_SESSION_MASK_PASS) && P.follow_mask_ok;
  // CEP_SESSION_FOLLOW_MANY: a pattern with oneOrMore stages (cep_pattern_follow_many), on sessions without
  // carry; implies CEP_SESSION_FOLLOW; the evaluated form again only with CEP_SESSION_MASK_PASS
  const bool many_flag = (opts->flags & CEP_SESSION_FOLLOW_MANY) != 0;
  const bool follow_flag =
      (((opts->flags & (CEP_SESSION_FOLLOW | CEP_SESSION_FOLLOW_MANY)) && !carry) || follow_carry) && (P.follow_ok || follow_eval);
  const bool follow_many =
      many_flag && !carry && P.follow_many_ok && (!P.follow_many_eval || (opts->flags & CEP_SESSION_MASK_PASS));
  if (path == 0)
    path = sp ? fast : follow_flag || follow_many ? CEP_PATH_FOLLOW : P.runs_ok ? CEP_PATH_RUNS : CEP_PATH_GENERAL;
  if (path == CEP_PATH_FOLLOW && many_flag && P.follow_many_ok && !follow_many)
    return fail(CEP_E_UNSUPPORTED,
                carry ? "follow path does not apply: CEP_SESSION_FOLLOW_MANY takes sessions without CEP_SESSION_CARRY "
                        "(a carried oneOrMore walk is not K words)"
                      : "follow path does not apply: CEP_SESSION_FOLLOW_MANY takes the pattern in the evaluated form, "
                        "which needs CEP_SESSION_MASK_PASS");
  if (path == CEP_PATH_FOLLOW && !P.follow_ok && !follow_eval && !follow_many)
    return fail(CEP_E_UNSUPPORTED, "follow path does not apply: " + P.follow_why);
  if (path == CEP_PATH_FOLLOW && carry && !follow_carry)
    return fail(CEP_E_UNSUPPORTED, "follow path does not apply: it takes sessions without CEP_SESSION_CARRY");
  if (path == CEP_PATH_RUNS && !P.runs_ok) return fail(CEP_E_UNSUPPORTED, "runs path does not apply: " + P.runs_why);
  if ((path == CEP_PATH_STENCIL || path == CEP_PATH_CHAIN) && !sp)
    return fail(CEP_E_UNSUPPORTED, "stencil path does not apply: " + P.stencil_why +
                                       (mask_flag ? "; mask pass does not apply: " + P.mask_why : std::string()));
  if (path == CEP_PATH_STENCIL || path == CEP_PATH_CHAIN) path = fast;
  if (path == CEP_PATH_GENERAL && !P.general_ok)
    return fail(CEP_E_UNSUPPORTED, "pattern cannot be lowered to the device NFA: " + P.general_why);
  if (path != CEP_PATH_STENCIL && path != CEP_PATH_CHAIN && path != CEP_PATH_GENERAL && path != CEP_PATH_RUNS &&
      path != CEP_PATH_FOLLOW)
    return fail(CEP_E_ARG, "bad path");
  if (!P.stencil_ok && path != CEP_PATH_STENCIL && path != CEP_PATH_CHAIN) sp = nullptr;   // (a forced other path)
  const bool follow = path == CEP_PATH_FOLLOW;
  if (carry && (opts->max_keys <= 0 || opts->max_keys > INT32_MAX))
    return fail(CEP_E_ARG, "carry sessions need max_keys (dense key ids in [0, max_keys))");
  if (carry && !P.general_ok)
    return fail(CEP_E_UNSUPPORTED, "pattern cannot be lowered to the device NFA: " + P.general_why);
  HIPCHECK(hipSetDevice(opts->device));
  auto* s = new cep_session();
  s->pat = p;
  s->opts = *opts;
  s->path = path;
  // (a pattern with oneOrMore stages has neither of the other follow forms)
  s->follow_many = follow && follow_many;
  s->follow_many_mask = s->follow_many ? P.follow_many_mask : 0;
  s->follow_eval = follow && (s->follow_many ? P.follow_many_eval : !P.follow_ok);   // (a pattern the direct lowering takes keeps it)
  s->follow_split = s->follow_eval && !s->follow_many && getenv_flag("KCEP_FOLLOW_MASK_SPLIT");
  s->follow_next = s->follow_many ? P.follow_many_next : s->follow_eval ? P.follow_mask_next : P.follow_next;
  // (never null: a collect before any push reads its k)
  s->sp = follow ? (s->follow_many ? &P.follow_many : s->follow_eval ? &P.follow_mask : &P.follow) : sp ? sp : &P.stencil;
  s->mask_pass = masked && (path == CEP_PATH_STENCIL || path == CEP_PATH_CHAIN);
  s->device = opts->device;
  auto cleanup = [&](int rc) {
    cep_session_close(s);
    return rc;
  };
  const int64_t cap = std::max<int64_t>(opts->max_events, 1);
  if (cap >= (int64_t(1) << 31)) return cleanup(fail(CEP_E_ARG, "max_events must be < 2^31 per batch"));
  if (s->scal.ensure(64) || hipMemset(s->scal.p, 0, 64)) return cleanup(fail(CEP_E_HIP, "device allocation failed"));
  if (follow) {
    // the rows of a stencil session without carry (a start completes at most once: cap rows), and the
    // bitmaps of follow.hip for a batch of max_events
    const StencilProgram& FP = *s->sp;
    const size_t nt = size_t(follow_tiles(cap)), planes = size_t(FP.k) + 1;
    if (s->prog.ensure(sizeof(StencilProgram)) || s->total.ensure(64) || s->sum.ensure(64) ||
        (!carry && !s->follow_many && s->out.ensure(sizeof(int32_t) * size_t(FP.k) * size_t(cap))) ||
        // (a session of a pattern with oneOrMore stages writes the CSR too, and sums the walks' lengths per word)
        (s->follow_many && (s->fw_len.ensure(nt * 64 * 8) || s->fw_lpre.ensure(nt * 64 * 8))) ||
        s->fw_bits.ensure(planes * nt * 64 * 8) ||
        s->fw_sum.ensure(planes * nt * 8) || s->fw_tile.ensure(nt * 8) || s->fw_cnt.ensure(nt * 64 * 8) ||
        s->fw_pre.ensure(nt * 64 * 8) || s->scan_tmp.ensure((nt / 16 + 4) * 8) ||
        // (a carry session writes the runs path's CSR instead of rows, and keeps the open starts apart)
        (carry && (s->fw_open.ensure(nt * 64 * 8) || s->fw_ocnt.ensure(nt * 64 * 8) || s->fw_opre.ensure(nt * 64 * 8))))
      return cleanup(fail(CEP_E_HIP, "device allocation failed"));
    s->out_cap = cap;
    if (hipMemcpy(s->prog.p, &FP, sizeof(StencilProgram), hipMemcpyHostToDevice) || hipMemset(s->total.p, 0, s->total.cap))
      return cleanup(fail(CEP_E_HIP, "device init failed"));
    // the evaluated form: the slots' bytecode for the streaming kernel; the split form's mask column
    if (s->follow_eval &&
        (s->mprog.ensure(sizeof(MaskProgram)) ||
         (s->follow_split && s->mcol.ensure(sizeof(int32_t) * size_t((cap + 3) & ~int64_t(3)))) ||
         hipMemcpy(s->mprog.p, s->follow_many ? &P.follow_many_prog : &P.follow_mask_prog, sizeof(MaskProgram),
                   hipMemcpyHostToDevice)))
      return cleanup(fail(CEP_E_HIP, "device allocation failed"));
  }
  if (sp && path != CEP_PATH_GENERAL && !follow) {
    const int k = sp->k;
    const int64_t nt = stencil_tiles(cap);
    // a run ends at most once, so a batch has at most one match per start: its records, plus on chain
    // carry sessions the (at most K-1) starts in each batch key's halo
    const int64_t out_cap = carry && sp->chain ? cap + std::min<int64_t>(cap, opts->max_keys) * (k - 1) : cap;
    if (s->prog.ensure(sizeof(StencilProgram)) || s->status.ensure(sizeof(int64_t) * size_t(2 * nt + 2)) ||
        s->counter.ensure(sizeof(int64_t) * size_t(nt / 1024 + 4)) || s->total.ensure(64) || s->sum.ensure(64) ||
        s->out.ensure(sizeof(int32_t) * size_t(k) * size_t(out_cap)) ||
        // (+ one super-tile of ints: a last, partial super-tile's aux bytes lie past its tiles' ints;
        // + the plain kernel's dense region, launch.h ST_SLOT_DENSE_ALLOC ints per tile)
        s->slots.ensure(sizeof(int32_t) * ((size_t(k) * size_t(nt) + 4) * 4096 +
                                           size_t(nt) * size_t(ST_SLOT_DENSE_ALLOC))))
      return cleanup(fail(CEP_E_HIP, "device allocation failed"));
    s->out_cap = out_cap;
    if (hipMemcpy(s->prog.p, sp, sizeof(StencilProgram), hipMemcpyHostToDevice) ||
        hipMemset(s->status.p, 0, s->status.cap) || hipMemset(s->counter.p, 0, s->counter.cap) ||
        hipMemset(s->total.p, 0, s->total.cap))
      return cleanup(fail(CEP_E_HIP, "device init failed"));
  }
  if (s->mask_pass) {
    if (s->mprog.ensure(sizeof(MaskProgram)) || s->mcol.ensure(sizeof(int32_t) * size_t((cap + 3) & ~int64_t(3))) ||
        hipMemcpy(s->mprog.p, &P.mask_prog, sizeof(MaskProgram), hipMemcpyHostToDevice))
      return cleanup(fail(CEP_E_HIP, "device allocation failed"));
  }
  if (P.general_ok) {
    if (s->dprog.ensure(sizeof(DevProgram)) ||
        hipMemcpy(s->dprog.p, &P.dev, sizeof(DevProgram), hipMemcpyHostToDevice))
      return cleanup(fail(CEP_E_HIP, "device allocation failed"));
  }
  if (carry && (path == CEP_PATH_STENCIL || path == CEP_PATH_CHAIN)) {   // per key two halo slots, none written yet
    s->carry = true;
    if (s->halo.ensure(size_t(opts->max_keys) * sizeof(HaloHdr)) || s->hflags.ensure(16) ||
        s->hpos.ensure(size_t(opts->max_keys) * 2 * size_t(std::max(1, sp->k - 1)) * 8) ||
        hipMemset(s->halo.p, 0, size_t(opts->max_keys) * sizeof(HaloHdr)) || hipMemset(s->hflags.p, 0, 16))
      return cleanup(fail(CEP_E_HIP, "device allocation failed"));
  } else if (carry && (path == CEP_PATH_RUNS || follow)) {   // per key a carried tail (runs.hip) / its waiting walks
                                                             // (follow.hip), none yet
    s->carry = true;
    if (s->rtab.ensure(size_t(opts->max_keys) * 16) || s->rtop.ensure(8) || s->kstamp.ensure(size_t(opts->max_keys) * 4) ||
        hipMemset(s->rtab.p, 0, size_t(opts->max_keys) * 16) || hipMemset(s->rtop.p, 0, 8) ||
        hipMemset(s->kstamp.p, 0, size_t(opts->max_keys) * 4))
      return cleanup(fail(CEP_E_HIP, "device allocation failed"));
    if (tail_reserve(s, std::min<int64_t>(cap, int64_t(1) << 20), nullptr)) return cleanup(CEP_E_HIP);
  } else if (carry) {                            // NFAStore: no key has state yet
    s->carry = true;
    s->cpool_words = std::max<int64_t>(int64_t(1) << 20, opts->max_keys * 64);
    if (s->ctab.ensure(size_t(opts->max_keys) * 8) || s->cpool.ensure(size_t(s->cpool_words) * 4) ||
        hipMemset(s->ctab.p, 0xFF, size_t(opts->max_keys) * 8) || s->kstamp.ensure(size_t(opts->max_keys) * 4) ||
        hipMemset(s->kstamp.p, 0, size_t(opts->max_keys) * 4))
      return cleanup(fail(CEP_E_HIP, "device allocation failed"));
  }
  if (hipEventCreate(&s->ev0.e) || hipEventCreate(&s->ev1.e) || hipEventCreate(&s->eb0.e) || hipEventCreate(&s->eb1.e))
    return cleanup(fail(CEP_E_HIP, "event create failed"));
  // general path kernel: one key per wave (nfa_wave.h) where a key's live runs can multiply -- a stage
  // with an IGNORE edge (skip-till-next / skip-till-any, the C4 run explosion) -- else one key per
  // lane: keys of strict patterns hold a few runs, and a wave round costs a light key more than a
  // lane's walk (C3 on the general path: 342 vs 107 ms, profiles/r03_ab_c3_general_wave_lane.log).
  // CEP_SESSION_LANE_NFA / CEP_SESSION_WAVE_NFA choose explicitly.
  bool grows = false;
  for (const auto& st : P.stages)
    for (const auto& e : st.edges) grows = grows || e.op == E_IGNORE;
  bool wave = grows;
  if (opts->flags & CEP_SESSION_LANE_NFA) wave = false;
  else if (opts->flags & CEP_SESSION_WAVE_NFA) wave = true;
  s->wave = P.general_ok && wave;
  const char* env_jit = getenv("KCEP_JIT");
  s->jit_on = !(opts->flags & CEP_SESSION_INTERPRET) && !(env_jit && !strcmp(env_jit, "0"));
  if (s->jit_on && path == CEP_PATH_RUNS) s->jit = jit_runs(P, s->jit_why);   // on failure: built-in kernels
  if (s->jit_on && s->mask_pass) s->jitm = jit_masks(P, s->jit_why);        // on failure: the built-in kernel
  if (s->jit_on && s->follow_eval)
    s->jitm = s->follow_split ? jit_masks(P, s->jit_why, true) : jit_follow_bits(P, s->jit_why, s->follow_many);
  if (s->jit_on && path == CEP_PATH_GENERAL) {
    s->jitg = jit_general(P, s->jit_why, s->opts.flags & CEP_SESSION_PROFILE);
    s->jitg_tried = true;
  }
  *out = s;
  return CEP_OK;
}


void cep_session_close(cep_session* s) { delete s; }

int cep_session_path(const cep_session* s) { return s ? s->path : 0; }

int cep_live_run_hwm(const cep_session* s, int64_t* hwm) {
  if (!s || !hwm) return fail(CEP_E_ARG, "null argument");
  *hwm = s->last_path == CEP_PATH_GENERAL ? s->live_hwm : -1;
  return CEP_OK;
}

int cep_batch_errors(const cep_session* s, int64_t* records, int32_t* codes, int64_t cap, int64_t* n) {
  if (!s || !n) return fail(CEP_E_ARG, "null argument");
  *n = int64_t(s->e_rec.size());
  if (!records && !codes) return CEP_OK;
  if (cap < *n) return fail(CEP_E_ARG, "capacity below the error count");
  for (size_t i = 0; i < s->e_rec.size(); i++) {
    if (records) records[i] = s->e_rec[i];
    if (codes) codes[i] = s->e_code[i];
  }
  return CEP_OK;
}

int cep_key_profile(cep_session* s, int64_t* out, int64_t cap, int64_t* n_keys) {
  if (!s || !n_keys) return fail(CEP_E_ARG, "null argument");
  if (!(s->opts.flags & CEP_SESSION_PROFILE) || s->last_path != CEP_PATH_GENERAL)
    return fail(CEP_E_UNSUPPORTED, "key profiles need CEP_SESSION_PROFILE and a general-path batch");
  *n_keys = s->nseg;
  if (!out) return CEP_OK;
  constexpr int W = 1 + NFA_PROFILE_W;
  if (cap < W * s->nseg) return fail(CEP_E_ARG, "buffer too small");
  std::vector<int64_t> p(size_t(NFA_PROFILE_W * s->nseg)), start(size_t(s->nseg));
  std::vector<int32_t> keys(size_t(std::max<int64_t>(s->n, 1)));
  HIPCHECK(hipMemcpy(p.data(), s->r_prof.p, p.size() * 8, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(start.data(), s->seg.p, start.size() * 8, hipMemcpyDeviceToHost));
  if (s->n > 0) HIPCHECK(hipMemcpy(keys.data(), s->d_key, size_t(s->n) * 4, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < s->nseg; i++) {
    out[W * i] = keys[size_t(start[size_t(i)])];
    for (int j = 0; j < NFA_PROFILE_W; j++) out[W * i + 1 + j] = p[size_t(NFA_PROFILE_W * i + j)];
  }
  return CEP_OK;
}

int cep_session_jit(const cep_session* s) {
  if (!s) return 0;
  const bool masks = (s->mask_pass || s->follow_eval) && s->jitm;
  return (s->path == CEP_PATH_RUNS && s->jit) || (s->path == CEP_PATH_GENERAL && s->jitg) || masks ? 1 : 0;
}

int cep_session_wave(const cep_session* s) { return s && s->path == CEP_PATH_GENERAL && s->wave ? 1 : 0; }

int cep_batch_stopped(const cep_session* s, int64_t* keys, int64_t* records) {
  if (!s || !keys || !records) return fail(CEP_E_ARG, "null argument");
  if (s->last_path != CEP_PATH_GENERAL) return fail(CEP_E_UNSUPPORTED, "the last batch did not run on the general path");
  *keys = s->stopped_keys;
  *records = s->stopped_records;
  return CEP_OK;
}

int cep_batch_attempts(const cep_session* s) { return s && s->last_path == CEP_PATH_GENERAL ? s->last_attempts : 0; }

// the stencil / chain path has a compiled kernel only in its mask-pass form: the pre-pass
static bool mask_pass_path(const Program& P, int path) {
  return P.mask_ok && (path == CEP_PATH_STENCIL || path == CEP_PATH_CHAIN);   // (either names it, as at cep_session_open)
}
static int no_kernels(const Program& P, int path) {
  if ((path == CEP_PATH_STENCIL || path == CEP_PATH_CHAIN) && !P.mask_ok)
    return fail(CEP_E_UNSUPPORTED, "no compiled kernels for this path: mask pass does not apply: " + P.mask_why);
  return fail(CEP_E_UNSUPPORTED, "no compiled kernels for this path");
}

int cep_pattern_mask_pass(const cep_pattern* p, int32_t* k, int32_t* chain) {
  if (!p) return fail(CEP_E_ARG, "null argument");
  const Program& P = p->prog;
  if (!P.mask_ok) return fail(CEP_E_UNSUPPORTED, "mask pass does not apply: " + P.mask_why);
  if (k) *k = P.mask_stencil.k;
  if (chain) *chain = P.mask_stencil.chain;
  return CEP_OK;
}

int cep_pattern_follow(const cep_pattern* p, int32_t* k, uint32_t* next_mask) {
  if (!p) return fail(CEP_E_ARG, "null argument");
  const Program& P = p->prog;
  if (!P.follow_ok) return fail(CEP_E_UNSUPPORTED, "follow path does not apply: " + P.follow_why);
  if (k) *k = P.follow.k;
  if (next_mask) *next_mask = P.follow_next;
  return CEP_OK;
}

int cep_pattern_follow_mask(const cep_pattern* p, int32_t* k, uint32_t* next_mask) {
  if (!p) return fail(CEP_E_ARG, "null argument");
  const Program& P = p->prog;
  if (!P.follow_mask_ok) return fail(CEP_E_UNSUPPORTED, "follow path's evaluated form does not apply: " + P.follow_mask_why);
  if (k) *k = P.follow_mask.k;
  if (next_mask) *next_mask = P.follow_mask_next;
  return CEP_OK;
}

int cep_pattern_follow_many(const cep_pattern* p, int32_t* k, uint32_t* next_mask, uint32_t* many_mask, int32_t* evaluated) {
  if (!p) return fail(CEP_E_ARG, "null argument");
  const Program& P = p->prog;
  if (!P.follow_many_ok) return fail(CEP_E_UNSUPPORTED, "follow path with oneOrMore stages does not apply: " + P.follow_many_why);
  if (k) *k = P.follow_many.k;
  if (next_mask) *next_mask = P.follow_many_next;
  if (many_mask) *many_mask = P.follow_many_mask;
  if (evaluated) *evaluated = P.follow_many_eval ? 1 : 0;
  return CEP_OK;
}

int cep_pattern_kernel_source(const cep_pattern* p, int path, char* buf, size_t cap, size_t* needed) {
  if (!p || !needed) return fail(CEP_E_ARG, "null argument");
  const bool runs = path == CEP_PATH_RUNS && p->prog.runs_ok, general = path == CEP_PATH_GENERAL && p->prog.general_ok;
  const bool masks = mask_pass_path(p->prog, path);
  const bool fmany = p->prog.follow_many_ok && p->prog.follow_many_eval;   // ... with oneOrMore stages
  const bool fbits = path == CEP_PATH_FOLLOW && (p->prog.follow_mask_ok || fmany);   // the follow path's evaluated form
  if (!runs && !general && !masks && !fbits) return no_kernels(p->prog, path);
  std::string why;
  const std::string src = fbits   ? jit_source_follow_bits(p->prog, why, fmany)
                          : masks ? jit_source_masks(p->prog, why)
                          : runs  ? jit_source_runs(p->prog, why)
                                  : jit_source_general(p->prog, why);
  if (src.empty()) return fail(CEP_E_UNSUPPORTED, "kernel generation failed: " + why);
  *needed = src.size() + 1;
  if (!buf) return CEP_OK;
  if (cap < *needed) return fail(CEP_E_ARG, "buffer too small");
  memcpy(buf, src.c_str(), src.size() + 1);
  return CEP_OK;
}

int cep_pattern_build_kernels(const cep_pattern* p, int path) {
  if (!p) return fail(CEP_E_ARG, "null argument");
  const bool runs = path == CEP_PATH_RUNS && p->prog.runs_ok, general = path == CEP_PATH_GENERAL && p->prog.general_ok;
  const bool masks = mask_pass_path(p->prog, path);
  const bool fbits = path == CEP_PATH_FOLLOW && (p->prog.follow_mask_ok || (p->prog.follow_many_ok && p->prog.follow_many_eval));
  if (!runs && !general && !masks && !fbits) return no_kernels(p->prog, path);
  std::string why;
  if (!(fbits   ? jit_check_follow_bits(p->prog, why)
        : masks ? jit_check_masks(p->prog, why)
        : runs  ? jit_check_runs(p->prog, why)
                : jit_check_general(p->prog, why)))
    return fail(CEP_E_UNSUPPORTED, "kernel build failed: " + why);
  return CEP_OK;
}

static int push_dispatch(cep_session* s, const cep_batch* b, hipStream_t st, bool stencil_batch);
int cep_push_batch(cep_session* s, const cep_batch* b, void* stream) {
  if (!s || !b) return fail(CEP_E_ARG, "null argument");
  static const char* const kRange[] = {"cep_push_batch", "cep_push_batch:stencil", "cep_push_batch:general",
                                       "cep_push_batch:chain", "cep_push_batch:runs", "cep_push_batch:follow"};
  RoctxRange range(kRange[s->path >= 1 && s->path <= 5 ? s->path : 0]);
  const Program& P = s->pat->prog;
  if (b->n < 0 || b->n > s->opts.max_events) return fail(CEP_E_ARG, "batch larger than the session capacity");
  if (b->n > 0 && !b->key_id) return fail(CEP_E_ARG, "key_id is required");
  if (b->n_cols != int32_t(P.coltypes.size())) return fail(CEP_E_ARG, "column count does not match the pattern schema");
  for (int c = 0; c < b->n_cols; c++)
    if (b->n > 0 && !b->cols[c]) return fail(CEP_E_ARG, "null value column");
  // records the processor would drop (null key/value, re-delivered offsets)
  // break contiguity: the stencil only takes batches without them
  // CEP_BATCH_FILTER: the library drops them itself (filter.hip) and the session's own path takes the rest;
  // the general path applies both rules already, there the flag does nothing
  const bool filtered = (b->flags & CEP_BATCH_FILTER) && s->carry && s->path != CEP_PATH_GENERAL;
  const bool stencil_batch = filtered || (!b->valid && !(s->opts.mode == CEP_MODE_PROCESSOR && b->offset &&
                                                         !(b->flags & CEP_BATCH_OFFSETS_MONOTONE)));
  // (rejected before any session state changes: cep_batch_id and the last batch's CSR stand)
  if ((b->flags & CEP_BATCH_ARRIVAL_ORDER) && !s->carry)
    return fail(CEP_E_UNSUPPORTED, "CEP_BATCH_ARRIVAL_ORDER needs a CEP_SESSION_CARRY session");
  if ((b->flags & CEP_BATCH_FILTER) && !s->carry)
    return fail(CEP_E_UNSUPPORTED, "CEP_BATCH_FILTER needs a CEP_SESSION_CARRY session");
  if ((b->flags & CEP_BATCH_STOP_AT_ERROR) && s->path != CEP_PATH_GENERAL && stencil_batch) {
    static const char* const kPath[] = {"", "stencil", "", "chain", "runs", "follow"};
    return fail(CEP_E_UNSUPPORTED, std::string("CEP_BATCH_STOP_AT_ERROR is for general-path batches: this batch runs on "
                                               "the ") + kPath[s->path >= 1 && s->path <= 5 ? s->path : 0] +
                                       " path (bounded work per record, no runaway keys)");
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  HIPCHECK(hipSetDevice(s->device));
  s->stream = st;
  s->n = b->n;
  s->push_id++;
  s->pending = true;
  s->collected = false;
  s->e_rec.clear();
  s->e_code.clear();
  if (s->timing) HIPCHECK(hipEventRecord(s->eb0, st));
  s->h2d_wait = false;
  s->delivered = false;
  s->zc_slot = -1;
  s->cur_pos = nullptr;
  s->last_gpos = nullptr;
  int rc = CEP_OK;
  const bool arrival = (b->flags & CEP_BATCH_ARRIVAL_ORDER) && b->n > 0;
  s->arrival_n = arrival ? b->n : 0;
  cep_batch gb;
  const void* gcols[16] = {};
  const int64_t base0 = s->base;
  if (filtered && b->n > 0) {                      // [group ->] filter -> the path, over the admitted records
    cep_batch fb;
    const void* fcols[16] = {};
    if (arrival) rc = group_batch(s, b, st, gb, gcols);
    if (!rc) rc = filter_batch(s, arrival ? &gb : b, st, fb, fcols);
    if (!rc) rc = push_dispatch(s, &fb, st, true);
    if (!rc) {
      // the path took the batch: its marks are committed with it, and the dropped records' positions stay used
      if (filter_commit_launch(s->f_args, b->n, st) != hipSuccess) rc = fail(CEP_E_HIP, "filter_commit launch failed");
      s->base = base0 + b->n;
    }
    if (!rc && arrival && csr_batch(s)) rc = arrival_csr(s, base0, b->n, st);
    s->cur_pos = nullptr;
  } else if (arrival) {
    rc = group_batch(s, b, st, gb, gcols);
    if (!rc) rc = push_dispatch(s, &gb, st, stencil_batch);
    if (!rc && csr_batch(s)) rc = arrival_csr(s, base0, b->n, st);
    s->cur_pos = nullptr;
  } else {
    rc = push_dispatch(s, b, st, stencil_batch);
  }
  if (s->zc_slot >= 0) {                           // the ring slot is free again once the kernels are done
    HIPCHECK(hipEventRecord(s->ring_ev[s->zc_slot], st));
    s->zc_slot = -1;
  }
  if (s->h2d_wait) {                               // the caller's pinned columns are borrowed only for the call
    s->h2d_wait = false;
    HIPCHECK(hipEventSynchronize(s->h2d_ev));
  }
  return rc;
}

static int push_dispatch(cep_session* s, const cep_batch* b, hipStream_t st, bool stencil_batch) {
  const Program& P = s->pat->prog;
  if (s->path == CEP_PATH_RUNS && stencil_batch) {
    s->last_path = CEP_PATH_RUNS;
    return push_runs(s, b, st);
  }
  if (s->path == CEP_PATH_FOLLOW && stencil_batch) {
    s->last_path = CEP_PATH_FOLLOW;
    return push_follow(s, b, st);
  }
  if (s->path != CEP_PATH_GENERAL && s->path != CEP_PATH_RUNS && s->path != CEP_PATH_FOLLOW && stencil_batch) {
    s->last_path = s->path;
    return push_stencil(s, b, st);
  }
  if (s->carry && (s->path == CEP_PATH_STENCIL || s->path == CEP_PATH_CHAIN))   // the halo cannot be carried through the general path
    return fail(CEP_E_UNSUPPORTED, "a stencil carry session takes batches without null records (valid) and with "
                                   "per-key increasing offsets (CEP_BATCH_OFFSETS_MONOTONE)");
  if (s->carry && s->path == CEP_PATH_RUNS)      // nor the runs path's carried tails
    return fail(CEP_E_UNSUPPORTED, "a runs carry session takes batches without null records (valid) and with "
                                   "per-key increasing offsets (CEP_BATCH_OFFSETS_MONOTONE)");
  if (s->carry && s->path == CEP_PATH_FOLLOW)    // nor the follow path's carried walks
    return fail(CEP_E_UNSUPPORTED, "a follow carry session takes batches without null records (valid) and with "
                                   "per-key increasing offsets (CEP_BATCH_OFFSETS_MONOTONE)");
  if (!P.general_ok)
    return fail(CEP_E_UNSUPPORTED, "batch needs the general NFA path, which this pattern cannot use: " + P.general_why);
  s->last_path = CEP_PATH_GENERAL;
  return push_general(s, b, st);
}

const int64_t* cep_device_match_count(const cep_session* s) {
  if (!s) return nullptr;
  // general, runs and follow carry batches keep the count where their compaction scan left it
  return csr_batch(s) ? s->scal.as<int64_t>() + 3 : s->total.as<int64_t>();
}

int cep_match_count_to(const cep_session* s, int64_t* dst, void* stream) {
  if (!s || !dst) return fail(CEP_E_ARG, "null argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  HIPCHECK(hipSetDevice(s->device));
  if (s->n == 0 || s->last_path == 0) HIPCHECK(hipMemsetAsync(dst, 0, 8, st));
  else HIPCHECK(hipMemcpyAsync(dst, cep_device_match_count(s), 8, hipMemcpyDeviceToDevice, st));
  return CEP_OK;
}

int cep_session_set_timing(cep_session* s, int on) {
  if (!s) return fail(CEP_E_ARG, "null argument");
  s->timing = on != 0;
  return CEP_OK;
}

int cep_last_kernel_ms(cep_session* s, float* ms) {
  if (!s || !ms) return fail(CEP_E_ARG, "null argument");
  if (!s->timing) return fail(CEP_E_UNSUPPORTED, "timing is off (cep_session_set_timing)");
  HIPCHECK(hipEventSynchronize(s->ev1));
  HIPCHECK(hipEventElapsedTime(ms, s->ev0, s->ev1));
  return CEP_OK;
}

int cep_last_batch_ms(cep_session* s, float* ms) {
  if (!s || !ms) return fail(CEP_E_ARG, "null argument");
  if (!s->timing) return fail(CEP_E_UNSUPPORTED, "timing is off (cep_session_set_timing)");
  HIPCHECK(hipEventSynchronize(s->eb1));
  HIPCHECK(hipEventElapsedTime(ms, s->eb0, s->eb1));
  return CEP_OK;
}

// A device-written CSR is checked before any host code walks it: a device bug then fails the call with
// CEP_E_HIP instead of crashing the JVM or Python process (the reference fails the task with an exception,
// SharedVersionedBufferStoreImpl.java:113-115, never with a crash).
int cep_csr_check(const cep_matches* m, int64_t n_records, int32_t n_names) {
  if (!m) return fail(CEP_E_ARG, "null argument");
  const int64_t nm = m->n_matches, ne = m->n_entries;
  if (nm < 0 || ne < 0) return fail(CEP_E_HIP, "device CSR inconsistent: negative counts");
  if (nm == 0) return ne == 0 && (!m->ent_off || m->ent_off[0] == 0) ? CEP_OK
                                                                   : fail(CEP_E_HIP, "device CSR inconsistent: entries without matches");
  if (!m->match_record || !m->ent_off || (ne > 0 && (!m->ent_name || !m->ent_record)))
    return fail(CEP_E_HIP, "device CSR inconsistent: missing arrays");
  if (m->ent_off[0] != 0 || m->ent_off[nm] != ne) return fail(CEP_E_HIP, "device CSR inconsistent: entry offsets' ends");
  bool bad = false;
  for (int64_t i = 0; i < nm; i++)
    bad |= m->ent_off[i + 1] < m->ent_off[i] || uint64_t(m->match_record[i]) >= uint64_t(n_records);
  if (bad) return fail(CEP_E_HIP, "device CSR inconsistent: entry offsets or match records out of range");
  for (int64_t e = 0; e < ne; e++)
    bad |= uint64_t(m->ent_record[e]) >= uint64_t(n_records) || uint32_t(m->ent_name[e]) >= uint32_t(n_names);
  if (bad) return fail(CEP_E_HIP, "device CSR inconsistent: entry records or stage names out of range");
  return CEP_OK;
}

// A delivered batch (CEP_BATCH_DELIVER) from host buffer `slot`, stamped `want`: spin until the delivery
// kernel has stamped it, then the host CSR.  latest: the last pushed batch (matches past the host buffer are
// still in the device arrays)
static int collect_delivered(cep_session* s, int slot, int64_t want, bool latest, cep_matches* o) {
  {
    const StencilProgram& SP = *s->sp;
    const int k = SP.k;
    int64_t* hdr;
    int32_t* hkey;
    int64_t* hpos;
    dl_layout(s, slot, hdr, hkey, hpos);
    // the delivery kernel's last workgroup stamps hdr[2] once every row is in host memory: spin on it (a
    // stream wait sleeps and wakes microseconds late); a stamp that does not come -- a fault -- is left
    // to the stream wait, which reports it
    const volatile int64_t* stamp = hdr + 2;
    const auto t0 = std::chrono::steady_clock::now();
    while (*stamp != want) {
      if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) {
        HIPCHECK(hipStreamSynchronize(s->stream));
        if (*stamp != want) return fail(CEP_E_HIP, "the delivery kernel did not complete");
        break;
      }
      __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    const int64_t nm = hdr[0];
    const uint64_t hf = uint64_t(hdr[1]);
    if (hf & 1) return fail(CEP_E_ARG, "carry sessions need key ids in [0, max_keys)");
    if (hf & 2) return fail(CEP_E_ARG, "carry batch is not grouped by key: a key has two segments");
    if (hf & 4) return fail(CEP_E_RUN_CAPACITY, "chain carry batch: more runs completing in one tile than its match space");
    if (nm > s->out_cap) return fail(CEP_E_RUN_CAPACITY, "match output exceeded the session capacity");
    const int64_t nh = std::min(nm, s->dl_cap);
    if (nm > nh && !latest)                        // the rest was on the device, which a later push reused
      return fail(CEP_E_UNSUPPORTED, "a batch with more matches than the host delivery buffer is collected only "
                                     "before the next push");
    std::vector<int64_t> rest_pos;
    std::vector<int32_t> rest_key;
    if (nm > nh) {                                 // past the host buffer: from the device arrays
      rest_pos.resize(size_t(nm - nh) * k);
      rest_key.resize(size_t(nm - nh));
      HIPCHECK(hipMemcpy(rest_pos.data(), s->opos.as<int64_t>() + nh * k, rest_pos.size() * 8, hipMemcpyDeviceToHost));
      HIPCHECK(hipMemcpy(rest_key.data(), s->mkey.as<int32_t>() + nh, rest_key.size() * 4, hipMemcpyDeviceToHost));
    }
    s->match_record.resize(size_t(nm));
    s->match_key.resize(size_t(nm));
    s->ent_off.resize(size_t(nm) + 1);
    s->ent_name.resize(size_t(nm) * k);
    s->ent_record.resize(size_t(nm) * k);
    int64_t ne = 0;
    for (int64_t m = 0; m < nm; m++) {             // peek traversal order: final stage first
      const int64_t* p = m < nh ? hpos + m * k : rest_pos.data() + (m - nh) * k;
      s->match_key[size_t(m)] = m < nh ? hkey[m] : rest_key[size_t(m - nh)];
      s->match_record[size_t(m)] = p[k - 1];
      s->ent_off[size_t(m)] = ne;
      for (int i = k - 1; i >= 0; i--) {
        if (p[i] == -1) continue;                   // a skipped optional stage
        s->ent_name[size_t(ne)] = SP.name[i];
        s->ent_record[size_t(ne)] = p[i];
        ne++;
      }
    }
    s->ent_off[size_t(nm)] = ne;
    s->ent_name.resize(size_t(ne));
    s->ent_record.resize(size_t(ne));
    o->n_matches = nm;
    o->n_entries = ne;
    o->path = s->last_path;
    o->err = CEP_OK;
    o->err_record = -1;
  }
  return CEP_OK;
}

int cep_collect(cep_session* s, cep_matches* o) {
  if (!s || !o) return fail(CEP_E_ARG, "null argument");
  RoctxRange range("cep_collect");
  memset(o, 0, sizeof *o);
  if (s->collected) {                              // nothing pushed since: the host CSR is current
    *o = s->last;
    if (o->err) g_err = "the reference NFA raises an exception on this batch";
    return CEP_OK;
  }
  HIPCHECK(hipSetDevice(s->device));
  if (csr_batch(s)) {
    HIPCHECK(hipStreamSynchronize(s->stream));
    const int64_t nm = s->g_matches, ne = s->g_entries;
    s->match_record.resize(size_t(nm));
    s->match_key.resize(size_t(nm));
    s->ent_off.resize(size_t(nm) + 1);
    s->ent_name.resize(size_t(ne));
    s->ent_record.resize(size_t(ne));
    if (nm > 0) {
      HIPCHECK(hipMemcpy(s->match_record.data(), s->o_record.p, size_t(nm) * 8, hipMemcpyDeviceToHost));
      HIPCHECK(hipMemcpy(s->match_key.data(), s->o_key.p, size_t(nm) * 4, hipMemcpyDeviceToHost));
      HIPCHECK(hipMemcpy(s->ent_off.data(), s->o_entoff.p, size_t(nm) * 8, hipMemcpyDeviceToHost));
    }
    if (ne > 0) {
      HIPCHECK(hipMemcpy(s->ent_name.data(), s->o_name.p, size_t(ne) * 4, hipMemcpyDeviceToHost));
      HIPCHECK(hipMemcpy(s->ent_record.data(), s->o_entrec.p, size_t(ne) * 8, hipMemcpyDeviceToHost));
    }
    s->ent_off[size_t(nm)] = ne;
    o->n_matches = nm;
    o->n_entries = ne;
    o->path = s->last_path;
    o->err = s->g_err;
    o->err_record = s->g_err_rec;
    o->match_record = s->match_record.data();
    o->ent_off = s->ent_off.data();
    o->ent_name = s->ent_name.data();
    o->ent_record = s->ent_record.data();
    // records: the batch's (stream positions on carry sessions: everything pushed so far)
    int rc = cep_csr_check(o, s->carry ? s->base : s->n, int32_t(s->pat->prog.names.size()));
    if (rc) return rc;
    if (s->g_err) g_err = "the reference NFA raises an exception on this batch";
  } else if (s->delivered) {                       // CEP_BATCH_DELIVER: the device wrote the CSR's inputs
    int rc = collect_delivered(s, int(s->dl_stamp & 1), s->dl_stamp, true, o);
    if (rc) return rc;
  } else {
    const StencilProgram& SP = *s->sp;
    const int k = SP.k;
    int64_t nm = 0;
    if (s->pending && s->n > 0) HIPCHECK(hipMemcpyAsync(&nm, s->total.p, sizeof nm, hipMemcpyDeviceToHost, s->stream));
    HIPCHECK(hipStreamSynchronize(s->stream));
    if (nm > s->out_cap) return fail(CEP_E_RUN_CAPACITY, "match output exceeded the session capacity");
    s->out_host.resize(size_t(nm) * k);
    s->match_key.resize(size_t(nm));
    if (nm > 0) {
      if (s->mkey.ensure(size_t(nm) * 4)) return fail(CEP_E_HIP, "allocation failed");
      HIPCHECK(stencil_post(s->d_key, s->out.as<int32_t>(), k, nm, s->mkey.as<int32_t>(), s->prog.as<StencilProgram>(),
                            nullptr, s->stream));
      HIPCHECK(hipMemcpyAsync(s->out_host.data(), s->out.p, size_t(nm) * k * 4, hipMemcpyDeviceToHost, s->stream));
      HIPCHECK(hipMemcpyAsync(s->match_key.data(), s->mkey.p, size_t(nm) * 4, hipMemcpyDeviceToHost, s->stream));
      HIPCHECK(hipStreamSynchronize(s->stream));
    }
    // carry sessions: every entry as a stream position (halo entries from the keys' halos)
    std::vector<int64_t> pos_host;
    if (s->carry) {
      unsigned long long hf = 0;
      HIPCHECK(hipMemcpy(&hf, s->hflags.as<unsigned long long>() + (s->halo_stamp & 1), 8, hipMemcpyDeviceToHost));
      if (hf & 1) return fail(CEP_E_ARG, "carry sessions need key ids in [0, max_keys)");
      if (hf & 2) return fail(CEP_E_ARG, "carry batch is not grouped by key: a key has two segments");
      if (hf & 4) return fail(CEP_E_RUN_CAPACITY, "chain carry batch: more runs completing in one tile than its match space");
    }
    if (s->carry && nm > 0) {
      if (s->opos.ensure(size_t(nm) * k * 8)) return fail(CEP_E_HIP, "allocation failed");
      HIPCHECK(stencil_resolve_launch(s->d_key, s->out.as<int32_t>(), k, nm, carry_args(s), s->opos.as<int64_t>(),
                                      nullptr, nullptr, s->stream));
      pos_host.resize(size_t(nm) * k);
      HIPCHECK(hipMemcpyAsync(pos_host.data(), s->opos.p, pos_host.size() * 8, hipMemcpyDeviceToHost, s->stream));
      HIPCHECK(hipStreamSynchronize(s->stream));
    }
    // traversal order of SharedVersionedBufferStoreImpl.peek: final stage first;
    // chain matches carry -1 for the optional stages they skipped
    s->match_record.resize(size_t(nm));
    s->ent_off.resize(size_t(nm) + 1);
    s->ent_name.resize(size_t(nm) * k);
    s->ent_record.resize(size_t(nm) * k);
    int64_t ne = 0;
    for (int64_t m = 0; m < nm; m++) {
      s->match_record[m] = s->carry ? pos_host[m * k + k - 1] : s->out_host[m * k + k - 1];
      s->ent_off[m] = ne;
      for (int i = 0; i < k; i++) {
        const int st = k - 1 - i;
        const int32_t r = s->out_host[m * k + st];
        if (r == -1) continue;
        s->ent_name[ne] = SP.name[st];
        s->ent_record[ne] = s->carry ? pos_host[m * k + st] : r;
        ne++;
      }
    }
    s->ent_off[nm] = ne;
    s->ent_name.resize(size_t(ne));
    s->ent_record.resize(size_t(ne));
    o->n_matches = nm;
    o->n_entries = ne;
    o->path = s->last_path;
    o->err = CEP_OK;
    o->err_record = -1;
  }
  o->match_record = s->match_record.data();
  o->match_key = s->match_key.data();
  o->ent_off = s->ent_off.data();
  o->ent_name = s->ent_name.data();
  o->ent_record = s->ent_record.data();
  s->pending = false;
  s->collected = true;
  s->last = *o;
  return CEP_OK;
}

int64_t cep_batch_id(const cep_session* s) { return s ? s->push_id : -1; }

int32_t cep_filter_tile_records(void) { return FILTER_TF; }

int32_t cep_follow_tile_records(void) { return FOLLOW_TILE; }

// the delivery buffer holding batch `id`, or -1
static int delivered_slot(const cep_session* s, int64_t id) {
  for (int j = 0; j < 2; j++)
    if (s->dl[j] && s->dl_pid[j] == id) return j;
  return -1;
}

int cep_batch_ready(cep_session* s, int64_t id) {
  if (!s) return fail(CEP_E_ARG, "null argument");
  if (id < 1 || id > s->push_id) return fail(CEP_E_ARG, "no such batch");
  const int slot = delivered_slot(s, id);
  if (slot >= 0) {                                 // delivered: its stamp is in host memory once complete
    const int64_t want = s->dl_stamp - ((s->dl_stamp & 1) == slot ? 0 : 1);
    return *reinterpret_cast<const volatile int64_t*>(static_cast<int64_t*>(s->dl[slot].p) + 2) == want ? 1 : 0;
  }
  if (id < s->push_id) return 1;                   // (an earlier batch: the stream has moved past it, or will)
  const hipError_t e = hipStreamQuery(s->stream);
  if (e == hipErrorNotReady) return 0;
  if (e != hipSuccess) return fail(CEP_E_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(e));
  return 1;
}

int cep_collect_batch(cep_session* s, int64_t id, cep_matches* o) {
  if (!s || !o) return fail(CEP_E_ARG, "null argument");
  if (id == s->push_id) return cep_collect(s, o);
  const int slot = delivered_slot(s, id);
  if (slot < 0 || id != s->push_id - 1)
    return fail(CEP_E_ARG, "only the last batch, or the delivered batch before it, can be collected");
  RoctxRange range("cep_collect");
  memset(o, 0, sizeof *o);
  HIPCHECK(hipSetDevice(s->device));
  const int64_t want = s->dl_stamp - ((s->dl_stamp & 1) == slot ? 0 : 1);
  int rc = collect_delivered(s, slot, want, false, o);
  if (rc) return rc;
  o->match_record = s->match_record.data();
  o->match_key = s->match_key.data();
  o->ent_off = s->ent_off.data();
  o->ent_name = s->ent_name.data();
  o->ent_record = s->ent_record.data();
  s->collected = false;                            // the host CSR now holds the older batch
  return CEP_OK;
}

int cep_checksum(cep_session* s, uint64_t* sum, int64_t* n_matches) {
  if (!s || !sum) return fail(CEP_E_ARG, "null argument");
  HIPCHECK(hipSetDevice(s->device));
  if (csr_batch(s)) {
    cep_matches m;
    int rc = cep_collect(s, &m);
    if (rc) return rc;
    uint64_t h_all = 0;
    for (int64_t i = 0; i < m.n_matches; i++) {
      uint64_t h = mix64(uint64_t(m.match_record[i]) * 0x9e3779b97f4a7c15ULL);
      for (int64_t e = m.ent_off[i]; e < m.ent_off[i + 1]; e++)
        h = mix64(h ^ (uint64_t(m.ent_record[e]) << 8) ^ uint64_t(m.ent_name[e]));
      h_all += h;
    }
    *sum = h_all;
    if (n_matches) *n_matches = m.n_matches;
    return CEP_OK;
  }
  int64_t nm = 0;
  HIPCHECK(hipMemcpyAsync(&nm, s->total.p, sizeof nm, hipMemcpyDeviceToHost, s->stream));
  HIPCHECK(hipStreamSynchronize(s->stream));
  nm = std::min(nm, s->out_cap);
  HIPCHECK(hipMemsetAsync(s->sum.p, 0, 8, s->stream));
  const StencilProgram& SP = *s->sp;
  if (s->carry) {                                  // over stream positions
    if (s->opos.ensure(size_t(std::max<int64_t>(nm, 1)) * SP.k * 8)) return fail(CEP_E_HIP, "allocation failed");
    HIPCHECK(stencil_resolve_launch(s->d_key, s->out.as<int32_t>(), SP.k, nm, carry_args(s), s->opos.as<int64_t>(),
                                    s->prog.as<StencilProgram>(), s->sum.as<unsigned long long>(), s->stream));
  } else {
    HIPCHECK(stencil_post(s->d_key, s->out.as<int32_t>(), SP.k, nm, nullptr, s->prog.as<StencilProgram>(),
                          s->sum.as<unsigned long long>(), s->stream));
  }
  uint64_t h = 0;
  HIPCHECK(hipMemcpyAsync(&h, s->sum.p, 8, hipMemcpyDeviceToHost, s->stream));
  HIPCHECK(hipStreamSynchronize(s->stream));
  *sum = h;
  if (n_matches) *n_matches = nm;
  return CEP_OK;
}

}  // extern "C"
