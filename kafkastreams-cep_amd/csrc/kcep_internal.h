// kcep_internal.h — compiled-pattern representation shared by the host
// compiler (compile.cpp) and the HIP kernels (stencil.hip, nfa.hip), and the carried halos of the
// stencil path.  The launch interfaces of the .hip files are in launch.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "kcep_dev.h"

#include <memory>
#include <string>
#include <vector>

namespace kcep {

struct Expr {
  uint8_t op = 0, t = 0, ct = 0;
  int32_t i32 = 0;
  int64_t i64 = 0;
  double f64 = 0;
  int col = 0, name = 0;
  std::string sname;                 // OP_SEQ_AGG: the stage name filter
  std::shared_ptr<Expr> a, b;
};
using ExprP = std::shared_ptr<Expr>;

struct Fold {
  int state;
  uint8_t type;
  ExprP expr;
};

struct PatternDef {                 // one select() of the DSL (pattern/Pattern.java)
  std::string name;
  int name_id = 0, level = 0;
  uint8_t strategy = S_STRICT;
  int32_t topic = -1;
  uint8_t one_or_more = 0, optional = 0;
  int32_t times = 1;
  int64_t window_ms = -1;
  ExprP pred;
  std::vector<Fold> folds;
};

struct EdgeDef {
  uint8_t op;
  ExprP pred;                       // nullptr = Matcher.TruePredicate
  int target;                       // stage id, -1 for IGNORE
};

struct StageDef {                   // nfa/Stage.java
  int id, name;
  uint8_t type;
  int64_t window_ms;
  int pattern;                      // index into patterns (aggregates), -1 for $final
  std::vector<EdgeDef> edges;
};

// ---- stencil (strict single-cardinality fast path) ----
constexpr int STENCIL_MAX_K = 8;
constexpr int STENCIL_MAX_TERMS = 6;
constexpr int STENCIL_MAX_ATOMS = 2;   // per term: one value-column range + one topic range

struct StencilAtomI { int64_t lo, hi; };
struct StencilAtomF { double lo, hi; };

// Predicate slot p (0..7): OR over terms of (value in [lo,hi] AND topic in [tlo,thi]).
// Slots 0..k-1 are the stage predicates (BEGIN edges, topic filter included).
// Chain patterns (strict with optional() stages, k <= 4) also use slot 4+i for
// the SKIP_PROCEED edge of optional stage i: the successor's predicate without
// its topic filter (StagesFactory.java:159-169); the edge is that AND NOT slot i.
constexpr int CHAIN_MAX_K = 4;
constexpr int STENCIL_LUT_MAX = 256;   // values a dense mask table spans at most
struct StencilProgram {
  int32_t k;
  int32_t col;                       // value column read by every predicate
  int32_t coltype;                   // T_I32 / T_I64 / T_F64
  int32_t use_topic;                 // 1 if any atom constrains the topic
  int32_t chain;                     // 1: some stage is optional (variable-length matches)
  int32_t optmask;                   // bit i: stage i is optional
  int32_t pslots;                    // bit p: predicate slot p is in use
  int32_t nterms[STENCIL_MAX_K];
  int32_t hasv[STENCIL_MAX_K][STENCIL_MAX_TERMS];   // 0: term does not constrain the value
  StencilAtomI vi[STENCIL_MAX_K][STENCIL_MAX_TERMS];
  StencilAtomF vf[STENCIL_MAX_K][STENCIL_MAX_TERMS];
  StencilAtomI tp[STENCIL_MAX_K][STENCIL_MAX_TERMS];
  int32_t name[STENCIL_MAX_K];       // stage name id of pattern s
  // Interval table: the breakpoints of every value/topic atom cut the value
  // (topic) axis into intervals on which each stage predicate is constant, so
  // a record's k-bit stage mask is table[it * 16 + iv] with iv = #{value
  // breakpoints <= v} and it = #{topic breakpoints <= topic}.
  int32_t nbp;                       // value breakpoints (<= 15), sorted ascending
  int32_t ntbp;                      // topic breakpoints (<= 3)
  int64_t bpi[15];                   // integer columns (clamped to int32 for i32 columns)
  double bpf[15];                    // double columns
  int32_t tbp[3];
  uint8_t table[64];
  uint8_t nan_mask[4];               // double columns: mask of a NaN value per topic interval
  // Dense form of the same table for integer columns without topic atoms whose breakpoints span
  // < STENCIL_LUT_MAX values (compile.cpp build_table): the mask of v is lut[clamp(v, lut_lo - 1,
  // lut_lo + lut_n) - (lut_lo - 1)], one clamp and one LDS read per record instead of nbp compares.
  // lut[0] = table[0] (below the range), lut[1 + r] = the mask of lut_lo + r, lut[1 + lut_n] =
  // table[nbp] (above); both clamp bounds are values of the column's type.  lut_n = 0: not used
  int64_t lut_lo;
  int32_t lut_n;
  uint8_t lut[STENCIL_LUT_MAX + 8];  // lut_n + 2 entries in use
};

struct Program {
  std::vector<uint8_t> coltypes;
  std::vector<PatternDef> pats;
  std::vector<StageDef> stages;
  std::vector<std::string> names;    // stage names, 0 = "$final"
  std::vector<std::string> states;   // aggregate state names
  std::vector<int> defined_states;   // Stages.getDefinedStates()
  int begin = -1;
  bool general_ok = false;
  std::string general_why;
  DevProgram dev{};
  bool stencil_ok = false;
  std::string stencil_why;           // reason the stencil path does not apply
  bool runs_ok = false;              // deterministic strict runs (compile.cpp analyse_runs)
  bool has_seq = false;              // some predicate or fold is a SequenceMatcher (OP_SEQ_*)
  std::string runs_why;
  StencilProgram stencil{};
  // mask-pass form (compile.cpp analyse_mask_pass; CEP_SESSION_MASK_PASS sessions): the structural
  // conditions of the stencil / chain path hold but the predicates do not lower to intervals of one
  // column, and every predicate slot is an event-only, total expression -- the slots as bytecode for the
  // pre-pass (masks.hip), and the stencil program that reads the mask column it writes
  bool mask_ok = false;
  std::string mask_why;
  StencilProgram mask_stencil{};
  MaskProgram mask_prog{};
  // follow form (compile.cpp analyse_follow; CEP_SESSION_FOLLOW sessions, CEP_PATH_FOLLOW): strict and
  // skip-till-next stages of cardinality ONE / times(n), each run one deterministic walk -- the expanded
  // slots lowered like stencil stages (k = slots, chain = 0), bit s of follow_next: slot s is skip-till-next
  bool follow_ok = false;
  std::string follow_why;
  StencilProgram follow{};
  uint32_t follow_next = 0;
  // evaluated follow form (compile.cpp analyse_follow_mask; sessions with CEP_SESSION_MASK_PASS and a follow
  // flag): the shape of the follow form, predicates its lowering does not take, every one event-only and
  // total -- the slots as bytecode for the streaming kernel (follow_bits_dev.h: a times(n) stage's n slots
  // share one code offset), and the program of k slots and their names the rest of the path reads (its
  // identity table serves follow_bits over a mask column, KCEP_FOLLOW_MASK_SPLIT=1)
  bool follow_mask_ok = false;
  std::string follow_mask_why;
  StencilProgram follow_mask{};
  MaskProgram follow_mask_prog{};
  uint32_t follow_mask_next = 0;
  // follow form with oneOrMore stages (compile.cpp analyse_follow_many; CEP_SESSION_FOLLOW_MANY sessions): the
  // follow shape with oneOrMore stages between the first and the last, each provably exclusive of its
  // successor -- a oneOrMore stage is one slot, bit s of follow_many_mask: slot s is one (a match holds every
  // record of the slot's plane between the slot's record and the next slot's).  follow_many: the slots lowered
  // directly, or (follow_many_eval) the program of the evaluated form with its bytecode in follow_many_prog
  bool follow_many_ok = false, follow_many_eval = false;
  std::string follow_many_why;
  StencilProgram follow_many{};
  MaskProgram follow_many_prog{};
  uint32_t follow_many_next = 0, follow_many_mask = 0;
};

// ---- carried state of the stencil / chain paths (CEP_SESSION_CARRY) ----
// A strict fixed-length match needs only the key's last K-1 records from earlier batches (SURVEY
// Q9): per key two slots (the batch that wrote it, its records oldest first: stage masks and
// stream positions).  A batch reads the newer slot written before it and writes the other one,
// so readers and the writer of one key never touch the same slot.  What a batch reads is one
// 32-byte header per key (both slots, dense by key id: consecutive keys of a batch share lines);
// the stream positions, written per batch and read only when a match reaches into the halo, sit
// in a separate dense array of (K-1) int64 per key and slot.
struct HaloHdr {
  int32_t stamp[2];                  // batch number that wrote slot s, 0 = never
  int32_t claim;                     // the last batch that had a segment of the key
  uint8_t cnt[2];                    // records held by slot s (<= K-1)
  uint8_t pad[2];
  uint64_t masks[2];                 // byte h of slot s: stage mask of its record h
};
static_assert(sizeof(HaloHdr) == 32, "HaloHdr is one 32-byte header per key");
struct StencilCarry {
  HaloHdr* hdr;                      // per key id
  int64_t* pos;                      // [(2 * key + slot) * km1 + h]: stream position of record h
  int32_t km1;                       // K - 1
  int32_t stamp;                     // this batch's number (>= 1)
  int32_t max_keys;
  int64_t base;                      // stream position of batch record 0
  unsigned long long* flags;         // bit 0: key id out of range, bit 1: a key in two segments,
                                     // bit 2: chain carry batch beyond a tile's match space
  const int64_t* gpos;               // stream position of each batch record (CEP_BATCH_ARRIVAL_ORDER: base + its
                                     // arrival index); null: base + record index
  int32_t grouped;                   // the device grouped the batch (CEP_BATCH_ARRIVAL_ORDER): each key is one
                                     // segment by construction, no claims (for an interleaved flush nearly every
                                     // record starts a segment, and its returning atomic was waited for in turn)
};
KCEP_HD inline int64_t halo_gpos(const StencilCarry& C, int64_t r) { return C.gpos ? C.gpos[r] : C.base + r; }
KCEP_HD inline int halo_old(const HaloHdr& h, int32_t stamp) {
  // the newer slot written before batch `stamp` (or an empty one)
  const int32_t a = h.stamp[0] < stamp ? h.stamp[0] : -1, b = h.stamp[1] < stamp ? h.stamp[1] : -1;
  return a >= b ? 0 : 1;
}

// compile.cpp
int lower_general(Program& P, std::string& why);
bool wave_stateful(const DevProgram& D);
int compile_ir(const uint8_t* ir, size_t len, Program& out, std::string& err);

}  // namespace kcep
