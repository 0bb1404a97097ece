// launch.h -- every host-callable launch interface of the .hip files, declared once (argument structs,
// the constants callers size buffers by, the functions).  The .hip files that define them include it, so
// each definition is compiled against the declaration its callers see.
#pragma once
#include <algorithm>

#include "../../include/kcep.h"
#include "kcep_internal.h"

namespace kcep {

struct JitModule;   // jit.h

static inline unsigned blocks256(int64_t n) { return unsigned((std::max<int64_t>(n, 1) + 255) / 256); }

// CEP_BATCH_DELIVER on a carry session: where the device hands the batch's matches to the host
struct DeliverArgs {
  int64_t* hdr = nullptr;         // pinned host: {match count, this batch's error flags}; null: no delivery
  int32_t* hkey = nullptr;        // pinned host: key id per match (the first host_cap matches)
  int64_t* hpos = nullptr;        // pinned host: k stream positions per match
  int32_t* dkey = nullptr;        // device: the same past host_cap
  int64_t* dpos = nullptr;
  int64_t host_cap = 0;
  unsigned* ticket = nullptr;     // device: workgroups done (the last one stamps hdr[2] = stamp; reset to 0)
  int64_t stamp = 0;              // this delivery's number: cep_collect spins until hdr[2] holds it
  // CEP_BATCH_ARRIVAL_ORDER (group.hip): the rows delivered in arrival order of their completing record --
  // per arrival record its matches (a_cnt, zeroed by group_gather), their prefix (a_moff), its first match
  int64_t* a_cnt = nullptr;       // null: grouped order
  int32_t* a_head = nullptr;
  int64_t* a_moff = nullptr;
  int64_t* a_tot = nullptr;
  int64_t* a_tmp = nullptr;       // the scan's scratch
  int64_t a_n = 0;                // the batch's records
};
// CEP_BATCH_ARRIVAL_ORDER: an arrival-order batch grouped by key (group.hip)
struct GroupArgs {
  const int32_t* key;             // in: arrival order
  int32_t* g_key;                 // out: grouped (stable by key id)
  int32_t* arr;                   // out: arrival index of each grouped record
  int64_t* pos;                   // out: its stream position, base + arrival index
  int64_t base;
  const uint8_t* valid; uint8_t* g_valid;
  const int32_t* topic; int32_t* g_topic;
  const int32_t* partition; int32_t* g_partition;
  const int64_t* offset; int64_t* g_offset;
  const int64_t* ts; int64_t* g_ts;
  const void* cols[16]; void* g_cols[16];
  int32_t coltype[16];
  int32_t ncols;
  int64_t* cnt;                   // zeroed (n): the reorder's per-record match / entry counts
  int64_t* ecnt;
  // the grouping's state and scratch (group.hip)
  int32_t max_keys;
  uint32_t stamp;                 // this grouping's number (>= 1)
  unsigned long long* head;       // max_keys + 1 epoch-tagged list heads
  int32_t* node_top;
  int32_t *node_key, *node_chunk, *node_cnt, *node_next, *node_prefix, *node_leader, *rec_node, *rec_rank;
  int64_t* start;                 // per leader node: its key's first grouped position
  unsigned long long* cursor;     // the groups placed so far (zeroed once)
};
hipError_t group_launch(const GroupArgs& G, int64_t n, hipStream_t st);
hipError_t arrival_reorder(const int64_t* mrec, const int32_t* mkey, const int64_t* eoff, const int32_t* ename,
                           const int64_t* erec, int64_t nm, int64_t ne, int64_t base, int64_t n, int64_t* cnt,
                           int64_t* ecnt, int32_t* head, int64_t* moff, int64_t* moff_e, int64_t* tot, int64_t* tmp,
                           int64_t* o_rec, int32_t* o_key, int64_t* o_eoff, int32_t* o_name, int64_t* o_erec,
                           hipStream_t st);
hipError_t stencil_arrival_ranks(const int32_t* out, int k, const int64_t* total, int64_t out_cap, const int64_t* gpos,
                                 int64_t base, int64_t n, int64_t* cnt, int32_t* head, int64_t* moff, int64_t* tot,
                                 int64_t* tmp, hipStream_t st);
// ---- filter.hip: CEP_BATCH_FILTER, the null and high-water-mark rules on a key-grouped device batch ----
constexpr int FILTER_TF = 1024;                   // records per workgroup of the admission scan (a tile)
constexpr int FILTER_MAX_TOPICS = CEP_FILTER_MAX_TOPICS;   // marks per key: topic ids in [0, FILTER_MAX_TOPICS)
struct FilterArgs {
  // in: the batch (optional columns may be null); pos: its records' stream positions (null: base + index)
  const int32_t* key;
  const uint8_t* valid;
  const int32_t* topic;
  const int32_t* partition;
  const int64_t* offset;
  const int64_t* ts;
  const int64_t* pos;
  int64_t base;
  const void* cols[16];
  int32_t coltype[16];
  int32_t ncols;
  // out: the admitted records, compacted in order (a column the batch lacks is not written)
  int32_t *o_key, *o_topic, *o_partition;
  int64_t *o_offset, *o_ts, *o_pos;
  void* o_cols[16];
  // the marks: FILTER_MAX_TOPICS per key id (-1: never set); stage: the same shape, this batch's new ones
  int32_t use_marks;              // 0: only the null rule (CEP_MODE_NFA, or a batch without offsets)
  int32_t max_keys;
  int64_t* marks;
  int64_t* stage;
  // scratch: per tile a word / FILTER_MAX_TOPICS words / a count / an offset; per record (padded to tiles) a slot
  int32_t* tile_f;
  int64_t* tile_v;
  int32_t* tile_cnt;
  int64_t* tile_off;
  uint16_t* slot;
  int64_t* n_dev;                 // device: the admitted count
  int64_t* bad;                   // device: a valid record's topic id was out of range
  int64_t* host;                  // pinned host, by its device address: {admitted count, bad, stamp}
  int64_t stamp;                  // this batch's number: the host spins until host[2] holds it
};
hipError_t filter_launch(const FilterArgs& A, int64_t n, hipStream_t st);
hipError_t filter_commit_launch(const FilterArgs& A, int64_t n, hipStream_t st);

// The plain stencil kernel without carry stores a super-tile's first ST_DENSE matches (one int each)
// in a dense region at the head of the slot buffer (super-tile t at t * ST_DENSE) and the rest in
// the super-tile's own region after it (nsuper * ST_DENSE + t * sub * 4096 + m): the dense runs sit
// a few KB apart instead of 196 KB, C2 kernel -7.5 us (profiles/r04_ab_stencil_stores.txt).
constexpr int ST_DENSE = 512;
// What the session allocates per tile for that region, in ints, on top of the tiles' own slots.  Only
// ST_DENSE of it is addressed by the layout above (a super-tile is at least one tile); the rest is
// what a removed keyed dense layout needed, kept so that the allocation stays what it was.
constexpr int ST_SLOT_DENSE_ALLOC = 1280;
static_assert(ST_DENSE <= ST_SLOT_DENSE_ALLOC, "the dense region lies inside its allocation");

struct StencilLaunch {
  const int32_t* key;
  const void* val;
  const int32_t* topic;
  int64_t n;
  const StencilProgram* prog_dev;
  int k, coltype, use_topic, chain;
  int32_t* slots;                 // per-tile match slots, ST_TILE * k ints each (+ ST_SLOT_DENSE_ALLOC per tile, see above)
  int64_t* tile_count;            // matches per tile
  int64_t* tile_pre;              // their exclusive prefix
  int64_t* scan_tmp;
  int32_t* out;                   // contiguous output, k ints per match
  int64_t out_cap;                // matches
  int64_t* total;                 // device: number of matches
  StencilCarry carry;             // halo != nullptr: carry session
  int plain;                      // plain stencil (no carry, no chain, k <= 7): the keyless kernel (KCEP_STENCIL_KEYED=1: off)
  unsigned long long* clear_flag; // carry: the next batch's error-flag word, zeroed by the scan kernel (or null)
  DeliverArgs deliver;            // carry sessions' CEP_BATCH_DELIVER batches
  // the plain kernel without carry reads keys at its candidates only (stencil_kernel.h window_same_keys):
  // 0 each wave chooses, 1 every wave gathers (KCEP_STENCIL_SPARSE_KEYS=1), 2 every wave loads all its
  // keys (KCEP_STENCIL_DENSE_KEYS=1)
  int key_mode = 0;
  // the plain kernel without carry also stores each super-tile's count as a 16-bit word (a super-tile holds
  // at most 16384 matches): 16-B aligned, in the tile_pre region, which the one-launch finish
  // (stencil.hip stencil_finish_dense) does not use
  uint16_t* tile_count16 = nullptr;
  int split_finish = 0;           // KCEP_STENCIL_SPLIT_FINISH=1: tile_scan + stencil_gather_dense instead of that launch
};

// ---- carried tails of the runs path (CEP_SESSION_CARRY, runs.hip) ----
// the batch's columns as runs_carry_build reads them (device pointers; optional ones may be null)
struct RcIn {
  const int64_t* pos;                // stream positions of the batch's records (null: base + index)
  const int32_t* key;
  const int32_t* topic;
  const int32_t* partition;
  const int64_t* offset;
  const int64_t* ts;
  const void* cols[16];
};
// the extended batch: each key's carried tail, then its records of the batch; seg = batch segment
struct RcExt {
  int32_t *key, *topic, *partition, *seg;
  int64_t *offset, *ts, *pos;
  void* cols[16];
  int32_t coltype[16];
  int32_t ncols;
  int64_t cap;                       // records the arrays hold: writes past it are dropped (a batch with a key
                                     // in two segments gives that key's tail to both; it is rejected anyway)
};
hipError_t runs_carry_build(const RcIn& B, int64_t n, int64_t base, const int64_t* seg_flag, const int64_t* seg_idx,
                            const int64_t* seg_start, const int64_t* nseg, const int64_t* rtab, const int64_t* rpool,
                            int64_t* tlen, int64_t* toff, int64_t* total, int64_t* scan_tmp, const RcExt& X,
                            hipStream_t st, bool lens_only, int32_t max_keys);
hipError_t runs_carry_count(int64_t* out, int64_t nb, const int64_t* tails, int64_t cap, hipStream_t st);
hipError_t runs_carry_tails(const RcExt& X, int64_t ext_n, int64_t n, const int64_t* nseg, const int64_t* seg_start,
                            const int32_t* key, const int64_t* toff, const int32_t* end_of, unsigned long long* tstart,
                            int64_t* newlen, int64_t* noff, int64_t* new_total, int64_t* scan_tmp, int64_t* top,
                            int64_t* rpool, int64_t* rtab, hipStream_t st, const int64_t* ext_n_dev, const int64_t* bad);
hipError_t runs_carry_gc(int64_t* rtab, int64_t nkeys, int RW, const int64_t* src, int64_t* dst, int64_t* len,
                         int64_t* off, int64_t* total, int64_t* scan_tmp, hipStream_t st);

// ---- stencil.hip ----
hipError_t stencil_launch(const StencilLaunch& L, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st);
int64_t stencil_tiles(int64_t n);
hipError_t stencil_post(const int32_t* key, const int32_t* out, int k, int64_t nm, int32_t* mkey,
                        const StencilProgram* P, unsigned long long* sum, hipStream_t st);
hipError_t stencil_resolve_launch(const int32_t* key, const int32_t* out, int k, int64_t nm, const StencilCarry& C,
                                  int64_t* pos, const StencilProgram* P, unsigned long long* sum, hipStream_t st);
hipError_t stencil_deliver_launch(const int32_t* key, const int32_t* out, int k, const int64_t* total, int64_t out_cap,
                                  const StencilCarry& C, const DeliverArgs& D, hipStream_t st);

// ---- follow.hip: the follow path (CEP_PATH_FOLLOW), skip-till-next walks over per-slot bitmaps ----
constexpr int FOLLOW_TILE = 4096;                 // records per workgroup of follow_bits: 64 bitmap words
struct FollowArgs {
  const int32_t* key;
  const void* val;
  const int32_t* topic;
  int64_t n;
  const StencilProgram* prog_dev;   // the pattern's slots (Program::follow)
  int k, coltype, use_topic;
  uint32_t next_mask;               // bit s: slot s is skip-till-next (Program::follow_next)
  // per tile t = follow_tiles(n): bits (k + 1) x 64 t words (slot-major, then the key starts), sum (k + 1) x t
  // words (bit w % 64 of word w / 64: bits word w is not zero), tile_starts t words (slot 0's set bits)
  unsigned long long* bits;
  unsigned long long* sum;
  int64_t* tile_starts;
  int64_t* wcnt;                    // 64 t words: completed walks per word of slot 0's bitmap
  int64_t* wpre;                    // their exclusive prefix
  int64_t* scan_tmp;                // t / 16 + 4 words
  int64_t* nm;                      // device: completed walks
  unsigned long long* max_span;     // device: the longest last record - start
  unsigned long long* keys;         // the completed walks in start order, (last record << 31) | start
  // carry sessions (CEP_SESSION_FOLLOW_CARRY): the records' stream positions (pos, or null: base + index), the
  // plane of the starts whose walk is open at the batch end (64 t words), their count per word and its prefix
  const int64_t* pos;
  int64_t base;
  unsigned long long* open;
  int64_t* wopen;
  int64_t* wopre;
  int64_t* nopen;                   // device: open in-batch walks
  // CEP_SESSION_FOLLOW_MANY sessions: bit s of many_mask: slot s is a oneOrMore stage (Program::follow_many_mask);
  // the completed walks' entries per word of slot 0's bitmap (64 t words), their prefix, their sum
  uint32_t many_mask = 0;
  int64_t* wlen = nullptr;
  int64_t* wlpre = nullptr;
  int64_t* ne = nullptr;            // device: entries of the completed walks (K + the collected records each)
};
// The carried walks of a follow carry session (follow.hip): a walk is k int64 words -- slots taken s, the
// stream positions of its s records, zeros -- in the runs path's tail pool (rtab: offset and count per key,
// records of k words).  The batch's segments (nfa_segments), per segment its key's walks (tlen, prefix toff,
// n + 1 entries each), their number *ncw <= bound (the host's: every walk the pool holds).
struct FollowCarry {
  const int64_t* nseg;
  const int64_t* seg_start;
  const int64_t* seg_flag;
  const int64_t* seg_idx;
  int64_t nseg_cap;                 // segments the continuation table holds (min(n, max_keys): a valid batch's bound)
  const int64_t* tlen;
  const int64_t* toff;
  const int64_t* ncw;
  int64_t bound;
  int64_t* rtab;
  int64_t* rpool;
  int64_t* rtop;
  int32_t* res;                     // per (segment, slot 1..k-1) k ints: the continuation (follow_resume)
  int64_t *cw_done, *cw_open;       // per carried walk of the batch's keys: completed / still open (bound entries)
  int64_t *cw_dpre, *cw_opre;       // their exclusive prefixes
  int64_t *ncd, *nco;               // device: their totals
  int64_t* cd_x;                    // per completed carried walk: its number in the enumeration
  int64_t* scan_tmp;                // 2 x (max(64 t, bound) / 1024 + 1) words
};
// the counts of a carry batch before its one host synchronisation: the continuations, the carried walks
// classified and scanned, the in-batch walks counted (completed: A.nm, open: A.nopen) and scanned
hipError_t follow_carry_count_launch(const FollowArgs& A, const FollowCarry& C, hipStream_t st);
// the sort input (A.keys): the ncd completed carried walks, then the in-batch ones; the surviving carried
// walks appended to the pool at *rtop (room reserved by the caller)
hipError_t follow_carry_keys_launch(const FollowArgs& A, const FollowCarry& C, int64_t ncd, hipStream_t st);
// the CSR of the nm ordered matches; *total = nm
hipError_t follow_carry_rows_launch(const FollowArgs& A, const FollowCarry& C, const unsigned long long* sorted,
                                    int64_t nm, int64_t* match_record, int32_t* match_key, int64_t* ent_off,
                                    int32_t* ent_name, int64_t* ent_record, int64_t* total, hipStream_t st);
// the open in-batch walks appended behind their keys' surviving carried ones, the batch's keys' table
// entries, *rtop advanced
hipError_t follow_carry_state_launch(const FollowArgs& A, const FollowCarry& C, hipStream_t st);
int64_t follow_tiles(int64_t n);
hipError_t follow_bits_launch(const FollowArgs& A, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st);
// the evaluated form (follow_bits_dev.h): the same planes from the columns the slots read (M; M.mask unused),
// between the same events; jf: the per-pattern kernel, or null for the built-in one
hipError_t follow_eval_bits_launch(const MaskArgs& M, const FollowArgs& A, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st,
                                   hipFunction_t jf);
hipError_t follow_count_launch(const FollowArgs& A, hipStream_t st);
hipError_t follow_write_launch(const FollowArgs& A, hipStream_t st);
hipError_t follow_rows_launch(const FollowArgs& A, const unsigned long long* sorted, int64_t nm, int32_t* out,
                              int64_t* total, hipStream_t st);

// CEP_SESSION_FOLLOW_MANY (follow.hip "oneOrMore slots"): the count pass, which also sums the walks' lengths
// (A.wlen, A.wlpre, A.ne; scan_tmp: t / 8 + 2 words); the write pass; then per ordered match its length (len),
// their prefix (ent_off; *len_total their sum; scan_tmp: nm / 1024 + 1 words) and the runs path's CSR with batch
// indices as positions, *total = nm
hipError_t follow_many_count_launch(const FollowArgs& A, hipStream_t st);
hipError_t follow_many_write_launch(const FollowArgs& A, hipStream_t st);
hipError_t follow_many_rows_launch(const FollowArgs& A, const unsigned long long* sorted, int64_t nm, int64_t* len,
                                   int64_t* len_total, int64_t* match_record, int32_t* match_key, int64_t* ent_off,
                                   int32_t* ent_name, int64_t* ent_record, int64_t* total, hipStream_t st);

// ---- masks.hip: the mask pre-pass of CEP_SESSION_MASK_PASS sessions (jf: the per-pattern kernel, or null) ----
hipError_t masks_launch(const MaskArgs& A, hipStream_t st, hipFunction_t jf);

// ---- scan.hip: the device utilities every path shares ----
hipError_t exclusive_scan(const int64_t* in, int64_t n, int64_t* out, int64_t* total, int64_t* tmp, hipStream_t st);
hipError_t exclusive_scan_pair(const int64_t* in0, const int64_t* in1, int64_t n, const int64_t* n_dev, int64_t* out0,
                               int64_t* out1, int64_t* total0, int64_t* total1, int64_t* tmp, hipStream_t st);
hipError_t nfa_segments(const int32_t* key, int64_t n, int64_t* flag, int64_t* idx, int64_t* seg_start, int64_t* nseg,
                        int64_t* tmp, hipStream_t st);
hipError_t set_words_launch(int64_t* w, int n, int at, int64_t v, hipStream_t st);
hipError_t gather_words_launch(const int64_t* a, int na, const int64_t* b, int nb, int64_t* h, hipStream_t st);

// ---- nfa.hip ----
hipError_t nfa_launch(const NfaArgs& A, hipStream_t st, hipFunction_t jf);
hipError_t nfa_wave_launch(const NfaArgs& A, int64_t grid, hipStream_t st, const JitModule* j);
int64_t nfa_wave_grid(int64_t nseg, bool agg, const JitModule* j, bool stop);
hipError_t nfa_order_launch(const NfaArgs& A, int64_t nseg, uint8_t* bits, unsigned* bcnt, int32_t* order,
                            hipStream_t st, const JitModule* j, int lo);
// The schedule's estimate buckets (log2 of the segment weight) below this one keep arrival order
// behind the heavier ones: only a key that could end the grid late needs to start early, and every
// key moved forward adds scratch lines in flight beside the other heavy keys (C4, lowest ordered
// bucket 0 / 4 / 6 / 8 / 10: kernel 4.240 / 4.255 / 4.282 / 4.273 / 4.573 ms, kcep_nfa_wave
// 201.2 / 201.3 / 200.9 / 197.6 / 183.0 MB per launch; profiles/r05_c4_order_lo.txt)
constexpr int NFA_ORDER_LO = 8;
hipError_t nfa_compact_launch(int64_t nseg, const int64_t* nseg_dev, int64_t nm, int64_t ne, const int64_t* tot_dev,
                              const int32_t* key, const int64_t* seg_start, const int64_t* res_out, const int64_t* res_ent,
                              const int64_t* moff, const int64_t* eoff, int64_t* match_record, int32_t* match_key,
                              int64_t* ent_off, int32_t* ent_name, int64_t* ent_record, hipStream_t st);
hipError_t nfa_trim_launch(const NfaArgs& A, int64_t nseg, hipStream_t st);
hipError_t carry_commit_launch(int64_t nseg, const int32_t* key, const int64_t* seg_start, const int64_t* res_carry,
                               const int32_t* res_err, int64_t* ctab, const unsigned long long* stop_at, hipStream_t st);
hipError_t carry_keycheck_launch(int64_t max_seg, const int64_t* nseg, const int32_t* key, const int64_t* seg_start,
                                int32_t max_keys, int32_t* stamp, int32_t batch_no, unsigned long long* flags,
                                hipStream_t st);
hipError_t carry_sizes_launch(const int64_t* ctab, int64_t nkeys, const int32_t* cpool, int64_t* words,
                              hipStream_t st);
hipError_t carry_move_launch(int64_t* ctab, int64_t nkeys, const int32_t* src, const int64_t* off, int32_t* dst,
                             hipStream_t st);

// ---- runs.hip ----
hipError_t runs_sim_launch(const RunsArgs& A, int64_t* flag, int32_t* end_of, hipStream_t st, hipFunction_t jf);
hipError_t runs_expand_launch(const RunsArgs& R, const unsigned long long* sorted, int64_t nm, const int64_t* ent_off,
                              int64_t ne, int64_t* match_record, int32_t* match_key, int64_t* ent_off_out, int32_t* ent_name,
                              int64_t* ent_record, hipStream_t st);
hipError_t runs_compact_launch(const int64_t* stat, const int32_t* end_of, int64_t n, int32_t chunk, int64_t* pre,
                               unsigned long long* out, int64_t* tot_cnt, int64_t* tot_len, int64_t* scan_tmp,
                               hipStream_t st, int64_t n_grid);
int64_t runs_sim_waves(int64_t n, int32_t chunk);
bool runs_emit_scan(const int64_t* stat, int64_t n, int32_t chunk, int64_t* pre, int64_t* tot_cnt, int64_t* tot_len,
                    hipStream_t st, const int64_t* n_dev);
hipError_t runs_emit_launch(const RunsArgs& R, const int32_t* end_of, const int64_t* pre, int span, int64_t* match_record,
                            int32_t* match_key, int64_t* ent_off, int32_t* ent_name, int64_t* ent_record, hipStream_t st,
                            int64_t n_grid);
hipError_t runs_results_launch(const unsigned long long* ctl, const int64_t* nm, const int64_t* top, int64_t* h,
                               hipStream_t st, const int64_t* x);
hipError_t runs_order_launch(const unsigned long long* in, int64_t nm, int w, unsigned long long* out, int64_t* len,
                             hipStream_t st);
hipError_t runs_sort(const unsigned long long* in, unsigned long long* out, int64_t nm, int bits, void* tmp,
                     size_t* tmp_bytes, hipStream_t st);
hipError_t runs_write_launch(const RunsArgs& R, const unsigned long long* sorted, int64_t nm, int64_t* len,
                             int64_t* ent_off, int64_t* total, int64_t* scan_tmp, int64_t* match_record,
                             int32_t* match_key, int64_t* ent_off_out, int32_t* ent_name, int64_t* ent_record,
                             hipStream_t st, bool lengths_only, hipFunction_t jf);

}  // namespace kcep
