// state.cpp -- the carried state of CEP_SESSION_CARRY sessions (cep_state_*): the general path's per-key NFA
// blobs, the stencil path's halos, the runs path's tails and the follow path's walks; a blob in the reference's
// own terms.
#include <string.h>

#include "session.h"

using namespace kcep;

// ---- carried state (CEP_SESSION_CARRY) ----
// export format: "KCST", version 1, int64 next stream position, int32 key count,
// then per key: int32 key id, int32 words, the blob (kcep_internal.h CB_*)
namespace {
constexpr uint32_t kStateMagic = 0x5453434Bu;   // "KCST"
int need_carry(cep_session* s) {
  if (!s) return fail(CEP_E_ARG, "null argument");
  if (!s->carry) return fail(CEP_E_ARG, "the session was not opened with CEP_SESSION_CARRY");
  return CEP_OK;
}
// before the host reads or writes the session's device state: on its device, its stream drained
int drain(cep_session* s) {
  HIPCHECK(hipSetDevice(s->device));
  if (s->stream) HIPCHECK(hipStreamSynchronize(s->stream));
  return CEP_OK;
}

// ---- the high-water marks of stencil / chain / runs carry sessions (CEP_BATCH_FILTER, filter.hip) ----
// "KCSH" and "KCSR" blobs of version 2 end with a marks section behind their key entries: int32 count, then
// per mark int32 key id, int32 topic id, int64 mark.  Version 2 is written only when a covered key has a
// mark: a session that never took a filtered batch writes version 1, byte for byte as before.
constexpr int64_t kNoMark = -1;
// the marks of key ids [key_lo, key_hi) (empty: the session has no mark table yet)
int marks_download(cep_session* s, int32_t key_lo, int32_t key_hi, std::vector<int64_t>& m) {
  m.clear();
  if (!s->f_marks.p || key_hi <= key_lo) return CEP_OK;
  m.resize(size_t(key_hi - key_lo) * FILTER_MAX_TOPICS);
  HIPCHECK(hipMemcpy(m.data(), s->f_marks.as<int64_t>() + int64_t(key_lo) * FILTER_MAX_TOPICS, m.size() * 8,
                     hipMemcpyDeviceToHost));
  return CEP_OK;
}
// appends key k's marks (row: its FILTER_MAX_TOPICS table entries) as section triples; returns how many
int32_t marks_triples(const int64_t* row, int32_t k, std::vector<uint8_t>& out) {
  int32_t cnt = 0;
  for (int32_t t = 0; t < FILTER_MAX_TOPICS; t++) {
    if (row[t] == kNoMark) continue;
    const size_t at = out.size();
    out.resize(at + 16);
    memcpy(&out[at], &k, 4); memcpy(&out[at + 4], &t, 4); memcpy(&out[at + 8], &row[t], 8);
    cnt++;
  }
  return cnt;
}
// the marks section of keys [key_lo, key_hi): count + triples, or empty when none of them has a mark
int marks_section(cep_session* s, int32_t key_lo, int32_t key_hi, std::vector<uint8_t>& sec) {
  std::vector<int64_t> m;
  int rc = marks_download(s, key_lo, key_hi, m);
  if (rc) return rc;
  sec.assign(4, 0);
  int32_t cnt = 0;
  for (size_t i = 0; i * FILTER_MAX_TOPICS < m.size(); i++)
    cnt += marks_triples(&m[i * FILTER_MAX_TOPICS], key_lo + int32_t(i), sec);
  memcpy(&sec[0], &cnt, 4);
  if (!cnt) sec.clear();
  return CEP_OK;
}
// the section at p[at, len) checked: its triples' count, or -1
int64_t marks_parse(const uint8_t* p, size_t at, size_t len) {
  int32_t cnt;
  if (at + 4 > len) return -1;
  memcpy(&cnt, p + at, 4);
  if (cnt < 0 || at + 4 + 16 * size_t(cnt) > len) return -1;
  return cnt;
}
// a version 2 blob's marks section (behind the key entries, at `at`) into the session's table
int marks_import(cep_session* s, const uint8_t* p, size_t at, size_t len) {
  const int64_t cnt = marks_parse(p, at, len);
  if (cnt < 0) return fail(CEP_E_ARG, "truncated marks section in the state blob");
  struct Mark { int32_t k, t; int64_t v; };
  std::vector<Mark> ms(static_cast<size_t>(cnt));
  for (int64_t i = 0; i < cnt; i++) {
    Mark& m = ms[size_t(i)];
    memcpy(&m.k, p + at + 4 + 16 * size_t(i), 4); memcpy(&m.t, p + at + 8 + 16 * size_t(i), 4);
    memcpy(&m.v, p + at + 12 + 16 * size_t(i), 8);
    if (m.k < 0 || m.k >= s->opts.max_keys || m.t < 0 || m.t >= FILTER_MAX_TOPICS)
      return fail(CEP_E_ARG, "bad mark in the state blob");
  }
  if (!cnt) return CEP_OK;
  int rc = marks_ensure(s, s->stream);
  if (rc || (rc = drain(s))) return rc;
  if (cnt <= 256) {                                // a few keys (cep_state_import_keys): mark by mark
    for (const Mark& m : ms)
      HIPCHECK(hipMemcpy(s->f_marks.as<int64_t>() + int64_t(m.k) * FILTER_MAX_TOPICS + m.t, &m.v, 8, hipMemcpyHostToDevice));
    return CEP_OK;
  }
  std::vector<int64_t> tab;
  if ((rc = marks_download(s, 0, max_keys32(s), tab))) return rc;
  for (const Mark& m : ms) tab[size_t(m.k) * FILTER_MAX_TOPICS + size_t(m.t)] = m.v;
  HIPCHECK(hipMemcpy(s->f_marks.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
  return CEP_OK;
}

// stencil carry sessions: "KCSH", version 1 (2: with a marks section), int64 next stream position, int32 key
// count, then per key with a halo: int32 key id, int32 records, uint64 stage masks, int64 stream positions[records]
constexpr uint32_t kHaloMagic = 0x4853434Bu;   // "KCSH"
int halo_newest(const HaloHdr& h) { return h.stamp[1] > h.stamp[0] ? 1 : 0; }

int halo_export(cep_session* s, int32_t key_lo, int32_t key_hi, void* buf, size_t cap, size_t* needed) {
  const int km1 = s->sp->k - 1;
  const size_t nk = size_t(std::max(0, key_hi - key_lo));
  std::vector<HaloHdr> tab(nk);
  std::vector<int64_t> pos(nk * 2 * size_t(km1));
  if (nk) {
    HIPCHECK(hipMemcpy(tab.data(), s->halo.as<HaloHdr>() + key_lo, nk * sizeof(HaloHdr), hipMemcpyDeviceToHost));
    if (km1)
      HIPCHECK(hipMemcpy(pos.data(), s->hpos.as<int64_t>() + 2 * int64_t(key_lo) * km1, pos.size() * 8,
                         hipMemcpyDeviceToHost));
  }
  size_t bytes = 20;
  int32_t nkeys = 0;
  for (size_t i = 0; i < nk; i++) {
    const int sl = halo_newest(tab[i]);
    if (tab[i].stamp[sl] > 0 && tab[i].cnt[sl] > 0) { bytes += 16 + 8 * size_t(tab[i].cnt[sl]); nkeys++; }
  }
  std::vector<uint8_t> sec;
  if (int rc = marks_section(s, key_lo, key_hi, sec)) return rc;
  bytes += sec.size();
  *needed = bytes;
  if (!buf) return CEP_OK;
  if (cap < bytes) return fail(CEP_E_ARG, "export buffer too small");
  uint8_t* p = static_cast<uint8_t*>(buf);
  const uint32_t ver = sec.empty() ? 1 : 2;
  memcpy(p, &kHaloMagic, 4); memcpy(p + 4, &ver, 4); memcpy(p + 8, &s->base, 8); memcpy(p + 16, &nkeys, 4);
  p += 20;
  for (size_t i = 0; i < nk; i++) {
    const int sl = halo_newest(tab[i]);
    const int32_t cnt = tab[i].cnt[sl];
    if (tab[i].stamp[sl] <= 0 || cnt <= 0) continue;
    const int32_t k = key_lo + int32_t(i);
    memcpy(p, &k, 4); memcpy(p + 4, &cnt, 4); memcpy(p + 8, &tab[i].masks[sl], 8);
    memcpy(p + 16, &pos[(2 * i + size_t(sl)) * size_t(km1)], 8 * size_t(cnt));
    p += 16 + 8 * size_t(cnt);
  }
  if (!sec.empty()) memcpy(p, sec.data(), sec.size());
  return CEP_OK;
}

int halo_import(cep_session* s, const uint8_t* p, size_t len, uint32_t ver) {
  int64_t base;
  int32_t nkeys;
  memcpy(&base, p + 8, 8); memcpy(&nkeys, p + 16, 4);
  const int K = s->sp->k;
  struct Row { int32_t k, cnt; uint64_t masks; int64_t pos[STENCIL_MAX_K - 1]; };
  std::vector<Row> rows;
  size_t at = 20;
  if (s->halo_stamp == 0) s->halo_stamp = 1;     // imported slots count as written before the next batch
  for (int32_t i = 0; i < nkeys; i++) {
    if (at + 16 > len) return fail(CEP_E_ARG, "truncated state blob");
    Row r{};
    memcpy(&r.k, p + at, 4); memcpy(&r.cnt, p + at + 4, 4); memcpy(&r.masks, p + at + 8, 8);
    if (r.k < 0 || r.k >= s->opts.max_keys || r.cnt < 0 || r.cnt > K - 1 || at + 16 + 8 * size_t(r.cnt) > len)
      return fail(CEP_E_ARG, "bad key entry in the state blob");
    memcpy(r.pos, p + at + 16, 8 * size_t(r.cnt));
    rows.push_back(r);
    at += 16 + 8 * size_t(r.cnt);
  }
  if (ver == 2)
    if (int rc = marks_import(s, p, at, len)) return rc;
  if (int rc = drain(s)) return rc;
  for (auto& r : rows) {                         // slot 0 holds the halo, slot 1 is empty
    HaloHdr h{};
    h.stamp[0] = s->halo_stamp;
    h.claim = s->halo_stamp;
    h.cnt[0] = uint8_t(r.cnt);
    h.masks[0] = r.masks;
    HIPCHECK(hipMemcpy(s->halo.as<HaloHdr>() + r.k, &h, sizeof h, hipMemcpyHostToDevice));
    if (K > 1)
      HIPCHECK(hipMemcpy(s->hpos.as<int64_t>() + 2 * int64_t(r.k) * (K - 1), r.pos, 8 * size_t(K - 1),
                         hipMemcpyHostToDevice));
  }
  s->base = std::max(s->base, base);
  return CEP_OK;
}

// runs carry sessions: "KCSR", version 1, int64 next stream position, int32 key count, then per key with
// a tail: int32 key id, int32 records, int32 words per record (5 + ncols), int32 0, then the records
// (runs.hip tail records: stream position first)
constexpr uint32_t kTailMagic = 0x5253434Bu;   // "KCSR"
// follow carry sessions: "KCSW", the same layout over the same pool -- a record is one waiting walk of
// k words: slots taken s, the stream positions of its s records, zeros (follow.hip)
constexpr uint32_t kWalkMagic = 0x5753434Bu;   // "KCSW"
uint32_t tail_magic(const cep_session* s) { return walk_session(s) ? kWalkMagic : kTailMagic; }
int tail_download(cep_session* s, std::vector<int64_t>& tab, std::vector<int64_t>& pool) {
  tab.resize(size_t(s->opts.max_keys) * 2);
  pool.resize(size_t(s->rpool_used) * size_t(tail_rw(s)));
  HIPCHECK(hipMemcpy(tab.data(), s->rtab.p, tab.size() * 8, hipMemcpyDeviceToHost));
  if (!pool.empty()) HIPCHECK(hipMemcpy(pool.data(), s->rpool.p, pool.size() * 8, hipMemcpyDeviceToHost));
  return CEP_OK;
}
// appends key k's tail entry (key, records, words) to out; returns its record count
int64_t tail_entry(const cep_session* s, const std::vector<int64_t>& tab, const std::vector<int64_t>& pool, int32_t k,
                   std::vector<uint8_t>& out) {
  const int64_t L = tab[2 * size_t(k) + 1];
  if (L <= 0) return 0;
  const size_t RW = size_t(tail_rw(s)), at = out.size();
  const int32_t cnt = int32_t(L), rw = int32_t(RW), zero = 0;
  out.resize(at + 16 + size_t(L) * RW * 8);
  memcpy(&out[at], &k, 4); memcpy(&out[at + 4], &cnt, 4); memcpy(&out[at + 8], &rw, 4); memcpy(&out[at + 12], &zero, 4);
  memcpy(&out[at + 16], pool.data() + size_t(tab[2 * size_t(k)]) * RW, size_t(L) * RW * 8);
  return L;
}
int tail_export(cep_session* s, int32_t key_lo, int32_t key_hi, void* buf, size_t cap, size_t* needed) {
  std::vector<int64_t> tab, pool;
  int rc = tail_download(s, tab, pool);
  if (rc) return rc;
  std::vector<uint8_t> out(20);
  int32_t nkeys = 0;
  for (int32_t k = key_lo; k < key_hi; k++) nkeys += tail_entry(s, tab, pool, k, out) > 0;
  std::vector<uint8_t> sec;
  if ((rc = marks_section(s, key_lo, key_hi, sec))) return rc;
  out.insert(out.end(), sec.begin(), sec.end());
  const uint32_t ver = sec.empty() ? 1 : 2;
  const uint32_t magic = tail_magic(s);
  memcpy(&out[0], &magic, 4); memcpy(&out[4], &ver, 4); memcpy(&out[8], &s->base, 8); memcpy(&out[16], &nkeys, 4);
  *needed = out.size();
  if (!buf) return CEP_OK;
  if (cap < out.size()) return fail(CEP_E_ARG, "export buffer too small");
  memcpy(buf, out.data(), out.size());
  return CEP_OK;
}
int tail_import(cep_session* s, const uint8_t* p, size_t len, uint32_t ver) {
  int64_t base;
  int32_t nkeys;
  memcpy(&base, p + 8, 8); memcpy(&nkeys, p + 16, 4);
  const size_t RW = size_t(tail_rw(s));
  std::vector<std::pair<int32_t, size_t>> ents;
  size_t at = 20, recs = 0;
  for (int32_t i = 0; i < nkeys; i++) {
    if (at + 16 > len) return fail(CEP_E_ARG, "truncated state blob");
    int32_t k, cnt, rw;
    memcpy(&k, p + at, 4); memcpy(&cnt, p + at + 4, 4); memcpy(&rw, p + at + 8, 4);
    if (rw != int32_t(RW)) return fail(CEP_E_ARG, "state blob does not match this pattern");
    if (k < 0 || k >= s->opts.max_keys || cnt <= 0 || at + 16 + size_t(cnt) * RW * 8 > len)
      return fail(CEP_E_ARG, "bad key entry in the state blob");
    if (walk_session(s))                             // every walk's slot count names words of its own
      for (int32_t j = 0; j < cnt; j++) {
        int64_t sl;
        memcpy(&sl, p + at + 16 + size_t(j) * RW * 8, 8);
        if (sl < 1 || sl >= int64_t(RW)) return fail(CEP_E_ARG, "bad walk in the state blob");
      }
    ents.push_back({k, at});
    recs += size_t(cnt);
    at += 16 + size_t(cnt) * RW * 8;
  }
  if (ver == 2)
    if (int rc = marks_import(s, p, at, len)) return rc;
  if (int rc = drain(s)) return rc;
  int rc = tail_reserve(s, int64_t(recs), s->stream);
  if (rc) return rc;
  std::vector<int64_t> tab(size_t(s->opts.max_keys) * 2);
  HIPCHECK(hipMemcpy(tab.data(), s->rtab.p, tab.size() * 8, hipMemcpyDeviceToHost));
  std::vector<int64_t> words(recs * RW);
  int64_t w0 = 0;
  for (auto& e : ents) {
    int32_t cnt;
    memcpy(&cnt, p + e.second + 4, 4);
    memcpy(words.data() + size_t(w0) * RW, p + e.second + 16, size_t(cnt) * RW * 8);
    tab[2 * size_t(e.first)] = s->rpool_used + w0;
    tab[2 * size_t(e.first) + 1] = cnt;
    w0 += cnt;
  }
  if (recs) HIPCHECK(hipMemcpy(s->rpool.as<int64_t>() + size_t(s->rpool_used) * RW, words.data(), words.size() * 8,
                               hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(s->rtab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
  s->rpool_used += int64_t(recs);
  HIPCHECK(hipMemcpy(s->rtop.p, &s->rpool_used, 8, hipMemcpyHostToDevice));
  s->base = std::max(s->base, base);
  return CEP_OK;
}
}  // namespace

extern "C" {

int cep_state_export(cep_session* s, int32_t key_lo, int32_t key_hi, void* buf, size_t cap, size_t* needed) {
  int rc = need_carry(s);
  if (rc) return rc;
  if (!needed) return fail(CEP_E_ARG, "null argument");
  if ((rc = drain(s))) return rc;
  key_lo = std::max<int32_t>(key_lo, 0);
  key_hi = int32_t(std::min<int64_t>(key_hi, s->opts.max_keys));
  if (halo_session(s)) return halo_export(s, key_lo, key_hi, buf, cap, needed);
  if (tail_session(s)) return tail_export(s, key_lo, key_hi, buf, cap, needed);
  std::vector<int64_t> tab(size_t(std::max(0, key_hi - key_lo)));
  if (!tab.empty()) HIPCHECK(hipMemcpy(tab.data(), s->ctab.as<int64_t>() + key_lo, tab.size() * 8, hipMemcpyDeviceToHost));
  std::vector<int32_t> pool(size_t(s->cpool_used));
  if (!pool.empty()) HIPCHECK(hipMemcpy(pool.data(), s->cpool.p, pool.size() * 4, hipMemcpyDeviceToHost));
  size_t bytes = 20;
  int32_t nkeys = 0;
  for (int64_t o : tab)
    if (o >= 0) { bytes += 8 + size_t(pool[size_t(o) + CB_WORDS]) * 4; nkeys++; }
  *needed = bytes;
  if (!buf) return CEP_OK;
  if (cap < bytes) return fail(CEP_E_ARG, "export buffer too small");
  uint8_t* p = static_cast<uint8_t*>(buf);
  const uint32_t ver = 1;
  const int64_t at_pos = s->base - s->stop_uncommitted;
  memcpy(p, &kStateMagic, 4); memcpy(p + 4, &ver, 4); memcpy(p + 8, &at_pos, 8); memcpy(p + 16, &nkeys, 4);
  p += 20;
  for (size_t i = 0; i < tab.size(); i++) {
    if (tab[i] < 0) continue;
    const int32_t k = key_lo + int32_t(i), w = pool[size_t(tab[i]) + CB_WORDS];
    memcpy(p, &k, 4); memcpy(p + 4, &w, 4);
    memcpy(p + 8, pool.data() + tab[i], size_t(w) * 4);
    p += 8 + size_t(w) * 4;
  }
  return CEP_OK;
}

int cep_state_import(cep_session* s, const void* buf, size_t len) {
  int rc = need_carry(s);
  if (rc) return rc;
  if (!buf || len < 20) return fail(CEP_E_ARG, "bad state blob");
  const uint8_t* p = static_cast<const uint8_t*>(buf);
  uint32_t magic, ver;
  int64_t base;
  int32_t nkeys;
  memcpy(&magic, p, 4); memcpy(&ver, p + 4, 4); memcpy(&base, p + 8, 8); memcpy(&nkeys, p + 16, 4);
  if (halo_session(s)) {
    if (magic != kHaloMagic || (ver != 1 && ver != 2) || nkeys < 0)
      return fail(CEP_E_ARG, "bad state blob (stencil sessions take KCSH)");
    return halo_import(s, p, len, ver);
  }
  if (tail_session(s)) {
    if (magic != tail_magic(s) || (ver != 1 && ver != 2) || nkeys < 0)
      return fail(CEP_E_ARG, walk_session(s) ? "bad state blob (follow carry sessions take KCSW)"
                                             : "bad state blob (runs sessions take KCSR)");
    return tail_import(s, p, len, ver);
  }
  if (magic != kStateMagic || ver != 1 || nkeys < 0) return fail(CEP_E_ARG, "bad state blob");
  const DevProgram& D = s->pat->prog.dev;
  std::vector<std::pair<int32_t, size_t>> keys;    // key, byte offset of its blob
  size_t at = 20, words = 0;
  for (int32_t i = 0; i < nkeys; i++) {
    if (at + 8 > len) return fail(CEP_E_ARG, "truncated state blob");
    int32_t k, w;
    memcpy(&k, p + at, 4); memcpy(&w, p + at + 4, 4);
    if (k < 0 || k >= s->opts.max_keys || w < CB_HDR || at + 8 + size_t(w) * 4 > len)
      return fail(CEP_E_ARG, "bad key entry in the state blob");
    int32_t hdr[CB_HDR];
    memcpy(hdr, p + at + 8, sizeof hdr);
    if (hdr[CB_WORDS] != w || hdr[CB_NCOLS] != D.ncols || hdr[CB_NSTATES] != D.nstates)
      return fail(CEP_E_ARG, "state blob does not match this pattern");
    keys.push_back({k, at + 8});
    words += size_t(w);
    at += 8 + size_t(w) * 4;
  }
  if ((rc = drain(s))) return rc;
  hipStream_t st = s->stream;
  if (s->cpool_used + int64_t(words) > s->cpool_words && (rc = carry_gc(s, 2 * (s->cpool_used + int64_t(words)), st)))
    return rc;
  std::vector<int32_t> blobs(words);
  std::vector<int64_t> tab(size_t(s->opts.max_keys));
  HIPCHECK(hipMemcpy(tab.data(), s->ctab.p, tab.size() * 8, hipMemcpyDeviceToHost));
  size_t w0 = 0;
  for (auto& kb : keys) {
    int32_t w;
    memcpy(&w, p + kb.second, 4);
    memcpy(blobs.data() + w0, p + kb.second, size_t(w) * 4);
    tab[size_t(kb.first)] = s->cpool_used + int64_t(w0);
    w0 += size_t(w);
  }
  if (words) HIPCHECK(hipMemcpy(s->cpool.as<int32_t>() + s->cpool_used, blobs.data(), words * 4, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(s->ctab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
  s->cpool_used += int64_t(words);
  s->base = std::max(s->base, base);
  return CEP_OK;
}

int cep_state_clear(cep_session* s) {
  int rc = need_carry(s);
  if (rc) return rc;
  if ((rc = drain(s))) return rc;
  s->base = 0;
  s->stop_uncommitted = 0;
  if (s->f_marks.p)                                // no key has a mark
    HIPCHECK(hipMemset(s->f_marks.p, 0xFF, size_t(s->opts.max_keys) * FILTER_MAX_TOPICS * 8));
  if (halo_session(s)) {
    HIPCHECK(hipMemset(s->halo.p, 0, size_t(s->opts.max_keys) * sizeof(HaloHdr)));
    HIPCHECK(hipMemset(s->hflags.p, 0, 16));       // both error-flag words (by stamp parity)
    s->halo_stamp = 0;
    return CEP_OK;
  }
  if (tail_session(s)) {
    HIPCHECK(hipMemset(s->rtab.p, 0, size_t(s->opts.max_keys) * 16));
    HIPCHECK(hipMemset(s->rtop.p, 0, 8));
    s->rpool_used = 0;
    return CEP_OK;
  }
  HIPCHECK(hipMemset(s->ctab.p, 0xFF, size_t(s->opts.max_keys) * 8));
  s->cpool_used = 0;
  return CEP_OK;
}

int cep_key_state(cep_session* s, int32_t key, int64_t* runs, int64_t* queue_len) {
  int rc = need_carry(s);
  if (rc) return rc;
  if (!runs || !queue_len || key < 0 || key >= s->opts.max_keys) return fail(CEP_E_ARG, "bad argument");
  if (halo_session(s))
    return fail(CEP_E_UNSUPPORTED, "a stencil carry session keeps each key's last records, not its NFA runs");
  if (walk_session(s))
    return fail(CEP_E_UNSUPPORTED, "a follow carry session keeps each key's waiting walks, not its NFA queue");
  if (tail_session(s))
    return fail(CEP_E_UNSUPPORTED, "a runs carry session keeps each key's records from its oldest open run, not its NFA queue");
  if ((rc = drain(s))) return rc;
  int64_t off = -1;
  HIPCHECK(hipMemcpy(&off, s->ctab.as<int64_t>() + key, 8, hipMemcpyDeviceToHost));
  if (off < 0) { *runs = 0; *queue_len = -1; return CEP_OK; }
  int32_t hdr[CB_HDR];
  HIPCHECK(hipMemcpy(hdr, s->cpool.as<int32_t>() + off, sizeof hdr, hipMemcpyDeviceToHost));
  *runs = int64_t(uint32_t(hdr[CB_RUNS_LO])) | (int64_t(hdr[CB_RUNS_HI]) << 32);
  *queue_len = hdr[CB_QLEN];
  return CEP_OK;
}

int64_t cep_stream_position(const cep_session* s) { return s ? s->base : -1; }

int cep_state_evict(cep_session* s, const int32_t* keys, int64_t n, const uint8_t** blobs, int64_t* offs) {
  int rc = need_carry(s);
  if (rc) return rc;
  if (n < 0 || !blobs || !offs || (n > 0 && !keys)) return fail(CEP_E_ARG, "null argument");
  for (int64_t i = 0; i < n; i++)
    if (keys[i] < 0 || keys[i] >= s->opts.max_keys) return fail(CEP_E_ARG, "key id out of [0, max_keys)");
  if ((rc = drain(s))) return rc;
  // one download of the key tables (and the carried pool), then one self-contained blob per key
  std::vector<uint8_t>& out = s->evict_buf;
  out.clear();
  offs[0] = 0;
  const int64_t at_pos = s->base - s->stop_uncommitted;
  auto header = [&](uint32_t magic, int32_t nk, uint32_t ver = 1) {
    const size_t at = out.size();
    out.resize(at + 20);
    memcpy(&out[at], &magic, 4); memcpy(&out[at + 4], &ver, 4); memcpy(&out[at + 8], &at_pos, 8);
    memcpy(&out[at + 16], &nk, 4);
  };
  // the evicted keys' marks leave with them (a key with marks but no records still gets a blob: version 2,
  // no key entry)
  std::vector<int64_t> marks;
  if ((rc = marks_download(s, 0, max_keys32(s), marks))) return rc;
  bool marks_dirty = false;
  auto has_marks = [&](int32_t k) {
    if (marks.empty()) return false;
    for (int t = 0; t < FILTER_MAX_TOPICS; t++)
      if (marks[size_t(k) * FILTER_MAX_TOPICS + size_t(t)] != kNoMark) return true;
    return false;
  };
  auto marks_out = [&](int32_t k) {                // the blob's marks section; the key's marks are cleared
    const size_t at = out.size();
    out.resize(at + 4);
    const int32_t cnt = marks_triples(&marks[size_t(k) * FILTER_MAX_TOPICS], k, out);
    memcpy(&out[at], &cnt, 4);
    for (int t = 0; t < FILTER_MAX_TOPICS; t++) marks[size_t(k) * FILTER_MAX_TOPICS + size_t(t)] = kNoMark;
    marks_dirty = true;
  };
  if (halo_session(s)) {
    const int km1 = s->sp->k - 1;
    const int64_t nk = s->opts.max_keys;
    std::vector<HaloHdr> tab(static_cast<size_t>(nk));
    std::vector<int64_t> pos(static_cast<size_t>(nk) * 2 * size_t(km1));
    HIPCHECK(hipMemcpy(tab.data(), s->halo.p, tab.size() * sizeof(HaloHdr), hipMemcpyDeviceToHost));
    if (km1) HIPCHECK(hipMemcpy(pos.data(), s->hpos.p, pos.size() * 8, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; i++) {
      HaloHdr& h = tab[size_t(keys[i])];
      const int sl = halo_newest(h);
      const int32_t cnt = h.cnt[sl];
      const bool hm = has_marks(keys[i]), hh = h.stamp[sl] > 0 && cnt > 0;
      if (hh || hm) header(kHaloMagic, hh ? 1 : 0, hm ? 2 : 1);
      if (hh) {
        const size_t at = out.size();
        out.resize(at + 16 + 8 * size_t(cnt));
        memcpy(&out[at], &keys[i], 4); memcpy(&out[at + 4], &cnt, 4); memcpy(&out[at + 8], &h.masks[sl], 8);
        memcpy(&out[at + 16], &pos[(2 * size_t(keys[i]) + size_t(sl)) * size_t(km1)], 8 * size_t(cnt));
      }
      if (hm) marks_out(keys[i]);
      h = HaloHdr{};                                 // no halo: the next batch starts the key afresh
      offs[i + 1] = int64_t(out.size());
    }
    HIPCHECK(hipMemcpy(s->halo.p, tab.data(), tab.size() * sizeof(HaloHdr), hipMemcpyHostToDevice));
  } else if (tail_session(s)) {
    std::vector<int64_t> tab, pool;
    int rc2 = tail_download(s, tab, pool);
    if (rc2) return rc2;
    for (int64_t i = 0; i < n; i++) {
      const bool hm = has_marks(keys[i]), ht = tab[2 * size_t(keys[i]) + 1] > 0;
      if (ht || hm) header(tail_magic(s), ht ? 1 : 0, hm ? 2 : 1);
      if (ht) tail_entry(s, tab, pool, keys[i], out);
      if (hm) marks_out(keys[i]);
      tab[2 * size_t(keys[i]) + 1] = 0;              // (the pool records are reclaimed by the next compaction)
      offs[i + 1] = int64_t(out.size());
    }
    HIPCHECK(hipMemcpy(s->rtab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
  } else {
    std::vector<int64_t> tab(size_t(s->opts.max_keys));
    HIPCHECK(hipMemcpy(tab.data(), s->ctab.p, tab.size() * 8, hipMemcpyDeviceToHost));
    std::vector<int32_t> pool(size_t(s->cpool_used));
    if (!pool.empty()) HIPCHECK(hipMemcpy(pool.data(), s->cpool.p, pool.size() * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; i++) {
      int64_t& o = tab[size_t(keys[i])];
      if (o >= 0) {
        const int32_t w = pool[size_t(o) + CB_WORDS];
        header(kStateMagic, 1);
        const size_t at = out.size();
        out.resize(at + 8 + 4 * size_t(w));
        memcpy(&out[at], &keys[i], 4); memcpy(&out[at + 4], &w, 4);
        memcpy(&out[at + 8], pool.data() + o, 4 * size_t(w));
      }
      o = -1;                                        // the blob's pool words are reclaimed by the next carry_gc
      offs[i + 1] = int64_t(out.size());
    }
    HIPCHECK(hipMemcpy(s->ctab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
  }
  if (marks_dirty) HIPCHECK(hipMemcpy(s->f_marks.p, marks.data(), marks.size() * 8, hipMemcpyHostToDevice));
  *blobs = out.data();
  return CEP_OK;
}

// A key's carried NFA state (one "KCST" key) in the reference's own terms -- "KCRF", version 1, little
// endian, strings as i32 length + UTF-8 bytes:
//   u32 magic, u32 version, i32 key id, i32 n_cols, i64 runs                      NFAStates.runs (NFA.runs)
//   i32 n, n x {i32 topic id, i64 offset}              NFAStates.latestOffsets: the next record's minimum
//   i32 n, n x {i64 stream position, i32 topic id, i32 partition, i64 offset, i64 timestamp,
//               n_cols x i64 value bits}               the events the buffer still holds (MatchedEvent)
//   i32 n, n x {i32 stage id, i32 epsilon target (-1: the stage itself), i32 flags (1 isBranching,
//               2 isIgnored), i64 sequence, i32 last event (index above, -1 null), i64 timestamp (-1:
//               never read -- within() is inert), i32 n_digits, n_digits x i32}
//                                                      the run queue (ComputationStage, FIFO order)
//   i32 n, n x {str stage name, i32 stage type, i32 event, i64 refs, i32 n_preds, n_preds x {i32 n_digits,
//               n_digits x i32, i32 has predecessor, str predecessor stage name, i32 its type, i32 its
//               event}}                                 buffer nodes Matched -> MatchedEvent, preds in order
//   i32 n, n x {str state name, i64 sequence, i32 type (1 int, 2 long, 3 double), i64 value bits}
//                                                      aggregates (record key, state, sequence) -> value
// Sequences are renumbered densely from 0 (runs sharing one share its aggregates); every new run the
// reference creates gets ++runs, beyond them.
int cep_state_to_reference(const cep_pattern* p, const void* blob, size_t len, void* out, size_t cap,
                           size_t* needed) {
  if (!p || !blob || !needed) return fail(CEP_E_ARG, "null argument");
  const Program& P = p->prog;
  const uint8_t* in = static_cast<const uint8_t*>(blob);
  uint32_t magic = 0;
  int32_t nkeys = 0;
  if (len < 20) return fail(CEP_E_ARG, "bad state blob");
  memcpy(&magic, in, 4);
  memcpy(&nkeys, in + 16, 4);
  if (magic != kStateMagic) return fail(CEP_E_ARG, "not a general-path (KCST) state blob");
  if (nkeys != 1) return fail(CEP_E_ARG, "cep_state_to_reference takes a single-key blob (cep_state_evict)");
  if (len < 28) return fail(CEP_E_ARG, "truncated state blob");
  int32_t key = 0, w = 0;
  memcpy(&key, in + 20, 4);
  memcpy(&w, in + 24, 4);
  if (w < CB_HDR || 28 + size_t(w) * 4 > len) return fail(CEP_E_ARG, "truncated state blob");
  std::vector<int32_t> b(static_cast<size_t>(w));
  memcpy(b.data(), in + 28, size_t(w) * 4);
  const int nhwm = b[CB_NHWM], qlen = b[CB_QLEN], nev = b[CB_NEV], nnode = b[CB_NNODE], npred = b[CB_NPRED];
  const int nver = b[CB_NVER], nseq = b[CB_NSEQ], ncols = b[CB_NCOLS], nst = b[CB_NSTATES];
  if (nhwm < 0 || qlen < 0 || nev < 0 || nnode < 0 || npred < 0 || nver < 0 || nseq < 0 || ncols < 0 || nst < 0)
    return fail(CEP_E_ARG, "bad state blob");
  const int64_t evw = 8 + 2 * int64_t(ncols);
  const int64_t total = int64_t(CB_HDR) + 3 * int64_t(nhwm) + 4 * int64_t(qlen) + evw * nev + 4 * int64_t(nnode) +
                        4 * int64_t(npred) + nver + int64_t(3) * nst * nseq;
  if (ncols != int(P.coltypes.size()) || nst != P.dev.nstates || total != w) return fail(CEP_E_ARG, "state blob does not match the pattern");
  // buffer-node slot -> (stage name, stage type), as lower_general numbers them (Matched.java:31-35)
  std::vector<std::pair<int, int>> slot(size_t(P.dev.nslots), {0, 0});
  for (const auto& st : P.stages) slot[size_t(P.dev.st[st.id].slot)] = {st.name, st.type};
  const int32_t* hw = b.data() + CB_HDR;
  const int32_t* q = hw + 3 * nhwm;
  const int32_t* ev = q + 4 * qlen;
  const int32_t* nd = ev + int64_t(evw) * nev;
  const int32_t* pr = nd + 4 * nnode;
  const int32_t* vs = pr + 4 * npred;
  const int32_t* ag = vs + nver;
  auto w64 = [](const int32_t* x) { return int64_t(uint64_t(uint32_t(x[0])) | (uint64_t(uint32_t(x[1])) << 32)); };
  std::vector<uint8_t> o;
  auto i32 = [&](int32_t v) { const size_t at = o.size(); o.resize(at + 4); memcpy(o.data() + at, &v, 4); };
  auto i64 = [&](int64_t v) { const size_t at = o.size(); o.resize(at + 8); memcpy(o.data() + at, &v, 8); };
  auto str = [&](const std::string& t) { i32(int32_t(t.size())); o.insert(o.end(), t.begin(), t.end()); };
  auto version = [&](int at) {
    if (at < 0 || at >= nver || vs[at] < 0 || at + vs[at] >= nver) return false;
    i32(vs[at]);
    for (int d = 1; d <= vs[at]; d++) i32(vs[at + d]);
    return true;
  };
  i32(int32_t(0x4652434Bu));                        // "KCRF"
  i32(1);
  i32(key);
  i32(ncols);
  i64(w64(b.data() + CB_RUNS_LO));
  i32(nhwm);
  for (int h = 0; h < nhwm; h++) { i32(hw[3 * h]); i64(w64(hw + 3 * h + 1)); }
  i32(nev);
  for (int e = 0; e < nev; e++) {
    const int32_t* x = ev + int64_t(evw) * e;
    i64(w64(x)); i32(x[2]); i32(x[3]); i64(w64(x + 4)); i64(w64(x + 6));
    for (int c = 0; c < ncols; c++) i64(w64(x + 8 + 2 * c));
  }
  i32(qlen);
  for (int r = 0; r < qlen; r++) {
    const int32_t w0 = q[4 * r];
    const int sid = w0 & 0xFF, eps = (w0 >> 8) & 0xFF;
    if (sid >= int(P.stages.size()) || (eps != 0xFF && eps >= int(P.stages.size()))) return fail(CEP_E_ARG, "bad run in state blob");
    if (q[4 * r + 2] < -1 || q[4 * r + 2] >= nev) return fail(CEP_E_ARG, "bad run event in state blob");
    i32(sid);
    i32(eps == 0xFF ? -1 : eps);
    i32(((w0 >> 16) & 1) | (((w0 >> 17) & 1) << 1));
    i64(q[4 * r + 3]);
    i32(q[4 * r + 2]);
    i64(-1);
    if (!version(q[4 * r + 1])) return fail(CEP_E_ARG, "bad version in state blob");
  }
  i32(nnode);
  for (int i = 0; i < nnode; i++) {
    const int32_t* x = nd + 4 * i;
    if (x[0] < 0 || x[0] >= P.dev.nslots) return fail(CEP_E_ARG, "bad node in state blob");
    if (x[1] < 0 || x[1] >= nev) return fail(CEP_E_ARG, "bad node event in state blob");
    str(P.names[size_t(slot[size_t(x[0])].first)]);
    i32(slot[size_t(x[0])].second);
    i32(x[1]);
    i64(x[2]);
    int cnt = 0;
    bool bad = false;
    for (int pi = x[3]; pi >= 0; pi = pr[4 * pi + 3])   // a link out of the list, or a cycle: malformed
      if (pi >= npred || ++cnt > npred) { bad = true; break; }
    if (bad) return fail(CEP_E_ARG, "bad predecessor list in state blob");
    i32(cnt);
    for (int pi = x[3]; pi >= 0; pi = pr[4 * pi + 3]) {
      const int32_t* y = pr + 4 * pi;
      if (!version(y[0])) return fail(CEP_E_ARG, "bad version in state blob");
      const bool has = y[1] >= 0;
      if (y[1] >= P.dev.nslots) return fail(CEP_E_ARG, "bad predecessor in state blob");
      if (has && (y[2] < 0 || y[2] >= nev)) return fail(CEP_E_ARG, "bad predecessor event in state blob");
      i32(has ? 1 : 0);
      str(has ? P.names[size_t(slot[size_t(y[1])].first)] : std::string());
      i32(has ? slot[size_t(y[1])].second : 0);
      i32(has ? y[2] : -1);
    }
  }
  int32_t nagg = 0;
  for (int64_t i = 0; i < int64_t(nst) * nseq; i++) {
    if (ag[3 * i] < 0 || ag[3 * i] > 3) return fail(CEP_E_ARG, "bad aggregate type in state blob");   // 1 int, 2 long, 3 double
    nagg += ag[3 * i] != 0;
  }
  i32(nagg);
  for (int sq = 0; sq < nseq; sq++)
    for (int st = 0; st < nst; st++) {
      const int32_t* a = ag + (int64_t(sq) * nst + st) * 3;
      if (!a[0]) continue;                          // unset: States.get would throw
      str(P.states[size_t(st)]);
      i64(sq);
      i32(a[0]);
      i64(w64(a + 1));
    }
  *needed = o.size();
  if (!out) return CEP_OK;
  if (cap < o.size()) return fail(CEP_E_ARG, "buffer too small");
  memcpy(out, o.data(), o.size());
  return CEP_OK;
}

int cep_state_import_keys(cep_session* s, const void* const* blobs, const size_t* lens, const int32_t* keys,
                          int64_t n) {
  int rc = need_carry(s);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!blobs || !lens || !keys))) return fail(CEP_E_ARG, "null argument");
  // one multi-key blob with the keys renumbered, then the ordinary import
  std::vector<uint8_t> all(20), msec(4);           // msec: the blobs' marks, re-keyed (version 2 blobs)
  const uint32_t magic = halo_session(s) ? kHaloMagic : tail_session(s) ? tail_magic(s) : kStateMagic;
  int64_t base = 0;
  int32_t nk = 0, nmarks = 0;
  for (int64_t i = 0; i < n; i++) {
    const uint8_t* p = static_cast<const uint8_t*>(blobs[i]);
    if (!p || lens[i] < 20) return fail(CEP_E_ARG, "bad state blob");
    uint32_t m, v;
    int64_t b;
    int32_t cnt;
    memcpy(&m, p, 4); memcpy(&v, p + 4, 4); memcpy(&b, p + 8, 8); memcpy(&cnt, p + 16, 4);
    const bool v2 = v == 2 && magic != kStateMagic;
    if (m != magic || (v != 1 && !v2) || cnt < 0 || cnt > 1)
      return fail(CEP_E_ARG, "cep_state_import_keys takes single-key blobs of this session's kind");
    if (keys[i] < 0 || keys[i] >= s->opts.max_keys) return fail(CEP_E_ARG, "key id out of [0, max_keys)");
    base = std::max(base, b);
    size_t end = lens[i];                            // of the key entry: a version 2 blob's marks follow it
    if (v2) {
      end = 20;
      if (cnt == 1) {
        int32_t w = 0, rw = 1;
        if (lens[i] < 36) return fail(CEP_E_ARG, "truncated state blob");
        memcpy(&w, p + 24, 4); memcpy(&rw, p + 28, 4);
        const bool tail = magic == kTailMagic || magic == kWalkMagic;
        if (w < 0 || (tail && rw < 0)) return fail(CEP_E_ARG, "bad key entry in the state blob");
        end = 36 + 8 * size_t(w) * (tail ? size_t(rw) : 1);
      }
      const int64_t mc = end <= lens[i] ? marks_parse(p, end, lens[i]) : -1;
      if (mc < 0) return fail(CEP_E_ARG, "truncated marks section in the state blob");
      const size_t at = msec.size();
      msec.insert(msec.end(), p + end + 4, p + end + 4 + 16 * size_t(mc));
      for (int64_t q = 0; q < mc; q++) memcpy(&msec[at + 16 * size_t(q)], &keys[i], 4);
      nmarks += int32_t(mc);
    }
    if (cnt == 0) continue;
    const size_t at = all.size();
    all.insert(all.end(), p + 20, p + end);
    memcpy(&all[at], &keys[i], 4);
    nk++;
  }
  const uint32_t ver = nmarks ? 2 : 1;
  if (nmarks) {
    memcpy(&msec[0], &nmarks, 4);
    all.insert(all.end(), msec.begin(), msec.end());
  }
  memcpy(&all[0], &magic, 4); memcpy(&all[4], &ver, 4); memcpy(&all[8], &base, 8); memcpy(&all[16], &nk, 4);
  return cep_state_import(s, all.data(), all.size());
}

int cep_state_positions(const void* buf, size_t len, int64_t* out, int64_t cap, int64_t* n) {
  if (!buf || !n || len < 20) return fail(CEP_E_ARG, "bad state blob");
  const uint8_t* p = static_cast<const uint8_t*>(buf);
  uint32_t magic, ver;
  int32_t nkeys;
  memcpy(&magic, p, 4); memcpy(&ver, p + 4, 4); memcpy(&nkeys, p + 16, 4);
  if ((magic != kStateMagic && magic != kHaloMagic && magic != kTailMagic && magic != kWalkMagic) || nkeys < 0)
    return fail(CEP_E_ARG, "bad state blob");
  int64_t cnt = 0;
  size_t at = 20;
  auto put = [&](int64_t v) { if (out && cnt < cap) out[cnt] = v; cnt++; };
  for (int32_t i = 0; i < nkeys; i++) {
    if (at + 8 > len) return fail(CEP_E_ARG, "truncated state blob");
    int32_t w;
    memcpy(&w, p + at + 4, 4);
    if (magic == kTailMagic) {                       // key, records, words per record, 0, records (pos first)
      int32_t rw;
      if (at + 16 > len) return fail(CEP_E_ARG, "truncated state blob");
      memcpy(&rw, p + at + 8, 4);
      if (w <= 0 || rw < 5 || at + 16 + size_t(w) * size_t(rw) * 8 > len) return fail(CEP_E_ARG, "truncated state blob");
      for (int32_t j = 0; j < w; j++) {
        int64_t v;
        memcpy(&v, p + at + 16 + size_t(j) * size_t(rw) * 8, 8);
        put(v);
      }
      at += 16 + size_t(w) * size_t(rw) * 8;
      continue;
    }
    if (magic == kWalkMagic) {                       // key, walks, words per walk, 0, walks (slots taken, their positions)
      int32_t rw;
      if (at + 16 > len) return fail(CEP_E_ARG, "truncated state blob");
      memcpy(&rw, p + at + 8, 4);
      if (w <= 0 || rw < 2 || at + 16 + size_t(w) * size_t(rw) * 8 > len) return fail(CEP_E_ARG, "truncated state blob");
      for (int32_t j = 0; j < w; j++) {
        const uint8_t* walk = p + at + 16 + size_t(j) * size_t(rw) * 8;
        int64_t sl, v;
        memcpy(&sl, walk, 8);
        if (sl < 1 || sl >= rw) return fail(CEP_E_ARG, "bad walk in the state blob");
        for (int64_t q = 1; q <= sl; q++) {
          memcpy(&v, walk + 8 * q, 8);
          put(v);
        }
      }
      at += 16 + size_t(w) * size_t(rw) * 8;
      continue;
    }
    if (magic == kHaloMagic) {                       // key, records, masks, positions[records]
      if (w < 0 || at + 16 + 8 * size_t(w) > len) return fail(CEP_E_ARG, "truncated state blob");
      for (int32_t j = 0; j < w; j++) {
        int64_t v;
        memcpy(&v, p + at + 16 + 8 * size_t(j), 8);
        put(v);
      }
      at += 16 + 8 * size_t(w);
      continue;
    }
    if (w < CB_HDR || at + 8 + 4 * size_t(w) > len) return fail(CEP_E_ARG, "truncated state blob");
    const int32_t* b = reinterpret_cast<const int32_t*>(p + at + 8);   // 4-byte aligned in every blob we write
    int32_t hdr[CB_HDR];
    memcpy(hdr, b, sizeof hdr);
    const int32_t nev = hdr[CB_NEV];
    if (nev > 0) {                                   // events: stream position (int64) first, carry_evw words each
      const int64_t evw = 8 + 2 * int64_t(hdr[CB_NCOLS]);
      const int64_t e0 = CB_HDR + 3 * int64_t(hdr[CB_NHWM]) + 4 * int64_t(hdr[CB_QLEN]);
      if (e0 + nev * evw > w) return fail(CEP_E_ARG, "bad state blob");
      for (int32_t e = 0; e < nev; e++) {
        uint32_t lo, hi;
        memcpy(&lo, b + e0 + e * evw, 4); memcpy(&hi, b + e0 + e * evw + 1, 4);
        put(int64_t(uint64_t(lo) | (uint64_t(hi) << 32)));
      }
    }
    at += 8 + 4 * size_t(w);
  }
  // (version 2: the marks section behind the key entries names no record; it only has to be whole)
  if (ver == 2 && magic != kStateMagic && marks_parse(p, at, len) < 0) return fail(CEP_E_ARG, "truncated marks section in the state blob");
  *n = cnt;
  return out && cnt > cap ? fail(CEP_E_ARG, "output too small") : CEP_OK;
}

int cep_session_set_max_key_words(cep_session* s, int64_t words) {
  if (!s || words < 0) return fail(CEP_E_ARG, "bad argument");
  s->opts.max_key_words = words;
  return CEP_OK;
}

}  // extern "C"
