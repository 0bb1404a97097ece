// push.cpp -- the push paths behind cep_push_batch (abi.cpp push_dispatch): host staging, the stencil / chain,
// runs and general batches, their carried pools (carry_gc, tail_reserve), CEP_BATCH_ARRIVAL_ORDER (group.hip).
#include <string.h>

#include <atomic>
#include <chrono>

#include "jit.h"
#include "session.h"

namespace kcep {

static bool host_pinned(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();      // pageable memory is unknown to the runtime: not an error
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

static int stage_host(cep_session* s, HostArr* arrs, int na, hipStream_t st, bool zero_copy = false) {
  size_t total = 0;
  std::vector<size_t> at(size_t(na), 0);
  for (int i = 0; i < na; i++) {
    if (!arrs[i].src || !arrs[i].bytes) continue;
    at[size_t(i)] = total;
    total += (arrs[i].bytes + 255) & ~size_t(255);
  }
  if (!total) return CEP_OK;
  // zero copy (the stencil path's one streaming pass, batches up to kZeroCopyMax): the kernel reads the
  // pinned ring over the link itself, no copy into HBM first.
  // Pinned caller memory takes it too: one host memcpy beats waiting for a DMA before the call may
  // return (r04 flush probe, 64 k records: 55.8 us per flush through the ring, 67-69 us pinned by DMA)
  if (zero_copy && total <= kZeroCopyMax) {
    const int j = s->ring_next;
    s->ring_next ^= 1;
    if (s->ring_ev[j]) HIPCHECK(hipEventSynchronize(s->ring_ev[j]));
    else HIPCHECK(hipEventCreateWithFlags(&s->ring_ev[j].e, hipEventDisableTiming));
    if (s->ring[j].cap < total) HIPCHECK(s->ring[j].alloc(std::max(total, size_t(1) << 20), hipHostMallocMapped));
    uint8_t* h = static_cast<uint8_t*>(s->ring[j].p);
    void* dptr = nullptr;
    HIPCHECK(hipHostGetDevicePointer(&dptr, h, 0));
    for (int i = 0; i < na; i++)
      if (arrs[i].src && arrs[i].bytes) {
        memcpy(h + at[size_t(i)], arrs[i].src, arrs[i].bytes);
        *arrs[i].dst = static_cast<uint8_t*>(dptr) + at[size_t(i)];
      }
    s->zc_slot = j;                                   // its event is recorded behind the kernels that read it
    return CEP_OK;
  }
  bool pinned = true;
  for (int i = 0; i < na && pinned; i++)
    if (arrs[i].src && arrs[i].bytes) pinned = host_pinned(arrs[i].src);
  if (s->dstage.ensure(total)) return fail(CEP_E_HIP, "staging allocation failed");
  uint8_t* dev = s->dstage.as<uint8_t>();
  for (int i = 0; i < na; i++)
    if (arrs[i].src && arrs[i].bytes) *arrs[i].dst = dev + at[size_t(i)];
  if (pinned) {                                       // DMA straight from the caller's pinned memory
    for (int i = 0; i < na; i++)
      if (arrs[i].src && arrs[i].bytes)
        HIPCHECK(hipMemcpyAsync(dev + at[size_t(i)], arrs[i].src, arrs[i].bytes, hipMemcpyHostToDevice, st));
    if (!s->h2d_ev) HIPCHECK(hipEventCreateWithFlags(&s->h2d_ev.e, hipEventDisableTiming));
    HIPCHECK(hipEventRecord(s->h2d_ev, st));
    s->h2d_wait = true;                               // cep_push_batch waits for it before returning
    return CEP_OK;
  }
  // pageable: through the pinned ring, in chunks so that the copy of one overlaps the filling of the next
  // (2 MB chunks: the copy of chunk i overlaps the filling of chunk i + 1; a smaller batch is one chunk)
  const size_t chunk = std::min(total, size_t(2) << 20);
  for (size_t c0 = 0; c0 < total; c0 += chunk) {
    const size_t c1 = std::min(total, c0 + chunk);
    const int j = s->ring_next;
    s->ring_next ^= 1;
    if (s->ring_ev[j]) HIPCHECK(hipEventSynchronize(s->ring_ev[j]));
    else HIPCHECK(hipEventCreateWithFlags(&s->ring_ev[j].e, hipEventDisableTiming));
    const size_t want = std::min(total, chunk);
    if (s->ring[j].cap < want) HIPCHECK(s->ring[j].alloc(want, hipHostMallocMapped));   // (the slot may serve a zero-copy batch later)
    uint8_t* h = static_cast<uint8_t*>(s->ring[j].p);
    for (int i = 0; i < na; i++) {                    // the parts of the columns inside [c0, c1)
      if (!arrs[i].src || !arrs[i].bytes) continue;
      const size_t a = std::max(c0, at[size_t(i)]), b = std::min(c1, at[size_t(i)] + arrs[i].bytes);
      if (a < b) memcpy(h + (a - c0), static_cast<const uint8_t*>(arrs[i].src) + (a - at[size_t(i)]), b - a);
    }
    HIPCHECK(hipMemcpyAsync(dev + c0, h, c1 - c0, hipMemcpyHostToDevice, st));
    HIPCHECK(hipEventRecord(s->ring_ev[j], st));
  }
  return CEP_OK;
}

// CEP_BATCH_DELIVER host buffer: {match count, error flags, completion stamp, 0}, host_cap keys (int32,
// padded to 8 bytes), then host_cap x k stream positions
void dl_layout(const cep_session* s, int slot, int64_t*& hdr, int32_t*& hkey, int64_t*& hpos) {
  hdr = static_cast<int64_t*>(s->dl[slot].p);
  hkey = reinterpret_cast<int32_t*>(hdr + 4);
  hpos = hdr + 4 + (s->dl_cap + 1) / 2 + 1;
}

static int stage_inputs(cep_session* s, const cep_batch* b, hipStream_t st, NfaArgs& A, bool zero_copy);

// A mask-pass session's batch (CEP_SESSION_MASK_PASS): every column on the device, then the pre-pass
// (masks.hip) over the columns the path is about to read -- the caller's, group_batch's or filter_batch's,
// with their stream positions -- writes the mask column the stencil / chain kernel takes as its value column
static int push_masks(cep_session* s, const cep_batch* b, hipStream_t st, const int32_t*& key, const void*& col) {
  const MaskProgram& MP = s->pat->prog.mask_prog;
  NfaArgs in{};
  int rc = stage_inputs(s, b, st, in, true);
  if (rc) return rc;
  MaskArgs M{};
  M.P = s->mprog.as<MaskProgram>();
  M.key = in.key;
  M.topic = (MP.meta & MASK_META_TOPIC) ? in.topic : nullptr;
  M.partition = (MP.meta & MASK_META_PARTITION) ? in.partition : nullptr;
  M.offset = (MP.meta & MASK_META_OFFSET) ? in.offset : nullptr;
  M.ts = (MP.meta & MASK_META_TS) ? in.ts : nullptr;
  M.pos = s->cur_pos;
  M.n = b->n;
  M.base = s->carry ? s->base : 0;
  M.mask = s->mcol.as<int32_t>();
  uintptr_t bits = reinterpret_cast<uintptr_t>(M.key) | reinterpret_cast<uintptr_t>(M.topic) |
                   reinterpret_cast<uintptr_t>(M.partition) | reinterpret_cast<uintptr_t>(M.offset) |
                   reinterpret_cast<uintptr_t>(M.ts) | reinterpret_cast<uintptr_t>(M.pos);
  for (int c = 0; c < b->n_cols && c < 16; c++)
    if (MP.used >> c & 1) {
      M.cols[c] = in.cols[c];
      bits |= reinterpret_cast<uintptr_t>(M.cols[c]);
    }
  if (bits & 15) return fail(CEP_E_ARG, "device columns must be 16-byte aligned");
  if (size_t(b->n) * 4 > s->mcol.cap) return fail(CEP_E_ARG, "batch larger than the session capacity");
  HIPCHECK(masks_launch(M, st, s->jitm ? s->jitm->masks : nullptr));
  key = in.key;
  col = M.mask;
  return CEP_OK;
}

int push_stencil(cep_session* s, const cep_batch* b, hipStream_t st) {
  const StencilProgram& SP = *s->sp;
  const void* col = b->n_cols && !s->mask_pass ? b->cols[SP.col] : nullptr;
  const int32_t* key = b->key_id;
  const int32_t* topic = SP.use_topic ? b->topic : nullptr;
  const size_t vs = type_size(SP.coltype);
  if (s->mask_pass) {
    int rc = push_masks(s, b, st, key, col);
    if (rc) return rc;
  } else if (b->mem == CEP_MEM_HOST && b->n > 0) {
    HostArr arrs[3] = {{key, size_t(b->n) * 4, reinterpret_cast<const void**>(&key)},
                       {col, size_t(b->n) * vs, &col},
                       {topic, size_t(b->n) * 4, reinterpret_cast<const void**>(&topic)}};
    int rc = stage_host(s, arrs, SP.use_topic ? 3 : 2, st, true);
    if (rc) return rc;
  }
  if (SP.use_topic && !topic && b->n > 0) {          // no topic column: every record on topic id 0
    if (s->h_topic.ensure(size_t(b->n) * 4)) return fail(CEP_E_HIP, "staging allocation failed");
    HIPCHECK(hipMemsetAsync(s->h_topic.p, 0, size_t(b->n) * 4, st));
    topic = s->h_topic.as<int32_t>();
  }
  if ((reinterpret_cast<uintptr_t>(key) | reinterpret_cast<uintptr_t>(col) | reinterpret_cast<uintptr_t>(topic)) & 15)
    return fail(CEP_E_ARG, "device columns must be 16-byte aligned");
  s->d_key = key;
  int64_t* tc = s->status.as<int64_t>();
  const int64_t ntiles = stencil_tiles(b->n);
  StencilLaunch L{key, col, topic, b->n, s->prog.as<StencilProgram>(), SP.k, SP.coltype, SP.use_topic, SP.chain,
                  s->slots.as<int32_t>(), tc, tc + ntiles + 1, s->counter.as<int64_t>(), s->out.as<int32_t>(),
                  s->out_cap, s->total.as<int64_t>(), StencilCarry{}, !getenv_flag("KCEP_STENCIL_KEYED"), nullptr};
  L.key_mode = getenv_flag("KCEP_STENCIL_SPARSE_KEYS") ? 1 : getenv_flag("KCEP_STENCIL_DENSE_KEYS") ? 2 : 0;
  // the 16-bit super-tile counts: the tile_pre region from its first 16-B boundary on (2 B per super-tile
  // where tile_pre has 8 B per tile: it fits from one tile up)
  L.tile_count16 = reinterpret_cast<uint16_t*>((reinterpret_cast<uintptr_t>(L.tile_pre) + 15) & ~uintptr_t(15));
  L.split_finish = getenv_flag("KCEP_STENCIL_SPLIT_FINISH");
  if (s->carry) {                                // the keys' halos: read the previous, write the next
    // the batch's error flags: one of two words by the stamp's parity; the other one, cleared by this
    // batch's scan kernel, serves the next batch (no memset launch per batch)
    L.clear_flag = s->hflags.as<unsigned long long>() + (s->halo_stamp & 1);
    L.carry = StencilCarry{s->halo.as<HaloHdr>(), s->hpos.as<int64_t>(), SP.k - 1, ++s->halo_stamp,
                           max_keys32(s), s->base,
                           s->hflags.as<unsigned long long>() + (s->halo_stamp & 1), s->cur_pos,
                           s->arrival_n > 0 ? 1 : 0};
    s->last_gpos = s->cur_pos;
    s->halo_base = s->base;
    s->base += b->n;
  }
  if (s->carry && (b->flags & CEP_BATCH_DELIVER)) {   // the matches to pinned host memory, by the device
    const int k = SP.k;
    const int64_t host_cap = std::min<int64_t>(s->out_cap, int64_t(1) << 20);
    if (!s->dl[0]) {
      const size_t bytes = 8 * (4 + size_t(host_cap + 1) / 2 + 1) + size_t(host_cap) * size_t(k) * 8;   // see dl_layout
      for (int j = 0; j < 2; j++) {
        HIPCHECK(s->dl[j].alloc(bytes, hipHostMallocMapped | hipHostMallocCoherent));
        memset(s->dl[j].p, 0, 32);
      }
      s->dl_cap = host_cap;
      if (s->dl_ticket.ensure(16)) return fail(CEP_E_HIP, "allocation failed");
      HIPCHECK(hipMemsetAsync(s->dl_ticket.p, 0, 16, st));
    }
    if (s->out_cap > host_cap &&
        (s->mkey.ensure(size_t(s->out_cap) * 4) || s->opos.ensure(size_t(s->out_cap) * size_t(k) * 8)))
      return fail(CEP_E_HIP, "allocation failed");
    const int slot = int((s->dl_stamp + 1) & 1);   // the next stamp's buffer (the other holds the batch before)
    dl_layout(s, slot, L.deliver.hdr, L.deliver.hkey, L.deliver.hpos);
    s->dl_pid[slot] = s->push_id;
    L.deliver.dkey = s->mkey.as<int32_t>();
    L.deliver.dpos = s->opos.as<int64_t>();
    L.deliver.host_cap = s->dl_cap;
    L.deliver.ticket = s->dl_ticket.as<unsigned>();
    L.deliver.stamp = ++s->dl_stamp;
    if (s->arrival_n > 0 && b->n > 0) {            // arrival order: rows delivered by their completing record's arrival
      const int64_t an = s->arrival_n;               // (the batch as pushed: a filtered one holds fewer records)
      if (s->a_moff.ensure(size_t(an) * 8) || s->a_tmp.ensure(size_t(an / 1024 + 4) * 8) || s->scal.ensure(64))
        return fail(CEP_E_HIP, "allocation failed");
      L.deliver.a_cnt = s->a_cnt.as<int64_t>();
      L.deliver.a_head = s->a_head.as<int32_t>();
      L.deliver.a_moff = s->a_moff.as<int64_t>();
      L.deliver.a_tot = s->scal.as<int64_t>() + 6;
      L.deliver.a_tmp = s->a_tmp.as<int64_t>();
      L.deliver.a_n = an;
    }
    s->delivered = true;
  }
  HIPCHECK(stencil_launch(L, s->timing ? s->ev0.e : nullptr, s->timing ? s->ev1.e : nullptr, st));
  if (s->timing) HIPCHECK(hipEventRecord(s->eb1, st));
  return CEP_OK;
}

static int64_t read_i64(const void* dev, hipStream_t st, int* rc) {
  int64_t v = 0;
  if (hipMemcpyAsync(&v, dev, sizeof v, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    *rc = CEP_E_HIP;
  return v;
}

// Carry pool: the live blobs move to a fresh buffer (dropping the blobs that
// later batches superseded); the table is rewritten in place.
int carry_gc(cep_session* s, int64_t min_words, hipStream_t st) {
  const int64_t nk = s->opts.max_keys;
  int rc = CEP_OK;
  if (s->flag.ensure(size_t(nk) * 8) || s->idx.ensure(size_t(nk) * 8) ||
      s->scan_tmp.ensure(size_t(nk / 1024 + 2) * 8) || s->scal.ensure(64))
    return fail(CEP_E_HIP, "allocation failed");
  int64_t* scal = s->scal.as<int64_t>();
  HIPCHECK(carry_sizes_launch(s->ctab.as<int64_t>(), nk, s->cpool.as<int32_t>(), s->flag.as<int64_t>(), st));
  HIPCHECK(exclusive_scan(s->flag.as<int64_t>(), nk, s->idx.as<int64_t>(), scal + 5, s->scan_tmp.as<int64_t>(), st));
  const int64_t live = read_i64(scal + 5, st, &rc);
  if (rc) return fail(rc, "carry size");
  const int64_t cap = std::max<int64_t>({2 * live, min_words, int64_t(1) << 20});
  DBuf fresh;
  if (fresh.ensure(size_t(cap) * 4)) return fail(CEP_E_RUN_CAPACITY, "cannot allocate the carried-state pool");
  HIPCHECK(carry_move_launch(s->ctab.as<int64_t>(), nk, s->cpool.as<int32_t>(), s->idx.as<int64_t>(),
                             fresh.as<int32_t>(), st));
  HIPCHECK(hipStreamSynchronize(st));
  s->cpool = std::move(fresh);
  s->cpool_words = cap;
  s->cpool_used = live;
  return CEP_OK;
}

// batch columns on the device: A gets the batch's columns, a host batch's staged through the session's
// buffers (stage_host; zero_copy: small ones read over the link in place)
static int stage_inputs(cep_session* s, const cep_batch* b, hipStream_t st, NfaArgs& A, bool zero_copy) {
  const Program& P = s->pat->prog;
  const int64_t n = b->n;
  A.key = b->key_id; A.valid = b->valid; A.topic = b->topic; A.partition = b->partition;
  A.offset = b->offset; A.ts = b->ts;
  for (int c = 0; c < b->n_cols; c++) A.cols[c] = b->cols[c];
  if (b->mem != CEP_MEM_HOST || n <= 0) return CEP_OK;
  HostArr arrs[6 + 16] = {{A.key, size_t(n) * 4, reinterpret_cast<const void**>(&A.key)},
                          {A.valid, size_t(n), reinterpret_cast<const void**>(&A.valid)},
                          {A.topic, size_t(n) * 4, reinterpret_cast<const void**>(&A.topic)},
                          {A.partition, size_t(n) * 4, reinterpret_cast<const void**>(&A.partition)},
                          {A.offset, size_t(n) * 8, reinterpret_cast<const void**>(&A.offset)},
                          {A.ts, size_t(n) * 8, reinterpret_cast<const void**>(&A.ts)}};
  for (int c = 0; c < b->n_cols; c++)
    arrs[6 + c] = HostArr{A.cols[c], size_t(n) * type_size(P.coltypes[c]), &A.cols[c]};
  return stage_host(s, arrs, 6 + b->n_cols, st, zero_copy);
}

// the tail pool with room for `more` records beyond the used ones (compacted / grown when short)
int tail_reserve(cep_session* s, int64_t more, hipStream_t st) {
  if (s->rpool_used + more <= s->rpool_cap) return CEP_OK;
  const int RW = tail_rw(s);
  const int64_t nk = s->opts.max_keys;
  const int64_t cap = std::max<int64_t>(2 * (s->rpool_used + more), int64_t(1) << 16);
  if (s->rpool2.ensure(size_t(cap) * RW * 8) || s->gc_len.ensure(size_t(nk + 1) * 8) || s->gc_off.ensure(size_t(nk + 1) * 8) ||
      s->scan_tmp.ensure(size_t(nk / 1024 + 4) * 8))
    return fail(CEP_E_HIP, "tail pool allocation failed");
  if (s->rpool_used > 0)
    HIPCHECK(runs_carry_gc(s->rtab.as<int64_t>(), nk, RW, s->rpool.as<int64_t>(), s->rpool2.as<int64_t>(),
                           s->gc_len.as<int64_t>(), s->gc_off.as<int64_t>(), s->rtop.as<int64_t>(), s->scan_tmp.as<int64_t>(),
                           st));
  else
    HIPCHECK(hipMemsetAsync(s->rtop.p, 0, 8, st));
  int64_t live = 0;
  HIPCHECK(hipMemcpyAsync(&live, s->rtop.p, 8, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  std::swap(s->rpool, s->rpool2);
  s->rpool2.release();
  s->rpool_cap = cap;
  s->rpool_used = live;
  return CEP_OK;
}

// the carry key checks' flag word (bit 0: a key id out of range, bit 1: a key in two segments)
static int key_check(uint64_t flags) {
  if (flags & 1) return fail(CEP_E_ARG, "carry sessions need key ids in [0, max_keys)");
  if (flags & 2) return fail(CEP_E_ARG, "carry batch is not grouped by key: a key has two segments");
  return CEP_OK;
}

// the device address of s->h_res, allocated at the first runs / general batch
static int results_page(cep_session* s, int64_t** dev) {
  if (!s->h_res) HIPCHECK(s->h_res.alloc(128, hipHostMallocMapped | hipHostMallocCoherent));
  HIPCHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(dev), s->h_res.p, 0));
  return CEP_OK;
}

// a runs / general batch starts with no exception and no matches
static void reset_results(cep_session* s) {
  s->g_err = CEP_OK;
  s->g_err_rec = -1;
  s->e_rec.clear();
  s->e_code.clear();
  s->g_matches = s->g_entries = 0;
}

// an empty runs / general batch: cep_device_match_count reads scal[3], zero it (with_ev0: not recorded yet)
static int push_empty(cep_session* s, hipStream_t st, bool with_ev0) {
  if (s->scal.ensure(64)) return fail(CEP_E_HIP, "allocation failed");
  HIPCHECK(hipMemsetAsync(s->scal.as<int64_t>() + 3, 0, 16, st));
  if (with_ev0) HIPCHECK(hipEventRecord(s->ev0, st));
  HIPCHECK(hipEventRecord(s->ev1, st));
  HIPCHECK(hipEventRecord(s->eb1, st));
  return CEP_OK;
}

// Deterministic strict runs (runs.hip): one lane per start record, completed runs
// ordered by (completing record, start), traversals written into the general CSR.
// Carry sessions prefix every key's records with its carried tail (runs.hip) and keep the tails of
// the runs still open at the batch end.
int push_runs(cep_session* s, const cep_batch* b, hipStream_t st) {
  const int64_t nb = b->n;                        // the batch's records
  int64_t n = nb;                                 // records simulated (carry: plus the keys' tails)
  NfaArgs in{};
  int rc = stage_inputs(s, b, st, in, false);
  if (rc) return rc;
  s->d_key = in.key;
  reset_results(s);
  HIPCHECK(hipEventRecord(s->ev0, st));
  if (n == 0) return push_empty(s, st, false);
  const bool rcarry = tail_session(s);
  bool nosync = false;                            // carry: the extended batch's size read after the launches
  RcExt X{};
  const int32_t* bkey = in.key;                   // the batch's own key column (segments index it)
  if (rcarry) {
    const Program& PP = s->pat->prog;
    if (s->flag.ensure(size_t(nb) * 8) || s->idx.ensure(size_t(nb) * 8) || s->seg.ensure(size_t(nb + 1) * 8) ||
        s->scan_tmp.ensure(size_t(nb / 1024 + 4) * 8) || s->rc_a.ensure(size_t(nb + 2) * 8) ||
        s->rc_b.ensure(size_t(nb + 2) * 8) || s->ctl.ensure(64))
      return fail(CEP_E_HIP, "allocation failed");
    int64_t* scal = s->scal.as<int64_t>();
    HIPCHECK(nfa_segments(in.key, nb, s->flag.as<int64_t>(), s->idx.as<int64_t>(), s->seg.as<int64_t>(), scal,
                          s->scan_tmp.as<int64_t>(), st));
    HIPCHECK(hipMemsetAsync(scal + 1, 0, 8, st));
    HIPCHECK(carry_keycheck_launch(nb, scal, in.key, s->seg.as<int64_t>(), max_keys32(s),
                                   s->kstamp.as<int32_t>(), ++s->batch_no, reinterpret_cast<unsigned long long*>(scal + 1), st));
    RcIn B{};
    B.pos = s->cur_pos;
    B.key = in.key; B.topic = in.topic; B.partition = in.partition; B.offset = in.offset; B.ts = in.ts;
    for (int c = 0; c < 16; c++) B.cols[c] = in.cols[c];
    HIPCHECK(runs_carry_build(B, nb, s->base, s->flag.as<int64_t>(), s->idx.as<int64_t>(), s->seg.as<int64_t>(), scal,
                              s->rtab.as<int64_t>(), s->rpool.as<int64_t>(), s->rc_a.as<int64_t>(), s->rc_b.as<int64_t>(),
                              scal + 5, s->scan_tmp.as<int64_t>(), X, st, true, max_keys32(s)));
    // The extended batch's size (the batch plus its keys' carried tails) stays on the device: the launches
    // are sized by a bound -- the batch plus every tail record the pool holds -- and read the count
    // (scal[7]); the key checks are read with the batch's results, and a failing batch leaves the tail
    // pool and table untouched (rc_tail_*).  Unless a forced ordering path or a batch too large for the
    // one-workgroup chunk scan needs the count first.
    const int64_t nmax = nb + s->rpool_used;
    nosync = !getenv_flag("KCEP_RUNS_RADIX") && !getenv_flag_off("KCEP_RUNS_EMIT") && nmax < (int64_t(1) << 31) &&
             (nmax + runs_chunk(nmax) - 1) / runs_chunk(nmax) <= (int64_t(1) << 16);
    if (nosync) {
      n = nmax;
      if ((rc = tail_reserve(s, n, st))) return rc;  // room for the new tails (at most every record)
      HIPCHECK(runs_carry_count(scal + 7, nb, scal + 5, nmax, st));
    } else {
      int64_t h[6];
      HIPCHECK(hipMemcpyAsync(h, scal, sizeof h, hipMemcpyDeviceToHost, st));
      HIPCHECK(hipStreamSynchronize(st));
      if ((rc = key_check(uint64_t(h[1])))) return rc;
      n = nb + h[5];
      if (n >= (int64_t(1) << 31)) return fail(CEP_E_RUN_CAPACITY, "carried tails make the batch exceed 2^31 records");
    }
    const size_t e4 = size_t(n) * 4, e8 = size_t(n) * 8;
    if (s->e_key.ensure(e4) || s->e_topic.ensure(e4) || s->e_part.ensure(e4) || s->e_seg.ensure(e4) ||
        s->e_off.ensure(e8) || s->e_ts.ensure(e8) || s->e_pos.ensure(e8))
      return fail(CEP_E_HIP, "allocation failed");
    X.key = s->e_key.as<int32_t>(); X.topic = s->e_topic.as<int32_t>(); X.partition = s->e_part.as<int32_t>();
    X.seg = s->e_seg.as<int32_t>(); X.offset = s->e_off.as<int64_t>(); X.ts = s->e_ts.as<int64_t>();
    X.pos = s->e_pos.as<int64_t>();
    X.cap = n;
    X.ncols = int32_t(PP.coltypes.size());
    for (int c = 0; c < X.ncols; c++) {
      X.coltype[c] = PP.coltypes[c];
      if (s->e_cols[c].ensure(size_t(n) * type_size(PP.coltypes[c]))) return fail(CEP_E_HIP, "allocation failed");
      X.cols[c] = s->e_cols[c].p;
    }
    HIPCHECK(runs_carry_build(B, nb, s->base, s->flag.as<int64_t>(), s->idx.as<int64_t>(), s->seg.as<int64_t>(), scal,
                              s->rtab.as<int64_t>(), s->rpool.as<int64_t>(), s->rc_a.as<int64_t>(), s->rc_b.as<int64_t>(),
                              scal + 5, s->scan_tmp.as<int64_t>(), X, st, false, max_keys32(s)));
    in.key = X.key; in.topic = X.topic; in.partition = X.partition; in.offset = X.offset; in.ts = X.ts;
    for (int c = 0; c < X.ncols; c++) in.cols[c] = X.cols[c];
    if (!nosync && (rc = tail_reserve(s, n, st))) return rc;   // room for the new tails (at most every record)
  }
  const int64_t n_grid = n;                       // what the runs_sim grid is sized by
  if (s->rk.ensure(size_t(n) * 8) || s->rk_sorted.ensure(size_t(n) * 8) || s->r_errcode.ensure(size_t(n) * 4) ||
      s->ctl.ensure(64) || s->scal.ensure(64) || s->scan_tmp.ensure(size_t(n / 1024 + 4) * 8) ||
      s->flag.ensure(size_t(6 * runs_sim_waves(n, runs_chunk(n)) + 8) * 8) ||
      s->idx.ensure(size_t(2 * runs_sim_waves(n, runs_chunk(n)) + 8) * 8) || s->r_endof.ensure(size_t(n) * 4) ||
      s->r_segs.ensure(size_t(n) * RUNS_MAX_SEGS * 2) ||
      s->r_errlist.ensure(size_t(std::min<int64_t>(n, kRunsErrCap)) * 24))
    return fail(CEP_E_HIP, "allocation failed");
  RunsArgs A{};
  A.P = s->dprog.as<DevProgram>();
  A.key = in.key; A.topic = in.topic; A.partition = in.partition; A.offset = in.offset; A.ts = in.ts;
  for (int c = 0; c < 16; c++) A.cols[c] = in.cols[c];
  A.n = n;
  A.n_dev = nosync ? s->scal.as<int64_t>() + 7 : nullptr;
  A.base = 0;
  A.pos = rcarry ? X.pos : nullptr;               // carry: stream positions; runs ending in a tail are old
  A.emit_from = s->base;
  A.chunk = runs_chunk(n);
  unsigned long long* ctl = s->ctl.as<unsigned long long>();
  A.nmatch = ctl;
  A.err_min = ctl + 1;
  A.match_key = s->rk.as<unsigned long long>();
  A.match_cap = n;
  A.err_code = s->r_errcode.as<int32_t>();
  A.segs = s->r_segs.as<uint16_t>();             // the runs' consumed stages, for runs_emit / runs_expand
  A.segn = s->pat->prog.dev.nstages - 1 <= 4 ? 4 : RUNS_MAX_SEGS;   // (a run consumes each stage at most once)
  A.seg_over = ctl + 3;
  A.err_list = s->r_errlist.as<unsigned long long>();
  A.err_n = ctl + 5;
  A.err_cap = std::min<int64_t>(n, kRunsErrCap);
  A.max_span = ctl + 4;
  // matches, first exception, entries, segment overflow, longest span, failing runs
  const unsigned long long init[6] = {0, ~0ull, 0, 0, 0, 0};
  HIPCHECK(hipMemcpyAsync(ctl, init, sizeof init, hipMemcpyHostToDevice, st));
  HIPCHECK(runs_sim_launch(A, s->flag.as<int64_t>(), s->r_endof.as<int32_t>(), st,
                           s->jit ? s->jit->runs_sim : nullptr));
  HIPCHECK(hipEventRecord(s->ev1, st));
  int64_t* scal0 = s->scal.as<int64_t>();
  // the completed runs counted by the chunk they end in and scanned (runs_emit's placement), or -- too
  // many chunks for that scan, or the sort forced -- compacted in start order for runs_order / the sort
  // (KCEP_RUNS_EMIT=0 / KCEP_RUNS_RADIX=1: the tests' hooks onto those paths for batches runs_emit takes)
  const bool emit_scan = !getenv_flag("KCEP_RUNS_RADIX") && !getenv_flag_off("KCEP_RUNS_EMIT") &&
                         runs_emit_scan(s->flag.as<int64_t>(), n, A.chunk, s->idx.as<int64_t>(), scal0 + 3,
                                        reinterpret_cast<int64_t*>(ctl + 2), st, A.n_dev);
  if (!emit_scan)                                  // (never with nosync: it was decided on the same bound)
    HIPCHECK(runs_compact_launch(s->flag.as<int64_t>(), s->r_endof.as<int32_t>(), n, A.chunk, s->idx.as<int64_t>(),
                                 s->rk.as<unsigned long long>(), scal0 + 3, reinterpret_cast<int64_t*>(ctl + 2),
                                 s->scan_tmp.as<int64_t>(), st, n_grid));
  if (rcarry) {                                    // the keys' new tails: from their oldest still-open start
    if (s->rc_c.ensure(size_t(nb + 2) * 8) || s->rc_d.ensure(size_t(nb + 2) * 8))
      return fail(CEP_E_HIP, "allocation failed");
    HIPCHECK(runs_carry_tails(X, n, nb, scal0, s->seg.as<int64_t>(), bkey, s->rc_b.as<int64_t>(), s->r_endof.as<int32_t>(),
                              reinterpret_cast<unsigned long long*>(s->rc_a.as<int64_t>()), s->rc_c.as<int64_t>(),
                              s->rc_d.as<int64_t>(), scal0 + 6, s->scan_tmp.as<int64_t>(), s->rtop.as<int64_t>(),
                              s->rpool.as<int64_t>(), s->rtab.as<int64_t>(), st, A.n_dev, scal0 + 1));
  }
  // the batch's one host synchronisation: completed runs, entries, first exception, segment overflow (one
  // small kernel writes them into pinned host memory: no copy commands, which cost ~25 us of gaps)
  int64_t* h_res_dev = nullptr;
  if ((rc = results_page(s, &h_res_dev))) return rc;
  HIPCHECK(runs_results_launch(ctl, scal0 + 3, rcarry ? s->rtop.as<int64_t>() : nullptr, h_res_dev, st,
                               rcarry ? scal0 : nullptr));
  HIPCHECK(hipStreamSynchronize(st));
  if (nosync) {                                    // the key checks and the extended batch's size, now
    if ((rc = key_check(uint64_t(s->h_res[7])))) return rc;
    n = nb + s->h_res[8];
    A.n = n;
    A.n_dev = nullptr;
  }
  unsigned long long res[6];
  for (int q = 0; q < 6; q++) res[q] = (unsigned long long)s->h_res[q];
  const int64_t top = s->h_res[6];
  if (rcarry) {
    s->rpool_used = top;
    s->base += nb;
  }
  const int64_t nm = int64_t(res[0]), ne = int64_t(res[2]);
  if (nm > n) return fail(CEP_E_RUN_CAPACITY, "more completed runs than records");
  if (res[1] != ~0ull) {                           // the reference's first exception
    int64_t at = int64_t(res[1] >> 31);
    const int64_t j = int64_t(res[1] & 0x7FFFFFFFull);
    int32_t code = 0;
    HIPCHECK(hipMemcpy(&code, s->r_errcode.as<int32_t>() + j, 4, hipMemcpyDeviceToHost));
    if (code == CEP_E_UNSUPPORTED) return fail(CEP_E_UNSUPPORTED, "sequence condition on the runs path");
    if (rcarry) HIPCHECK(hipMemcpy(&at, X.pos + at, 8, hipMemcpyDeviceToHost));   // its stream position
    s->g_err = code;
    s->g_err_rec = at;
    const int64_t nerr = int64_t(res[5]);
    if (nerr <= A.err_cap) {                       // every failing key's first exception (cep_batch_errors)
      std::vector<unsigned long long> el(size_t(nerr) * 3);
      HIPCHECK(hipMemcpy(el.data(), A.err_list, el.size() * 8, hipMemcpyDeviceToHost));
      std::vector<size_t> ord(static_cast<size_t>(nerr));
      for (size_t q = 0; q < ord.size(); q++) ord[q] = q;
      // per key the smallest (record << 31 | start): its first failure in the reference's order
      std::sort(ord.begin(), ord.end(), [&](size_t x, size_t y) {
        const uint32_t kx = uint32_t(el[3 * x + 2] >> 32), ky = uint32_t(el[3 * y + 2] >> 32);
        return kx != ky ? kx < ky : el[3 * x] < el[3 * y];
      });
      std::vector<std::pair<int64_t, int32_t>> first;
      for (size_t q = 0; q < ord.size(); q++) {
        const size_t x = ord[q];
        if (q > 0 && (el[3 * x + 2] >> 32) == (el[3 * ord[q - 1] + 2] >> 32)) continue;
        first.emplace_back(int64_t(el[3 * x + 1]), int32_t(uint32_t(el[3 * x + 2])));
      }
      std::sort(first.begin(), first.end());
      for (const auto& f : first) {
        s->e_rec.push_back(f.first);
        s->e_code.push_back(f.second);
      }
    } else {                                       // more failing runs than the list holds: the first only
      s->e_rec.push_back(at);
      s->e_code.push_back(code);
    }
  }
  int bits = 1;                                    // bits of the completing record
  while ((int64_t(1) << bits) <= n) bits++;
  size_t tmp_bytes = 0;
  HIPCHECK(runs_sort(nullptr, nullptr, nm, bits, nullptr, &tmp_bytes, st));
  const size_t nmb = size_t(std::max<int64_t>(nm, 1)), neb = size_t(std::max<int64_t>(ne, 1));
  if (s->rk_tmp.ensure(std::max<size_t>(tmp_bytes, 16)) || s->r_len.ensure(nmb * 8) || s->r_entoff.ensure(nmb * 8) ||
      s->scan_tmp.ensure(size_t(nm / 1024 + 4) * 8) || s->o_record.ensure(nmb * 8) || s->o_key.ensure(nmb * 4) ||
      s->o_entoff.ensure(nmb * 8) || s->o_name.ensure(neb * 4) || s->o_entrec.ensure(neb * 8))
    return fail(CEP_E_HIP, "allocation failed");
  int64_t* scal = s->scal.as<int64_t>();
  if (emit_scan && nm > 0 && !res[3] && res[4] < uint64_t(A.chunk)) {
    // every run shorter than a chunk: the CSR in one pass over the end chunks (runs_emit)
    HIPCHECK(runs_emit_launch(A, s->r_endof.as<int32_t>(), s->idx.as<int64_t>(), int(res[4]), s->o_record.as<int64_t>(),
                              s->o_key.as<int32_t>(), s->o_entoff.as<int64_t>(), s->o_name.as<int32_t>(),
                              s->o_entrec.as<int64_t>(), st, n_grid));
    HIPCHECK(hipEventRecord(s->eb1, st));
    s->g_matches = nm;
    s->g_entries = ne;
    return CEP_OK;
  }
  if (emit_scan)                                   // (the start-ordered list the paths below read)
    HIPCHECK(runs_compact_launch(s->flag.as<int64_t>(), s->r_endof.as<int32_t>(), n, A.chunk, s->idx.as<int64_t>(),
                                 s->rk.as<unsigned long long>(), scal0 + 3, reinterpret_cast<int64_t*>(ctl + 2),
                                 s->scan_tmp.as<int64_t>(), st, n_grid));
  // (completing record, start) order: a windowed rank when every run spans <= 1024 records
  // (runs_order), else rocPRIM's radix sort over the completing record's bits
  // the entry offsets are scanned straight into the output's ent_off (runs_expand reads them there);
  // runs_order writes the sorted runs' lengths itself
  if (nm > 0 && res[4] <= 1024 && !getenv_flag("KCEP_RUNS_RADIX")) {
    HIPCHECK(runs_order_launch(s->rk.as<unsigned long long>(), nm, int(res[4]), s->rk_sorted.as<unsigned long long>(),
                               s->r_len.as<int64_t>(), st));
    HIPCHECK(exclusive_scan(s->r_len.as<int64_t>(), nm, s->o_entoff.as<int64_t>(), scal + 4, s->scan_tmp.as<int64_t>(), st));
  } else {
    if (nm > 0)
      HIPCHECK(runs_sort(s->rk.as<unsigned long long>(), s->rk_sorted.as<unsigned long long>(), nm, bits, s->rk_tmp.p,
                         &tmp_bytes, st));
    HIPCHECK(runs_write_launch(A, s->rk_sorted.as<unsigned long long>(), nm, s->r_len.as<int64_t>(),
                               s->o_entoff.as<int64_t>(), scal + 4, s->scan_tmp.as<int64_t>(), nullptr, nullptr,
                               nullptr, nullptr, nullptr, st, true,
                               s->jit ? s->jit->runs_write : nullptr));
  }
  if (!res[3]) {
    // the traversals from the stage segments runs_sim recorded
    HIPCHECK(runs_expand_launch(A, s->rk_sorted.as<unsigned long long>(), nm, s->o_entoff.as<int64_t>(), ne,
                                s->o_record.as<int64_t>(), s->o_key.as<int32_t>(), s->o_entoff.as<int64_t>(),
                                s->o_name.as<int32_t>(), s->o_entrec.as<int64_t>(), st));
  } else {                                         // a run beyond RUNS_MAX_SEGS segments: walk every run again
    A.segs = nullptr;
    HIPCHECK(runs_write_launch(A, s->rk_sorted.as<unsigned long long>(), nm, s->r_len.as<int64_t>(),
                               s->o_entoff.as<int64_t>(), scal + 4, s->scan_tmp.as<int64_t>(), s->o_record.as<int64_t>(),
                               s->o_key.as<int32_t>(), s->o_entoff.as<int64_t>(), s->o_name.as<int32_t>(),
                               s->o_entrec.as<int64_t>(), st, false,
                               s->jit ? s->jit->runs_write : nullptr));
  }
  HIPCHECK(hipEventRecord(s->eb1, st));
  s->g_matches = nm;
  s->g_entries = ne;
  return CEP_OK;
}

// The slots' bitmaps of a follow batch, between the session's kernel timing events: follow_bits over the one
// column the direct form reads; in the evaluated form (M: the columns its predicates read) follow_eval_bits,
// compiled for the pattern or built in -- or, split (KCEP_FOLLOW_MASK_SPLIT=1), the mask pre-pass into the
// mask column and follow_bits over that column through the program's identity table.
static hipError_t follow_planes_launch(cep_session* s, const FollowArgs& A, const MaskArgs& M, hipStream_t st) {
  hipEvent_t ev0 = s->timing ? s->ev0.e : nullptr, ev1 = s->timing ? s->ev1.e : nullptr;
  if (!s->follow_eval) return follow_bits_launch(A, ev0, ev1, st);
  if (!s->follow_split) return follow_eval_bits_launch(M, A, ev0, ev1, st, s->jitm ? s->jitm->follow_bits : nullptr);
  if (ev0) (void)hipEventRecord(ev0, st);
  const hipError_t e = masks_launch(M, st, s->jitm ? s->jitm->masks : nullptr);
  if (e != hipSuccess) return e;
  FollowArgs B = A;
  B.val = M.mask;
  B.topic = nullptr;
  B.coltype = T_I32;
  B.use_topic = 0;
  return follow_bits_launch(B, nullptr, ev1, st);
}

// A follow carry session's batch (CEP_SESSION_FOLLOW_CARRY, follow.hip "carried walks"): the batch is read in
// place; its keys' waiting walks are continued once per (segment, slot), the in-batch walks counted with the
// open ones kept apart; after the one host synchronisation the matches are ordered and written as the runs
// path's CSR, and the keys' new walk lists appended to the pool.  Nothing of the session's state is written
// before the key checks are read: a rejected push leaves it as it was.
static int push_follow_carry(cep_session* s, FollowArgs& A, const MaskArgs& M, hipStream_t st) {
  const int64_t n = A.n, nt = follow_tiles(n);
  const int K = A.k;
  const int64_t bound = s->rpool_used;            // every walk the pool holds: the carried kernels' launch bound
  const int64_t nseg_cap = std::min<int64_t>(n, s->opts.max_keys);
  int rc = CEP_OK;
  if (s->flag.ensure(size_t(n) * 8) || s->idx.ensure(size_t(n) * 8) || s->seg.ensure(size_t(n + 1) * 8) ||
      s->rc_a.ensure(size_t(n + 2) * 8) || s->rc_b.ensure(size_t(n + 2) * 8) || s->ctl.ensure(128) ||
      s->scan_tmp.ensure(size_t(2 * (std::max({nt * 64, bound, n}) / 1024 + 2) + 4) * 8) ||
      (bound > 0 && (s->fw_res.ensure(size_t(nseg_cap) * size_t(K - 1) * size_t(K) * 4) || s->fw_cdone.ensure(size_t(bound) * 8) ||
                     s->fw_copen.ensure(size_t(bound) * 8) || s->fw_cdpre.ensure(size_t(bound) * 8) ||
                     s->fw_copre.ensure(size_t(bound) * 8) || s->fw_cdx.ensure(size_t(bound) * 8))))
    return fail(CEP_E_HIP, "allocation failed");
  int64_t* scal = s->scal.as<int64_t>();
  int64_t* ctl = s->ctl.as<int64_t>();            // in-batch completed, open; carried walks, completed, open; span
  A.pos = s->cur_pos;
  A.base = s->base;
  A.scan_tmp = s->scan_tmp.as<int64_t>();
  A.open = s->fw_open.as<unsigned long long>();
  A.wopen = s->fw_ocnt.as<int64_t>();
  A.wopre = s->fw_opre.as<int64_t>();
  A.nm = ctl;
  A.nopen = ctl + 1;
  A.max_span = reinterpret_cast<unsigned long long*>(ctl + 5);
  FollowCarry C{};
  C.nseg = scal;
  C.seg_start = s->seg.as<int64_t>();
  C.seg_flag = s->flag.as<int64_t>();
  C.seg_idx = s->idx.as<int64_t>();
  C.nseg_cap = nseg_cap;
  C.tlen = s->rc_a.as<int64_t>();
  C.toff = s->rc_b.as<int64_t>();
  C.ncw = ctl + 2;
  C.bound = bound;
  C.rtab = s->rtab.as<int64_t>();
  C.rpool = s->rpool.as<int64_t>();
  C.rtop = s->rtop.as<int64_t>();
  C.res = s->fw_res.as<int32_t>();
  C.cw_done = s->fw_cdone.as<int64_t>(); C.cw_open = s->fw_copen.as<int64_t>();
  C.cw_dpre = s->fw_cdpre.as<int64_t>(); C.cw_opre = s->fw_copre.as<int64_t>();
  C.ncd = ctl + 3; C.nco = ctl + 4;
  C.cd_x = s->fw_cdx.as<int64_t>();
  C.scan_tmp = s->scan_tmp.as<int64_t>();
  HIPCHECK(set_words_launch(ctl, 6, 0, 0, st));
  HIPCHECK(nfa_segments(A.key, n, s->flag.as<int64_t>(), s->idx.as<int64_t>(), s->seg.as<int64_t>(), scal,
                        s->scan_tmp.as<int64_t>(), st));
  HIPCHECK(hipMemsetAsync(scal + 1, 0, 8, st));
  HIPCHECK(carry_keycheck_launch(n, scal, A.key, s->seg.as<int64_t>(), max_keys32(s), s->kstamp.as<int32_t>(),
                                 ++s->batch_no, reinterpret_cast<unsigned long long*>(scal + 1), st));
  RcIn B{};
  B.key = A.key;
  // per segment its key's waiting walks and their prefix (the runs path's tail lengths: the same table)
  HIPCHECK(runs_carry_build(B, n, s->base, nullptr, nullptr, s->seg.as<int64_t>(), scal, s->rtab.as<int64_t>(),
                            s->rpool.as<int64_t>(), s->rc_a.as<int64_t>(), s->rc_b.as<int64_t>(), ctl + 2,
                            s->scan_tmp.as<int64_t>(), RcExt{}, st, true, max_keys32(s)));
  HIPCHECK(follow_planes_launch(s, A, M, st));
  HIPCHECK(follow_carry_count_launch(A, C, st));
  // the batch's one host synchronisation: the completed and open walks, in-batch and carried, the longest
  // in-batch span, the key-check flags
  int64_t* h_res_dev = nullptr;
  if ((rc = results_page(s, &h_res_dev))) return rc;
  HIPCHECK(gather_words_launch(ctl, 6, scal, 2, h_res_dev, st));
  HIPCHECK(hipStreamSynchronize(st));
  if ((rc = key_check(uint64_t(s->h_res[7])))) return rc;
  const int64_t nm_in = s->h_res[0], nopen = s->h_res[1], ncd = s->h_res[3], nco = s->h_res[4], span = s->h_res[5];
  const int64_t nm = nm_in + ncd;                 // (carried walks complete too: more matches than records, possibly)
  if (nm_in < 0 || nm_in > n || ncd < 0 || ncd > bound || nm >= (int64_t(1) << 31))
    return fail(CEP_E_RUN_CAPACITY, "a follow carry batch completes 2^31 walks or more");
  if ((rc = tail_reserve(s, nopen + nco, st))) return rc;   // room for the keys' new lists (the pool may move)
  C.rpool = s->rpool.as<int64_t>();
  int bits = 1;                                    // bits of the completing record
  while ((int64_t(1) << bits) <= n) bits++;
  const bool ranked = ncd == 0 && span <= 1024 && !getenv_flag("KCEP_RUNS_RADIX");
  size_t tmp_bytes = 0;
  if (!ranked && nm > 0) HIPCHECK(runs_sort(nullptr, nullptr, nm, bits, nullptr, &tmp_bytes, st));
  const size_t nmb = size_t(std::max<int64_t>(nm, 1)), neb = nmb * size_t(K);
  if (s->rk.ensure(nmb * 8) || s->rk_sorted.ensure(nmb * 8) ||
      (ranked ? s->r_len.ensure(nmb * 8) : s->rk_tmp.ensure(std::max<size_t>(tmp_bytes, 16))) ||
      s->o_record.ensure(nmb * 8) || s->o_key.ensure(nmb * 4) || s->o_entoff.ensure(nmb * 8) || s->o_name.ensure(neb * 4) ||
      s->o_entrec.ensure(neb * 8))
    return fail(CEP_E_HIP, "allocation failed");
  A.keys = s->rk.as<unsigned long long>();
  HIPCHECK(follow_carry_keys_launch(A, C, ncd, st));
  // (completing record, start) order: the stable sort over the completing record's bits keeps the carried
  // walks in front of their key's in-batch ones; the windowed rank only where none completed
  if (nm > 0) {
    if (ranked)
      HIPCHECK(runs_order_launch(A.keys, nm, int(span), s->rk_sorted.as<unsigned long long>(), s->r_len.as<int64_t>(), st));
    else
      HIPCHECK(runs_sort(A.keys, s->rk_sorted.as<unsigned long long>(), nm, bits, s->rk_tmp.p, &tmp_bytes, st));
  }
  HIPCHECK(follow_carry_rows_launch(A, C, s->rk_sorted.as<unsigned long long>(), nm, s->o_record.as<int64_t>(),
                                    s->o_key.as<int32_t>(), s->o_entoff.as<int64_t>(), s->o_name.as<int32_t>(),
                                    s->o_entrec.as<int64_t>(), scal + 3, st));
  HIPCHECK(follow_carry_state_launch(A, C, st));
  s->rpool_used += nopen + nco;
  s->base += n;
  s->g_matches = nm;
  s->g_entries = nm * K;
  if (s->timing) HIPCHECK(hipEventRecord(s->eb1, st));
  return CEP_OK;
}

// A batch of a pattern with oneOrMore stages (CEP_SESSION_FOLLOW_MANY, follow.hip "oneOrMore slots"): the same
// planes, the walks counted with their lengths; the one host synchronisation yields matches, entries and the
// longest span; then the write pass and the ordering of every follow batch, and the runs path's CSR -- batch
// indices as positions, the device match count at scal[3] -- instead of K-int rows.
static int push_follow_many(cep_session* s, FollowArgs& A, const MaskArgs& M, hipStream_t st) {
  const int64_t n = A.n, nt = follow_tiles(n);
  if (s->scan_tmp.ensure(size_t(std::max(nt / 8, n / 1024) + 4) * 8)) return fail(CEP_E_HIP, "allocation failed");
  int64_t* scal = s->scal.as<int64_t>();
  A.scan_tmp = s->scan_tmp.as<int64_t>();
  A.many_mask = s->follow_many_mask;
  A.wlen = s->fw_len.as<int64_t>();
  A.wlpre = s->fw_lpre.as<int64_t>();
  A.ne = scal + 6;
  HIPCHECK(follow_planes_launch(s, A, M, st));
  HIPCHECK(follow_many_count_launch(A, st));
  // the batch's one host synchronisation: the completed walks, their longest span, their entries
  int64_t h[3] = {0, 0, 0};
  HIPCHECK(hipMemcpyAsync(h, scal + 4, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  const int64_t nm = h[0], span = h[1], ne = h[2];
  if (nm < 0 || nm > n) return fail(CEP_E_RUN_CAPACITY, "more completed walks than records");
  if (ne < nm * A.k || ne >= (int64_t(1) << 31)) return fail(CEP_E_RUN_CAPACITY, "a follow batch's matches hold 2^31 entries or more");
  const size_t nmb = size_t(std::max<int64_t>(nm, 1)), neb = size_t(std::max<int64_t>(ne, 1));
  if (nm > 0) {
    int bits = 1;                                  // bits of the completing record
    while ((int64_t(1) << bits) <= n) bits++;
    const bool ranked = span <= 1024 && !getenv_flag("KCEP_RUNS_RADIX");
    size_t tmp_bytes = 0;
    if (!ranked) HIPCHECK(runs_sort(nullptr, nullptr, nm, bits, nullptr, &tmp_bytes, st));
    if (s->rk.ensure(nmb * 8) || s->rk_sorted.ensure(nmb * 8) || s->r_len.ensure(nmb * 8) ||
        (!ranked && s->rk_tmp.ensure(std::max<size_t>(tmp_bytes, 16))) || s->o_record.ensure(nmb * 8) ||
        s->o_key.ensure(nmb * 4) || s->o_entoff.ensure(nmb * 8) || s->o_name.ensure(neb * 4) || s->o_entrec.ensure(neb * 8))
      return fail(CEP_E_HIP, "allocation failed");
    A.keys = s->rk.as<unsigned long long>();
    HIPCHECK(follow_many_write_launch(A, st));
    if (ranked)
      HIPCHECK(runs_order_launch(A.keys, nm, int(span), s->rk_sorted.as<unsigned long long>(), s->r_len.as<int64_t>(), st));
    else
      HIPCHECK(runs_sort(A.keys, s->rk_sorted.as<unsigned long long>(), nm, bits, s->rk_tmp.p, &tmp_bytes, st));
  }
  // (r_len: the ordering's scratch, then the ordered matches' lengths; scal[7]: their sum, which is ne)
  HIPCHECK(follow_many_rows_launch(A, s->rk_sorted.as<unsigned long long>(), nm, s->r_len.as<int64_t>(), scal + 7,
                                   s->o_record.as<int64_t>(), s->o_key.as<int32_t>(), s->o_entoff.as<int64_t>(),
                                   s->o_name.as<int32_t>(), s->o_entrec.as<int64_t>(), scal + 3, st));
  s->g_matches = nm;
  s->g_entries = ne;
  if (s->timing) HIPCHECK(hipEventRecord(s->eb1, st));
  return CEP_OK;
}

// Skip-till-next walks (follow.hip): the slots' bitmaps in one streaming pass, the completed walks counted
// and compacted in start order, ordered by (completing record, start) as the runs path orders its runs, then
// written as K-int rows -- from there the batch is a finished stencil batch without carry (cep_collect).
int push_follow(cep_session* s, const cep_batch* b, hipStream_t st) {
  const StencilProgram& SP = *s->sp;               // the pattern's follow form, direct or evaluated
  const int64_t n = b->n;
  NfaArgs in{};
  int rc = stage_inputs(s, b, st, in, true);
  if (rc) return rc;
  s->d_key = in.key;
  if (s->carry || s->follow_many) reset_results(s);
  if (n == 0) {
    HIPCHECK(hipMemsetAsync(s->total.p, 0, 8, st));
    return push_empty(s, st, true);
  }
  const void* col = nullptr;
  const int32_t* topic = nullptr;
  MaskArgs M{};
  if (s->follow_eval) {
    // the evaluated form: the columns and metadata its predicates read -- the caller's, group_batch's or
    // filter_batch's, with their stream positions (a default ts / offset is the position)
    const MaskProgram& MP = s->follow_many ? s->pat->prog.follow_many_prog : s->pat->prog.follow_mask_prog;
    M.P = s->mprog.as<MaskProgram>();
    M.key = in.key;
    M.topic = (MP.meta & MASK_META_TOPIC) ? in.topic : nullptr;
    M.partition = (MP.meta & MASK_META_PARTITION) ? in.partition : nullptr;
    M.offset = (MP.meta & MASK_META_OFFSET) ? in.offset : nullptr;
    M.ts = (MP.meta & MASK_META_TS) ? in.ts : nullptr;
    M.pos = s->cur_pos;
    M.n = n;
    M.base = s->carry ? s->base : 0;
    M.mask = s->follow_split ? s->mcol.as<int32_t>() : nullptr;
    uintptr_t bits = reinterpret_cast<uintptr_t>(M.key) | reinterpret_cast<uintptr_t>(M.topic) |
                     reinterpret_cast<uintptr_t>(M.partition) | reinterpret_cast<uintptr_t>(M.offset) |
                     reinterpret_cast<uintptr_t>(M.ts) | reinterpret_cast<uintptr_t>(M.pos);
    for (int c = 0; c < b->n_cols && c < 16; c++)
      if (MP.used >> c & 1) {
        M.cols[c] = in.cols[c];
        bits |= reinterpret_cast<uintptr_t>(M.cols[c]);
      }
    if (bits & 15) return fail(CEP_E_ARG, "device columns must be 16-byte aligned");
    if (s->follow_split && size_t(n) * 4 > s->mcol.cap) return fail(CEP_E_ARG, "batch larger than the session capacity");
  } else {
    col = b->n_cols ? in.cols[SP.col] : nullptr;
    topic = SP.use_topic ? in.topic : nullptr;
    if (SP.use_topic && !topic) {                  // no topic column: every record on topic id 0
      if (s->h_topic.ensure(size_t(n) * 4)) return fail(CEP_E_HIP, "staging allocation failed");
      HIPCHECK(hipMemsetAsync(s->h_topic.p, 0, size_t(n) * 4, st));
      topic = s->h_topic.as<int32_t>();
    }
    if (!col) return fail(CEP_E_ARG, "null value column");
    if ((reinterpret_cast<uintptr_t>(in.key) | reinterpret_cast<uintptr_t>(col) | reinterpret_cast<uintptr_t>(topic)) & 15)
      return fail(CEP_E_ARG, "device columns must be 16-byte aligned");
  }
  const int64_t nt = follow_tiles(n);
  if (size_t(nt) * 64 * size_t(SP.k + 1) * 8 > s->fw_bits.cap) return fail(CEP_E_ARG, "batch larger than the session capacity");
  if (s->scan_tmp.ensure(size_t(nt / 16 + 4) * 8)) return fail(CEP_E_HIP, "allocation failed");
  int64_t* scal = s->scal.as<int64_t>();
  FollowArgs A{};
  A.key = in.key; A.val = col; A.topic = topic; A.n = n;
  A.prog_dev = s->prog.as<StencilProgram>();
  A.k = SP.k; A.coltype = SP.coltype; A.use_topic = SP.use_topic; A.next_mask = s->follow_next;
  A.bits = s->fw_bits.as<unsigned long long>();
  A.sum = s->fw_sum.as<unsigned long long>();
  A.tile_starts = s->fw_tile.as<int64_t>();
  A.wcnt = s->fw_cnt.as<int64_t>();
  A.wpre = s->fw_pre.as<int64_t>();
  A.scan_tmp = s->scan_tmp.as<int64_t>();
  A.nm = scal + 4;
  A.max_span = reinterpret_cast<unsigned long long*>(scal + 5);
  if (s->carry) return push_follow_carry(s, A, M, st);
  if (s->follow_many) return push_follow_many(s, A, M, st);
  HIPCHECK(follow_planes_launch(s, A, M, st));
  HIPCHECK(follow_count_launch(A, st));
  // the batch's one host synchronisation: the completed walks and their longest span
  int64_t h[2] = {0, 0};
  HIPCHECK(hipMemcpyAsync(h, scal + 4, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  const int64_t nm = h[0], span = h[1];
  if (nm < 0 || nm > n) return fail(CEP_E_RUN_CAPACITY, "more completed walks than records");
  if (nm > 0) {
    int bits = 1;                                  // bits of the completing record
    while ((int64_t(1) << bits) <= n) bits++;
    const bool ranked = span <= 1024 && !getenv_flag("KCEP_RUNS_RADIX");
    size_t tmp_bytes = 0;
    if (!ranked) HIPCHECK(runs_sort(nullptr, nullptr, nm, bits, nullptr, &tmp_bytes, st));
    if (s->rk.ensure(size_t(nm) * 8) || s->rk_sorted.ensure(size_t(nm) * 8) ||
        (ranked ? s->r_len.ensure(size_t(nm) * 8) : s->rk_tmp.ensure(std::max<size_t>(tmp_bytes, 16))))
      return fail(CEP_E_HIP, "allocation failed");
    A.keys = s->rk.as<unsigned long long>();
    HIPCHECK(follow_write_launch(A, st));
    // (completing record, start) order: the runs path's windowed rank when every walk spans <= 1024
    // records, else its radix sort over the completing record's bits
    if (ranked)
      HIPCHECK(runs_order_launch(A.keys, nm, int(span), s->rk_sorted.as<unsigned long long>(), s->r_len.as<int64_t>(), st));
    else
      HIPCHECK(runs_sort(A.keys, s->rk_sorted.as<unsigned long long>(), nm, bits, s->rk_tmp.p, &tmp_bytes, st));
  }
  HIPCHECK(follow_rows_launch(A, s->rk_sorted.as<unsigned long long>(), nm, s->out.as<int32_t>(), s->total.as<int64_t>(), st));
  if (s->timing) HIPCHECK(hipEventRecord(s->eb1, st));
  return CEP_OK;
}

int push_general(cep_session* s, const cep_batch* b, hipStream_t st) {
  const Program& P = s->pat->prog;
  const int64_t n = b->n;
  if (s->jit_on && !s->jitg_tried) {           // a stencil / runs session's first batch that needs the NFA
    s->jitg = jit_general(P, s->jit_why, s->opts.flags & CEP_SESSION_PROFILE);
    s->jitg_tried = true;
  }
  NfaArgs A{};
  A.P = s->dprog.as<DevProgram>();
  A.n = n;
  A.mode = s->opts.mode;
  int rc = stage_inputs(s, b, st, A, false);
  if (rc) return rc;
  s->d_key = A.key;
  reset_results(s);
  s->nseg = 0;
  s->stopped_keys = s->stopped_records = 0;
  const bool stop = (b->flags & CEP_BATCH_STOP_AT_ERROR) != 0;
  A.base = s->carry ? s->base : 0;
  A.pos = s->cur_pos;
  if (n == 0) return push_empty(s, st, true);
  // segments: one per key run of the grouped batch.  A wave-kernel batch of a session that has run one
  // before leaves the count on the device (NfaArgs.nseg_dev, read by the kernel and the scans): no host
  // round trip before the kernel -- per-segment buffers are sized for n segments, the pool estimate is the
  // last batch's (a pool overflow re-runs the batch with a larger one, as always)
  const bool dev_count = s->wave && !s->carry && s->nseg_hint > 0 && n < (int64_t(1) << 31);
  const size_t nb = size_t(n / 1024 + 2) * 16;
  if (s->seg.ensure(size_t(n + 1) * 8) || s->scan_tmp.ensure(nb) || s->scal.ensure(64) || s->ctl.ensure(128))
    return fail(CEP_E_HIP, "allocation failed");
  int64_t* scal = s->scal.as<int64_t>();
  HIPCHECK(nfa_segments(A.key, n, nullptr, nullptr, s->seg.as<int64_t>(), scal, s->scan_tmp.as<int64_t>(), st));
  int64_t nseg = n;                               // (an upper bound until the kernel's results are read)
  if (!dev_count) {
    int64_t segs[2] = {0, 0};                     // segment count, carry key-check flags
    if (s->carry) {
      HIPCHECK(hipMemsetAsync(scal + 1, 0, 8, st));
      HIPCHECK(carry_keycheck_launch(n, scal, A.key, s->seg.as<int64_t>(), max_keys32(s),
                                     s->kstamp.as<int32_t>(), ++s->batch_no, reinterpret_cast<unsigned long long*>(scal + 1),
                                     st));
    }
    HIPCHECK(hipMemcpyAsync(segs, scal, sizeof segs, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    nseg = segs[0];
    if ((rc = key_check(uint64_t(segs[1])))) return rc;
    if (nseg >= (int64_t(1) << 31)) return fail(CEP_E_ARG, "too many keys in one batch");
  }
  const int64_t nseg_est = dev_count ? s->nseg_hint : nseg;
  s->nseg = nseg;
  A.nseg = int32_t(nseg);
  A.nseg_dev = dev_count ? scal : nullptr;
  A.seg_start = s->seg.as<int64_t>();
  const DevProgram& D = P.dev;
  NfaCaps cap = kCaps;
  const double scale = s->opts.arena_scale > 0 ? s->opts.arena_scale : 1.0;
  cap.heap_mult = std::max<int32_t>(1, int32_t(cap.heap_mult * scale));
  cap.out_mult = std::max<int32_t>(1, int32_t(cap.out_mult * scale));
  const size_t sb = size_t(nseg) * 8;
  if (s->r_matches.ensure(sb) || s->r_words.ensure(sb) || s->r_out.ensure(sb) || s->r_ent.ensure(sb) || s->r_err.ensure(sb) ||
      s->r_errrec.ensure(sb) || s->r_carry.ensure(sb) || s->moff.ensure(sb) || s->eoff.ensure(sb))
    return fail(CEP_E_HIP, "allocation failed");
  // first-allocation words of every key (NfaCaps) plus the events carried into the batch
  const int64_t per_key = 48 + 16 * cap.q0 + 3 * D.nstates * (cap.seq_base + 1) + cap.heap_base + cap.out_base + 16;
  const int64_t per_ev = 4 * D.nslots + cap.heap_mult + cap.out_mult + 4 + 3 * D.nstates;
  int64_t est = nseg_est * per_key + (n + (s->carry ? s->cpool_used / 4 : 0)) * per_ev;
  s->pool_est = std::max<int64_t>(s->pool_est, est + est / 2 + (int64_t(1) << 20));
  // a workload that needed a regrown pool starts from that size (no re-run per batch), until kPoolQuiet
  // batches in a row fit the estimate again
  s->pool_words = std::max(s->pool_est, s->pool_learned);
  A.cap = cap;
  A.carry = s->carry ? 1 : 0;
  A.max_keys = max_keys32(s);
  A.res_matches = s->r_matches.as<int64_t>();
  A.res_words = s->r_words.as<int64_t>();
  A.res_out = s->r_out.as<int64_t>();
  A.res_ent = s->r_ent.as<int64_t>();
  A.res_err = s->r_err.as<int32_t>();
  A.res_err_rec = s->r_errrec.as<int64_t>();
  A.res_carry = s->r_carry.as<int64_t>();
  unsigned long long* ctl = s->ctl.as<unsigned long long>();
  A.pool_top = ctl;
  A.cpool_top = ctl + 1;
  A.flags = reinterpret_cast<int32_t*>(ctl + 2);
  A.err_any = ctl + 4;
  // CEP_BATCH_STOP_AT_ERROR: ctl[6] the earliest exception (~position, 0 none), ctl[7..8] stopped segments / records
  A.stop_at = stop ? ctl + 6 : nullptr;
  const int nctl = stop ? 9 : 5;                   // ctl words the host reads back
  bool stop_hit = false;                           // the batch raised with the flag on: it stops at p*
  // the kernels' build with the early-out in it: compiled for the pattern at the session's first flagged
  // batch (on failure the built-in interpreting one, as for every compiled kernel)
  if (stop && s->jitg && !s->jitg_stop_tried) {
    s->jitg_stop = jit_general(P, s->jit_why, s->opts.flags & CEP_SESSION_PROFILE, true);
    s->jitg_stop_tried = true;
  }
  const JitModule* jm = stop ? s->jitg_stop.get() : s->jitg.get();
  // lane kernel: 64 key segments per wave (fewer diverge less but leave the chip emptier: C4 gained 5 %
  // at 8 per wave, light keys lost 2x, profiles/r01_s5_nfa_spread_*.log)
  A.wave_agg = (wave_stateful(D) ? 1 : 0) | (P.has_seq ? 2 : 0);
  A.spread = 64;
  if (s->opts.flags & CEP_SESSION_PROFILE) {
    if (s->r_prof.ensure(sb * NFA_PROFILE_W)) return fail(CEP_E_HIP, "allocation failed");
    A.profile = s->r_prof.as<int64_t>();
  }
  // the wave kernel's persistent grid and its workgroups' scratch regions (nfa_wave.h): 16 K words
  // each by default (KCEP_WAVE_SCRATCH words, 0: none -- every workspace from the pool)
  int64_t wgrid = 0;
  if (s->wave) {
    const char* scr_env = getenv("KCEP_WAVE_SCRATCH");
    const int64_t scr_words = scr_env ? std::max<int64_t>(0, atoll(scr_env)) & ~int64_t(3) : int64_t(1) << 14;
    wgrid = nfa_wave_grid(nseg, A.wave_agg != 0, jm, stop);
    A.scratch_words = scr_words;
    if (scr_words > 0) {
      if (s->wscratch.ensure(size_t(wgrid * scr_words) * 4)) return fail(CEP_E_HIP, "allocation failed");
      A.scratch = s->wscratch.as<int32_t>();
    }
  }
  // the wave kernel's schedule: segments by estimated cost, heaviest first (nfa_dev.h stage_may_take;
  // KCEP_NFA_ORDER=0: as they come, the tests' hook onto that order)
  if (s->wave && !getenv_flag_off("KCEP_NFA_ORDER")) {
    // ord_bucket: a byte per segment, then a byte per record (the per-record estimate bits)
    // ord_cnt: 16 bucket sizes per 256 segments
    if (s->ord.ensure(size_t(nseg) * 4) || s->ord_bucket.ensure(size_t(nseg) + size_t(n)) ||
        s->ord_cnt.ensure(size_t((nseg + 255) / 256) * 64))
      return fail(CEP_E_HIP, "allocation failed");
    A.seg_bucket = s->ord_bucket.as<uint8_t>();
    HIPCHECK(nfa_order_launch(A, nseg, s->ord_bucket.as<uint8_t>() + nseg, s->ord_cnt.as<unsigned>(), s->ord.as<int32_t>(),
                              st, s->jitg.get(), NFA_ORDER_LO));
    A.seg_order = s->ord.as<int32_t>();
  }
  bool timed = false;
  bool grew = false;                               // the pool was regrown for this batch: given back after it
  bool pool_at_limit = false;                      // the pool cannot grow further: overflowing keys are handed back
  int64_t tots[2] = {0, 0};                        // matches, entries of the batch
  // the CSR's arrays as the earlier batches left them: a first attempt that fits them is compacted
  // before the host reads its totals (one synchronisation per batch instead of two)
  const int64_t cap_m = int64_t(std::min({s->o_record.cap / 8, s->o_key.cap / 4, s->o_entoff.cap / 8}));
  const int64_t cap_e = int64_t(std::min(s->o_name.cap / 4, s->o_entrec.cap / 8));
  bool spec = false;                               // the first attempt's compaction is enqueued
  int attempts = 0;
  for (int attempt = 0;; attempt++) {
    attempts = attempt + 1;
    if (s->pool.ensure(size_t(s->pool_words) * 4)) {
      if (s->pool_words <= s->pool_est) return fail(CEP_E_RUN_CAPACITY, "cannot allocate the NFA pool");
      (void)hipGetLastError();                     // the learned size no longer fits: back to the estimate
      s->pool_learned = 0;
      s->pool_words = s->pool_est;
      if (s->pool.ensure(size_t(s->pool_words) * 4)) return fail(CEP_E_RUN_CAPACITY, "cannot allocate the NFA pool");
    }
    if (s->carry && s->cpool_used + nseg * 64 > s->cpool_words) {
      if ((rc = carry_gc(s, 2 * (s->cpool_used + nseg * 64), st))) return rc;
    }
    A.pool = s->pool.as<int32_t>();
    A.pool_cap = s->pool_words;
    A.ctab = s->carry ? s->ctab.as<int64_t>() : nullptr;
    A.cpool = s->carry ? s->cpool.as<int32_t>() : nullptr;
    A.cpool_cap = s->carry ? s->cpool_words : 0;
    A.last_attempt = attempt >= kMaxRetry || pool_at_limit ? 1 : 0;   // then an overflowing key is handed back per key
    A.max_key_words = s->opts.max_key_words;
    // ctl: pool top, carry-pool top, flags (2 words), err_any, next segment, then the stop words (a kernel,
    // not a copy command)
    HIPCHECK(set_words_launch(reinterpret_cast<int64_t*>(ctl), stop ? 9 : 6, 1, s->cpool_used, st));
    if (!timed) HIPCHECK(hipEventRecord(s->ev0, st));
    A.seg_next = reinterpret_cast<int32_t*>(ctl + 5);
    if (s->wave) HIPCHECK(nfa_wave_launch(A, wgrid, st, jm));
    else HIPCHECK(nfa_launch(A, st, jm ? jm->nfa : nullptr));
    if (!timed) HIPCHECK(hipEventRecord(s->ev1, st));
    timed = true;
    // CEP_BATCH_STOP_AT_ERROR: the keys' counts cut to the matches before the earliest exception
    if (stop) HIPCHECK(nfa_trim_launch(A, nseg, st));
    // the CSR's match / entry counts are scanned right away, so that one synchronisation reads them
    // with the pool flags (a retried attempt scans again)
    HIPCHECK(exclusive_scan_pair(s->r_matches.as<int64_t>(), s->r_words.as<int64_t>(), nseg, A.nseg_dev,
                                 s->moff.as<int64_t>(), s->eoff.as<int64_t>(), scal + 3, scal + 4,
                                 s->scan_tmp.as<int64_t>(), st));
    if (attempt == 0 && cap_m > 0 && cap_e > 0) {
      HIPCHECK(nfa_compact_launch(nseg, A.nseg_dev, cap_m, cap_e, scal + 3, A.key, A.seg_start, s->r_out.as<int64_t>(),
                                  s->r_ent.as<int64_t>(), s->moff.as<int64_t>(), s->eoff.as<int64_t>(),
                                  s->o_record.as<int64_t>(), s->o_key.as<int32_t>(), s->o_entoff.as<int64_t>(),
                                  s->o_name.as<int32_t>(), s->o_entrec.as<int64_t>(), st));
      spec = true;
    }
    // the flags and counts into pinned host memory by one small kernel (two copy commands cost ~25 us
    // of gaps), then the batch's one synchronisation
    int64_t* h_res_dev = nullptr;
    if ((rc = results_page(s, &h_res_dev))) return rc;
    HIPCHECK(gather_words_launch(reinterpret_cast<const int64_t*>(ctl), nctl, scal, 5, h_res_dev, st));
    HIPCHECK(hipStreamSynchronize(st));
    unsigned long long res[5];
    int64_t sc[5];                                 // [0] segments, [3] matches, [4] entries
    for (int q = 0; q < 5; q++) {
      res[q] = (unsigned long long)s->h_res[q];
      sc[q] = s->h_res[nctl + q];
    }
    stop_hit = stop && s->h_res[6] != 0;
    s->stopped_keys = stop_hit ? s->h_res[7] : 0;
    s->stopped_records = stop_hit ? s->h_res[8] : 0;
    tots[0] = sc[3];
    tots[1] = sc[4];
    if (dev_count && attempt == 0) {               // the exact count from here on
      nseg = sc[0];
      s->nseg = nseg;
      A.nseg = int32_t(nseg);
    }
    s->g_any_err = res[4] != 0;
    const int32_t* fl = reinterpret_cast<const int32_t*>(res + 2);
    if ((rc = key_check(fl[2] ? 1 : 0))) return rc;   // (the kernel's own check: a key id out of range)
    s->live_hwm = fl[3];
    if (!fl[0] && !fl[1]) {
      if (s->carry && !stop_hit) s->cpool_used = int64_t(res[1]);   // (a stopped batch commits no state)
      break;
    }
    if ((attempt >= kMaxRetry || pool_at_limit) && fl[0])
      return fail(CEP_E_RUN_CAPACITY, "the NFA workspace pool cannot grow");
    if (attempt >= kMaxRetry && fl[1]) return fail(CEP_E_RUN_CAPACITY, "the carried-state pool cannot grow");
    if (fl[0]) {                                   // workspace pool exhausted: twice the pool, same inputs,
      s->pool.release();                           // within the session's budget (cep_opts.max_pool_bytes,
      size_t free_b = 0, total_b = 0;              // default a quarter of the HBM) and the free HBM (keeping
      HIPCHECK(hipMemGetInfo(&free_b, &total_b));  // 1/16 of it): past that a key is handed back per key
      // (the wave kernel's scratch regions count against the budget too)
      const int64_t budget = ((s->opts.max_pool_bytes > 0 ? s->opts.max_pool_bytes : int64_t(total_b / 4)) -
                              int64_t(s->wscratch.cap)) / 4;
      const int64_t room = std::min<int64_t>(int64_t(free_b / 4) - int64_t(free_b / 64), budget);
      const int64_t want = std::min<int64_t>(s->pool_words * 2, room);
      if (want <= s->pool_words) pool_at_limit = true;
      else s->pool_words = want;
      grew = true;
    }
    if (fl[1]) {                                   // carry pool exhausted: compact into a larger one
      if ((rc = carry_gc(s, 2 * s->cpool_words, st))) return rc;
    }
  }
  // compaction into the CSR (counts scanned with the last attempt)
  s->nseg_hint = nseg;
  s->last_attempts = attempts;
  const int64_t pool_used = s->h_res[0];           // the successful attempt's pool top
  s->g_matches = tots[0];
  s->g_entries = tots[1];
  if (!(spec && attempts == 1 && tots[0] <= cap_m && tots[1] <= cap_e)) {
    // (arrays grown with a quarter of headroom, so that the next batches compact speculatively)
    const size_t nm = size_t(std::max<int64_t>(tots[0], 1)), ne = size_t(std::max<int64_t>(tots[1], 1));
    const size_t hm = nm + nm / 4 + 256, he = ne + ne / 4 + 256;
    if ((s->o_record.cap < nm * 8 && s->o_record.ensure(hm * 8)) || (s->o_key.cap < nm * 4 && s->o_key.ensure(hm * 4)) ||
        (s->o_entoff.cap < nm * 8 && s->o_entoff.ensure(hm * 8)) || (s->o_name.cap < ne * 4 && s->o_name.ensure(he * 4)) ||
        (s->o_entrec.cap < ne * 8 && s->o_entrec.ensure(he * 8)))
      return fail(CEP_E_HIP, "allocation failed");
    HIPCHECK(nfa_compact_launch(nseg, nullptr, tots[0], tots[1], nullptr, A.key, A.seg_start, s->r_out.as<int64_t>(),
                                s->r_ent.as<int64_t>(), s->moff.as<int64_t>(), s->eoff.as<int64_t>(),
                                s->o_record.as<int64_t>(), s->o_key.as<int32_t>(), s->o_entoff.as<int64_t>(),
                                s->o_name.as<int32_t>(), s->o_entrec.as<int64_t>(), st));
  }
  if (s->carry) {                                  // NFAStore.put of every key of the batch
    HIPCHECK(carry_commit_launch(nseg, A.key, A.seg_start, s->r_carry.as<int64_t>(), s->r_err.as<int32_t>(),
                                 s->ctab.as<int64_t>(), A.stop_at, st));
    s->base += n;
    s->stop_uncommitted = stop_hit ? s->stop_uncommitted + n : 0;
  }
  HIPCHECK(hipEventRecord(s->eb1, st));
  if (grew) {                                      // the next batches start from the grown size
    s->pool_learned = s->pool_words;
    s->pool_quiet = 0;
  } else if (s->pool_learned > 0) {
    s->pool_quiet = pool_used > s->pool_est ? 0 : s->pool_quiet + 1;
    if (s->pool_quiet >= kPoolQuiet) {
      // kPoolQuiet batches in a row within the estimate: the grown pool is given back, so one heavy stretch
      // does not hold the device for the session's lifetime (the compaction has read the matches out of it)
      HIPCHECK(hipStreamSynchronize(st));
      s->pool.release();
      s->wscratch.release();
      s->pool_learned = 0;
      s->pool_quiet = 0;
    }
  }
  // the reference fails the task at its first exception: report the earliest failing record
  if (s->g_any_err) {                              // (no key raised: nothing to read back)
    std::vector<int32_t> err(static_cast<size_t>(nseg));
    std::vector<int64_t> erec(static_cast<size_t>(nseg));
    HIPCHECK(hipMemcpyAsync(err.data(), s->r_err.p, size_t(nseg) * 4, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(erec.data(), s->r_errrec.p, size_t(nseg) * 8, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    for (int64_t i = 0; i < nseg; i++)
      if (err[size_t(i)]) {
        if (s->g_err_rec < 0 || erec[size_t(i)] < s->g_err_rec) {
          s->g_err = err[size_t(i)];
          s->g_err_rec = erec[size_t(i)];
        }
        s->e_rec.push_back(erec[size_t(i)]);       // segments are in stream order, so e_rec ascends
        s->e_code.push_back(err[size_t(i)]);
      }
  }
  if (s->carry && s->cpool_used > s->cpool_words / 4 * 3) {   // keep room for the next batch
    if ((rc = carry_gc(s, 0, st))) return rc;
  }
  return CEP_OK;
}

// CEP_BATCH_ARRIVAL_ORDER: the batch (records in arrival order, host or device) grouped by key on the device
// (group.hip) into the session's grouped columns; gb describes them (device memory, flags without
// CEP_BATCH_ARRIVAL_ORDER, CEP_BATCH_DELIVER added for the stencil / chain paths, whose rows the delivery
// then writes in arrival order); s->cur_pos = every grouped record's stream position (base + arrival index)
int group_batch(cep_session* s, const cep_batch* b, hipStream_t st, cep_batch& gb, const void** gcols) {
  const Program& P = s->pat->prog;
  const int64_t n = b->n;
  NfaArgs in{};                                    // the batch's columns on the device (host ones staged)
  // small batches are read over the link in place (staged by DMA instead, the grouping kernels took 12 us
  // less but the flush 16 us more: the copy sits on the stream in front of them)
  int rc = stage_inputs(s, b, st, in, true);
  if (rc) return rc;
  const size_t n4 = size_t(n) * 4, n8 = size_t(n) * 8;
  const size_t heads = size_t(s->opts.max_keys + 1) * 8;
  if (!s->g_head.p || !s->g_top.p) {               // epoch-tagged list heads and the node counter: zeroed once
    if (s->g_head.ensure(heads) || s->g_top.ensure(16) || hipMemsetAsync(s->g_head.p, 0, heads, st) ||
        hipMemsetAsync(s->g_top.p, 0, 16, st))
      return fail(CEP_E_HIP, "allocation failed");
  }
  if (s->g_key.ensure(n4) || s->g_arr.ensure(n4) || s->g_pos.ensure(n8) || s->g_nodes.ensure(8 * n4) ||
      s->g_start.ensure(n8) || s->scal.ensure(64) ||
      s->a_cnt.ensure(n8) || s->a_ecnt.ensure(n8) || s->a_head.ensure(n4) || (in.valid && s->g_valid.ensure(size_t(n))) ||
      (in.topic && s->g_topic.ensure(n4)) || (in.partition && s->g_part.ensure(n4)) || (in.offset && s->g_off.ensure(n8)) ||
      (in.ts && s->g_ts.ensure(n8)))
    return fail(CEP_E_HIP, "allocation failed");
  GroupArgs G{};
  G.max_keys = int32_t(std::min<int64_t>(s->opts.max_keys, INT32_MAX - 1));
  G.stamp = ++s->group_stamp;
  G.head = s->g_head.as<unsigned long long>();
  G.node_top = s->g_top.as<int32_t>();
  int32_t* nodes = s->g_nodes.as<int32_t>();
  G.node_key = nodes; G.node_chunk = nodes + n; G.node_cnt = nodes + 2 * n; G.node_next = nodes + 3 * n;
  G.node_prefix = nodes + 4 * n; G.node_leader = nodes + 5 * n; G.rec_node = nodes + 6 * n; G.rec_rank = nodes + 7 * n;
  G.start = s->g_start.as<int64_t>();
  G.cursor = s->g_top.as<unsigned long long>() + 1;
  G.key = in.key; G.g_key = s->g_key.as<int32_t>(); G.arr = s->g_arr.as<int32_t>(); G.pos = s->g_pos.as<int64_t>();
  G.base = s->base;
  G.valid = in.valid; G.g_valid = in.valid ? s->g_valid.as<uint8_t>() : nullptr;
  G.topic = in.topic; G.g_topic = in.topic ? s->g_topic.as<int32_t>() : nullptr;
  G.partition = in.partition; G.g_partition = in.partition ? s->g_part.as<int32_t>() : nullptr;
  G.offset = in.offset; G.g_offset = in.offset ? s->g_off.as<int64_t>() : nullptr;
  G.ts = in.ts; G.g_ts = in.ts ? s->g_ts.as<int64_t>() : nullptr;
  G.ncols = b->n_cols;
  for (int c = 0; c < b->n_cols; c++) {
    if (s->g_cols[c].ensure(size_t(n) * type_size(P.coltypes[c]))) return fail(CEP_E_HIP, "allocation failed");
    G.cols[c] = in.cols[c];
    G.g_cols[c] = s->g_cols[c].p;
    G.coltype[c] = P.coltypes[c];
    gcols[c] = s->g_cols[c].p;
  }
  G.cnt = s->a_cnt.as<int64_t>();
  G.ecnt = s->a_ecnt.as<int64_t>();
  HIPCHECK(group_launch(G, n, st));
  gb = *b;
  gb.key_id = G.g_key; gb.valid = G.g_valid; gb.topic = G.g_topic; gb.partition = G.g_partition;
  gb.offset = G.g_offset; gb.ts = G.g_ts;
  gb.cols = gcols;
  gb.mem = CEP_MEM_DEVICE;
  gb.flags = (b->flags & ~uint32_t(CEP_BATCH_ARRIVAL_ORDER)) | CEP_BATCH_DELIVER;
  s->cur_pos = G.pos;
  return CEP_OK;
}

// the general / runs CSR of an arrival-order batch into arrival order of the completing record (group.hip);
// base: the batch's first stream position
int arrival_csr(cep_session* s, int64_t base, int64_t n, hipStream_t st) {
  if (!s->e_rec.empty()) {                         // exceptions: ascending position, the first one reported
    std::vector<std::pair<int64_t, int32_t>> e;
    for (size_t i = 0; i < s->e_rec.size(); i++) e.emplace_back(s->e_rec[i], s->e_code[i]);
    std::sort(e.begin(), e.end());
    for (size_t i = 0; i < e.size(); i++) {
      s->e_rec[i] = e[i].first;
      s->e_code[i] = e[i].second;
    }
    s->g_err_rec = e[0].first;
    s->g_err = e[0].second;
  }
  const int64_t nm = s->g_matches, ne = s->g_entries;
  if (nm <= 0) return CEP_OK;
  const size_t hm = size_t(nm + nm / 4 + 256), he = size_t(ne + ne / 4 + 256);
  if ((s->a_record.cap < size_t(nm) * 8 && s->a_record.ensure(hm * 8)) ||
      (s->a_key.cap < size_t(nm) * 4 && s->a_key.ensure(hm * 4)) ||
      (s->a_entoff.cap < size_t(nm) * 8 && s->a_entoff.ensure(hm * 8)) ||
      (s->a_name.cap < size_t(ne) * 4 && s->a_name.ensure(he * 4)) ||
      (s->a_entrec.cap < size_t(ne) * 8 && s->a_entrec.ensure(he * 8)) || s->a_moff.ensure(size_t(n) * 8) ||
      s->a_moffe.ensure(size_t(n) * 8) || s->a_tmp.ensure(size_t(n / 1024 + 4) * 16) || s->scal.ensure(64))
    return fail(CEP_E_HIP, "allocation failed");
  HIPCHECK(arrival_reorder(s->o_record.as<int64_t>(), s->o_key.as<int32_t>(), s->o_entoff.as<int64_t>(),
                           s->o_name.as<int32_t>(), s->o_entrec.as<int64_t>(), nm, ne, base, n, s->a_cnt.as<int64_t>(),
                           s->a_ecnt.as<int64_t>(), s->a_head.as<int32_t>(), s->a_moff.as<int64_t>(),
                           s->a_moffe.as<int64_t>(), s->scal.as<int64_t>() + 6, s->a_tmp.as<int64_t>(),
                           s->a_record.as<int64_t>(), s->a_key.as<int32_t>(), s->a_entoff.as<int64_t>(),
                           s->a_name.as<int32_t>(), s->a_entrec.as<int64_t>(), st));
  std::swap(s->o_record, s->a_record);
  std::swap(s->o_key, s->a_key);
  std::swap(s->o_entoff, s->a_entoff);
  std::swap(s->o_name, s->a_name);
  std::swap(s->o_entrec, s->a_entrec);
  return CEP_OK;
}

// the high-water marks of a stencil / chain / runs carry session: FILTER_MAX_TOPICS per key id, none set
// (allocated at the first filtered push, or by an imported blob that carries marks)
int marks_ensure(cep_session* s, hipStream_t st) {
  if (s->f_marks.p) return CEP_OK;
  const size_t bytes = size_t(s->opts.max_keys) * FILTER_MAX_TOPICS * 8;
  if (s->f_marks.ensure(bytes) || s->f_stage.ensure(bytes)) {
    s->f_marks.release();
    return fail(CEP_E_HIP, "mark table allocation failed");
  }
  HIPCHECK(hipMemsetAsync(s->f_marks.p, 0xFF, bytes, st));   // -1: the reference's latestOffsets default
  return CEP_OK;
}

// CEP_BATCH_FILTER: the key-grouped batch b (the caller's, host or device, or group_batch's output with
// s->cur_pos) through filter.hip into the session's filtered columns; fb describes them (device memory,
// no valid column, offsets monotone by construction, fb.n = the admitted records), s->cur_pos = their stream
// positions.  Waits for the admitted count -- the paths' launches are sized by it -- the way cep_collect
// waits for a delivery.  The marks are staged; the caller commits them once the path has taken the batch.
int filter_batch(cep_session* s, const cep_batch* b, hipStream_t st, cep_batch& fb, const void** fcols) {
  const Program& P = s->pat->prog;
  const int64_t n = b->n;
  NfaArgs in{};
  int rc = stage_inputs(s, b, st, in, true);
  if (rc) return rc;
  const bool marks = s->opts.mode == CEP_MODE_PROCESSOR && in.offset;
  if (marks && (rc = marks_ensure(s, st))) return rc;
  const size_t nt = size_t((n + FILTER_TF - 1) / FILTER_TF), n4 = size_t(n) * 4, n8 = size_t(n) * 8;
  if (s->f_tile_f.ensure(nt * 4) || s->f_tile_v.ensure(nt * FILTER_MAX_TOPICS * 8) || s->f_tile_cnt.ensure(nt * 4) ||
      s->f_tile_off.ensure(nt * 8) || s->f_slot.ensure(nt * FILTER_TF * 2) || s->f_scal.ensure(16) ||
      s->f_key.ensure(n4) || s->f_pos.ensure(n8) || (in.topic && s->f_topic.ensure(n4)) ||
      (in.partition && s->f_part.ensure(n4)) || (in.offset && s->f_off.ensure(n8)) || (in.ts && s->f_ts.ensure(n8)))
    return fail(CEP_E_HIP, "allocation failed");
  if (!s->f_host) {
    HIPCHECK(s->f_host.alloc(64, hipHostMallocMapped | hipHostMallocCoherent));
    memset(s->f_host.p, 0, 64);
  }
  FilterArgs F{};
  F.key = in.key; F.valid = in.valid; F.topic = in.topic; F.partition = in.partition; F.offset = in.offset; F.ts = in.ts;
  F.pos = s->cur_pos;
  F.base = s->base;
  F.ncols = b->n_cols;
  for (int c = 0; c < b->n_cols; c++) {
    if (s->f_cols[c].ensure(size_t(n) * type_size(P.coltypes[c]))) return fail(CEP_E_HIP, "allocation failed");
    F.cols[c] = in.cols[c];
    F.coltype[c] = P.coltypes[c];
    F.o_cols[c] = s->f_cols[c].p;
    fcols[c] = s->f_cols[c].p;
  }
  F.o_key = s->f_key.as<int32_t>(); F.o_topic = s->f_topic.as<int32_t>(); F.o_partition = s->f_part.as<int32_t>();
  F.o_offset = s->f_off.as<int64_t>(); F.o_ts = s->f_ts.as<int64_t>(); F.o_pos = s->f_pos.as<int64_t>();
  F.use_marks = marks ? 1 : 0;
  F.max_keys = max_keys32(s);
  F.marks = s->f_marks.as<int64_t>();
  F.stage = s->f_stage.as<int64_t>();
  F.tile_f = s->f_tile_f.as<int32_t>(); F.tile_v = s->f_tile_v.as<int64_t>(); F.tile_cnt = s->f_tile_cnt.as<int32_t>();
  F.tile_off = s->f_tile_off.as<int64_t>(); F.slot = s->f_slot.as<uint16_t>();
  F.n_dev = s->f_scal.as<int64_t>();
  F.bad = s->f_scal.as<int64_t>() + 1;
  HIPCHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&F.host), s->f_host.p, 0));
  F.stamp = ++s->f_stamp;
  HIPCHECK(filter_launch(F, n, st));
  s->f_args = F;
  // filter_offsets stamps the host words once the count is there: spin on the stamp (a stream wait sleeps
  // and wakes microseconds late); a stamp that does not come -- a fault -- is left to the stream wait
  const volatile int64_t* stamp = s->f_host.p + 2;
  const auto t0 = std::chrono::steady_clock::now();
  while (*stamp != F.stamp) {
    if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) {
      HIPCHECK(hipStreamSynchronize(st));
      if (*stamp != F.stamp) return fail(CEP_E_HIP, "the filter kernels did not complete");
      break;
    }
    __builtin_ia32_pause();
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  const int64_t adm = s->f_host.p[0];
  if (s->f_host.p[1])
    return fail(CEP_E_UNSUPPORTED, "CEP_BATCH_FILTER: a record's topic id is outside [0, CEP_FILTER_MAX_TOPICS)");
  if (adm < 0 || adm > n) return fail(CEP_E_HIP, "the filter's admitted count is out of range");
  fb = *b;
  fb.n = adm;
  fb.key_id = F.o_key;
  fb.valid = nullptr;
  fb.topic = in.topic ? F.o_topic : nullptr;
  fb.partition = in.partition ? F.o_partition : nullptr;
  fb.offset = in.offset ? F.o_offset : nullptr;
  fb.ts = in.ts ? F.o_ts : nullptr;
  fb.cols = fcols;
  fb.mem = CEP_MEM_DEVICE;
  fb.flags = (b->flags & ~uint32_t(CEP_BATCH_FILTER)) | CEP_BATCH_OFFSETS_MONOTONE;
  s->cur_pos = F.o_pos;
  return CEP_OK;
}

}  // namespace kcep
