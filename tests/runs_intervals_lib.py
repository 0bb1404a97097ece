"""Directed tests of the runs path's match placement (test_runs_intervals_cpu.py, test_runs_intervals_gpu.py):
a pattern whose set of (start, end) pairs the input chooses freely, the closed form of its matches, the expected
CSR built with numpy alone, and builders of the interval sets that aim at runs_emit's chunks, buckets and entry
windows and at runs_order's rank window.

Schema (lim, idx): idx[j] is record j's index within its key segment, lim[j] is 0 or the idx at which the run
started at j shall end.  A start j with lim[j] = idx[j] + span matches iff span >= the form's smallest span and
record j + span lies in j's key segment; the match is emitted at e = j + span with span + 1 entries, the last
stage's first.  Matches come in (e, j) order.

A batch is a list of keys, (key id, segment length, {start offset: span}), laid out one after the other."""
from collections import namedtuple

import numpy as np

from kcep import QueryBuilder, Schema, Event, States

SCHEMA = Schema([("lim", "i32"), ("idx", "i32")])
COLTYPES = [1, 1]

_lim, _idx = Event.field("lim"), Event.field("idx")


def three_stages():
    """first, mid+, last: runs_sim records four segment words per run (runs_emit<SEG4 = true>)"""
    return (QueryBuilder().select("first").where(_lim > 0).fold("L", _lim).then()
            .select("mid").oneOrMore().where(States.getInt("L") > _idx).then()
            .select("last").where(States.getInt("L") <= _idx).build())


def six_stages():
    """first, p1, p2, p3, mid+, last: a run consumes six stages, so eight segment words (SEG4 = false)"""
    b = QueryBuilder().select("first").where(_lim > 0).fold("L", _lim)
    for nm in ("p1", "p2", "p3"):
        b = b.then().select(nm).where(_idx >= 0)
    return (b.then().select("mid").oneOrMore().where(States.getInt("L") > _idx).then()
            .select("last").where(States.getInt("L") <= _idx).build())


# smin: the smallest span that matches (mid needs one record); pre: the single stages between first and mid
Form = namedtuple("Form", "name build smin pre")
THREE = Form("three", three_stages, 2, ())
SIX = Form("six", six_stages, 5, ("p1", "p2", "p3"))
FORMS = {"three": THREE, "six": SIX}


def chunk_of(n):
    """the records per chunk of a batch of n"""
    # a copy of runs_chunk (csrc/kcep_dev.h): RUNS_CHUNK = 1024, halved while n < chunk * 3072, not below 128
    c = 1024
    while c > 128 and n < c * 3072:
        c >>= 1
    return c


CHUNK_FROM = {256: 786_432, 512: 1_572_864, 1024: 3_145_728}     # the first n of each class


# ---- columns, model, expected CSR ----
def n_records(keys):
    return sum(k[1] for k in keys)


def columns(keys):
    """key, lim, idx (int32) of the batch"""
    ids = np.array([k[0] for k in keys], np.int64)
    lens = np.array([k[1] for k in keys], np.int64)
    bases = np.concatenate([[0], np.cumsum(lens)[:-1]])
    n = int(lens.sum())
    key = np.repeat(ids, lens).astype(np.int32)
    idx = (np.arange(n, dtype=np.int64) - np.repeat(bases, lens)).astype(np.int32)
    lim = np.zeros(n, np.int32)
    for (_, seglen, runs), base in zip(keys, bases):
        if runs:
            off = np.fromiter(runs.keys(), np.int64, len(runs))
            assert off.min() >= 0 and off.max() < seglen
            lim[base + off] = off + np.fromiter(runs.values(), np.int64, len(runs))
    return key, lim, idx


def intervals(keys, form):
    """(start, end, key) of every match as int64 arrays, in the output's order: by (end, start)"""
    js, es, ks = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    base = 0
    for kid, seglen, runs in keys:
        if runs:
            off = np.fromiter(runs.keys(), np.int64, len(runs))
            sp = np.fromiter(runs.values(), np.int64, len(runs))
            ok = (sp >= form.smin) & (off + sp < seglen)
            js.append(base + off[ok])
            es.append(base + off[ok] + sp[ok])
            ks.append(np.full(int(ok.sum()), kid, np.int64))
        base += seglen
    j, e, k = np.concatenate(js), np.concatenate(es), np.concatenate(ks)
    order = np.lexsort((j, e))
    return j[order], e[order], k[order]


def model(keys, form):
    """the match list in the form of gpu_util.product_matches / oracle_matches"""
    j, e, k = intervals(keys, form)
    pre = list(form.pre)
    out = []
    for a, b, key in zip(j.tolist(), e.tolist(), k.tolist()):
        trav = [("last", b)] + [("mid", r) for r in range(b - 1, a + len(pre), -1)]
        trav += [(nm, a + 1 + q) for q, nm in reversed(list(enumerate(pre)))] + [("first", a)]
        out.append((b, key, trav))
    return out


def expected_csr(keys, form, names):
    """match_record, match_key, ent_off, ent_name, ent_record as Session.collect returns them; names:
    CompiledPattern.names"""
    j, e, k = intervals(keys, form)
    sp = e - j
    ln = sp + 1
    ent_off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    pos = np.arange(int(ent_off[-1]), dtype=np.int64) - np.repeat(ent_off[:-1], ln)    # 0: last ... span: first
    left = np.repeat(sp, ln) - pos                                                     # records after the start
    ent_record = np.repeat(e, ln) - pos
    ent_name = np.full(len(pos), names.index("mid"), np.int32)
    ent_name[pos == 0] = names.index("last")
    ent_name[left == 0] = names.index("first")
    for q, nm in enumerate(form.pre, 1):
        ent_name[left == q] = names.index(nm)
    return dict(match_record=e.astype(np.int64), match_key=k.astype(np.int32), ent_off=ent_off, ent_name=ent_name,
                ent_record=ent_record.astype(np.int64))


def unpack(csr, names):
    """gpu_util.product_matches over the five arrays"""
    off, nm, rec = csr["ent_off"].tolist(), csr["ent_name"].tolist(), csr["ent_record"].tolist()
    return [(int(csr["match_record"][m]), int(csr["match_key"][m]),
             [(names[nm[i]], rec[i]) for i in range(off[m], off[m + 1])]) for m in range(len(csr["match_record"]))]


def longest_span(keys, form):
    j, e, _ = intervals(keys, form)
    return int((e - j).max())


def inversions(keys, form):
    """pairs of matches whose start order and output order differ"""
    j, _, _ = intervals(keys, form)
    return int(np.sum(np.triu(j[:, None] > j[None, :], 1)))


def chunk_entries(keys, form, C):
    """per match: its end chunk and the range [a, b) of its entries counted from the chunk's first entry"""
    j, e, _ = intervals(keys, form)
    ln = e - j + 1
    off = np.concatenate([[0], np.cumsum(ln)])
    ch = e // C
    first = np.searchsorted(ch, ch, side="left")           # the chunk's first match
    a = off[:-1] - off[first]
    return ch, a, a + ln


# ---- scenario builders: (C, base, form, ...) -> (segment length, {start offset: span}) ----
# base is the batch record at which the key begins: chunks are counted in batch records.
def boundary(C, base, lead):
    """the first multiple of C at least `lead` records past base and 2C past the batch start"""
    return -(-max(base + lead, 2 * C) // C) * C


class _Runs:
    def __init__(self, base):
        self.base, self.runs = base, {}

    def put(self, start, span):
        assert start >= self.base and start - self.base not in self.runs and span >= 1, (start, span)
        self.runs[start - self.base] = int(span)

    def free(self, start):
        return start >= self.base and start - self.base not in self.runs

    def seg(self, end):
        return end - self.base, self.runs


def chunk_edges(C, base, form):
    """shortest runs and runs of span C-1 ending on B-1, B, B+1 (the one ending on B starts exactly C-1
    records before the chunk); a run starting on a chunk's last record and one on its first"""
    B, s, r = boundary(C, base, C), form.smin, _Runs(base)
    for d in (-1, 0, 1):
        r.put(B + d - (C - 1), C - 1)
        r.put(B + d - s, s)
    if r.free(B - 1):
        r.put(B - 1, s)
    r.put(B, s)
    return r.seg(B + s + 2)


def fat_bucket(C, base, form):
    """min(C - smin, 300) consecutive starts that all end on B+5; around them in start order, runs ending
    on B+4 and B+6"""
    B, s, r = boundary(C, base, C + 48), form.smin, _Runs(base)
    m, E = min(C - s, 300), B + 5
    for i in range(m):
        r.put(E - s - i, s + i)
    for k in range(1, 41):                                  # before the block, alternating B+4 / B+6
        start = E - s - m + 1 - k
        span = (E - 1 if k & 1 else E + 1) - start
        if s <= span <= C - 1:
            r.put(start, span)
    r.put(E + 1 - s, s)                                     # after the block: ends on B+6
    return r.seg(E + 3)


def fat_bucket_size(C, form):
    return min(C - form.smin, 300)


def onion(C, base, form):
    """nested runs: start s+q, end s+C-1-q, down to the shortest span that matches.  The output order is the
    start order reversed."""
    B, r = boundary(C, base, C), _Runs(base)
    s0 = B - 3 * C // 4
    m = 0
    while C - 1 - 2 * m >= form.smin:
        r.put(s0 + m, C - 1 - 2 * m)
        m += 1
    return r.seg(s0 + C + 1)


def onion_size(C, form):
    return (C - 1 - form.smin) // 2 + 1


def entry_windows(C, base, form):
    """40 runs of span C-1 (at C = 128: of span 100..127) ending in one chunk: more than 4096 entries there.  A
    shortest run onto the chunk's first record keeps the others (C entries each) off the multiples of 2048."""
    B, r = boundary(C, base, C), _Runs(base)
    r.put(B - form.smin, form.smin)
    end = 0
    for k in range(40):
        start, span = (B - 99 + k, 100 + 7 * k % 28) if C == 128 else (B - (C - 1) + k, C - 1)
        r.put(start, span)
        end = max(end, start + span)
    assert B <= end < B + C
    return r.seg(end + 2)


def batch_end(C, base, form, n):
    """the batch's last key: a run of span C-1 and a shortest one ending on record n-1, and an open run that
    would end on record n"""
    r, s = _Runs(base), form.smin
    assert n - base >= C + 1
    r.put(n - C, C - 1)
    r.put(n - 1 - s, s)
    r.put(n - s, s)
    return r.seg(n)


def random_key(C, base, form, rng, length):
    """start density 0.3; 90 % of the spans in smin..8, the rest uniform in smin..C-1"""
    r = _Runs(base)
    for o in np.flatnonzero(rng.random(length) < 0.3).tolist():
        span = rng.integers(form.smin, 9) if rng.random() < 0.9 else rng.integers(form.smin, C)
        r.put(base + o, span)
    return r.seg(base + length)


def window_edge(C, base, form, long=1024):
    """One run of span `long` whose next 1023 - smin records each start a shortest run: all of those end before
    it, so it moves that many places.  Three copies: at the key's start, after 1300 more matches, and ending on
    the key's last record."""
    r, s = _Runs(base), form.smin
    k = 1023 - s

    def copy(j):
        r.put(j, long)
        for i in range(1, k + 1):
            r.put(j + i, s)
        return j + long

    p = copy(base) + 1
    for i in range(1300):
        r.put(p + i, s)
    p = copy(p + 1300 + s + 1) + 1
    for i in range(10):
        r.put(p + i, s)
    end = copy(p + 10 + s + 1)
    return r.seg(end + 1)


def window_edge_moves(form):
    return 1023 - form.smin


def group_skip(C, base, form, rng):
    """4000 consecutive starts of the shortest span, 2 % of them raised to a span uniform in 256..1024 (two at
    fixed places, so that both ends of a group of 16 hold one)"""
    r = _Runs(base)
    span = np.full(4000, form.smin)
    long = rng.random(4000) < 0.02
    long[[16 * 10 + 15, 16 * 20]] = True
    span[long] = rng.integers(256, 1025, int(long.sum()))
    for o in range(4000):
        r.put(base + o, span[o])
    return r.seg(base + 4000 + 1024 + 1)


def ties(C, base, form, rng):
    """900 consecutive starts: 700 end on one record E, 200 (seeded) are shortest runs that end before E"""
    r, s = _Runs(base), form.smin
    s0 = base + 1
    E = s0 + 899 + s
    short = set(rng.choice(880, 200, replace=False).tolist())
    for o in range(900):
        r.put(s0 + o, s if o in short else E - (s0 + o))
    return r.seg(E + 2)


def span_equals_chunk(C, base, form):
    """runs of span exactly C ending on B-1, B, B+1, next to shortest ones and one of half a chunk"""
    B, s, r = boundary(C, base, C + 2), form.smin, _Runs(base)
    for d in (-1, 0, 1):
        r.put(B + d - C, C)
        r.put(B + d - s, s)
    r.put(B - C // 2, C // 2 + 3)
    return r.seg(B + s + 3)


# ---- batches ----
class Layout:
    def __init__(self, C, form):
        self.C, self.form, self.keys, self.n = C, form, [], 0

    def add(self, builder, *a):
        seglen, runs = builder(self.C, self.n, self.form, *a)
        self.keys.append((len(self.keys), seglen, runs))
        self.n += seglen
        return len(self.keys) - 1

    def filler(self, upto):
        """a key that starts no run, up to batch record `upto`"""
        assert upto > self.n
        self.keys.append((len(self.keys), upto - self.n, {}))
        self.n = upto


def front(L, seed):
    """scenarios 1-4 and 6, one key each (6: four keys of 50..3C records); the key numbers by scenario"""
    rng = np.random.default_rng(seed)
    at = dict(edges=L.add(chunk_edges), fat=L.add(fat_bucket), onion=L.add(onion), windows=L.add(entry_windows))
    at["random"] = [L.add(random_key, rng, int(rng.integers(50, 3 * L.C + 1))) for _ in range(4)]
    return at


def small_batch(form, tail, seed=1):
    """scenarios 1-6 at C = 128 in one batch of n records, n % 128 == tail"""
    L = Layout(128, form)
    at = front(L, seed)
    n = L.n + 128 + 8
    n += (tail - n) % 128
    at["end"] = L.add(batch_end, n)
    return L.keys, at


def large_batch(C, n, form, seed=2):
    """scenarios 1-6 at the front, a key that starts no run, scenarios 1 and 5 again in the last 3C records"""
    L = Layout(C, form)
    at = front(L, seed)
    at["end"] = L.add(batch_end, L.n + 2 * C)
    Bt = (n - C - form.smin - 4) // C * C                  # the tail's chunk boundary
    L.filler(Bt - C)
    at["tail_edges"] = L.add(chunk_edges)
    assert boundary(C, Bt - C, C) == Bt and n - (Bt - C) <= 3 * C + form.smin + 4
    at["tail_end"] = L.add(batch_end, n)
    assert L.n == n
    return L.keys, at


def span_chunk_batch(C, n, form):
    """scenario 10 in a batch of n records (n: None -- as short as it comes)"""
    L = Layout(C, form)
    L.add(span_equals_chunk)
    if n is not None:
        L.filler(n)
    return L.keys


def single(builder, C, form, *a):
    """one scenario as a batch of one key"""
    L = Layout(C, form)
    L.add(builder, *a)
    return L.keys
