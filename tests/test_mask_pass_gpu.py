"""CEP_SESSION_MASK_PASS on the device: strict patterns whose predicates read several columns, arithmetic
or event metadata run on the stencil / chain path behind the mask pre-pass (csrc/masks.hip), in both
builds of the pre-pass (compiled for the pattern, and the built-in interpreting kernel).  Every comparison
is an exact list against the CPU oracle."""
import functools
import os

import numpy as np
import pytest

import oracle as O
from kcep import native as N
from kcep import synth, Schema, QueryBuilder, Event, Selected
from kcep.ingest import ColumnDecoder
from kcep.processor import GpuCEPProcessor
from kcep.sequence import Event as Ev, sequence_from_traversal
from gpu_util import oracle_matches, product_matches
import filter_util as U
import mask_pass_lib as ML

pytestmark = pytest.mark.gpu

BUILDS = pytest.mark.parametrize("interpret", [False, True], ids=["jit", "interp"])
I32 = Schema([("value", "i32")])
PV_T = [2, 2]
RICH_T = [1, 2, 3]


@functools.lru_cache(maxsize=None)
def ir_of(name):
    sch, build = {"p2": (ML.PV, ML.p2), "cyc3": (ML.PV, ML.cyc3), "chain3": (ML.PV, ML.chain3),
                  "chain4": (ML.PV, ML.chain4), "rich": (ML.RICH, ML.rich)}.get(name, (ML.PV, None))
    if build is None:                                    # "k<n>"
        return ML.k_stages(int(name[1:])).to_ir(ML.PV)
    return build().to_ir(sch)


def run_mp(ir, key, cols, interpret, mode=N.MODE_PROCESSOR, mask_pass=True, **kw):
    cp = N.CompiledPattern(ir)
    s = N.Session(cp, max(1, len(key)), mode=mode, mask_pass=mask_pass, interpret=interpret)
    s.push(len(key), np.ascontiguousarray(key, np.int32), [np.ascontiguousarray(c) for c in cols], **kw)
    out = s.collect()
    return product_matches(s, out), s, out


# ---- 1. path choice ----
@BUILDS
def test_path_choice(interpret):
    key, cols = ML.pv_stream(20_000, 200, 1)
    ir = ir_of("p2")
    want = oracle_matches(ir, key, cols, PV_T, O.MODE_PROCESSOR)
    assert len(want) > 0
    got0, s0, _ = run_mp(ir, key, cols, interpret, mask_pass=False)
    assert s0.path != N.PATH_STENCIL and got0 == want    # the path it always opened on
    got, s, out = run_mp(ir, key, cols, interpret)
    assert s.path == N.PATH_STENCIL and out["path"] == N.PATH_STENCIL
    assert s.jit == (not interpret)
    assert got == want
    # the direct form keeps the direct form: C2 with the flag is the same session
    k2, v2, order = synth.c2_stream_np(20_000, 300)
    c2 = synth.c2_pattern().to_ir(I32)
    a, sa, _ = run_mp(c2, k2, [v2], interpret, mask_pass=False)
    b, sb, _ = run_mp(c2, k2, [v2], interpret)
    assert sa.path == sb.path == N.PATH_STENCIL and not sb.jit
    assert a == b == oracle_matches(c2, k2, [v2], [1], O.MODE_PROCESSOR) and len(a) > 0


# ---- 2. sizes: the pre-pass's vector tails, one thread, one tile, several tiles ----
@functools.lru_cache(maxsize=None)
def sized(n, keys):
    if n <= 5:                                           # every record takes every stage of P2: (price, volume) = (1, 2)
        key = np.sort(np.arange(n) % keys).astype(np.int32)
        cols = [np.full(n, 1, np.int64), np.full(n, 2, np.int64)]
    else:
        key, cols = ML.pv_stream(n, keys, n + keys)
    return key, cols, oracle_matches(ir_of("p2"), key, cols, PV_T, O.MODE_PROCESSOR)


@BUILDS
@pytest.mark.parametrize("kk", ["1", "13", "n/2"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 4095, 4096, 4097, 12289, 65537])
def test_sizes(n, kk, interpret):
    keys = max(1, n // 2) if kk == "n/2" else int(kk)
    key, cols, want = sized(n, keys)
    if n > 5 or -(-n // keys) >= 3:                      # some key holds three records
        assert len(want) > 0
    else:
        assert want == []                                # n <= 5, records dealt round over the keys: no key holds three
    got, s, _ = run_mp(ir_of("p2"), key, cols, interpret)
    assert s.path == N.PATH_STENCIL
    assert got == want


# ---- 3. tile boundaries: the record before a tile goes through mask_of ----
N_B = 3 * 4096 + 5
BREAKS = [None] + [b + off for b in (16 * 40, 1024 * 2, 4096 * 2) for off in range(3)]


@functools.lru_cache(maxsize=None)
def boundary_case(brk, shift):
    i = np.arange(N_B)
    key = np.zeros(N_B, np.int32) if brk is None else (i >= brk).astype(np.int32)
    t = (i + shift) % 3                                  # the stage record i takes
    vol = (i // 2) % 3
    pri = (t - 2 * vol) % 3                              # (price + 2 * volume) % 3 == t: the two fields jointly
    cols = [pri.astype(np.int64), vol.astype(np.int64)]
    return key, cols, oracle_matches(ir_of("cyc3"), key, cols, PV_T, O.MODE_PROCESSOR)


@BUILDS
@pytest.mark.parametrize("knob", ["KCEP_STENCIL_KEYED", "KCEP_STENCIL_SPARSE_KEYS", "KCEP_STENCIL_DENSE_KEYS"])
@pytest.mark.parametrize("brk", BREAKS)
def test_boundaries(brk, knob, interpret, monkeypatch):
    monkeypatch.setenv(knob, "1")
    for shift in range(3):
        key, cols, want = boundary_case(brk, shift)
        assert len(want) > 0
        got, s, _ = run_mp(ir_of("cyc3"), key, cols, interpret)
        assert s.path == N.PATH_STENCIL
        assert got == want, shift
        if brk is None:                                  # every record of stage 2 from record 2 on completes a match
            t = (np.arange(N_B) + shift) % 3
            assert [m[0] for m in got] == [j for j in np.flatnonzero(t == 2).tolist() if j >= 2]


# ---- 4. k = 1..8 (k = 8: mask bit 7, the keyed kernel) ----
@functools.lru_cache(maxsize=None)
def k_case(k):
    key, cols = ML.pv_stream(50_000, 300, k)
    return key, cols, oracle_matches(ir_of(f"k{k}"), key, cols, PV_T, O.MODE_PROCESSOR)


@BUILDS
@pytest.mark.parametrize("k", range(1, 9))
def test_k_stages(k, interpret):
    key, cols, want = k_case(k)
    assert len(want) > 0
    got, s, _ = run_mp(ir_of(f"k{k}"), key, cols, interpret)
    assert s.path == N.PATH_STENCIL
    assert got == want


# ---- 5. chain: skip slots are mask bits 4..7 ----
@functools.lru_cache(maxsize=None)
def chain_case(name, n):
    key, cols = ML.pv_stream(n, 300 if n > 10_000 else 30, n)
    return key, cols, oracle_matches(ir_of(name), key, cols, PV_T, O.MODE_PROCESSOR)


@BUILDS
@pytest.mark.parametrize("n", [4097, 50_000])
@pytest.mark.parametrize("name", ["chain3", "chain4"])
def test_chain(name, n, interpret):
    key, cols, want = chain_case(name, n)
    assert len(want) > 0
    assert any(len(m[2]) < int(name[-1]) for m in want)  # some match skipped an optional stage
    got, s, out = run_mp(ir_of(name), key, cols, interpret)
    assert s.path == N.PATH_CHAIN and out["path"] == N.PATH_CHAIN
    assert got == want


# ---- 6. types and metadata ----
@BUILDS
@pytest.mark.parametrize("mode", [N.MODE_NFA, N.MODE_PROCESSOR], ids=["nfa", "processor"])
@pytest.mark.parametrize("explicit", [True, False], ids=["arrays", "null"])
def test_types_and_metadata(explicit, mode, interpret):
    key, cols, topic, partition, offset, ts = ML.rich_stream(20_000, 100, 6)
    assert np.isnan(cols[2]).any() and (cols[0].astype(np.int64) ** 2 > 2 ** 31).any()
    kw = dict(topic=topic, partition=partition, offset=offset, ts=ts) if explicit else {}
    omode = O.MODE_PROCESSOR if mode == N.MODE_PROCESSOR else O.MODE_NFA_PER_KEY
    want = oracle_matches(ir_of("rich"), key, cols, RICH_T, omode, **kw)
    assert len(want) > 0
    got, s, _ = run_mp(ir_of("rich"), key, cols, interpret, mode=mode,
                       flags=N.BATCH_OFFSETS_MONOTONE if explicit else 0, **kw)
    assert s.path == N.PATH_STENCIL
    assert got == want


# ---- 7. carry ----
def filter_stream(seed, n, n_keys):
    """an arrival-order (price, volume) stream with null records and re-deliveries (filter_util.make_stream);
    the volume follows from key and offset, so a re-delivered record carries the same contents"""
    rng = np.random.default_rng(seed)
    st = U.make_stream(rng, rng.integers(0, n_keys, n).astype(np.int32), ntopics=1)
    st["vol"] = ((st["off"] * 7 + st["key"] * 3) % 4).astype(np.int64)
    st["pri"] = st.pop("val").astype(np.int64)
    return st


def _cuts(seed, n, m):
    rng = np.random.default_rng(seed)
    c = sorted(rng.choice(np.arange(1, n), m, replace=False).tolist())
    return [0] + c[:2] + [c[2], c[2], c[2] + 1] + c[3:] + [n]      # an empty batch and a 1-record batch among them


def _oracle_pv(ir, st, with_valid):
    kw = dict(valid=st["valid"], offset=st["off"]) if with_valid else {}
    return oracle_matches(ir, st["key"], [st["pri"], st["vol"]], PV_T, O.MODE_PROCESSOR, topic=st["topic"], ts=st["ts"], **kw)


@BUILDS
@pytest.mark.parametrize("variant", ["grouped", "arrival", "filter"])
@pytest.mark.parametrize("name", ["p2", "chain3"])
def test_carry(name, variant, interpret):
    n, n_keys = 20_000, 120
    ir = ir_of(name)
    st = filter_stream(17 if name == "p2" else 18, n, n_keys)
    bounds = _cuts(5, n, 9)
    flt = variant == "filter"
    if not flt:                                          # a clean stream: every record valid, no offsets handed over
        st["valid"][:] = 1
    parts = [U.take(st, np.arange(a, b)) for a, b in zip(bounds[:-1], bounds[1:])]
    if variant == "grouped":
        parts = [U.grouped(p) for p in parts]
    pushed = U.concat(parts)                             # the stream as the device sees it
    want = _oracle_pv(ir, pushed, flt)
    assert len(want) > 0
    flags = {"grouped": N.BATCH_OFFSETS_MONOTONE,
             "arrival": N.BATCH_OFFSETS_MONOTONE | N.BATCH_ARRIVAL_ORDER | N.BATCH_DELIVER,
             "filter": N.BATCH_FILTER | N.BATCH_ARRIVAL_ORDER | N.BATCH_DELIVER}[variant]
    cp = N.CompiledPattern(ir)
    cap = max(len(p["key"]) for p in parts)

    def open_session():
        s = N.Session(cp, cap, carry=True, max_keys=n_keys, mask_pass=True, interpret=interpret)
        assert s.path == (N.PATH_CHAIN if name == "chain3" else N.PATH_STENCIL)
        return s

    def push(s, p):
        kw = dict(valid=p["valid"], offset=p["off"]) if flt else {}
        s.push(len(p["key"]), p["key"], [p["pri"], p["vol"]], topic=p["topic"], ts=p["ts"], flags=flags, **kw)

    s = open_session()
    got, late = [], None
    for i, p in enumerate(parts):
        if i == len(parts) // 2:                         # checkpoint, restore into a fresh session, go on there
            blob = s.state_export()
            pos = s.stream_position()
            s = open_session()
            s.state_import(blob)
            assert s.stream_position() == pos
        push(s, p)
        if variant == "arrival" and i == 1:              # collected after the next push (cep_collect_batch)
            late = s.batch_id()
            continue
        if late is not None:
            got += product_matches(s, s.collect(batch_id=late))
            late = None
        got += product_matches(s, s.collect())
    assert s.stream_position() == n
    assert got == want, (len(got), len(want))


# ---- 8. the processor ----
def pv_records(seed, n_keys, n):
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        recs.append([f"user-{int(rng.integers(0, n_keys))}", (int(rng.integers(0, 4)), int(rng.integers(0, 4))),
                     "events", 0, i, 1000 + i])
    for _ in range(n // 20):                             # the same record delivered again later
        i = int(rng.integers(0, n))
        recs.insert(int(rng.integers(i + 1, len(recs) + 1)), list(recs[i]))
    for i in rng.choice(len(recs), len(recs) // 20, replace=False):
        recs[i][int(rng.random() < 0.5)] = None          # a null key or a null value
    return [tuple(r) for r in recs]


def seq_view(seq):
    return [(s.getStage(), [e.offset for e in s.getEvents()]) for s in seq.matched()]


def oracle_forward(ir, recs):
    keys, kid, pri, vol, valid = {}, [], [], [], []
    for k, v, *_ in recs:
        kid.append(keys.setdefault(k, len(keys)) if k is not None else 0)
        pri.append(0 if v is None else v[0])
        vol.append(0 if v is None else v[1])
        valid.append(0 if (k is None or v is None) else 1)
    p = O.OraclePattern(ir)
    r = O.OracleRun(p, O.MODE_PROCESSOR)
    r.process(O.BatchArrays(np.asarray(kid, np.int32), [np.asarray(pri, np.int64), np.asarray(vol, np.int64)], PV_T,
                            valid=np.asarray(valid, np.uint8), offset=np.asarray([x[4] for x in recs], np.int64),
                            ts=np.asarray([x[5] for x in recs], np.int64)))

    def event_of(i):
        k, v, t, pa, o, ts_ = recs[i]
        return Ev(k, v, ts_, t, pa, o)
    return [(recs[m.record][0], seq_view(sequence_from_traversal(m.traversal, p.names, event_of)))
            for m in r.matches(with_groups=False)]


@BUILDS
@pytest.mark.parametrize("device_filter", [False, True], ids=["host_marks", "device_filter"])
@pytest.mark.parametrize("batch", [1, 7, 1000])
def test_processor(batch, device_filter, interpret, monkeypatch):
    if interpret:
        monkeypatch.setenv("KCEP_JIT", "0")
    recs = pv_records(batch, 12, 400 if batch == 1 else 1500)
    want = oracle_forward(ir_of("p2"), recs)
    assert len(want) > 0
    dec = ColumnDecoder(ML.PV, [lambda v: v[0], lambda v: v[1]])
    proc = GpuCEPProcessor("p2", ML.p2(), ML.PV, dec, batch_size=batch, max_keys=64, mask_pass=True,
                           device_filter=device_filter)
    got = []
    proc.init(lambda k, s: got.append((k, seq_view(s))))
    assert proc.session.path == N.PATH_STENCIL and proc.session.jit == (not interpret)
    for r in recs:
        proc.process(*r)
    proc.close()
    assert got == want


# ---- 9. random eligible patterns ----
_a, _b = map(int, os.environ.get("KCEP_FUZZ_SEEDS", "0:12").split(":"))
SEEDS = range(_a, _b)


def random_pattern(rng):
    """An eligible pattern by construction: k in 1..8, optionals only when k <= 4 (never first or last),
    every predicate an OR / AND of the accepted forms over the rich schema; stage 0 compares two columns,
    so the direct lowering never takes it."""
    A, B, Cc = ML.A, ML.B, ML.Cc

    def atom():
        f = int(rng.integers(0, 10))
        if f == 0:
            return A * A > int(rng.integers(0, 2000))                    # i32 overflow
        if f == 1:
            return B % int(rng.integers(2, 8)) <= int(rng.integers(0, 3))
        if f == 2:
            return B.asDouble() / Cc > float(rng.integers(0, 4))         # NaN, division by +-0.0
        if f == 3:
            return A + B > int(rng.integers(0, 40))
        if f == 4:
            return Event.timestamp() % 3 != int(rng.integers(0, 3))
        if f == 5:
            return Event.timestamp() - Event.offset() <= int(rng.integers(1, 5))
        if f == 6:
            return Event.partition() != int(rng.integers(0, 3))
        if f == 7:
            return Cc * 2.0 >= float(rng.integers(-2, 3))
        if f == 8:
            return ~(A.asLong() * 3 - B == int(rng.integers(0, 10)))
        return B - A.asLong() / 7 > int(rng.integers(-5, 10))

    k = int(rng.integers(1, 9))
    opt = set()
    if 3 <= k <= 4:
        opt = {i for i in range(1, k - 1) if rng.random() < 0.6}
    b = None
    for i in range(k):
        sel = Selected.withStrictContiguity()
        if rng.random() < 0.15:
            sel = sel.withTopic("t0")
        st = (QueryBuilder() if b is None else b.then()).select(f"f{i}", sel)
        if i in opt:
            st = st.optional()
        pred = atom() | atom()
        if i == 0:
            pred = (A < B) | pred
        elif rng.random() < 0.3:
            pred = pred & (atom() | atom())
        b = st.where(pred)
    return b.build()


def fuzz_stream(rng, n, n_keys):
    """arrival order: (key, [a, b, c], topic, partition, offset, ts)"""
    key = rng.integers(0, n_keys, n).astype(np.int32)
    a = rng.choice(np.array([0, 3, 40, -50, 46341, 65536, -2 ** 31, 2 ** 31 - 1], np.int64), n).astype(np.int32)
    b = rng.integers(0, 32, n).astype(np.int64)
    c = rng.choice(np.array([np.nan, 0.0, -0.0, 1.0, 4.0, 13.0, -2.0]), n)
    topic = (rng.random(n) < 0.2).astype(np.int32)
    partition = rng.integers(0, 3, n).astype(np.int32)
    offset = np.arange(n, dtype=np.int64)
    ts = offset + rng.integers(0, 6, n)
    return dict(key=key, a=a, b=b, c=c, topic=topic, partition=partition, offset=offset, ts=ts)


def _fz_kw(st):
    return dict(topic=st["topic"], partition=st["partition"], offset=st["offset"], ts=st["ts"])


def fuzz_case(seed):
    rng = np.random.default_rng(1000 + seed)
    ir = random_pattern(rng).to_ir(ML.RICH)
    return ir, fuzz_stream(rng, 12_000, 48)


@BUILDS
@pytest.mark.parametrize("seed", SEEDS)
def test_random_patterns(seed, interpret):
    ir, st = fuzz_case(seed)
    cp = N.CompiledPattern(ir)
    ok, k, chain, why = cp.mask_pass
    assert ok, why                                       # eligible by construction: no seed is skipped
    n = len(st["key"])
    # one batch, grouped by key
    g = U.take(st, np.argsort(st["key"], kind="stable"))
    cols = [g["a"], g["b"], g["c"]]
    want = oracle_matches(ir, g["key"], cols, RICH_T, O.MODE_PROCESSOR, **_fz_kw(g))
    assert len(want) > 0
    s = N.Session(cp, n, mask_pass=True, interpret=interpret)
    assert s.path == (N.PATH_CHAIN if chain else N.PATH_STENCIL)
    s.push(n, g["key"], cols, flags=N.BATCH_OFFSETS_MONOTONE, **_fz_kw(g))
    got = product_matches(s, s.collect())
    assert got == want
    if cp.info.runs_ok:                                  # the path it runs on without the flag
        r = N.Session(cp, n, force_path=N.PATH_RUNS, interpret=interpret)
        r.push(n, g["key"], cols, flags=N.BATCH_OFFSETS_MONOTONE, **_fz_kw(g))
        assert product_matches(r, r.collect()) == got
    # a carry session over three cuts, every batch grouped by key
    rng = np.random.default_rng(seed)
    bounds = [0] + sorted(rng.choice(np.arange(1, n), 3, replace=False).tolist()) + [n]
    parts = [U.grouped(U.take(st, np.arange(a, b))) for a, b in zip(bounds[:-1], bounds[1:])]
    pushed = U.concat(parts)
    want_c = oracle_matches(ir, pushed["key"], [pushed["a"], pushed["b"], pushed["c"]], RICH_T, O.MODE_PROCESSOR,
                            **_fz_kw(pushed))
    assert len(want_c) > 0
    sc = N.Session(cp, max(len(p["key"]) for p in parts), carry=True, max_keys=48, mask_pass=True, interpret=interpret)
    got_c = []
    for p in parts:
        sc.push(len(p["key"]), p["key"], [p["a"], p["b"], p["c"]], flags=N.BATCH_OFFSETS_MONOTONE, **_fz_kw(p))
        got_c += product_matches(sc, sc.collect())
    assert got_c == want_c
