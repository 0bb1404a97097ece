"""CEP_BATCH_FILTER on the stencil, chain and runs carry sessions: the null rule and the per-topic
high-water-mark rule of CEPProcessor.process (CEPProcessor.java:136-160) applied on the device.  Every case
pushes the raw stream -- nulls and re-deliveries included -- with the flag and compares matches, entries and
positions, element by element, with the oracle's single MODE_PROCESSOR pass over the same records."""
import numpy as np
import pytest

import oracle as O
from kcep import native as N, Schema
from kcep.ingest import StockEvent, stock_columns, scalar_column, STOCK_SCHEMA
from kcep.processor import GpuCEPProcessor, ProcessorFailed
from kcep.sequence import Event as Ev, sequence_from_traversal
import filter_util as U
from golden_util import scenarios
import patterns_lib as PL

pytestmark = pytest.mark.gpu

FILTER = N.BATCH_FILTER
ARRIVAL = N.BATCH_ARRIVAL_ORDER | N.BATCH_DELIVER
NAMES = list(U.PATTERNS)


def test_refusal_without_the_flag():
    """A stencil carry session refuses a batch with a valid column and a re-delivered offset, exactly as
    before; with the flag the same batch is taken and matches the oracle."""
    st = dict(key=np.zeros(6, np.int32), val=np.array([0, 1, 0, 2, 0, 0], np.int32), topic=np.zeros(6, np.int32),
              valid=np.array([1, 1, 1, 1, 0, 1], np.uint8), off=np.array([0, 1, 0, 2, 9, 3], np.int64),
              ts=np.arange(6, dtype=np.int64))
    s = U.open_session("c2", 16, 4)
    with pytest.raises(N.CepError, match="Unsupported"):
        U.push(s, st, 0)
    assert s.stream_position() == 0
    U.push(s, st, FILTER)
    got = U.matches(s, s.collect())
    # A(0) B(1) [A again: a re-delivery] C(3): the match closes over the gap
    assert got == [(3, 0, [("C", 3), ("B", 1), ("A", 0)])]
    assert got == U.oracle("c2", st)
    assert s.stream_position() == 6


def _keys(dist, n, rng):
    if dist == "one":                                    # one key: its segment crosses every tile boundary
        return np.full(n, 2, np.int32)
    if dist == "singles":                                # keys of one record each
        return rng.permutation(n).astype(np.int32)
    k = rng.integers(0, max(2, n // 8), n)               # a mix: a hot key holding half, the rest short
    k[rng.random(n) < 0.5] = 1
    return k.astype(np.int32)


def _sizes():
    tf = 1024                                            # (checked against the library in the test)
    return [1, tf - 1, tf, tf + 1, 3 * tf + 5]


@pytest.mark.parametrize("arrival", [False, True], ids=["grouped", "arrival"])
@pytest.mark.parametrize("dist", ["one", "singles", "mix"])
@pytest.mark.parametrize("n", _sizes())
@pytest.mark.parametrize("name", NAMES)
def test_size_classes(name, n, dist, arrival):
    """n around the admission scan's tile, two batches of n records each: the second re-delivers records of
    the first, so the carried marks are read in every tile."""
    assert N.filter_tile_records() == 1024
    rng = np.random.default_rng(n * 7 + len(dist))
    keys = np.concatenate([_keys(dist, n, rng)] * 2)
    st = U.make_stream(rng, keys, ntopics=8 if name == "topic" else 2, p_re=0.2)
    parts = [U.take(st, np.arange(a, a + n)) for a in (0, n)]
    if not arrival:
        parts = [U.grouped(p) for p in parts]
    want = U.oracle(name, U.concat(parts))
    s = U.open_session(name, n, int(keys.max()) + 1)
    got = U.run(s, parts, FILTER | (ARRIVAL if arrival else 0))
    assert s.stream_position() == 2 * n
    assert got == want, (len(got), len(want))


def _single_key(vals, offs, valid=None, topics=None):
    n = len(vals)
    return dict(key=np.zeros(n, np.int32), val=np.asarray(vals, np.int32),
                topic=np.asarray(topics if topics is not None else [0] * n, np.int32),
                valid=np.asarray(valid if valid is not None else [1] * n, np.uint8), off=np.asarray(offs, np.int64),
                ts=np.arange(n, dtype=np.int64))


@pytest.mark.parametrize("arrival", [False, True], ids=["grouped", "arrival"])
def test_offset_shapes(arrival):
    """Per key and topic: the mark minus one is dropped, the mark itself admitted; a jump back, then forward
    past the mark; nulls with high offsets move no mark; topics 0..7 interleaved keep a mark each."""
    fl = FILTER | (ARRIVAL if arrival else 0)
    # every valid record has value 0: with the 1-stage pattern the matches are exactly the admitted records
    cases = {
        "mark-1 dropped, mark admitted": _single_key([0] * 5, [0, 1, 1, 2, 1]),
        "back, then past the mark": _single_key([0] * 6, [5, 6, 2, 3, 7, 6]),
        "nulls move no mark": _single_key([0] * 5, [0, 900, 1, 901, 2], valid=[1, 0, 1, 0, 1]),
        "a mark per topic": _single_key([0] * 12, [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1],
                                        topics=[0, 1, 2, 3, 4, 5, 6, 7, 3, 4, 4, 3]),
    }
    admitted = {"mark-1 dropped, mark admitted": [0, 1, 3], "back, then past the mark": [0, 1, 4],
                "nulls move no mark": [0, 2, 4], "a mark per topic": [0, 1, 2, 3, 4, 5, 6, 7, 9, 11]}
    for label, st in cases.items():
        s = U.open_session("one", 16, 2)
        got = U.run(s, [st], fl)
        assert [m[0] for m in got] == admitted[label], label
        assert got == U.oracle("one", st), label
        # the same records cut in two batches: the marks carried across
        s = U.open_session("one", 16, 2)
        h = len(st["key"]) // 2
        got = U.run(s, [U.take(st, np.arange(0, h)), U.take(st, np.arange(h, len(st["key"])))], fl)
        assert got == U.oracle("one", st), label
    # a re-delivery between two records of a would-be match, on every multi-stage pattern: it closes over the gap
    for name, st, want in (("c2", _single_key([0, 1, 1, 2], [0, 1, 1, 2]), [(3, [3, 1, 0])]),
                           ("chain", _single_key([0, 1, 1, 2], [0, 1, 1, 2]), None),
                           ("topic", _single_key([0, 0, 1], [0, 0, 0], topics=[3, 3, 4]), [(2, [2, 0])])):
        s = U.open_session(name, 16, 2)
        got = U.run(s, [st], fl)
        assert want is None or [(m[0], [e[1] for e in m[2]]) for m in got] == want, name
        assert len(got) > 0 and got == U.oracle(name, st), name
    # a re-delivery on topic 3 does not block topic 4 (three keys, interleaved)
    rng = np.random.default_rng(5)
    st = U.make_stream(rng, rng.integers(0, 3, 400).astype(np.int32), ntopics=8, p_re=0.3)
    for name in ("topic", "runs"):
        s = U.open_session(name, 400, 3)
        got = U.run(s, [st if arrival else U.grouped(st)], fl)
        assert got == U.oracle(name, st if arrival else U.grouped(st)), name


@pytest.mark.parametrize("deliver", [False, True], ids=["plain", "deliver"])
@pytest.mark.parametrize("name", NAMES)
def test_every_record_dropped(name, deliver):
    """A batch without an admitted record is still a batch: an empty CSR, the position advanced by n, and
    the next batch continues from the state before it."""
    rng = np.random.default_rng(11)
    st = U.make_stream(rng, rng.integers(0, 5, 300).astype(np.int32), ntopics=8 if name == "topic" else 1)
    a, c = U.grouped(U.take(st, np.arange(0, 150))), U.grouped(U.take(st, np.arange(150, 300)))
    nulls = {k: v.copy() for k, v in a.items()}
    nulls["valid"][:] = 0                                # all null
    parts = [a, nulls, a, c]                             # ... then all re-deliveries (the first batch again)
    want = U.oracle(name, U.concat(parts))
    s = U.open_session(name, 150, 5)
    fl = FILTER | (N.BATCH_DELIVER if deliver else 0)
    got = []
    for i, b in enumerate(parts):
        U.push(s, b, fl)
        out = s.collect()
        if i in (1, 2):
            assert len(out["match_record"]) == 0 and len(out["ent_record"]) == 0 and list(out["ent_off"]) == [0]
        assert s.stream_position() == 150 * (i + 1)
        got += U.matches(s, out)
    assert len(want) > 0 and got == want


@pytest.mark.parametrize("name", NAMES)
def test_nothing_dropped_equals_monotone(name):
    rng = np.random.default_rng(3)
    st = U.grouped(U.make_stream(rng, rng.integers(0, 40, 2500).astype(np.int32), ntopics=8 if name == "topic" else 1,
                                 p_null=0, p_re=0))
    outs = []
    for fl in (FILTER, N.BATCH_OFFSETS_MONOTONE):
        s = U.open_session(name, 2500, 40)
        U.push(s, st, fl, with_valid=fl == FILTER)
        outs.append(s.collect())
    for f in ("match_record", "match_key", "ent_off", "ent_name", "ent_record"):
        assert np.array_equal(outs[0][f], outs[1][f]), f
    assert len(outs[0]["match_record"]) > 0


@pytest.mark.parametrize("arrival", [False, True], ids=["grouped", "arrival"])
@pytest.mark.parametrize("name", NAMES)
def test_carry(name, arrival):
    """Five batches with random cuts and re-deliveries of records of earlier batches; key 0 is absent from the
    third.  Between them: export / import into a fresh session, evict / import under another key id; then
    state_clear and a fresh stream."""
    rng = np.random.default_rng(21 + len(name))
    n, nk = 3000, 12
    keys = rng.integers(0, nk, n).astype(np.int32)
    cuts = [0] + sorted(rng.choice(np.arange(200, n - 200), 4, replace=False).tolist()) + [n]
    keys[cuts[2]:cuts[3]][keys[cuts[2]:cuts[3]] == 0] = 1
    st = U.make_stream(rng, keys, ntopics=8 if name == "topic" else 2, p_re=0.15)
    parts = [U.take(st, np.arange(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
    if not arrival:
        parts = [U.grouped(p) for p in parts]
    fl = FILTER | (ARRIVAL if arrival else 0)
    mk = lambda: U.open_session(name, n, nk + 1)
    s = mk()
    got = U.run(s, parts[:2], fl)
    blob = s.state_export()
    assert blob[4] == 2                                  # version 2: the marks travel with the halos / tails
    s2 = mk()
    s2.state_import(blob)
    assert s2.stream_position() == s.stream_position()
    got += U.run(s2, parts[2:3], fl)
    # key 3 leaves the device and comes back under the free id nk
    (b3,) = s2.state_evict([3])
    assert len(b3) > 0
    s2.state_import_keys([b3], [nk])
    renamed, asis = [], []
    for p in parts[3:]:
        q = {k: v.copy() for k, v in p.items()}
        q["key"][q["key"] == 3] = nk
        q = q if arrival else U.grouped(q)               # (the renamed key's segment moves to the batch's end)
        renamed.append(q)
        asis.append(dict(q, key=np.where(q["key"] == nk, 3, q["key"]).astype(np.int32)))
    got += [(r, 3 if k == nk else k, e) for r, k, e in U.run(s2, renamed, fl)]
    want = U.oracle(name, U.concat(parts[:3] + asis))    # the stream as pushed, under the keys' first ids
    assert len(want) > 0 and got == want
    s2.state_clear()
    assert s2.stream_position() == 0
    assert s2.state_export()[4] == 1                     # no mark left
    assert U.run(s2, parts[:1], fl) == U.oracle(name, parts[0])


@pytest.mark.parametrize("name", ["c2", "chain"])
def test_pipelined_collect(name):
    """Push batch i + 1, then collect batch i (the delivered batch before the last)."""
    rng = np.random.default_rng(8)
    st = U.make_stream(rng, rng.integers(0, 9, 2400).astype(np.int32), ntopics=2)
    parts = [U.take(st, np.arange(a, a + 600)) for a in range(0, 2400, 600)]
    want = U.oracle(name, st)
    s = U.open_session(name, 600, 9)
    got = []
    for i, p in enumerate(parts):
        U.push(s, p, FILTER | ARRIVAL)
        if i > 0:
            got += U.matches(s, s.collect(batch_id=s.batch_id() - 1))
    got += U.matches(s, s.collect())
    assert got == want


@pytest.mark.parametrize("name", ["topic", "runs"])
def test_topic_out_of_range(name):
    """A valid record with topic id 8 fails the push with CEP_E_UNSUPPORTED and leaves the marks as they
    were: the next, valid batch gives what the oracle gives without the failed one."""
    rng = np.random.default_rng(13)
    st = U.grouped(U.make_stream(rng, rng.integers(0, 4, 500).astype(np.int32), ntopics=8))
    a, c = U.take(st, np.arange(0, 250)), U.take(st, np.arange(250, 500))
    a, c = U.grouped(a), U.grouped(c)
    bad = {k: v.copy() for k, v in c.items()}
    bad["off"] += 500                                    # (would move every mark far ahead if committed)
    bad["topic"][7] = 8
    bad["valid"][7] = 1
    s = U.open_session(name, 250, 4)
    got = U.run(s, [a], FILTER)
    with pytest.raises(N.CepError, match="Unsupported"):
        U.push(s, bad, FILTER)
        s.collect()
    ok = {k: v.copy() for k, v in bad.items()}
    ok["valid"][7] = 0                                   # an invalid record's topic id is not looked at
    ok["off"] -= 500
    got += U.run(s, [ok], FILTER)
    assert got == U.oracle(name, U.concat([a, ok]))


def test_sessions_the_flag_is_not_for():
    rng = np.random.default_rng(17)
    st = U.grouped(U.make_stream(rng, rng.integers(0, 6, 400).astype(np.int32), ntopics=2))
    ir, cp, _ = U.compiled("c2")
    # without CEP_SESSION_CARRY: refused before the session changes
    s = N.Session(cp, 400, mode=N.MODE_PROCESSOR)
    U.push(s, st, N.BATCH_OFFSETS_MONOTONE, with_valid=False)
    before = s.collect()
    bid = s.batch_id()
    with pytest.raises(N.CepError, match="Unsupported"):
        U.push(s, st, FILTER)
    assert s.batch_id() == bid
    after = s.collect()
    for f in ("match_record", "ent_off", "ent_record"):
        assert np.array_equal(before[f], after[f])
    # a general-path carry session: the flag does nothing
    outs = []
    for fl in (0, FILTER):
        g = U.open_session("c2", 400, 6, force_path=N.PATH_GENERAL)
        U.push(g, st, fl)
        outs.append(U.matches(g, g.collect()))
    assert outs[0] == outs[1] == U.oracle("c2", st)


@pytest.mark.parametrize("name,p_re", [("c2", 0.12), ("runs", 0.0)])
def test_mode_nfa_drops_only_nulls(name, p_re):
    """CEP_MODE_NFA knows no marks: re-delivered offsets are evaluated like any record (the runs pattern's
    stream has none: the reference's buffer, keyed by offset, raises on them), nulls are dropped."""
    rng = np.random.default_rng(19)
    st = U.grouped(U.make_stream(rng, rng.integers(0, 6, 1500).astype(np.int32), ntopics=1, p_re=p_re))
    keep = np.flatnonzero(st["valid"])
    live = U.take(st, keep)                              # the oracle's NFA modes know no null records
    want = [(int(keep[r]), k, [(nm, int(keep[e])) for nm, e in ents])
            for r, k, ents in U.oracle(name, live, O.MODE_NFA_PER_KEY)]
    s = U.open_session(name, 1500, 6, mode=N.MODE_NFA)
    got = U.run(s, [st], FILTER)
    assert len(want) > 0 and got == want


def _view(seq):
    return [(st.getStage(), [(e.topic, e.offset) for e in st.getEvents()]) for st in seq.matched()]


def _feed(mk, recs, snapshot_at=None):
    out = []
    fw = lambda k, seq: out.append((k, _view(seq)))
    proc = mk()
    proc.init(fw)
    for i, r in enumerate(recs):
        if i == snapshot_at:
            snap = proc.checkpoint()
            assert not snap["hwm"] or not proc.device_filter
            proc.close()
            proc = mk()
            proc.init(fw)
            proc.restore(snap)
        proc.process(*r)
    proc.close()
    return out


def _oracle_forward(pat, schema, dec, coltypes, recs):
    """The oracle over the arrival-order stream (nulls as invalid records), as (key, sequence view)."""
    live = next(r for r in recs if r[1] is not None)
    keys = {}
    kid = np.array([keys.setdefault(r[0], len(keys)) for r in recs], np.int32)
    cols = dec.columns([dec.row(r[1] if r[1] is not None else live[1]) for r in recs])
    p = O.OraclePattern(pat.to_ir(schema))
    run = O.OracleRun(p, O.MODE_PROCESSOR)
    run.process(O.BatchArrays(kid, cols, coltypes, valid=np.array([r[1] is not None for r in recs], np.uint8),
                              topic=np.array([schema.topic_id(r[2]) for r in recs], np.int32),
                              offset=np.array([r[4] for r in recs], np.int64), ts=np.array([r[5] for r in recs], np.int64)))
    ev = lambda i: Ev(recs[i][0], recs[i][1], recs[i][5], recs[i][2], recs[i][3], recs[i][4])
    return [(recs[m.record][0], _view(sequence_from_traversal(m.traversal, p.names, ev)))
            for m in run.matches(with_groups=False)]


@pytest.mark.parametrize("which", ["stock", "letters"])
def test_processor_device_filter(which):
    """GpuCEPProcessor with device_filter on and off forwards the same (key, Sequence) stream -- nulls and
    re-deliveries in the input -- which is the oracle's, and a snapshot / restore mid-stream changes nothing."""
    rng = np.random.default_rng(23)
    n = 600
    if which == "stock":                                 # the stock demo (CEPStockDemoTest's quotes): a general-path session
        fx = [f for f in scenarios() if f["name"] == "stock_demo"][0]
        ev = fx["events"]
        schema, pat, dec, coltypes = STOCK_SCHEMA, PL.stock_demo(), stock_columns(), [2, 2]
        base = [("ALXN", StockEvent("ALXN", ev["cols"][0][i], ev["cols"][1][i]), "stock-events", 0, ev["offset"][i],
                 ev["ts"][i]) for i in range(len(ev["key"]))]
        recs = []
        for i, r in enumerate(base):                     # every quote delivered, some again, nulls in between
            recs.append(r)
            if i % 3 == 1:
                recs.append(base[i - 1])
            if i % 4 == 2:
                recs.append(("ALXN", None, "stock-events", 0, r[4] + 100, r[5]))
        batch = 3
    else:                                                # interleaved keys, two topics, on the stencil path
        schema, pat, coltypes = Schema([("value", "i32")], topics=["T0", "T1"]), U.PATTERNS["c2"][0], [1]
        dec = scalar_column(schema)
        vals = [int(x) for x in rng.integers(0, 3, n)]
        topics = [f"T{int(t)}" for t in rng.integers(0, 2, n)]
        keys = [f"k{int(k)}" for k in rng.integers(0, 7, n)]
        recs, nxt, hist = [], {}, {}
        for i in range(n):
            k, t = keys[i], topics[i]
            if k in hist and rng.random() < 0.1:         # a re-delivery of one of the key's last records
                recs.append(recs[int(rng.choice(hist[k][-3:]))])
            elif rng.random() < 0.05:                    # a null value, its offset far ahead
                recs.append((k, None, t, 0, nxt.get(t, 0) + 5000, 1000 + i))
            else:
                recs.append((k, vals[i], t, 0, nxt.get(t, 0), 1000 + i))
                nxt[t] = nxt.get(t, 0) + 1
            hist.setdefault(k, []).append(i)
        batch = 128
    mk = lambda df: (lambda: GpuCEPProcessor("q", pat, schema, dec, batch_size=batch, max_keys=16, device_filter=df))
    want = _oracle_forward(pat, schema, dec, coltypes, recs)
    assert len(want) > 0
    assert _feed(mk(False), recs) == want
    assert _feed(mk(True), recs) == want
    assert _feed(mk(True), recs, snapshot_at=len(recs) // 2) == want
    if which == "letters":                               # a snapshot with host marks is not for a device_filter processor
        p0 = mk(False)()
        p0.init(lambda k, q: None)
        for r in recs[:200]:
            p0.process(*r)
        snap = p0.checkpoint()
        p0.close()
        p1 = mk(True)()
        p1.init(lambda k, q: None)
        with pytest.raises(ProcessorFailed, match="device_filter"):
            p1.restore(snap)
        p1.close()
