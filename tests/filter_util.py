"""Shared pieces of the CEP_BATCH_FILTER tests: the patterns (one per fast path), streams with null
records and re-deliveries as a topic partition hands them to CEPProcessor.process, and the comparison of a
carry session's filtered pushes with the oracle's single MODE_PROCESSOR pass over the raw stream."""
import numpy as np

import oracle as O
from kcep import QueryBuilder, Selected, Schema, Event, synth, native as N

TOPICS = [f"T{i}" for i in range(N.FILTER_MAX_TOPICS)]
SCHEMA = Schema([("value", "i32")], topics=TOPICS)      # topic ids 0..7: every id the marks cover


def _patterns():
    v = Event.value()
    return {
        # 1-stage stencil: no halo; every admitted record with value 0 is a match
        "one": (QueryBuilder().select("A").where(v == 0).build(), N.PATH_STENCIL),
        # the 3-stage C2 stencil
        "c2": (synth.c2_pattern(), N.PATH_STENCIL),
        # a chain: strict with an optional() stage
        "chain": (QueryBuilder().select("A").where(v == 0).then().select("B").optional().where(v == 1).then()
                  .select("C").where(v == 2).build(), N.PATH_CHAIN),
        # the runs path: folds read by the next stages' predicates (C3's shape)
        "runs": (synth.c3_pattern(), N.PATH_RUNS),
        # stages reading one topic each (Selected.withTopic): A from T3, B from T4
        "topic": (QueryBuilder().select("A", Selected.withStrictContiguity().withTopic("T3")).where(v < 2).then()
                  .select("B", Selected.withStrictContiguity().withTopic("T4")).where(v >= 1).build(), N.PATH_STENCIL),
    }


PATTERNS = _patterns()
_compiled = {}


def compiled(name):
    """(ir, CompiledPattern, expected path) of a pattern, compiled once."""
    if name not in _compiled:
        pat, path = PATTERNS[name]
        ir = pat.to_ir(SCHEMA)
        _compiled[name] = (ir, N.CompiledPattern(ir), path)
    return _compiled[name]


def open_session(name, max_events, max_keys, mode=N.MODE_PROCESSOR, **kw):
    ir, cp, path = compiled(name)
    # (the runs pattern on its built-in kernels: no per-test compile of the pattern's own)
    s = N.Session(cp, max_events, mode=mode, carry=True, max_keys=max_keys, interpret=True, **kw)
    if not kw.get("force_path"):
        assert s.path == path, (name, s.path)
    return s


def make_stream(rng, keys, ntopics=1, nvals=4, p_null=0.06, p_re=0.12):
    """Records of `keys` (arrival order) as CEPProcessor sees them: offsets increasing per topic (one
    partition each: the reference's buffer names an event by topic, partition and offset), sometimes with a
    gap, ~p_re re-deliveries of one of the key's last four records (same offset, topic and contents: a jump
    back; the next fresh record jumps forward past the mark again), ~p_null null records
    whose offset is high (they must move no mark).  Returns a dict of arrays."""
    n = len(keys)
    val = rng.integers(0, nvals, n).astype(np.int32)
    # (eight topics: T3 and T4, which the "topic" pattern reads, take most records, so that it matches)
    tp = np.full(ntopics, 1.0 / ntopics) if ntopics < 8 else np.array([.04, .04, .04, .38, .38, .04, .04, .04])
    topic = rng.choice(ntopics, n, p=tp).astype(np.int32)
    valid = (rng.random(n) >= p_null).astype(np.uint8)
    off = np.zeros(n, np.int64)
    ts = np.cumsum(rng.integers(1, 4, n)).astype(np.int64)
    nxt, hist = {}, {}
    for i in range(n):
        k = int(keys[i])
        if k in hist and rng.random() < p_re:
            j = int(rng.choice(hist[k][-4:]))
            val[i], topic[i], valid[i], off[i] = val[j], topic[j], valid[j], off[j]
        elif not valid[i]:
            off[i] = nxt.get(int(topic[i]), 0) + 1000
        else:
            t = int(topic[i])
            off[i] = nxt.get(t, 0) + (3 if rng.random() < 0.1 else 0)
            nxt[t] = off[i] + 1
        hist.setdefault(k, []).append(i)
    return dict(key=np.asarray(keys, np.int32), val=val, topic=topic, valid=valid, off=off, ts=ts)


def take(st, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in st.items()}


def concat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def grouped(st):
    """The batch stable-sorted by key: what a host that groups on its side hands over."""
    return take(st, np.argsort(st["key"], kind="stable"))


def oracle(name, st, mode=O.MODE_PROCESSOR):
    """[(position, key, [(stage, position)])] of the stream in one pass, in forward order."""
    ir = compiled(name)[0]
    p = O.OraclePattern(ir)
    r = O.OracleRun(p, mode)
    r.process(O.BatchArrays(st["key"], [st["val"]], [1], valid=st["valid"], topic=st["topic"], offset=st["off"],
                            ts=st["ts"]))
    return [(m.record, m.key, [(p.names[nm], ev) for nm, ev in m.traversal]) for m in r.matches(with_groups=False)]


def push(s, st, flags, with_valid=True):
    s.push(len(st["key"]), st["key"], [st["val"]], valid=st["valid"] if with_valid else None, topic=st["topic"],
           offset=st["off"], ts=st["ts"], flags=flags)


def matches(s, out):
    names = s.pattern.names
    res = []
    for m in range(len(out["match_record"])):
        a, b = out["ent_off"][m], out["ent_off"][m + 1]
        res.append((int(out["match_record"][m]), int(out["match_key"][m]),
                    [(names[out["ent_name"][i]], int(out["ent_record"][i])) for i in range(a, b)]))
    return res


def run(s, batches, flags):
    """Every batch pushed with `flags` and collected; the matches in the order they came, and the batch
    errors (none expected: the patterns raise nothing)."""
    got = []
    for b in batches:
        push(s, b, flags)
        out = s.collect(raise_on_error=False)
        assert not out["err"], out["err"]
        assert len(s.batch_errors()[0]) == 0
        got += matches(s, out)
    return got
