"""The follow path's evaluated form (CEP_SESSION_MASK_PASS with CEP_SESSION_FOLLOW / CEP_SESSION_FOLLOW_CARRY;
test_follow_mask_cpu.py, test_follow_mask_gpu.py): skip-till-next patterns whose predicates read several
columns, arithmetic or event metadata.  Patterns, schemas, streams, and a reference model: each slot's truth
computed with numpy, then follow_lib.follow_model's closed form over it.

A stage is a dict: name, next (skip-till-next, else strict), times, topic (a topic name or None), expr (the
predicate as a kcep expression) and hit (the same predicate over numpy arrays: hit(env) -> bool array, env
holding every column by its field name plus ts, offset, partition and topic)."""
import numpy as np

import oracle as O
from kcep import QueryBuilder, Selected, Schema, Event, States, SequenceAgg
import follow_lib as FL
import mask_pass_lib as ML

PV, RICH = ML.PV, ML.RICH
PVT = Schema([("price", "i64"), ("volume", "i64")], topics=["t0", "t1"])
SIX = Schema([(f"c{i}", "i32") for i in range(6)])
PVF = Schema([("price", "f64"), ("volume", "f64")])
PV_T, RICH_T, SIX_T, PVF_T = [2, 2], [1, 2, 3], [1] * 6, [3, 3]
TOPIC_ID = {"t0": 0, "t1": 1}

price, volume = ML.price, ML.volume
A, B, Cc = ML.A, ML.B, ML.Cc


def stage(name, nxt, expr, hit, times=1, topic=None):
    return dict(name=name, next=nxt, expr=expr, hit=hit, times=times, topic=topic)


def build(stages):
    b = None
    for st in stages:
        sel = Selected.withSkipTilNextMatch() if st["next"] else Selected.withStrictContiguity()
        if st["topic"] is not None:
            sel = sel.withTopic(st["topic"])
        sb = (QueryBuilder() if b is None else b.then()).select(st["name"], sel)
        if st["times"] > 1:
            sb = sb.times(st["times"])
        b = sb.where(st["expr"])
    return b.build()


slots_of, next_mask = FL.slots_of, FL.next_mask


# ---- the model ----
def env_of(schema, cols, n, topic=None, partition=None, offset=None, ts=None, pos=None):
    """the arrays a predicate reads; a ts / offset the batch lacks is the record's stream position (pos, or
    its index), topic and partition default to 0"""
    pos = np.arange(n, dtype=np.int64) if pos is None else np.asarray(pos, np.int64)
    env = {name: np.asarray(c) for (name, _), c in zip(schema.columns, cols)}
    env["topic"] = np.zeros(n, np.int32) if topic is None else np.asarray(topic)
    env["partition"] = np.zeros(n, np.int32) if partition is None else np.asarray(partition)
    env["offset"] = pos if offset is None else np.asarray(offset, np.int64)
    env["ts"] = pos if ts is None else np.asarray(ts, np.int64)
    return env


def stage_hits(st, env):
    with np.errstate(all="ignore"):
        h = np.asarray(st["hit"](env), bool)
    if st["topic"] is not None:
        h = h & (env["topic"] == TOPIC_ID[st["topic"]])
    return h


def model_matches(stages, key, env):
    """what gpu_util.oracle_matches returns for the pattern over a key-grouped batch"""
    key = np.asarray(key)
    n = len(key)
    slots, owner = slots_of(stages)
    hits = [stage_hits(st, env) for st in stages]
    ends = np.empty(n, np.int64)
    e = n
    for j in range(n - 1, -1, -1):
        if j + 1 < n and key[j + 1] != key[j]:
            e = j + 1
        ends[j] = e
    res = FL.follow_model(slots, lambda s, p: bool(hits[owner[s]][p]), n, lambda j: int(ends[j]))
    return [(e, int(key[e]), trav) for e, trav in res]


# ---- FM2: P2's three predicates (mask_pass_lib.p2), stages 2 and 3 skip-till-next ----
def fm2():
    return [stage("s0", False, (price >= 0) & (price + volume == 3), lambda e: (e["price"] >= 0) & (e["price"] + e["volume"] == 3)),
            stage("s1", True, (price <= volume) & (volume - price <= 1),
                  lambda e: (e["price"] <= e["volume"]) & (e["volume"] - e["price"] <= 1)),
            stage("s2", True, (price > 1) | (volume > 1), lambda e: (e["price"] > 1) | (e["volume"] > 1))]


# ---- RICHF: i32 overflow, an f64 division with NaNs, a topic filter, times(2), metadata ----
def _r1(e):
    return (e["b"].astype(np.float64) / e["c"] > 0.5) | (e["a"] < 0)


def richf():
    return [stage("r0", False, (A * A > 1000) & (B >= 0), lambda e: (e["a"] * e["a"] > 1000) & (e["b"] >= 0)),   # (int32: wraps)
            stage("r1", True, (B.asDouble() / Cc > 0.5) | (A < 0), _r1, times=2, topic="t0"),
            stage("r2", False, (Event.timestamp() - Event.offset() > 2) | (B % 7 == 3),
                  lambda e: (e["ts"] - e["offset"] > 2) | (e["b"] % 7 == 3))]


# ---- two fields spelling one symbol: A = (3, 0), B = (1, 0), C = (0, 2), none = (0, 0); stage `a` is
# price + volume == 3, `b` price - volume == 1, `c` volume - price == 2, `d` price + volume == 3 again ----
SYM = np.array([[3, 0], [1, 0], [0, 2], [0, 0]], np.int64)


def sym_cols(val):
    v = np.asarray(val)
    return [np.ascontiguousarray(SYM[v, 0]), np.ascontiguousarray(SYM[v, 1])]


def sym_stage(name, nxt, c, times=1):
    expr, hit = {0: (price + volume == 3, lambda e: e["price"] + e["volume"] == 3),
                 1: (price - volume == 1, lambda e: e["price"] - e["volume"] == 1),
                 2: (volume - price == 2, lambda e: e["volume"] - e["price"] == 2)}[c]
    return stage(name, nxt, expr, hit, times=times)


def sym_abc(nxt=(True, True)):
    return [sym_stage("a", False, 0), sym_stage("b", nxt[0], 1), sym_stage("c", nxt[1], 2)]


def k8():
    """eight slots through times: a, followedBy b x 3, c x 3 strictly, followedBy a"""
    return [sym_stage("a", False, 0), sym_stage("b", True, 1, times=3), sym_stage("c", False, 2, times=3),
            sym_stage("d", True, 0)]


def k2():
    return [sym_stage("a", False, 0), sym_stage("b", True, 1)]


# ---- six i32 columns, the predicates on columns 4 and 5: past the four the interpreted table holds ----
_c0, _c4, _c5 = Event.field("c0"), Event.field("c4"), Event.field("c5")


def six():
    return [stage("x", False, (_c4 + _c5 == 3) & (_c0 >= 0), lambda e: (e["c4"] + e["c5"] == 3) & (e["c0"] >= 0)),
            stage("y", True, _c4 < _c5, lambda e: e["c4"] < e["c5"]),
            stage("z", False, _c5 - _c4 != 1, lambda e: e["c5"] - e["c4"] != 1)]


def six_stream(n, n_keys, seed):
    r = np.random.default_rng(seed)
    key = np.sort(r.integers(0, n_keys, n)).astype(np.int32)
    return key, [r.integers(0, 4, n).astype(np.int32) for _ in range(6)]


# ---- f64 with NaNs, i64 beyond 2^32 ----
_pf, _vf = Event.field("price"), Event.field("volume")


def f64_nan():
    return [stage("a", False, _pf < _vf, lambda e: e["price"] < e["volume"]),
            stage("b", True, _pf + _vf >= 1.5, lambda e: e["price"] + e["volume"] >= 1.5),
            stage("c", True, _pf == _vf, lambda e: e["price"] == e["volume"])]


def i64_big():
    return [stage("a", False, price > volume + 2 ** 32, lambda e: e["price"] > e["volume"] + 2 ** 32),
            stage("b", True, price + volume <= -2 ** 40, lambda e: e["price"] + e["volume"] <= -2 ** 40),
            stage("c", False, price - volume == 2 ** 32 + 5, lambda e: e["price"] - e["volume"] == 2 ** 32 + 5)]


# ---- random FM2-like patterns for the model-against-oracle test ----
def _atom(rng, meta):
    c = int(rng.integers(0, 5))
    f = int(rng.integers(0, 10 if meta else 8))
    p, v = price, volume
    return [(p + v >= c, lambda e: e["price"] + e["volume"] >= c),
            (p <= v, lambda e: e["price"] <= e["volume"]),
            ((p > c % 3) | (v > c % 2 + 1), lambda e: (e["price"] > c % 3) | (e["volume"] > c % 2 + 1)),
            (p * v < c + 1, lambda e: e["price"] * e["volume"] < c + 1),
            (p != v + 1, lambda e: e["price"] != e["volume"] + 1),
            ((p + v) % 2 == c % 2, lambda e: (e["price"] + e["volume"]) % 2 == c % 2),
            (v - p < c - 1, lambda e: e["volume"] - e["price"] < c - 1),
            (p + v == c, lambda e: e["price"] + e["volume"] == c),
            (Event.timestamp() - Event.offset() > c - 2, lambda e: e["ts"] - e["offset"] > c - 2),
            ((Event.offset() + p) % 3 == c % 3, lambda e: (e["offset"] + e["price"]) % 3 == c % 3)][f]


def random_stages(rng, variant):
    """variant: "plain" (2-6 stages), "topics" (2-4, topic filters on some), "times" (times(1..3) on non-first
    stages, at most 8 slots), "meta" (2-5, predicates reading timestamp() / offset() too).  The first stage is
    strict and compares the two fields; one stage at least is skip-till-next."""
    while True:
        k = int(rng.integers(2, 7 if variant == "plain" else 6 if variant == "meta" else 5))
        stages = []
        for i in range(k):
            expr, hit = _atom(rng, variant == "meta")
            if i == 0:                                   # (no single column decides it: never the direct form)
                e0, h0 = expr, hit
                expr, hit = (price + volume == 3) | e0, (lambda h0: lambda e: (e["price"] + e["volume"] == 3) | h0(e))(h0)
            st = stage(f"s{i}", bool(i > 0 and rng.random() < 0.6), expr, hit)
            if variant == "topics" and rng.random() < 0.5:
                st["topic"] = str(rng.choice(["t0", "t1"]))
            if variant == "times" and i > 0:
                st["times"] = int(rng.integers(1, 4))
            stages.append(st)
        if sum(st["times"] for st in stages) <= 8 and any(st["next"] for st in stages):
            return stages


def random_stream(rng, n_keys, max_len):
    """(key, [price, volume], topic, offset, ts): contiguous keys of 1..max_len records, fields in 0..3, offsets
    increasing over the batch, ts a little ahead of them"""
    lens = rng.integers(1, max_len + 1, n_keys)
    key = np.repeat(np.arange(n_keys, dtype=np.int32), lens)
    n = len(key)
    offset = np.arange(n, dtype=np.int64) * 2 + 5
    return (key, [rng.integers(0, 4, n).astype(np.int64), rng.integers(0, 4, n).astype(np.int64)],
            rng.integers(0, 2, n).astype(np.int32), offset, offset + rng.integers(0, 6, n))


# ---- carry sessions: a whole stream (grouped by key) cut into batches, and the oracle's per-batch expectation ----
def cut_stream(rng, key, n_batches):
    """per batch the indices (ascending) of the whole stream's records it holds: every key's records are cut
    at n_batches - 1 random points of their own, so a key may miss a batch"""
    key = np.asarray(key)
    batch_of = np.zeros(len(key), np.int64)
    for k in np.unique(key):
        idx = np.flatnonzero(key == k)
        cuts = np.sort(rng.integers(0, len(idx) + 1, n_batches - 1))
        batch_of[idx] = np.searchsorted(cuts, np.arange(len(idx)), side="right")
    return [np.flatnonzero(batch_of == b) for b in range(n_batches)]


def positions(parts, n):
    """the stream position of every record of the whole stream: batches in order, records in batch order"""
    pos = np.zeros(n, np.int64)
    base = 0
    for idx in parts:
        pos[idx] = base + np.arange(len(idx))
        base += len(idx)
    return pos


def oracle_batches(ir, coltypes, st, parts, mode=O.MODE_NFA_PER_KEY, explicit_ts=True, explicit_offset=True):
    """follow_carry_lib.oracle_batches' comparison over any schema: the oracle over every key's whole stream
    (st: key, cols, topic, partition, offset, ts; grouped by key), its records mapped to stream positions; per
    batch the matches completing in it, by (completing record's place in the batch, start).  explicit_*=False:
    the session is not given that array, so its values are the stream positions."""
    n = len(st["key"])
    pos = positions(parts, n)
    where = np.zeros((n, 2), np.int64)
    for b, idx in enumerate(parts):
        where[idx, 0], where[idx, 1] = b, np.arange(len(idx))
    p = O.OraclePattern(ir)
    r = O.OracleRun(p, mode)
    r.process(O.BatchArrays(st["key"], st["cols"], coltypes, topic=st["topic"], partition=st["partition"],
                            offset=st["offset"] if explicit_offset else pos, ts=st["ts"] if explicit_ts else pos))
    out = [[] for _ in parts]
    for m in r.matches(with_groups=False):
        b, i = where[m.record]
        trav = [(p.names[nm], int(pos[ev])) for nm, ev in m.traversal]
        out[b].append((int(i), trav[-1][1], (int(pos[m.record]), int(m.key), trav)))
    return [[t[2] for t in sorted(lst, key=lambda t: (t[0], t[1]))] for lst in out]


# ---- eligibility tables ----
ACCEPTED = [
    ("fm2", PV, fm2),
    ("richf", RICH, richf),
    ("k8_via_times", PV, k8),
    ("k2", PV, k2),
    ("six_columns", SIX, six),
    ("f64_nan", PVF, f64_nan),
    ("i64_big", PV, i64_big),
    ("strict_after_next", PV, lambda: sym_abc((True, False))),
    # follow_lib.REJECTED's "more than one column": one column per predicate, two in the pattern
    ("two_columns", FL.TWO, lambda: [stage("a", False, Event.field("a") == 0, lambda e: e["a"] == 0),
                                     stage("b", True, Event.field("b") == 1, lambda e: e["b"] == 1)]),
]

NEXT = Selected.withSkipTilNextMatch


def _two(first, second):
    """x strictly, followedBy y: a follow shape whatever the predicates"""
    return lambda: QueryBuilder().select("x").where(first).then().select("y", NEXT()).where(second).build()


# (name, schema, pattern builder, the reason's words)
REJECTED = [r for r in FL.REJECTED if r[0] != "two_columns"] + [
    ("states_get", PV, _two(price < volume, price > States.getLong("avg")), "States.get"),
    ("sequence_agg", PV, _two(price < volume, price > SequenceAgg.sum("price")), "sequence"),
    ("div_by_field", PV, _two(price < volume, (volume != 0) & (10 / volume > 1)), "divisor"),
    ("rem_by_field", PV, _two(price < volume, price % volume == 1), "divisor"),
    ("direct_form", FL.I32T, lambda: FL.build(FL.abc()), "directly"),
]
