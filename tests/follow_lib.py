"""The follow path's tests (CEP_SESSION_FOLLOW, test_follow_cpu.py, test_follow_gpu.py): the closed form of
skip-till-next patterns as a reference model, pattern builders over it, and stream generators.

A stage is a dict: name, next (skip-till-next, else strict), times, kind + c (the predicate: value <kind> c),
topic (a topic name or None)."""
import numpy as np

from kcep import QueryBuilder, Selected, Schema, Event

I32T = Schema([("value", "i32")], topics=["t0", "t1"])
F64 = Schema([("value", "f64")])
I64 = Schema([("value", "i64")])
TWO = Schema([("a", "i32"), ("b", "i32")])
TOPIC_ID = {"t0": 0, "t1": 1}


def follow_model(slots, ok, n, seg_end):      # slots: [(name, is_next)], ok(s, p) -> bool
    out = []
    for j0 in range(n):
        if not ok(0, j0): continue
        recs, p, E = [j0], j0, seg_end(j0)
        for s in range(1, len(slots)):
            p += 1
            if slots[s][1]:
                while p < E and not ok(s, p): p += 1
            if p >= E or not ok(s, p): recs = None; break
            recs.append(p)
        if recs: out.append((recs[-1], j0, recs))
    out.sort(key=lambda t: (t[0], t[1]))
    return [(e, [(slots[s][0], r) for s, r in reversed(list(enumerate(rs)))]) for e, _, rs in out]


# ---- patterns ----
def stage(name, nxt, kind="eq", c=0, times=1, topic=None):
    return dict(name=name, next=nxt, kind=kind, c=c, times=times, topic=topic)


def _pred(v, st):
    k, c = st["kind"], st["c"]
    return {"eq": v == c, "ne": v != c, "le": v <= c, "ge": v >= c, "lt": v < c, "gt": v > c}[k]


def build(stages, field="value"):
    v = Event.field(field)
    b = None
    for st in stages:
        sel = Selected.withSkipTilNextMatch() if st["next"] else Selected.withStrictContiguity()
        if st["topic"] is not None:
            sel = sel.withTopic(st["topic"])
        sb = (QueryBuilder() if b is None else b.then()).select(st["name"], sel)
        if st["times"] > 1:
            sb = sb.times(st["times"])
        b = sb.where(_pred(v, st))
    return b.build()


def slots_of(stages):
    """[(name, is_next)] per expanded slot, and per slot the index of its stage"""
    slots, owner = [], []
    for i, st in enumerate(stages):
        for _ in range(st["times"]):
            slots.append((st["name"], st["next"]))
            owner.append(i)
    return slots, owner


def next_mask(stages):
    slots, _ = slots_of(stages)
    return sum(1 << s for s, (_, nx) in enumerate(slots) if nx)


def stage_hits(st, val, topic):
    """the records satisfying a stage's predicate, topic filter included (numpy comparisons: a NaN fails
    every one of them, as in Java)"""
    val = np.asarray(val)
    c = st["c"]
    with np.errstate(invalid="ignore"):
        h = {"eq": val == c, "ne": val != c, "le": val <= c, "ge": val >= c, "lt": val < c, "gt": val > c}[st["kind"]]
    if st["topic"] is not None:
        h = h & (np.asarray(topic) == TOPIC_ID[st["topic"]])
    return h


def model_matches(stages, key, val, topic=None):
    """what oracle_matches returns for the pattern over a key-grouped batch: (record, key, traversal)"""
    key = np.asarray(key)
    n = len(key)
    slots, owner = slots_of(stages)
    hits = [stage_hits(st, val, topic) for st in stages]
    ends = np.empty(n, np.int64)                         # E(j): the end of j's key segment
    e = n
    for j in range(n - 1, -1, -1):
        if j + 1 < n and key[j + 1] != key[j]:
            e = j + 1
        ends[j] = e
    res = follow_model(slots, lambda s, p: bool(hits[owner[s]][p]), n, lambda j: int(ends[j]))
    return [(e, int(key[e]), trav) for e, trav in res]


def random_stages(rng, variant, alphabet, min_next=0):
    """variant: "plain" (2-6 stages), "topics" (2-4 stages, topic filters on some), "times" (times(1..3) on
    non-first stages, at most 8 slots).  The first stage is strict; min_next: at least so many skip-till-next."""
    while True:
        k = int(rng.integers(2, 7 if variant == "plain" else 5))
        stages = []
        for i in range(k):
            st = stage(f"s{i}", bool(i > 0 and rng.random() < 0.6),
                       kind=str(rng.choice(["eq", "eq", "eq", "le", "ge", "ne"])), c=int(rng.integers(0, alphabet)))
            if variant == "topics" and rng.random() < 0.5:
                st["topic"] = str(rng.choice(["t0", "t1"]))
            if variant == "times" and i > 0:
                st["times"] = int(rng.integers(1, 4))
            stages.append(st)
        if sum(st["times"] for st in stages) <= 8 and sum(st["next"] for st in stages) >= min_next:
            return stages


def random_stream(rng, n_keys, max_len, alphabet, min_len=1):
    """(key, value, topic): n_keys contiguous keys of min_len..max_len records, values in [0, alphabet)"""
    lens = rng.integers(min_len, max_len + 1, n_keys)
    key = np.repeat(np.arange(n_keys, dtype=np.int32), lens)
    n = len(key)
    return key, rng.integers(0, alphabet, n).astype(np.int32), rng.integers(0, 2, n).astype(np.int32)


# ---- the fixed patterns of the tests: A = 0, B = 1, C = 2 over one value column ----
def abc(nxt=(True, True)):
    return [stage("a", False, c=0), stage("b", nxt[0], c=1), stage("c", nxt[1], c=2)]


# ---- eligibility tables: (name, schema, stages or pattern builder[, reason]) ----
def _k8():
    return [stage("a", False, c=0), stage("b", True, c=1, times=3), stage("c", False, c=2, times=3), stage("d", True, c=3)]


ACCEPTED = [
    ("two_stages", I32T, [stage("a", False, c=0), stage("b", True, c=1)]),
    ("strict_after_next", I32T, abc((True, False))),
    ("times3_middle", I32T, [stage("a", False, c=0), stage("b", True, c=1, times=3), stage("c", True, c=2)]),
    ("k8_via_times", I32T, _k8()),
    ("topics", I32T, [stage("a", False, c=0, topic="t0"), stage("b", True, c=1, topic="t1"), stage("c", False, kind="ge", c=1)]),
    ("f64_column", F64, [stage("a", False, kind="lt", c=0.5), stage("b", True, kind="ge", c=1.5)]),
    ("i64_column", I64, [stage("a", False, kind="gt", c=2 ** 40), stage("b", True, kind="le", c=-2 ** 40)]),
]

_v, _a, _b = Event.field("value"), Event.field("a"), Event.field("b")
NEXT, ANY = Selected.withSkipTilNextMatch, Selected.withSkipTilAnyMatch


def _q():
    return QueryBuilder()


REJECTED = [
    ("skip_till_any", I32T, lambda: _q().select("a").where(_v == 0).then().select("b", ANY()).where(_v == 1).build(),
     "skip-till-any"),
    ("non_strict_first", I32T, lambda: _q().select("a", NEXT()).where(_v == 0).then().select("b", NEXT()).where(_v == 1).build(),
     "non-strict first"),
    ("times_first", I32T, lambda: _q().select("a").times(2).where(_v == 0).then().select("b", NEXT()).where(_v == 1).build(),
     "times on the first"),
    ("optional", I32T, lambda: _q().select("a").where(_v == 0).then().select("b", NEXT()).optional().where(_v == 1).then()
     .select("c", NEXT()).where(_v == 2).build(), "optional"),
    ("one_or_more", I32T, lambda: _q().select("a").where(_v == 0).then().select("b", NEXT()).oneOrMore().where(_v == 1).then()
     .select("c", NEXT()).where(_v == 2).build(), "oneOrMore"),
    ("fold", I32T, lambda: _q().select("a").where(_v == 0).fold("sum", _v).then().select("b", NEXT()).where(_v == 1).build(),
     "fold"),
    ("duplicate_names", I32T, lambda: _q().select("a").where(_v == 0).then().select("a", NEXT()).where(_v == 1).build(),
     "duplicate"),
    ("k9", I32T, lambda: build([stage("a", False, c=0), stage("b", True, c=1, times=3), stage("c", True, c=2, times=3),
                                stage("d", True, c=3, times=2)]), "more than 8"),
    ("two_columns", TWO, lambda: _q().select("a").where(_a == 0).then().select("b", NEXT()).where(_b == 1).build(),
     "more than one column"),
    ("all_strict", I32T, lambda: build(abc((False, False))), "stencil path takes"),
    ("strict_times_only", I32T, lambda: build([stage("a", False, c=0), stage("b", False, c=1, times=2)]),
     "runs path takes"),
]
