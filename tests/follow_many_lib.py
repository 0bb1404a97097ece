"""The follow path with oneOrMore stages (CEP_SESSION_FOLLOW_MANY; test_follow_many_cpu.py,
test_follow_many_gpu.py): the closed form of such patterns as a reference model, pattern builders over it, and
stream generators.

A stage is follow_lib's dict -- name, next (skip-till-next, else strict), times, kind + c (the predicate:
value <kind> c), topic (a topic name or None) -- with one more entry, many: the stage is oneOrMore."""
import numpy as np

from kcep import QueryBuilder, Selected, Schema, Event
import follow_lib as FL

I32T, TWO = FL.I32T, FL.TWO


def stage(name, nxt, kind="eq", c=0, times=1, topic=None, many=False):
    st = FL.stage(name, nxt, kind=kind, c=c, times=times, topic=topic)
    st["many"] = many
    return st


def build(stages, field="value"):
    v = Event.field(field)
    b = None
    for st in stages:
        sel = Selected.withSkipTilNextMatch() if st["next"] else Selected.withStrictContiguity()
        if st["topic"] is not None:
            sel = sel.withTopic(st["topic"])
        sb = (QueryBuilder() if b is None else b.then()).select(st["name"], sel)
        if st["many"]:
            sb = sb.oneOrMore()
        if st["times"] > 1:
            sb = sb.times(st["times"])
        b = sb.where(FL._pred(v, st))
    return b.build()


def slots_of(stages):
    """[(name, is_next, is_many)] per slot (a times(n) stage is n slots, a oneOrMore stage one), and per slot
    the index of its stage"""
    slots, owner = [], []
    for i, st in enumerate(stages):
        for _ in range(st["times"]):
            slots.append((st["name"], st["next"], st["many"]))
            owner.append(i)
    return slots, owner


def next_mask(stages):
    return sum(1 << s for s, sl in enumerate(slots_of(stages)[0]) if sl[1])


def many_mask(stages):
    return sum(1 << s for s, sl in enumerate(slots_of(stages)[0]) if sl[2])


# ---- the model ----
def many_model(slots, ok, n, seg_end, stats=None):
    """slots: [(name, is_next, is_many)], ok(s, p) -> bool (topic filter included), seg_end(j): the end of j's
    key segment.  stats (a dict, or None) counts the walks that reach a hop out of a strict many slot into a
    strict slot: ss_die -- killed there by a record that is neither, ss_done -- through it and completed."""
    K = len(slots)
    out = []
    for j0 in range(n):
        if not ok(0, j0): continue
        E, r, fwd = seg_end(j0), j0, [(0, j0)]           # fwd: (slot, record) in the order taken
        through = False
        for s in range(1, K):
            if not slots[s - 1][2]:                      # as follow_lib.follow_model
                p = r + 1
                if slots[s][1]:
                    while p < E and not ok(s, p): p += 1
                if p >= E or not ok(s, p): fwd = None; break
                r = p
            else:
                both_strict = not (slots[s - 1][1] or slots[s][1])
                q, got = r + 1, None
                while q < E:
                    if ok(s - 1, q):
                        fwd.append((s - 1, q))           # collected: one more entry of the many slot
                    elif ok(s, q):
                        got = q
                        break
                    elif both_strict:
                        if stats is not None: stats["ss_die"] = stats.get("ss_die", 0) + 1
                        break
                    q += 1
                if got is None: fwd = None; break
                through = through or both_strict
                r = got
            fwd.append((s, r))
        if fwd: out.append((r, j0, fwd))
        if fwd and through and stats is not None: stats["ss_done"] = stats.get("ss_done", 0) + 1
    out.sort(key=lambda t: (t[0], t[1]))
    # entries final slot first; a many slot's collected records (descending) before the slot's own: the
    # forward order reversed
    return [(e, [(slots[s][0], p) for s, p in reversed(fwd)]) for e, _, fwd in out]


def segment_ends(key):
    key = np.asarray(key)
    n = len(key)
    ends = np.empty(n, np.int64)
    e = n
    for j in range(n - 1, -1, -1):
        if j + 1 < n and key[j + 1] != key[j]:
            e = j + 1
        ends[j] = e
    return ends


def model_from_hits(stages, key, hits, stats=None):
    """hits: per stage the records satisfying it (bool arrays)"""
    key = np.asarray(key)
    slots, owner = slots_of(stages)
    ends = segment_ends(key)
    res = many_model(slots, lambda s, p: bool(hits[owner[s]][p]), len(key), lambda j: int(ends[j]), stats)
    return [(e, int(key[e]), trav) for e, trav in res]


def model_matches(stages, key, val, topic=None, stats=None):
    """what oracle_matches returns for the pattern over a key-grouped batch: (record, key, traversal)"""
    return model_from_hits(stages, key, [FL.stage_hits(st, val, topic) for st in stages], stats)


def n_slots(stages):
    return sum(st["times"] for st in stages)


# ---- generators ----
def exclusive(p, q):
    """two `value == c` stages that no record satisfies together: distinct constants, or distinct topics"""
    return p["c"] != q["c"] or (p["topic"] is not None and q["topic"] is not None and p["topic"] != q["topic"])


def random_stages(rng, variant, alphabet):
    """3-5 stages of `value == c`, adjacent constants distinct, the first strict and plain, oneOrMore on some
    middle stages (at least one), at least one skip-till-next stage.  variant: "plain"; "topics" (topic filters
    on some stages; a oneOrMore stage and its successor may then share the constant on different topics);
    "times" (times(1..2) on stages that are not oneOrMore nor first); "strict" (4-5 stages, a strict oneOrMore
    stage before a strict successor)."""
    while True:
        k = int(rng.integers(4, 6)) if variant == "strict" else int(rng.integers(3, 6))
        stages, prev = [], -1
        for i in range(k):
            c = int(rng.integers(0, alphabet))
            while c == prev:
                c = int(rng.integers(0, alphabet))
            prev = c
            st = stage(f"s{i}", bool(i > 0 and rng.random() < 0.6), c=c,
                       many=bool(0 < i < k - 1 and rng.random() < 0.6))
            if variant == "topics" and rng.random() < 0.5:
                st["topic"] = str(rng.choice(["t0", "t1"]))
            if variant == "times" and i > 0 and not st["many"]:
                st["times"] = int(rng.integers(1, 3))
            stages.append(st)
        if variant == "topics":                          # a topic-disjoint pair now and then
            for i in range(1, k - 1):
                if stages[i]["many"] and rng.random() < 0.4:
                    stages[i]["topic"], stages[i + 1]["topic"] = "t0", "t1"
                    stages[i + 1]["c"] = stages[i]["c"]
        if variant == "strict":
            i = int(rng.integers(1, k - 1))
            stages[i]["many"], stages[i]["next"], stages[i + 1]["next"] = True, False, False
        if (any(st["many"] for st in stages) and any(st["next"] for st in stages) and n_slots(stages) <= 8 and
                all(exclusive(stages[i], stages[i + 1]) for i in range(k - 1) if stages[i]["many"])):
            return stages


random_stream = FL.random_stream


# ---- the fixed patterns of the tests: A = 0, B = 1, C = 2 over one value column ----
def abc(nxt=(True, True)):
    """A followedBy / next B+ followedBy / next C"""
    return [stage("a", False, c=0), stage("b", nxt[0], c=1, many=True), stage("c", nxt[1], c=2)]


def strict_pair():
    """A, then strict B+ and strict C, then a skip-till-next D: the one combination sensitive to contiguity"""
    return [stage("a", False, c=0), stage("b", False, c=1, many=True), stage("c", False, c=2), stage("d", True, c=3)]


# ---- two columns: the evaluated form.  a: x == 0; b+: x == 1; c: x == 2 and y == 1 ----
_x, _y = Event.field("a"), Event.field("b")
NEXT = Selected.withSkipTilNextMatch


def two_column_pattern():
    return (QueryBuilder().select("a").where(_x == 0).then().select("b", NEXT()).oneOrMore().where(_x == 1).then()
            .select("c", NEXT()).where((_x == 2) & (_y == 1)).build())


TWO_STAGES = [stage("a", False), stage("b", True, many=True), stage("c", True)]    # (its shape, for the model)


def two_column_hits(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return [x == 0, x == 1, (x == 2) & (y == 1)]


# ---- eligibility tables ----
# (name, schema, stages or pattern builder, slots, next_mask, many_mask, evaluated)
ACCEPTED = [
    ("next_b_next_c", I32T, abc((True, True)), 3, 0b110, 0b010, False),
    ("strict_b_next_c", I32T, abc((False, True)), 3, 0b100, 0b010, False),
    ("next_b_strict_c", I32T, abc((True, False)), 3, 0b010, 0b010, False),
    ("b_many_c_many_d", I32T, [stage("a", False, c=0), stage("b", True, c=1, many=True), stage("c", True, c=2, many=True),
                               stage("d", False, c=3)], 4, 0b0110, 0b0110, False),
    ("times_after_many", I32T, [stage("a", False, c=0), stage("b", True, c=1, many=True), stage("c", True, c=2, times=2)],
     4, 0b1110, 0b0010, False),
    ("strict_pair", I32T, strict_pair(), 4, 0b1000, 0b0010, False),
    ("topic_disjoint", I32T, [stage("a", False, c=0), stage("b", True, c=1, many=True, topic="t0"),
                              stage("c", True, c=1, topic="t1")], 3, 0b110, 0b010, False),
    ("evaluated", TWO, two_column_pattern, 3, 0b110, 0b010, True),
]

_v = Event.field("value")


def _q():
    return QueryBuilder()


REJECTED = [
    ("first_many", I32T, lambda: _q().select("a").oneOrMore().where(_v == 0).then().select("b", NEXT()).where(_v == 1).then()
     .select("c", NEXT()).where(_v == 2).build(), "oneOrMore on the first"),
    ("last_many", I32T, lambda: _q().select("a").where(_v == 0).then().select("b", NEXT()).where(_v == 1).then()
     .select("c", NEXT()).oneOrMore().where(_v == 2).build(), "final stage expecting multiple"),   # (the compiler's own)
    ("zero_or_more", I32T, lambda: _q().select("a").where(_v == 0).then().select("b", NEXT()).zeroOrMore().where(_v == 1).then()
     .select("c", NEXT()).where(_v == 2).build(), "zeroOrMore"),
    ("times_with_many", I32T, lambda: _q().select("a").where(_v == 0).then().select("b", NEXT()).oneOrMore().times(2)
     .where(_v == 1).then().select("c", NEXT()).where(_v == 2).build(), "times together with oneOrMore"),
    ("non_disjoint", I32T, lambda: build([stage("a", False, c=0), stage("b", True, kind="ge", c=1, many=True),
                                          stage("c", True, c=2)]), "not provably exclusive"),
    ("same_constant_one_topic", I32T, lambda: build([stage("a", False, c=0), stage("b", True, c=1, many=True, topic="t0"),
                                                     stage("c", True, c=1)]), "not provably exclusive"),
    ("fold", I32T, lambda: _q().select("a").where(_v == 0).then().select("b", NEXT()).oneOrMore().where(_v == 1)
     .fold("sum", _v).then().select("c", NEXT()).where(_v == 2).build(), "fold"),
    ("all_strict", I32T, lambda: build(abc((False, False))), "runs path takes"),
    ("no_many", I32T, lambda: FL.build(FL.abc()), "no oneOrMore stage"),
    ("k9", I32T, lambda: build([stage("a", False, c=0), stage("b", True, c=1, many=True), stage("c", True, c=2, times=4),
                                stage("d", True, c=3, times=3)]), "more than 8"),
]
