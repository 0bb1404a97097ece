"""Patterns, schemas and streams of the mask-pass tests (CEP_SESSION_MASK_PASS): strict patterns whose
predicates read several columns, arithmetic or event metadata (test_mask_pass_cpu.py, test_mask_pass_gpu.py)."""
import numpy as np

from kcep import QueryBuilder, Selected, Schema, Event, States, SequenceAgg, Long

PV = Schema([("price", "i64"), ("volume", "i64")])
RICH = Schema([("a", "i32"), ("b", "i64"), ("c", "f64")], topics=["t0", "t1"])

price, volume = Event.field("price"), Event.field("volume")
A, B, Cc = Event.field("a"), Event.field("b"), Event.field("c")


def p2():
    """Three strict stages over (price, volume), each `where` reading both fields (dense hits for fields
    uniform in 0..3)."""
    return (QueryBuilder().select("s0").where((price >= 0) & (price + volume == 3)).then()
            .select("s1").where((price <= volume) & (volume - price <= 1)).then()
            .select("s2").where((price > 1) | (volume > 1)).build())


def cyc3():
    """Stage s takes (price + 2 * volume) % 3 == s: one stage per record, cycled by the two fields jointly."""
    v = (price + 2 * volume) % 3
    return (QueryBuilder().select("c0").where((v == 0) & (price >= 0)).then()
            .select("c1").where((v == 1) & (volume >= 0)).then()
            .select("c2").where((v == 2) & (price + volume >= 0)).build())


def two_field_stage(i):
    """a predicate over both fields that no single column decides (fields in 0..3)"""
    forms = [price + volume >= 2, price <= volume, (price > 0) | (volume > 1), price * volume < 6,
             price != volume + 1, (price + volume) % 2 == 0, volume - price < 2, (price >= 1) & (volume <= 2)]
    return forms[i % len(forms)]


def k_stages(k, optional=()):
    b = None
    for i in range(k):
        sel = (QueryBuilder() if b is None else b.then()).select(f"st{i}")
        if i in optional:
            sel = sel.optional()
        b = sel.where(two_field_stage(i))
    return b.build()


def chain3():
    return k_stages(3, optional=(1,))


def chain4():
    return k_stages(4, optional=(1, 2))


def rich():
    """i32 overflow, (double) casts and f64 division with NaNs, metadata, a topic filter."""
    return (QueryBuilder().select("r0").where((A * A > 1000) & (B >= 0)).then()
            .select("r1", Selected.withStrictContiguity().withTopic("t0"))
            .where((B.asDouble() / Cc > 0.5) | (A < 0)).then()
            .select("r2").where((Event.timestamp() - Event.offset() > 2) | (B % 7 == 3)).build())


def rich_stream(n, n_keys, seed):
    """(key, [a, b, c], topic, partition, offset, ts) grouped by key; c has NaNs and zeros, a * a overflows."""
    r = np.random.default_rng(seed)
    key = np.sort(r.integers(0, n_keys, n)).astype(np.int32)
    a = r.choice(np.array([0, 3, 40, -50, 46341, 65536, -2 ** 31, 2 ** 31 - 1], np.int64), n).astype(np.int32)
    b = r.integers(0, 16, n).astype(np.int64)
    c = r.choice(np.array([np.nan, 0.0, -0.0, 1.0, 4.0, 13.0, -2.0]), n)
    topic = r.integers(0, 2, n).astype(np.int32)
    partition = r.integers(0, 3, n).astype(np.int32)
    offset = np.arange(n, dtype=np.int64) * 2 + 5
    ts = offset + r.integers(0, 6, n)
    return key, [a, b, c], topic, partition, offset, ts


def pv_stream(n, n_keys, seed):
    """(key, [price, volume]) grouped by key, fields uniform in 0..3"""
    r = np.random.default_rng(seed)
    key = np.sort(r.integers(0, max(1, n_keys), n)).astype(np.int32)
    return key, [r.integers(0, 4, n).astype(np.int64), r.integers(0, 4, n).astype(np.int64)]


# ---- eligibility table: (name, schema, pattern builder) ----
def _one(pred, schema=PV):
    return lambda: QueryBuilder().select("x").where(pred).then().select("y").where(pred).build()


def _intervals20():
    """one column, 4 stages of 5 disjoint value intervals each: 20 intervals, at most 5 terms per stage"""
    v = Event.field("price")
    b = None
    for st in range(4):
        e = None
        for i in range(5):
            lo = 100 * st + 10 * i
            r = (v >= lo) & (v < lo + 4)
            e = r if e is None else e | r
        b = (QueryBuilder() if b is None else b.then()).select(f"i{st}").where(e)
    return b.build()


ACCEPTED = [
    ("two_i64_fields", PV, _one((price > 100) & (volume > 1000))),
    ("field_vs_field", PV, _one(price < volume)),
    ("i32_overflow", RICH, _one(A * A + 1 > 7)),
    ("double_cast_div", RICH, _one(B.asDouble() / Cc > 0.5)),
    ("rem_const", RICH, _one((B % 7 == 3) & (A > 0))),
    ("timestamp", RICH, _one(Event.timestamp() > 5)),
    ("offset", RICH, _one(Event.offset() % 2 == 0)),
    ("partition", RICH, _one(Event.partition() == 1)),
    ("topic_and_field", RICH, lambda: QueryBuilder().select("x", Selected.withStrictContiguity().withTopic("t1"))
        .where((A > 0) & (B > 1)).then().select("y").where(B < A).build()),
    ("optional_middle", PV, chain3),
    ("two_optionals", PV, chain4),
    ("k8", PV, lambda: k_stages(8)),
    ("intervals20", PV, _intervals20),
]

REJECTED = [
    ("states_get", PV, _one(price > States.getLong("avg")), "state"),
    ("fold", PV, lambda: QueryBuilder().select("x").where(price < volume).fold("avg", price).then()
        .select("y").where(price > volume).build(), "fold"),
    ("sequence_agg", PV, lambda: QueryBuilder().select("x").where(price < volume).then()
        .select("y").where(price > SequenceAgg.sum("price")).build(), "sequence"),
    ("div_by_field", PV, _one((volume != 0) & (10 / volume > 1)), "divisor"),
    ("rem_by_field", PV, _one(price % volume == 1), "divisor"),
    ("div_by_zero", PV, _one(price / Long(0) == 1), "divisor"),
    ("non_strict", PV, lambda: QueryBuilder().select("x").where(price < volume).then()
        .select("y", Selected.withSkipTilNextMatch()).where(price > volume).build(), "non-strict"),
    ("one_or_more", PV, lambda: QueryBuilder().select("x").where(price < volume).then()
        .select("y").oneOrMore().where(price > volume).then().select("z").where(price == volume).build(), "quantifier"),
    ("k9", PV, lambda: k_stages(9), "more than 8 stages"),
    ("optional_first", PV, lambda: k_stages(3, optional=(0,)), "optional first"),
    ("k5_optional", PV, lambda: k_stages(5, optional=(2,)), "more than 4 stages"),
    ("duplicate_names", PV, lambda: QueryBuilder().select("x").where(price < volume).then()
        .select("x").where(price > volume).build(), "duplicate"),
]
