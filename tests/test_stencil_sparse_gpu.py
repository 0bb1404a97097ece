"""The plain stencil kernel's key reads (csrc/stencil_kernel.h window_same_keys): a wave reads keys only
where the stage bits alone already make a candidate (sparse), or all its 1024 keys (dense), chosen per
wave.  Every test runs through the C-ABI in the three launch modes -- every wave sparse
(KCEP_STENCIL_SPARSE_KEYS=1), every wave dense (KCEP_STENCIL_DENSE_KEYS=1), adaptive (neither) -- and
compares with the CPU oracle."""
import os

import numpy as np
import pytest

import oracle as O
from kcep import native as N
from kcep import synth, Schema, QueryBuilder, Event, Selected
from gpu_util import oracle_matches, run_product

pytestmark = pytest.mark.gpu

I32 = Schema([("value", "i32")])
MODES = ["sparse", "dense", "adaptive"]


def set_mode(monkeypatch, mode):
    monkeypatch.setenv("KCEP_STENCIL_KEYED", "0")
    monkeypatch.setenv("KCEP_STENCIL_SPARSE_KEYS", "1" if mode == "sparse" else "0")
    monkeypatch.setenv("KCEP_STENCIL_DENSE_KEYS", "1" if mode == "dense" else "0")


def c2_ir():
    return synth.c2_pattern().to_ir(I32)


def always_true_ir():
    return (QueryBuilder().select("a").where(True).then().select("b").where(True).then()
            .select("c").where(True).build().to_ir(I32))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,K", [(1, 1), (2, 1), (3, 1), (4095, 3), (4096, 7), (4097, 1), (12289, 13), (65_537, 1),
                                 (200_000, 100_000)])
def test_c2_random(n, K, mode, monkeypatch):
    """(200000, 100000): two events per key, nearly every candidate rejected by its keys; K = 1: none."""
    set_mode(monkeypatch, mode)
    key, val, order = synth.c2_stream_np(n, K)
    want = oracle_matches(c2_ir(), key, [val], [1], O.MODE_PROCESSOR, offset=order, ts=order)
    got, s = run_product(c2_ir(), key, [val])
    assert s.path == N.PATH_STENCIL
    assert got == want


N_B = 3 * 4096 + 5                     # the tail is no multiple of 4
BREAKS = [None] + [b + off for b in (16 * 40, 1024 * 2, 4096 * 2) for off in range(3)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("brk", BREAKS)
def test_boundaries(brk, mode, monkeypatch):
    """Values cycle 0,1,2 (every third record completes a candidate), one key break at offset 0..K-1
    after a thread (16), a wave (1024) and a tile (4096) boundary, or none.  The three phases of the
    cycle put a candidate at record 0 and at record 1 (their windows start before the batch: no
    match) and a match on the batch's last record."""
    set_mode(monkeypatch, mode)
    i = np.arange(N_B)
    key = np.zeros(N_B, np.int32) if brk is None else (i >= brk).astype(np.int32)
    for shift in range(3):
        val = ((i + shift) % 3).astype(np.int32)
        want = oracle_matches(c2_ir(), key, [val], [1], O.MODE_PROCESSOR)
        got, _ = run_product(c2_ir(), key, [val])
        assert got == want, shift
        recs = [m[0] for m in got]
        if brk is None:                # every record of value 2 from record 2 on completes a match
            assert recs == [j for j in np.flatnonzero(val == 2).tolist() if j >= 2]
            assert shift != 1 or recs[-1] == N_B - 1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7])
def test_k_stages(k, mode, monkeypatch):
    set_mode(monkeypatch, mode)
    rng = np.random.default_rng(k)
    n = 50_000
    key = np.sort(rng.integers(0, 300, n)).astype(np.int32)
    val = rng.integers(0, 3, n).astype(np.int32)          # dense hits: long overlapping runs
    q = QueryBuilder().select("s0").where(Event.value() <= (0 if k > 1 else 1))
    for s in range(1, k):
        q = q.then().select(f"s{s}").where((Event.value() == s % 3) | (Event.value() == 2))
    ir = q.build().to_ir(I32)
    want = oracle_matches(ir, key, [val], [1], O.MODE_PROCESSOR)
    got, s = run_product(ir, key, [val])
    assert s.path == N.PATH_STENCIL
    assert got == want and len(got) > 0


@pytest.mark.parametrize("mode", MODES)
def test_always_true(mode, monkeypatch):
    """Every record a candidate: 16 per thread in the forced sparse mode."""
    set_mode(monkeypatch, mode)
    n = 20_000
    key = (np.arange(n) // 37).astype(np.int32)
    val = np.zeros(n, np.int32)
    want = oracle_matches(always_true_ir(), key, [val], [1], O.MODE_PROCESSOR)
    got, _ = run_product(always_true_ir(), key, [val])
    assert got == want and len(got) == n - 2 * len(np.unique(key))


@pytest.mark.parametrize("mode", MODES)
def test_half_dense_half_selective(mode, monkeypatch):
    """First half: a value every stage accepts (all candidates); second half: C2 values.  Adaptive takes
    both branches in one launch."""
    set_mode(monkeypatch, mode)
    h = 20_000
    k2, v2, _ = synth.c2_stream_np(h, 200)
    key = np.concatenate([(np.arange(h) // 37).astype(np.int32), k2 + 1000]).astype(np.int32)
    val = np.concatenate([np.full(h, 9, np.int32), v2])
    q = QueryBuilder().select("A").where((Event.value() == 0) | (Event.value() == 9))
    q = q.then().select("B").where((Event.value() == 1) | (Event.value() == 9))
    q = q.then().select("C").where((Event.value() == 2) | (Event.value() == 9))
    ir = q.build().to_ir(I32)
    want = oracle_matches(ir, key, [val], [1], O.MODE_PROCESSOR)
    got, s = run_product(ir, key, [val])
    assert s.path == N.PATH_STENCIL
    assert got == want
    recs = np.array([m[0] for m in got])
    assert (recs < h).sum() > h // 2 and 0 < (recs >= h).sum() < h // 20


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("t", ["i64", "f64"])
def test_wide_columns(t, mode, monkeypatch):
    set_mode(monkeypatch, mode)
    rng = np.random.default_rng(7)
    n = 60_000
    key = np.sort(rng.integers(0, 500, n)).astype(np.int32)
    raw = rng.integers(-5, 6, n)
    val = (raw * 1_000_000_007).astype(np.int64) if t == "i64" else raw.astype(np.float64) * 0.5
    sch = Schema([("value", t)])
    c = 1_000_000_007 if t == "i64" else 0.5
    q = (QueryBuilder().select("lo").where(Event.value() < 0).then()
         .select("mid").where((Event.value() >= 0) & (Event.value() <= c * 2)).then()
         .select("hi").where(Event.value() > c).build())
    ir = q.to_ir(sch)
    ty = 2 if t == "i64" else 3
    want = oracle_matches(ir, key, [val], [ty], O.MODE_PROCESSOR)
    got, s = run_product(ir, key, [val])
    assert s.path == N.PATH_STENCIL
    assert got == want and len(got) > 0


@pytest.mark.parametrize("mode", MODES)
def test_topic_filter(mode, monkeypatch):
    set_mode(monkeypatch, mode)
    rng = np.random.default_rng(3)
    n = 40_000
    key = np.sort(rng.integers(0, 400, n)).astype(np.int32)
    val = rng.integers(0, 3, n).astype(np.int32)
    topic = rng.integers(0, 2, n).astype(np.int32)
    sch = Schema([("value", "i32")], topics=["t0", "t1"])
    q = (QueryBuilder().select("a", Selected.withStrictContiguity().withTopic("t1")).where(Event.value() == 0)
         .then().select("b").where(Event.value() != 0).then()
         .select("c", Selected.withStrictContiguity().withTopic("t0")).where(Event.value() == 2).build())
    ir = q.to_ir(sch)
    want = oracle_matches(ir, key, [val], [1], O.MODE_PROCESSOR, topic=topic)
    got, s = run_product(ir, key, [val], topic=topic)
    assert s.path == N.PATH_STENCIL
    assert got == want and len(got) > 0


def test_contract_breaker(monkeypatch):
    """An unsorted key column (the grouping contract broken): the three modes return the same CSR, which
    is the every-adjacent-pair answer of the all-keys kernel -- with keys drawn from four values, many
    windows have first == last around a different middle key."""
    n = 100_003
    _, val, _ = synth.c2_stream_np(n, 1000)
    key = np.random.default_rng(11).integers(0, 4, n).astype(np.int32)
    outs = []
    for mode in MODES:
        set_mode(monkeypatch, mode)
        s = N.Session(N.CompiledPattern(c2_ir()), n)
        s.push(n, key, [val])
        outs.append(s.collect())
    for o in outs[1:]:
        for f in ("match_record", "match_key", "ent_off", "ent_name", "ent_record"):
            assert np.array_equal(o[f], outs[0][f]), f
    j = np.arange(2, n)
    ok = ((val[j - 2] == 0) & (val[j - 1] == 1) & (val[j] == 2) & (key[j - 2] == key[j - 1]) & (key[j - 1] == key[j]))
    shortened = (val[j - 2] == 0) & (val[j - 1] == 1) & (val[j] == 2) & (key[j - 2] == key[j])
    assert ok.sum() < shortened.sum()                      # the data tells the two tests apart
    assert np.array_equal(np.asarray(outs[0]["match_record"]), j[ok])


@pytest.fixture(scope="module")
def four_tile_stream():
    """The smallest batch that runs four tiles per workgroup (8192 tiles): C2 values, 1M keys."""
    import torch
    n = 8192 * 4096 + 1000
    key, val, order = synth.c2_stream_torch(n, 1_000_000, "cuda")
    hk, hv, ho = key.cpu().numpy(), val.cpu().numpy(), order.cpu().numpy()
    del order
    b = O.BatchArrays(hk, [hv], [1], offset=ho, ts=ho)
    want = O.baseline(O.OraclePattern(c2_ir()), b, O.MODE_PROCESSOR, min(16, os.cpu_count() or 1))
    yield n, key, val, want
    del key, val
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mode", MODES)
def test_four_tile_loop(four_tile_stream, mode, monkeypatch):
    """The in-workgroup tile loop and its prefetch."""
    import torch
    set_mode(monkeypatch, mode)
    n, key, val, want = four_tile_stream
    s = N.Session(N.CompiledPattern(c2_ir()), n)
    s.push(n, key.data_ptr(), [val.data_ptr()], mem=N.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    assert s.checksum() == tuple(want) and want[0] > 100_000
