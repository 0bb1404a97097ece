"""The stencil kernels' stage masks and window test (csrc/stencil_kernel.h): the dense-table look-up
(one clamp, one LDS read per record) at its edges, the breakpoint arm where the table does not fit, the
full-tile and tail arms of the tile image, and the byte-wise window test for every K -- each against the
oracle, the ordered CSR of collect() element by element.

A pattern here is a list of stages, a stage a list of inclusive value ranges (None: open), so the test
knows the breakpoints compile.cpp build_table derives (every range start, every range end + 1) and can
draw the values around them: lo - 2 .. lo and lo + lut_n - 1 .. lo + lut_n + 1 for the table's range
[lo, lo + lut_n), the extremes of the column type, and one value inside every range."""
import functools
import os

import numpy as np
import pytest

import oracle as O
from kcep import native as N
from kcep import synth, Schema, QueryBuilder, Event, Selected
import mask_pass_lib as ML
from gpu_util import oracle_matches, product_matches
from test_carry_gpu import _strict_pattern, batches_of, oracle_run, run_carry
from test_stencil_finish_gpu import FIELDS, TILE, k_stage_ir, same

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
IMIN, IMAX = -2**31, 2**31 - 1
SIZES = [1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5]
TYPES = {"i32": (1, np.int32), "i64": (2, np.int64), "f64": (3, np.float64)}

# name -> (stages, the arm an i32 column takes).  Breakpoints: range starts and range ends + 1.
PATTERNS = {
    # 1 breakpoint {5}: a table of one entry between below and above
    "bp1": ([[(5, None)], [(5, None)], [(5, None)]], "lut"),
    # 4 {0, 1, 2, 3}: C2's
    "bp4": ([[(0, 0)], [(1, 1)], [(2, 2)]], "lut"),
    # 6 {-3, -1, 0, 2, 3, 7}
    "bp6": ([[(-3, -2)], [(0, 1)], [(3, 6)]], "lut"),
    # 15: seven points three apart (14) and one open range
    "bp15": ([[(100, 100), (103, 103), (106, 106)], [(109, 109), (112, 112), (115, 115)], [(118, 118), (121, None)]], "lut"),
    # lo - 1 == INT32_MIN, the lowest clamp bound an int32 holds: breakpoints {MIN + 1, MIN + 3, MIN + 4}
    "min_fits": ([[(None, IMIN)], [(IMIN + 3, None)], [(IMIN + 4, None)]], "lut"),
    # a breakpoint at INT32_MIN itself (lo - 1 is no int32): {MIN, MIN + 1, MIN + 2, MIN + 3}
    "min_over": ([[(IMIN, IMIN)], [(IMIN + 1, IMIN + 1)], [(IMIN + 2, None)]], "bp"),
    # lo + lut_n == INT32_MAX, the highest clamp bound: {MAX - 4, MAX - 2, MAX - 1}
    "max_fits": ([[(None, IMAX - 5)], [(IMAX - 2, None)], [(IMAX - 1, None)]], "lut"),
    # a breakpoint at INT32_MAX (lo + lut_n is no int32): {MAX - 2, MAX - 1, MAX}
    "max_over": ([[(None, IMAX - 3)], [(IMAX - 1, None)], [(IMAX, IMAX)]], "bp"),
    # a range of 1001 values: no table
    "wide": ([[(0, 0)], [(300, 300)], [(1000, None)]], "bp"),
}


def pattern_ir(stages, t):
    q = None
    for i, ranges in enumerate(stages):
        pred = None
        for a, b in ranges:
            v = Event.value()
            term = (v >= a) & (v <= b) if a is not None and b is not None else v >= a if b is None else v <= b
            pred = term if pred is None else pred | term
        q = (QueryBuilder() if q is None else q.then()).select(f"s{i}").where(pred)
    return q.build().to_ir(Schema([("value", t)]))


def edge_values(stages, t):
    """The values the module docstring lists, as the column's type."""
    bps = sorted({a for st in stages for a, b in st if a is not None} | {b + 1 for st in stages for a, b in st if b is not None})
    lo, n = bps[0], bps[-1] - bps[0] + 1
    vals = {lo - 2, lo - 1, lo, lo + n - 1, lo + n, lo + n + 1, IMIN, IMAX}
    vals |= {a if a is not None else b for st in stages for a, b in st}
    vals |= {b if b is not None else a + 7 for st in stages for a, b in st}
    if t == "i32":
        return np.array(sorted(v for v in vals if IMIN <= v <= IMAX), np.int32)
    if t == "i64":
        return np.array(sorted(vals | {-2**63, 2**63 - 1, IMIN - 1, IMAX + 1}), np.int64)
    return np.array(sorted(vals) + [-np.inf, np.inf, np.nan, -0.0, 0.5], np.float64)


def want_csr(ir, key, val, ty):
    return O.baseline_csr(O.OraclePattern(ir), O.BatchArrays(key, [val], [ty]), O.MODE_PROCESSOR, THREADS)


def collect(ir, key, cols, path=N.PATH_STENCIL, **kw):
    s = N.Session(N.CompiledPattern(ir), max(1, len(key)))
    assert s.path == path
    s.push(len(key), key, cols, **kw)
    return s.collect()


@functools.lru_cache(maxsize=None)
def stream(name, t, n):
    """keys in runs of ~6; half the values drawn evenly from the pattern's edge values, half from the
    first value of every range (so that matches are not rare)"""
    rng = np.random.default_rng([sum(map(ord, name)), len(t) + ord(t[0]), n])
    key = np.sort(rng.integers(0, max(1, n // 6), n)).astype(np.int32)
    stages = PATTERNS[name][0]
    edges = edge_values(stages, t)
    inside = np.array([a if a is not None else b for st in stages for a, b in st]).astype(edges.dtype)
    val = np.where(rng.random(n) < 0.5, rng.choice(edges, n), rng.choice(inside, n))
    return key, val


@pytest.mark.parametrize("t", sorted(TYPES))
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_lookup_edges_and_sizes(name, t):
    """Every pattern at every size on every column type: one tile, a partial tile, several tiles; the
    values at the table's edges and the type's extremes (f64: with NaN, infinities and -0.0)."""
    ir = pattern_ir(PATTERNS[name][0], t)
    total = 0
    for n in SIZES:
        key, val = stream(name, t, n)
        want = want_csr(ir, key, val, TYPES[t][0])
        total += len(want["match_record"])
        same(collect(ir, key, [val]), want, (name, t, n))
    assert total > 20


def test_lookup_edges_cover_both_arms():
    """The values reach below, inside and above every table, and both clamp bounds are hit where they
    are the type's extremes."""
    for name, (stages, arm) in PATTERNS.items():
        v = edge_values(stages, "i32").astype(np.int64)
        bps = sorted({a for st in stages for a, b in st if a is not None} | {b + 1 for st in stages for a, b in st if b is not None})
        fits = bps[-1] - bps[0] < 256 and bps[0] > IMIN and bps[-1] < IMAX
        assert fits == (arm == "lut"), name
        assert {IMIN, IMAX} <= set(v.tolist())
        if arm == "lut":
            assert (v < bps[0]).any() and (v > bps[-1]).any() and ((v >= bps[0]) & (v <= bps[-1])).any(), name
    assert sorted({len({a for st in s for a, b in st if a is not None} | {b + 1 for st in s for a, b in st if b is not None})
                   for s, _ in PATTERNS.values()} & {1, 4, 6, 15}) == [1, 4, 6, 15]


def test_four_tiles_per_workgroup_one_record_last_tile():
    """8192 * 4096 + 1 records: the smallest batch at four tiles per workgroup; the last workgroup has one
    tile of one record, every other tile is whole (no tail masks)."""
    import torch
    n = 8192 * TILE + 1
    dk, dv, order = synth.c2_stream_torch(n, 1_000_000, "cuda")
    del order
    key, val = dk.cpu().numpy(), dv.cpu().numpy()
    val[-3:] = [0, 1, 2]                                 # a match that completes at the batch's last record
    key[-3:] = key[-1]
    dv = torch.from_numpy(val).cuda()
    dk = torch.from_numpy(key).cuda()
    ir = synth.c2_pattern().to_ir(Schema([("value", "i32")]))
    want = want_csr(ir, key, val, 1)
    assert want["match_record"][-1] == n - 1 and len(want["match_record"]) > 100_000
    s = N.Session(N.CompiledPattern(ir), n)
    assert s.path == N.PATH_STENCIL
    s.push(n, dk.data_ptr(), [dv.data_ptr()], mem=N.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    got = s.collect()
    same(got, want, "8192 tiles + 1 record")
    del dk, dv, s
    torch.cuda.empty_cache()


def test_topic_column():
    """A topic column keeps the breakpoint arm (test_stencil_gpu.test_topic_filter's pattern), three tiles
    and a tail."""
    rng = np.random.default_rng(3)
    n = 3 * TILE + 5
    key = np.sort(rng.integers(0, n // 8, n)).astype(np.int32)
    val = rng.integers(0, 3, n).astype(np.int32)
    topic = rng.integers(0, 2, n).astype(np.int32)
    sch = Schema([("value", "i32")], topics=["t0", "t1"])
    q = (QueryBuilder().select("a", Selected.withStrictContiguity().withTopic("t1")).where(Event.value() == 0)
         .then().select("b").where(Event.value() != 0).then()
         .select("c", Selected.withStrictContiguity().withTopic("t0")).where(Event.value() == 2).build())
    ir = q.to_ir(sch)
    want = O.baseline_csr(O.OraclePattern(ir), O.BatchArrays(key, [val], [1], topic=topic), O.MODE_PROCESSOR, THREADS)
    assert len(want["match_record"]) > 20
    same(collect(ir, key, [val], topic=topic), want, "topic")


@pytest.mark.parametrize("k", [1, 2, 3, 4, 7])
def test_k_stages(k):
    """The window test for K = 1, 2, 3, 4, 7 (a window reaches K - 1 records back: across threads' 16-record
    runs, waves and tiles), dense in matches; one tile, and three tiles with a tail."""
    ir = k_stage_ir(k)
    for n in (17, 4096, 3 * TILE + 5):
        rng = np.random.default_rng([k, n])
        key = np.sort(rng.integers(0, max(1, n // 40), n)).astype(np.int32)
        val = rng.integers(0, 3, n).astype(np.int32)
        want = want_csr(ir, key, val, 1)
        if n > 17:
            # not vacuous.  The sparsest case, K = 7: a window matches with probability 16/2187 (the stages
            # accept 1, 2, 1, 2, 2, 1, 2 of the three values) and ~85 % of the windows lie inside one key's
            # run of ~40: ~25 expected matches in 4096 records, standard deviation ~5
            assert len(want["match_record"]) >= 8
        same(collect(ir, key, [val]), want, (k, n))


def test_chain_with_optional_stage():
    """C5's pattern (an optional stage, 8 breakpoints: the dense table in stencil_kernel), three tiles and a tail."""
    n = 3 * TILE + 5
    rng = np.random.default_rng(n)
    key = np.sort(rng.integers(0, n // 15, n)).astype(np.int32)
    val = rng.integers(0, 64, n).astype(np.int32)
    ir = synth.c5_pattern().to_ir(Schema([("value", "i32")]))
    want = want_csr(ir, key, val, 1)
    per = np.diff(want["ent_off"])
    assert (per == 2).any() and (per == 3).any()
    same(collect(ir, key, [val], path=N.PATH_CHAIN), want, "chain")


def test_carry_two_batches_cut_mid_key():
    """A carry session (the plain kernel's carry variant) over one stream in two batches, the cut inside
    a key's records: against one oracle run of the whole stream."""
    rng = np.random.default_rng(11)
    n_keys = 300
    key = np.repeat(np.arange(n_keys, dtype=np.int32), rng.integers(1, 60, n_keys))
    val = rng.integers(0, 2, len(key)).astype(np.int32)
    cut = int(np.flatnonzero(key == n_keys // 2)[0]) + 2
    assert key[cut - 1] == key[cut] == key[cut - 2]      # mid-key, two of its records before the cut
    val[cut - 2:cut + 1] = [0, 1, 0]                     # a match whose first two stages lie before the cut
    ir = _strict_pattern(3)
    want, _, oerr = oracle_run(ir, key, [val], [1], O.MODE_PROCESSOR)
    assert oerr is None and len(want) > 100
    bounds, order = batches_of(key, [cut])
    assert np.array_equal(order, np.arange(len(key)))    # (already grouped: positions are stream positions)
    got, sess, err = run_carry(ir, key, [val], bounds, max_keys=n_keys)
    assert sess.path == N.PATH_STENCIL and err is None
    assert sorted(got) == sorted(want)
    assert any(m[0] >= cut and any(r < cut for _, r in m[2]) for m in got)   # a match across the cut


def test_mask_pass_identity_table():
    """CEP_SESSION_MASK_PASS: the stencil kernel reads the mask column through the 256-entry identity table."""
    n = 3 * TILE + 5
    key, cols = ML.pv_stream(n, n // 8, 5)
    ir = ML.p2().to_ir(ML.PV)
    want = oracle_matches(ir, key, cols, [2, 2], O.MODE_PROCESSOR)
    assert len(want) > 20
    s = N.Session(N.CompiledPattern(ir), n, mask_pass=True)
    assert s.path == N.PATH_STENCIL
    s.push(n, np.ascontiguousarray(key, np.int32), [np.ascontiguousarray(c) for c in cols])
    assert product_matches(s, s.collect()) == want


def test_c2_small():
    """C2 at 2,000,003 events over 20,011 keys, device-resident: count and checksum against the oracle."""
    import torch
    n, K = 2_000_003, 20_011
    key, val, order = synth.c2_stream_torch(n, K, "cuda")
    ir = synth.c2_pattern().to_ir(Schema([("value", "i32")]))
    s = N.Session(N.CompiledPattern(ir), n)
    assert s.path == N.PATH_STENCIL
    s.push(n, key.data_ptr(), [val.data_ptr()], mem=N.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    nm, cs = s.checksum()
    hk, hv, ho = key.cpu().numpy(), val.cpu().numpy(), order.cpu().numpy()
    want = O.baseline(O.OraclePattern(ir), O.BatchArrays(hk, [hv], [1], offset=ho, ts=ho), O.MODE_PROCESSOR, THREADS)
    assert (nm, cs) == tuple(want) and nm > 10_000
