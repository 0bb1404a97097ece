"""The follow path's evaluated form on the device (CEP_SESSION_MASK_PASS with CEP_SESSION_FOLLOW /
CEP_SESSION_FOLLOW_CARRY, csrc/follow_bits_dev.h): skip-till-next patterns whose predicates read several columns,
arithmetic or event metadata, evaluated by the streaming kernel straight into the slots' bitmaps -- in both builds
of that kernel (compiled for the pattern, and the built-in interpreting one).  Every comparison is an exact list
against the CPU oracle, nothing excluded."""
import functools

import numpy as np
import pytest

import oracle as O
from kcep import native as N
from kcep.ingest import ColumnDecoder
from kcep.processor import GpuCEPProcessor
from kcep.sequence import Event as Ev, sequence_from_traversal
from gpu_util import oracle_matches, product_matches
import filter_util as U
import follow_mask_lib as FM

pytestmark = pytest.mark.gpu

BUILDS = pytest.mark.parametrize("interpret", [False, True], ids=["jit", "interp"])
T = 4096                                                 # (asserted below: the ids must not need the library)


@functools.lru_cache(maxsize=None)
def ir_of(name):
    schema, st = {"fm2": (FM.PV, FM.fm2), "richf": (FM.RICH, FM.richf), "k8": (FM.PV, FM.k8), "k2": (FM.PV, FM.k2),
                  "six": (FM.SIX, FM.six), "f64": (FM.PVF, FM.f64_nan), "i64": (FM.PV, FM.i64_big),
                  "abc": (FM.PV, FM.sym_abc), "abC": (FM.PV, lambda: FM.sym_abc((True, False)))}[name]
    return FM.build(st()).to_ir(schema)


def omode(mode):
    return O.MODE_PROCESSOR if mode == N.MODE_PROCESSOR else O.MODE_NFA_PER_KEY


def run_fm(ir, key, cols, interpret=False, mode=N.MODE_NFA, forced=False, **kw):
    """one batch through a session opened on the evaluated form by the two flags, or by force_path and mask_pass"""
    cp = N.CompiledPattern(ir)
    s = N.Session(cp, max(1, len(key)), mode=mode, mask_pass=True, follow=not forced,
                  force_path=N.PATH_FOLLOW if forced else 0, interpret=interpret)
    assert s.path == N.PATH_FOLLOW
    assert s.jit == (not interpret)
    s.push(len(key), np.ascontiguousarray(key, np.int32), [np.ascontiguousarray(c) for c in cols], **kw)
    out = s.collect()
    assert out["path"] == N.PATH_FOLLOW
    return product_matches(s, out), s, out


def check(name, coltypes, key, cols, interpret=False, mode=N.MODE_NFA, min_matches=1, **kw):
    okw = {k: v for k, v in kw.items() if k != "flags"}
    want = oracle_matches(ir_of(name), key, cols, coltypes, omode(mode), **okw)
    assert len(want) >= min_matches
    got, s, _ = run_fm(ir_of(name), key, cols, interpret, mode, **kw)
    assert got == want
    return want, s


# ---- 1. sizes: words, tiles, the last partial group ----
@functools.lru_cache(maxsize=None)
def sized(n):
    if n <= 5:                                           # (price, volume) = (1, 2) takes every stage of FM2
        key, cols = np.zeros(n, np.int32), [np.full(n, 1, np.int64), np.full(n, 2, np.int64)]
    else:
        key, cols = FM.ML.pv_stream(n, 1, n)
    return key, cols, oracle_matches(ir_of("fm2"), key, cols, FM.PV_T, O.MODE_NFA_PER_KEY)


@BUILDS
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 5])
def test_sizes_one_key(n, interpret):
    assert N.follow_tile_records() == T
    key, cols, want = sized(n)
    assert len(want) >= (1 if n >= 3 else 0) and (n < 4095 or len(want) > 1000)
    got, _, _ = run_fm(ir_of("fm2"), key, cols, interpret)
    assert got == want


# ---- 2. key changes at the edges of words, tiles and inside a group of four ----
@pytest.mark.parametrize("cut", [64, 4096, 4097, 1001, 1002, 1003, 1004])
def test_key_changes_at_an_edge(cut):
    n = 2 * T + 5
    rng = np.random.default_rng(cut)
    key = (np.arange(n) >= cut).astype(np.int32)         # the last key runs to n
    val = rng.integers(0, 3, n)
    # a strict hop whose next record is the next key's first and satisfies the slot: a b | c
    val[cut - 4:cut + 1] = [3, 3, 0, 1, 2]
    want, _ = check("abC", FM.PV_T, key, FM.sym_cols(val))
    assert not any(m[0] == cut for m in want)
    # a skip-till-next hop whose next set bit lies in the next key: a, then no b before the cut
    val2 = val.copy()
    val2[cut - 6:cut + 2] = [0, 3, 3, 3, 3, 3, 1, 2]
    want2, _ = check("abc", FM.PV_T, key, FM.sym_cols(val2), interpret=True)
    assert not any(r == cut - 6 for m in want2 for _, r in m[2])
    # the last key's last records complete a walk at n - 1
    val3 = val.copy()
    val3[-3:] = [0, 1, 2]
    want3, _ = check("abc", FM.PV_T, key, FM.sym_cols(val3))
    assert want3[-1][0] == n - 1


# ---- 3. RICHF: i32 overflow, f64 division with NaNs, a topic filter, times(2), metadata and its defaults ----
@BUILDS
@pytest.mark.parametrize("mode", [N.MODE_NFA, N.MODE_PROCESSOR], ids=["nfa", "processor"])
@pytest.mark.parametrize("given", ["arrays", "no_offset", "positions"])
def test_richf(given, mode, interpret):
    key, cols, topic, partition, offset, ts = FM.ML.rich_stream(1500, 40, 6)
    assert np.isnan(cols[2]).any() and (cols[0].astype(np.int64) ** 2 > 2 ** 31).any()
    kw = dict(topic=topic, partition=partition)
    if given == "arrays":
        kw.update(offset=offset, ts=ts, flags=N.BATCH_OFFSETS_MONOTONE)
    elif given == "no_offset":                           # offset() is the record's position, timestamp() given
        kw.update(ts=np.arange(1500, dtype=np.int64) + (ts - offset))
    check("richf", FM.RICH_T, key, cols, interpret, mode, min_matches=5, **kw)


# ---- 4. columns past the four the interpreted table keeps in registers; K = 8 and K = 2 ----
@BUILDS
def test_six_columns(interpret):
    key, cols = FM.six_stream(3000, 30, 7)
    check("six", FM.SIX_T, key, cols, interpret, min_matches=50)


@BUILDS
def test_k8_and_k2(interpret):
    rng = np.random.default_rng(5)
    key = np.sort(rng.integers(0, 60, 5000)).astype(np.int32)
    val = rng.integers(0, 4, 5000)
    at = int(np.flatnonzero(key == 30)[0])
    val[at:at + 8] = [0, 1, 1, 1, 2, 2, 2, 0]            # (one match of the eight slots at least)
    assert key[at + 7] == 30
    want, _ = check("k8", FM.PV_T, key, FM.sym_cols(val), interpret)
    assert any(len({r for _, r in m[2]}) == 8 for m in want)
    check("k2", FM.PV_T, key, FM.sym_cols(val), interpret, min_matches=100)


# ---- 5. column types ----
@BUILDS
def test_f64_with_nans(interpret):
    rng = np.random.default_rng(6)
    key = np.sort(rng.integers(0, 100, 3000)).astype(np.int32)
    vals = np.array([np.nan, 0.0, 0.25, 1.0, 1.5, 2.0, -np.inf, np.inf])
    cols = [rng.choice(vals, 3000), rng.choice(vals, 3000)]
    assert np.isnan(cols[0]).sum() > 100
    check("f64", FM.PVF_T, key, cols, interpret, min_matches=50)


@BUILDS
def test_i64_beyond_int32(interpret):
    rng = np.random.default_rng(7)
    key = np.sort(rng.integers(0, 100, 3000)).astype(np.int32)
    vals = np.array([2 ** 40 + 1, 2 ** 40, -2 ** 40, 5, 2 ** 32 + 5, 0, -2 ** 62, 2 ** 33], np.int64)
    cols = [rng.choice(vals, 3000), rng.choice(vals[2:6], 3000)]
    check("i64", FM.PV_T, key, cols, interpret, min_matches=5)


# ---- 6. sparse hits: the second level of the bitmaps ----
def test_long_gap_one_key():
    n = 300_000
    val = np.full(n, 3)
    val[0], val[n - 2], val[n - 1] = 0, 1, 2
    want, _ = check("abc", FM.PV_T, np.zeros(n, np.int32), FM.sym_cols(val))
    assert want == [(n - 1, 0, [("c", n - 1), ("b", n - 2), ("a", 0)])]


# ---- 7. ways onto the path, and off it ----
@functools.lru_cache(maxsize=None)
def small():
    key, cols = FM.ML.pv_stream(6000, 80, 9)
    return key, cols, oracle_matches(ir_of("fm2"), key, cols, FM.PV_T, O.MODE_NFA_PER_KEY)


def test_ways_onto_the_path():
    key, cols, want = small()
    assert len(want) > 100
    by_flags, _, _ = run_fm(ir_of("fm2"), key, cols)
    forced, _, _ = run_fm(ir_of("fm2"), key, cols, forced=True)
    assert by_flags == forced == want
    cp = N.CompiledPattern(ir_of("fm2"))
    with pytest.raises(N.CepError) as e:                 # the forced path without the flag: as it always failed
        N.Session(cp, 64, mode=N.MODE_NFA, force_path=N.PATH_FOLLOW, follow=True)
    assert e.value.code == 12 and "follow path does not apply" in str(e.value)
    for kw in (dict(follow=True), dict(mask_pass=True), dict()):   # one flag alone: where it always opened
        s = N.Session(cp, len(key), mode=N.MODE_NFA, **kw)
        assert s.path == N.PATH_GENERAL
        s.push(len(key), key, cols)
        assert product_matches(s, s.collect()) == want
    # carry sessions: CEP_SESSION_FOLLOW alone does nothing there, CEP_SESSION_FOLLOW_CARRY opens the path
    assert N.Session(cp, 64, carry=True, max_keys=8, mask_pass=True, follow=True).path == N.PATH_GENERAL
    assert N.Session(cp, 64, carry=True, max_keys=8, follow_carry=True).path == N.PATH_GENERAL
    assert N.Session(cp, 64, carry=True, max_keys=8, mask_pass=True, follow_carry=True).path == N.PATH_FOLLOW


@BUILDS
def test_split_form_gives_the_same(interpret, monkeypatch):
    key, cols, want = small()
    fused, s, _ = run_fm(ir_of("fm2"), key, cols, interpret)
    monkeypatch.setenv("KCEP_FOLLOW_MASK_SPLIT", "1")    # read at session open
    split, s2, _ = run_fm(ir_of("fm2"), key, cols, interpret)
    assert fused == split == want
    assert s.checksum() == s2.checksum()
    key, cols, topic, partition, offset, ts = FM.ML.rich_stream(1500, 40, 6)
    kw = dict(topic=topic, partition=partition, offset=offset, ts=ts, flags=N.BATCH_OFFSETS_MONOTONE)
    split, s2, _ = run_fm(ir_of("richf"), key, cols, interpret, **kw)
    monkeypatch.delenv("KCEP_FOLLOW_MASK_SPLIT")
    fused, s, _ = run_fm(ir_of("richf"), key, cols, interpret, **kw)
    assert fused == split and len(fused) > 5 and s.checksum() == s2.checksum()


def test_checksum_count_and_second_collect():
    import torch
    key, cols, want = small()
    got, s, out = run_fm(ir_of("fm2"), key, cols)
    n, h = s.checksum()
    assert n == len(want)
    g = N.Session(N.CompiledPattern(ir_of("fm2")), len(key), mode=N.MODE_NFA, force_path=N.PATH_GENERAL)
    g.push(len(key), key, cols)
    assert product_matches(g, g.collect()) == got
    assert g.checksum() == (n, h)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    s.match_count_to(cnt.data_ptr())
    torch.cuda.synchronize()
    assert int(cnt.item()) == n
    again = s.collect()
    for f in ("match_record", "match_key", "ent_off", "ent_name", "ent_record"):
        assert np.array_equal(out[f], again[f])
    s.push(0, key[:0], [c[:0] for c in cols])            # an empty batch
    assert product_matches(s, s.collect()) == [] and s.checksum()[0] == 0


def test_device_resident_input():
    import torch
    key, cols, want = small()
    n = len(key)
    s = N.Session(N.CompiledPattern(ir_of("fm2")), n, mode=N.MODE_NFA, mask_pass=True, follow=True)
    assert s.path == N.PATH_FOLLOW
    dk, dp, dv = (torch.from_numpy(a).cuda() for a in (key, cols[0], cols[1]))
    s.push(n, dk.data_ptr(), [dp.data_ptr(), dv.data_ptr()], mem=N.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    out = s.collect()
    assert out["path"] == N.PATH_FOLLOW and product_matches(s, out) == want
    assert s.last_kernel_ms() > 0 and s.last_batch_ms() >= s.last_kernel_ms()
    with pytest.raises(N.CepError) as e:                 # the second column 8 bytes off a 16-byte boundary
        s.push(n - 1, dk.data_ptr(), [dp.data_ptr(), dv.data_ptr() + 8], mem=N.MEM_DEVICE)
    assert e.value.code == 11 and "aligned" in str(e.value)


def test_fallback_batch_and_the_next_push():
    key, cols, _ = small()
    n = len(key)
    ir = ir_of("fm2")
    s = N.Session(N.CompiledPattern(ir), n, mode=N.MODE_PROCESSOR, mask_pass=True, follow=True)
    assert s.path == N.PATH_FOLLOW
    valid = (np.arange(n) % 7 != 3).astype(np.uint8)
    s.push(n, key, cols, valid=valid)
    out = s.collect()
    assert out["path"] == N.PATH_GENERAL
    dropped = oracle_matches(ir, key, cols, FM.PV_T, O.MODE_PROCESSOR, valid=valid)
    assert product_matches(s, out) == dropped
    clean = oracle_matches(ir, key, cols, FM.PV_T, O.MODE_PROCESSOR)
    s.push(n, key, cols)
    out = s.collect()
    assert out["path"] == N.PATH_FOLLOW and product_matches(s, out) == clean and clean != dropped


# ---- 8. carry sessions: walks that wait across cuts, positions as the defaults, a checkpoint mid-stream ----
def _carry_stream(name, seed):
    if name == "fm2":
        key, cols = FM.ML.pv_stream(2400, 40, seed)
        n = len(key)
        z = np.zeros(n, np.int32)
        return dict(key=key, cols=cols, topic=z, partition=z, offset=np.arange(n, dtype=np.int64), ts=np.arange(n, dtype=np.int64))
    key, cols, topic, partition, offset, ts = FM.ML.rich_stream(2400, 40, seed)
    return dict(key=key, cols=cols, topic=topic, partition=partition, offset=offset, ts=ts)


@BUILDS
@pytest.mark.parametrize("name,given", [("fm2", "positions"), ("richf", "arrays"), ("richf", "no_offset"), ("richf", "positions")])
def test_carry(name, given, interpret):
    rng = np.random.default_rng(len(name) * 10 + len(given))
    st = _carry_stream(name, 8)
    n, nk = len(st["key"]), 40
    parts = FM.cut_stream(rng, st["key"], int(rng.integers(3, 6)))
    pos = FM.positions(parts, n)
    if given == "no_offset":                             # timestamps a little ahead of the positions
        st["ts"] = pos + (st["ts"] - st["offset"])
    coltypes = FM.PV_T if name == "fm2" else FM.RICH_T
    ir = ir_of(name)
    want = FM.oracle_batches(ir, coltypes, st, parts, explicit_ts=given != "positions", explicit_offset=given == "arrays")
    assert sum(len(w) for w in want) > 20
    # matches whose start lies in an earlier batch: walks waited across a cut
    first = np.cumsum([0] + [len(p) for p in parts])
    assert sum(m[2][-1][1] < first[b] for b, w in enumerate(want) for m in w) > 3
    cp = N.CompiledPattern(ir)

    def open_session():
        s = N.Session(cp, max(len(p) for p in parts), mode=N.MODE_NFA, carry=True, max_keys=nk, mask_pass=True,
                      follow_carry=True, interpret=interpret)
        assert s.path == N.PATH_FOLLOW and s.jit == (not interpret)
        return s

    s = open_session()
    for b, idx in enumerate(parts):
        if b == len(parts) // 2:                         # checkpoint, restore into a fresh session, go on there
            blob, at = s.state_export(), s.stream_position()
            assert blob[:4] == b"KCSW" and at == first[b] > 0
            s = open_session()
            s.state_import(blob)
            assert s.stream_position() == at
        kw = dict(topic=st["topic"][idx], partition=st["partition"][idx])
        if given != "positions":
            kw["ts"] = np.ascontiguousarray(st["ts"][idx])
        if given == "arrays":
            kw.update(offset=np.ascontiguousarray(st["offset"][idx]), flags=N.BATCH_OFFSETS_MONOTONE)
        s.push(len(idx), np.ascontiguousarray(st["key"][idx]), [np.ascontiguousarray(c[idx]) for c in st["cols"]], **kw)
        out = s.collect()
        assert out["path"] == N.PATH_FOLLOW
        assert product_matches(s, out) == want[b], b
    assert s.stream_position() == n


# ---- 9. the processor: an interleaved stream with nulls and re-deliveries, filtered on the device ----
def _seq_view(seq):
    return [(st.getStage(), [e.offset for e in st.getEvents()]) for st in seq.matched()]


@pytest.mark.parametrize("batch,n", [(1, 300), (7, 700), (64, 2000)])
def test_processor(batch, n):
    rng = np.random.default_rng(batch)
    st = U.make_stream(rng, rng.integers(0, 12, n).astype(np.int32), ntopics=1)
    pri = st["val"].astype(np.int64)
    vol = ((st["off"] * 7 + st["key"] * 3) % 4).astype(np.int64)   # follows from key and offset: a re-delivery repeats it
    assert (st["valid"] == 0).sum() > 5
    recs = [(f"k{int(k)}", (int(p), int(v)) if ok else None, "events", 0, int(o), int(t))
            for k, p, v, ok, o, t in zip(st["key"], pri, vol, st["valid"], st["off"], st["ts"])]
    stages = FM.fm2()
    ir = FM.build(stages).to_ir(FM.PV)
    p = O.OraclePattern(ir)
    r = O.OracleRun(p, O.MODE_PROCESSOR)
    r.process(O.BatchArrays(st["key"], [pri, vol], FM.PV_T, valid=st["valid"], offset=st["off"], ts=st["ts"]))
    ev = lambda i: Ev(recs[i][0], recs[i][1], recs[i][5], recs[i][2], recs[i][3], recs[i][4])
    want = [(recs[m.record][0], _seq_view(sequence_from_traversal(m.traversal, p.names, ev)))
            for m in r.matches(with_groups=False)]
    assert len(want) > 20
    dec = ColumnDecoder(FM.PV, [lambda v: v[0], lambda v: v[1]])
    proc = GpuCEPProcessor("fm2", FM.build(stages), FM.PV, dec, batch_size=batch, max_keys=64, follow=True, mask_pass=True,
                           device_filter=True)
    got = []
    proc.init(lambda k, s: got.append((k, _seq_view(s))))
    assert proc.session.path == N.PATH_FOLLOW and proc.session.jit
    for rec in recs:
        proc.process(*rec)
    proc.close()
    assert got == want
