"""The follow path on the device (CEP_SESSION_FOLLOW / CEP_PATH_FOLLOW, csrc/follow.hip): patterns of strict and
skip-till-next stages as deterministic walks over per-slot bitmaps.  Every comparison is an exact list against
the CPU oracle, nothing excluded."""
import functools

import numpy as np
import pytest

import oracle as O
from kcep import native as N
from gpu_util import oracle_matches, product_matches
import follow_lib as FL

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("mode", [N.MODE_PROCESSOR, N.MODE_NFA], ids=["processor", "nfa"])


def omode(mode):
    return O.MODE_PROCESSOR if mode == N.MODE_PROCESSOR else O.MODE_NFA_PER_KEY


def run_follow(ir, key, cols, mode=N.MODE_NFA, forced=False, topic=None, **kw):
    """one batch through a follow session opened by the flag, or by force_path without it"""
    cp = N.CompiledPattern(ir)
    s = N.Session(cp, max(1, len(key)), mode=mode, follow=not forced, force_path=N.PATH_FOLLOW if forced else 0)
    assert s.path == N.PATH_FOLLOW
    s.push(len(key), np.ascontiguousarray(key, np.int32), [np.ascontiguousarray(c) for c in cols], topic=topic, **kw)
    out = s.collect()
    return product_matches(s, out), s, out


def check(stages, schema, coltype, key, val, topic=None, mode=N.MODE_NFA, min_matches=1, forced=False):
    ir = FL.build(stages).to_ir(schema)
    want = oracle_matches(ir, key, [val], [coltype], omode(mode), topic=topic)
    assert len(want) >= min_matches
    got, s, out = run_follow(ir, key, [val], mode, forced=forced, topic=topic)
    assert out["path"] == N.PATH_FOLLOW
    assert got == want
    return want, s


# ---- 1. random parity: three pattern variants, both modes, both ways onto the path ----
@MODES
@pytest.mark.parametrize("seed", range(40))
def test_random_parity(seed, mode):
    rng = np.random.default_rng(1000 + seed)
    variant = ["plain", "topics", "times"][seed % 3]
    alphabet = int(rng.integers(2, 5))
    stages = FL.random_stages(rng, variant, alphabet, min_next=1)
    key, val, topic = FL.random_stream(rng, int(rng.integers(200, 2001)), 120, alphabet)
    ir = FL.build(stages).to_ir(FL.I32T)
    want = oracle_matches(ir, key, [val], [1], omode(mode), topic=topic)
    assert want == FL.model_matches(stages, key, val, topic)
    for forced in (False, True):
        got, _, out = run_follow(ir, key, [val], mode, forced=forced, topic=topic)
        assert out["path"] == N.PATH_FOLLOW
        assert got == want, (stages, forced)


# ---- 2. boundaries of words, tiles and key segments ----
def sizes():
    t = 4096                                             # (asserted below: the ids must not need the library)
    return sorted({1, 3, 63, 64, 65, 4095, 4097, t - 1, t + 1, 2 * t + 5})


MIXED = [FL.stage("a", False, c=0), FL.stage("b", True, c=1), FL.stage("c", False, c=2), FL.stage("d", True, c=0)]


@pytest.mark.parametrize("n", sizes())
def test_sizes_one_key(n):
    assert N.follow_tile_records() == 4096
    rng = np.random.default_rng(n)
    val = rng.integers(0, 3, n).astype(np.int32)
    check(FL.abc(), FL.I32T, 1, np.zeros(n, np.int32), val, min_matches=1 if n >= 63 else 0)
    check(MIXED, FL.I32T, 1, np.zeros(n, np.int32), val, min_matches=1 if n >= 63 else 0)


@pytest.mark.parametrize("cut", [64, 4096, "T"])
def test_key_changes_at_an_edge(cut):
    t = N.follow_tile_records()
    cut = t if cut == "T" else cut
    n = 2 * t + 5
    rng = np.random.default_rng(cut)
    key = (np.arange(n) >= cut).astype(np.int32)         # the last key runs to n
    val = rng.integers(0, 3, n).astype(np.int32)
    # a strict hop whose next record is the next key's first and satisfies the slot: a(0) b(1) | c(2)
    val[cut - 4:cut + 1] = [3, 3, 0, 1, 2]
    pat = [FL.stage("a", False, c=0), FL.stage("b", True, c=1), FL.stage("c", False, c=2)]
    want, _ = check(pat, FL.I32T, 1, key, val)
    assert not any(m[0] == cut for m in want)
    # a skip-till-next hop whose next set bit lies in the next key: a(0) then no 1 before the cut
    val2 = val.copy()
    val2[cut - 6:cut + 2] = [0, 3, 3, 3, 3, 3, 1, 2]
    want2, _ = check(FL.abc(), FL.I32T, 1, key, val2)
    assert not any(r == cut - 6 for m in want2 for _, r in m[2])
    # the last key's last records complete a walk at n - 1
    val3 = val.copy()
    val3[-3:] = [0, 1, 2]
    want3, _ = check(FL.abc(), FL.I32T, 1, key, val3)
    assert want3[-1][0] == n - 1


# ---- 3. long gaps: the second level of the bitmaps ----
def test_long_gap_one_key():
    n = 300_000
    val = np.full(n, 3, np.int32)
    val[0], val[n - 2], val[n - 1] = 0, 1, 2
    want, _ = check(FL.abc(), FL.I32T, 1, np.zeros(n, np.int32), val)
    assert want == [(n - 1, 0, [("c", n - 1), ("b", n - 2), ("a", 0)])]


def test_long_gap_many_keys():
    nk, L = 50, 6000
    val = np.full((nk, L), 3, np.int32)
    val[:, 0], val[:, L - 2], val[:, L - 1] = 0, 1, 2
    key = np.repeat(np.arange(nk, dtype=np.int32), L)
    want, _ = check(FL.abc(), FL.I32T, 1, key, val.reshape(-1))
    assert len(want) == nk


# ---- 4. many matches on one record: the sort route (span > 1024) and the ranked route ----
@pytest.mark.parametrize("starts", [1500, 900])
def test_many_matches_on_one_record(starts):
    val = np.concatenate([np.zeros(starts, np.int32), np.array([1, 2], np.int32)])
    want, _ = check(FL.abc(), FL.I32T, 1, np.zeros(len(val), np.int32), val)
    assert [m[0] for m in want] == [starts + 1] * starts
    assert [m[2][-1][1] for m in want] == list(range(starts))        # by ascending start


# ---- 5. slots, column types, topics ----
def test_k8_and_k2():
    rng = np.random.default_rng(5)
    key, val, _ = FL.random_stream(rng, 300, 100, 4)
    k8 = dict((a[0], a[2]) for a in FL.ACCEPTED)["k8_via_times"]
    val8 = val.copy()
    val8[100:108] = [0, 1, 1, 1, 2, 2, 2, 3]             # (one match at least)
    key8 = key.copy()
    key8[100:108] = key8[100]
    key8 = np.sort(key8)
    check(k8, FL.I32T, 1, key8, val8)
    check([FL.stage("a", False, c=0), FL.stage("b", True, c=1)], FL.I32T, 1, key, val, min_matches=100)


def test_f64_with_nans():
    rng = np.random.default_rng(6)
    key, _, _ = FL.random_stream(rng, 300, 60, 3)
    val = rng.choice(np.array([np.nan, 0.0, 0.25, 1.0, 1.5, 2.0, -np.inf, np.inf]), len(key))
    pat = [FL.stage("a", False, kind="lt", c=0.5), FL.stage("b", True, kind="ge", c=1.5), FL.stage("c", True, kind="eq", c=1.0)]
    want, _ = check(pat, FL.F64, 3, key, val, min_matches=100)
    assert np.isnan(val).sum() > 100


def test_i64_beyond_int32():
    rng = np.random.default_rng(7)
    key, _, _ = FL.random_stream(rng, 300, 60, 3)
    val = rng.choice(np.array([2 ** 40 + 1, 2 ** 40, -2 ** 40, 5, 2 ** 32 + 5, -2 ** 62], np.int64), len(key))
    pat = [FL.stage("a", False, kind="gt", c=2 ** 40), FL.stage("b", True, kind="le", c=-2 ** 40),
           FL.stage("c", False, kind="eq", c=2 ** 32 + 5)]
    check(pat, FL.I64, 2, key, val, min_matches=20)


def test_topics_and_a_batch_without_topic_column():
    rng = np.random.default_rng(8)
    key, val, topic = FL.random_stream(rng, 400, 80, 3)
    pat = dict((a[0], a[2]) for a in FL.ACCEPTED)["topics"]
    check(pat, FL.I32T, 1, key, val, topic=topic, min_matches=50)
    # no topic column: every record is on topic id 0, so the stage on t1 never holds
    ir = FL.build(pat).to_ir(FL.I32T)
    got, _, out = run_follow(ir, key, [val])
    assert out["path"] == N.PATH_FOLLOW and got == [] == oracle_matches(ir, key, [val], [1], O.MODE_NFA_PER_KEY)


# ---- 6. batches the path does not take, and the session afterwards ----
@functools.lru_cache(maxsize=None)
def small():
    rng = np.random.default_rng(9)
    key, val, _ = FL.random_stream(rng, 120, 60, 3)
    return key, val, FL.build(FL.abc()).to_ir(FL.I32T)


def test_fallback_batches_and_the_next_push():
    key, val, ir = small()
    n = len(key)
    cp = N.CompiledPattern(ir)
    s = N.Session(cp, n, mode=N.MODE_PROCESSOR, follow=True)
    assert s.path == N.PATH_FOLLOW
    valid = (np.arange(n) % 7 != 3).astype(np.uint8)
    s.push(n, key, [val], valid=valid)
    out = s.collect()
    assert out["path"] == N.PATH_GENERAL
    assert product_matches(s, out) == oracle_matches(ir, key, [val], [1], O.MODE_PROCESSOR, valid=valid)
    off = np.arange(n, dtype=np.int64)
    off[5::11] -= 3                                      # re-delivered offsets: the high-water-mark rule drops them
    s.push(n, key, [val], offset=off)
    out = s.collect()
    assert out["path"] == N.PATH_GENERAL
    want = oracle_matches(ir, key, [val], [1], O.MODE_PROCESSOR, offset=off)
    assert product_matches(s, out) == want and len(want) > 0
    clean = oracle_matches(ir, key, [val], [1], O.MODE_PROCESSOR)
    for kw in (dict(), dict(offset=np.arange(n, dtype=np.int64), flags=N.BATCH_OFFSETS_MONOTONE)):
        s.push(n, key, [val], **kw)
        out = s.collect()
        assert out["path"] == N.PATH_FOLLOW and product_matches(s, out) == clean
    assert clean != want


def test_checksum_count_and_second_collect():
    import torch
    key, val, ir = small()
    got, s, out = run_follow(ir, key, [val])
    assert len(got) > 100
    n, h = s.checksum()
    assert n == len(got)
    g = N.Session(N.CompiledPattern(ir), len(key), mode=N.MODE_NFA, force_path=N.PATH_GENERAL)
    g.push(len(key), key, [val])
    assert product_matches(g, g.collect()) == got
    assert g.checksum() == (n, h)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    s.match_count_to(cnt.data_ptr())
    torch.cuda.synchronize()
    assert int(cnt.item()) == n
    again = s.collect()
    for f in ("match_record", "match_key", "ent_off", "ent_name", "ent_record"):
        assert np.array_equal(out[f], again[f])
    assert again["path"] == N.PATH_FOLLOW
    s.push(0, key[:0], [val[:0]])                        # an empty batch
    assert product_matches(s, s.collect()) == [] and s.checksum()[0] == 0


def test_device_resident_input():
    import torch
    key, val, ir = small()
    got, _, _ = run_follow(ir, key, [val])
    s = N.Session(N.CompiledPattern(ir), len(key), mode=N.MODE_NFA, follow=True)
    dk, dv = torch.from_numpy(key).cuda(), torch.from_numpy(val).cuda()
    s.push(len(key), dk.data_ptr(), [dv.data_ptr()], mem=N.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    out = s.collect()
    assert out["path"] == N.PATH_FOLLOW and product_matches(s, out) == got
    assert s.last_kernel_ms() > 0 and s.last_batch_ms() >= s.last_kernel_ms()
    with pytest.raises(N.CepError) as e:                 # the stencil path's alignment rule
        s.push(len(key) - 1, dk.data_ptr() + 4, [dv.data_ptr() + 4], mem=N.MEM_DEVICE)
    assert e.value.code == 11 and "aligned" in str(e.value)


def test_stop_at_error_is_refused():
    key, val, ir = small()
    s = N.Session(N.CompiledPattern(ir), len(key), mode=N.MODE_NFA, follow=True)
    with pytest.raises(N.CepError) as e:
        s.push(len(key), key, [val], flags=N.BATCH_STOP_AT_ERROR)
    assert e.value.code == 12 and "follow" in str(e.value)


def test_carry_session_stays_on_the_general_path():
    rng = np.random.default_rng(10)
    nk, l1, l2 = 40, 30, 25
    ir = FL.build(FL.abc()).to_ir(FL.I32T)
    v1, v2 = rng.integers(0, 3, (nk, l1)).astype(np.int32), rng.integers(0, 3, (nk, l2)).astype(np.int32)
    k1, k2 = np.repeat(np.arange(nk, dtype=np.int32), l1), np.repeat(np.arange(nk, dtype=np.int32), l2)
    s = N.Session(N.CompiledPattern(ir), nk * l1, mode=N.MODE_NFA, carry=True, max_keys=nk, follow=True)
    assert s.path == N.PATH_GENERAL
    got = []
    for k, v in ((k1, v1), (k2, v2)):
        s.push(len(k), k, [np.ascontiguousarray(v.reshape(-1))])
        out = s.collect()
        assert out["path"] == N.PATH_GENERAL
        got += product_matches(s, out)
    # the oracle over every key's whole stream, its records mapped to their stream positions
    whole = np.concatenate([v1, v2], axis=1)
    pos = np.concatenate([np.arange(nk * l1).reshape(nk, l1), nk * l1 + np.arange(nk * l2).reshape(nk, l2)], axis=1).reshape(-1)
    want = oracle_matches(ir, np.repeat(np.arange(nk, dtype=np.int32), l1 + l2), [whole.reshape(-1)], [1], O.MODE_NFA_PER_KEY)
    want = sorted((int(pos[r]), k, [(nm, int(pos[e])) for nm, e in tr]) for r, k, tr in want)
    assert sorted(got) == want and any(m[0] >= nk * l1 > m[2][-1][1] for m in want)
