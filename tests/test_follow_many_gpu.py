"""The follow path with oneOrMore stages on the device (CEP_SESSION_FOLLOW_MANY, csrc/follow.hip "oneOrMore
slots"): variable-length matches from walks over per-slot bitmaps.  Every test compares the session's collected
CSR with the CPU oracle, element for element and in order, and the path, the device match count and the checksum
with a general-path session of the same batch."""
import functools

import numpy as np
import pytest

import oracle as O
from kcep import native as N
from gpu_util import oracle_matches, product_matches
import follow_many_lib as FM

pytestmark = pytest.mark.gpu

TILE, WORD = 4096, 64                                    # (asserted in test_tile: the ids must not need the library)


def omode(mode):
    return O.MODE_PROCESSOR if mode == N.MODE_PROCESSOR else O.MODE_NFA_PER_KEY


def device_count(s):
    import torch
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    s.match_count_to(cnt.data_ptr())
    torch.cuda.synchronize()
    return int(cnt.item())


def check(ir, key, cols, coltypes, want, mode=N.MODE_NFA, topic=None, mask_pass=False, device=False, interpret=False):
    """one batch through a follow-many session and through a general session; want: the oracle's matches"""
    import torch
    n = len(key)
    key = np.ascontiguousarray(key, np.int32)
    cols = [np.ascontiguousarray(c) for c in cols]
    cp = N.CompiledPattern(ir)
    s = N.Session(cp, max(1, n), mode=mode, follow_many=True, mask_pass=mask_pass, interpret=interpret)
    assert s.path == N.PATH_FOLLOW
    if device:
        dk, dc = torch.from_numpy(key).cuda(), [torch.from_numpy(c).cuda() for c in cols]
        dt = None if topic is None else torch.from_numpy(np.ascontiguousarray(topic, np.int32)).cuda()
        s.push(n, dk.data_ptr(), [c.data_ptr() for c in dc], topic=None if dt is None else dt.data_ptr(), mem=N.MEM_DEVICE,
               stream=torch.cuda.current_stream().cuda_stream)
    else:
        s.push(n, key, cols, topic=topic)
    out = s.collect()
    assert out["path"] == N.PATH_FOLLOW
    got = product_matches(s, out)
    assert len(got) == len(want)
    assert got == want
    assert device_count(s) == len(want)
    g = N.Session(cp, max(1, n), mode=mode, force_path=N.PATH_GENERAL, interpret=True)
    g.push(n, key, cols, topic=topic)
    gout = g.collect()
    assert gout["path"] == N.PATH_GENERAL and product_matches(g, gout) == want
    assert s.checksum() == g.checksum() and s.checksum()[0] == len(want)
    return s, out


def check_stages(stages, key, val, topic=None, mode=N.MODE_NFA, min_matches=1, **kw):
    ir = FM.build(stages).to_ir(FM.I32T)
    want = oracle_matches(ir, key, [val], [1], omode(mode), topic=topic)
    assert want == FM.model_matches(stages, key, val, topic)
    assert len(want) >= min_matches
    check(ir, key, [val], [1], want, mode=mode, topic=topic, **kw)
    return want


def test_tile():
    assert N.follow_tile_records() == TILE


# ---- 1. random parity: 300 cases of the CPU test's variants, n <= 200, both modes ----
@pytest.mark.parametrize("variant", ["plain", "topics", "times", "strict"])
def test_random_parity(variant):
    rng = np.random.default_rng({"plain": 31, "topics": 32, "times": 33, "strict": 34}[variant])
    total = longer = 0
    for case in range(75):
        alphabet = int(rng.integers(2, 5))
        stages = FM.random_stages(rng, variant, alphabet)
        key, val, topic = FM.random_stream(rng, int(rng.integers(1, 5)), 50, alphabet)
        assert len(key) <= 200
        mode = [N.MODE_PROCESSOR, N.MODE_NFA][case & 1]
        want = check_stages(stages, key, val, topic, mode=mode, min_matches=0, device=bool(case % 3 == 0))
        total += len(want)
        longer += sum(len(m[2]) > FM.n_slots(stages) for m in want)
    assert total > 75 and 3 * longer >= total


# ---- 2. one key of three tiles + 17 records ----
N3 = 3 * TILE + 17


def test_stretches_across_words_and_tiles_and_a_long_gap():
    val = np.full(N3, 3, np.int32)
    val[20:23] = [0, 1, 2]                               # L = K: nothing collected
    val[60], val[61:71], val[71] = 0, 1, 2               # collected records across a word boundary
    val[TILE - 6], val[TILE - 5:TILE + 5], val[TILE + 9] = 0, 1, 2          # ... across a tile boundary
    # a gap longer than a tile before c, with one more b inside it and a whole tile without any
    val[TILE + 104], val[TILE + 105], val[TILE + 2000], val[N3 - 5] = 0, 1, 1, 2
    want = check_stages(FM.abc(), np.zeros(N3, np.int32), val, min_matches=4)
    by_start = {m[2][-1][1]: m for m in want}
    assert len(by_start[20][2]) == 3 and len(by_start[60][2]) == 12 and len(by_start[TILE - 6][2]) == 12
    assert [r for _, r in by_start[TILE + 104][2]] == [N3 - 5, TILE + 2000, TILE + 105, TILE + 104]
    assert by_start[TILE + 104][0] - (TILE + 105) > TILE + 64 * WORD // 2      # (tile 2 lies inside the gap, without a b)


@pytest.mark.parametrize("after", ["c", "neither"])
def test_all_b_stretch_strict_strict(after):
    """more than 64 words of B under strict B+ / strict C: the first record that is not B completes the walk if
    it is C and kills it if it is neither; a match of K entries in the same batch"""
    stretch = 64 * WORD + 100
    val = np.full(N3, 4, np.int32)                       # (4: no stage's constant)
    val[10], val[11:11 + stretch], val[11 + stretch] = 0, 1, 2 if after == "c" else 4
    val[11 + stretch + 50] = 3
    short = 2 * TILE + 1000
    val[short:short + 4] = [0, 1, 2, 3]
    want = check_stages(FM.strict_pair(), np.zeros(N3, np.int32), val)
    lens = sorted(len(m[2]) for m in want)
    assert lens == ([4, 4 + stretch - 1] if after == "c" else [4])
    assert stretch - 1 > 1024


# ---- 3. key segments ----
@pytest.mark.parametrize("nxt", [(True, True), (False, True), (True, False)], ids=["next_next", "strict_next", "next_strict"])
def test_walk_open_at_a_key_boundary_inside_a_word(nxt):
    key = np.repeat(np.arange(2, dtype=np.int32), 100)   # the boundary: record 100, bit 36 of word 1
    val = np.full(200, 3, np.int32)
    val[90], val[91:100] = 0, 1                          # key 0 ends inside the stretch: no c
    val[100:106], val[106] = 1, 2                        # key 1 goes on with b ... c: not key 0's
    val[110:114] = [0, 1, 1, 2]
    want = check_stages(FM.abc(nxt), key, val)
    assert [(m[0], m[1], [r for _, r in m[2]]) for m in want] == [(113, 1, [113, 112, 111, 110])]


@pytest.mark.parametrize("nxt", [(True, True), (False, True), (True, False)], ids=["next_next", "strict_next", "next_strict"])
def test_several_keys_per_word(nxt):
    rng = np.random.default_rng(41)
    n = 3000
    key = (np.arange(n) // 20).astype(np.int32)          # three or four keys in every word
    val = rng.integers(0, 3, n).astype(np.int32)
    val[63:68] = [0, 1, 1, 1, 2]                         # a start in the last bit of a word (key 3: records 60..79)
    want = check_stages(FM.abc(nxt), key, val, min_matches=100)
    assert any(m[2][-1][1] == 63 and len(m[2]) == 5 for m in want)


# ---- 4. the evaluated form: two columns, CEP_SESSION_MASK_PASS ----
@pytest.mark.parametrize("interpret", [False, True], ids=["compiled", "interpreted"])
def test_evaluated_form_two_columns(interpret):
    rng = np.random.default_rng(42)
    key, x, _ = FM.random_stream(rng, 40, 120, 3)
    y = rng.integers(0, 2, len(key)).astype(np.int32)
    ir = FM.two_column_pattern().to_ir(FM.TWO)
    want = oracle_matches(ir, key, [x, y], [1, 1], O.MODE_NFA_PER_KEY)
    assert want == FM.model_from_hits(FM.TWO_STAGES, key, FM.two_column_hits(x, y))
    assert len(want) > 100 and any(len(m[2]) > 3 for m in want)
    s, _ = check(ir, key, [x, y], [1, 1], want, mask_pass=True, interpret=interpret)
    assert s.jit == (not interpret)
    # without CEP_SESSION_MASK_PASS the pattern stays where it was
    g = N.Session(N.CompiledPattern(ir), len(key), mode=N.MODE_NFA, follow_many=True)
    assert g.path == N.PATH_GENERAL


# ---- 5. the session around the batches ----
@functools.lru_cache(maxsize=None)
def small():
    rng = np.random.default_rng(43)
    key, val, _ = FM.random_stream(rng, 120, 60, 3)
    ir = FM.build(FM.abc()).to_ir(FM.I32T)
    return key, val, ir, oracle_matches(ir, key, [val], [1], O.MODE_NFA_PER_KEY)


def test_device_resident_input_and_second_collect():
    key, val, ir, want = small()
    assert len(want) > 100
    s, out = check(ir, key, [val], [1], want, device=True)
    again = s.collect()
    for f in ("match_record", "match_key", "ent_off", "ent_name", "ent_record"):
        assert np.array_equal(out[f], again[f])
    assert s.last_kernel_ms() > 0 and s.last_batch_ms() >= s.last_kernel_ms()
    s.push(0, key[:0], [val[:0]])                        # an empty batch
    assert product_matches(s, s.collect()) == [] and s.checksum()[0] == 0 and device_count(s) == 0
    s.push(len(key), key, [val])                         # and the session afterwards
    assert product_matches(s, s.collect()) == want


def test_fallback_batch_and_the_next_push():
    key, val, ir, want = small()
    n = len(key)
    s = N.Session(N.CompiledPattern(ir), n, mode=N.MODE_PROCESSOR, follow_many=True)
    assert s.path == N.PATH_FOLLOW
    valid = (np.arange(n) % 7 != 3).astype(np.uint8)
    s.push(n, key, [val], valid=valid)
    out = s.collect()
    assert out["path"] == N.PATH_GENERAL
    assert product_matches(s, out) == oracle_matches(ir, key, [val], [1], O.MODE_PROCESSOR, valid=valid)
    s.push(n, key, [val])
    out = s.collect()
    assert out["path"] == N.PATH_FOLLOW and product_matches(s, out) == oracle_matches(ir, key, [val], [1], O.MODE_PROCESSOR)


def test_flag_does_nothing_elsewhere():
    key, val, ir, want = small()
    # a carry session stays on the general path
    s = N.Session(N.CompiledPattern(ir), len(key), mode=N.MODE_NFA, carry=True, max_keys=int(key.max()) + 1, follow_many=True)
    assert s.path == N.PATH_GENERAL
    # a pattern without a oneOrMore stage opens as with CEP_SESSION_FOLLOW, fixed-length rows and all
    import follow_lib as FL
    fir = FL.build(FL.abc()).to_ir(FL.I32T)
    f = N.Session(N.CompiledPattern(fir), len(key), mode=N.MODE_NFA, follow_many=True)
    assert f.path == N.PATH_FOLLOW                       # (the flag implies CEP_SESSION_FOLLOW)
    f.push(len(key), key, [val])
    out = f.collect()
    fwant = oracle_matches(fir, key, [val], [1], O.MODE_NFA_PER_KEY)
    assert out["path"] == N.PATH_FOLLOW and product_matches(f, out) == fwant and len(fwant) > 100
    assert np.all(np.diff(out["ent_off"]) == 3)
