"""The plain stencil path's finish step for 1024 < super-tiles <= 8192 (csrc/stencil.hip): one launch,
stencil_finish_dense, sums the 16-bit super-tile counts and writes the rows; KCEP_STENCIL_SPLIT_FINISH=1
selects the two launches it replaced (tile_scan + stencil_gather_dense).  The step decides where every
match lands, so every test compares the ordered CSR of collect() -- match_record, match_key, ent_off,
ent_name, ent_record -- with oracle.baseline_csr element by element, with the switch off and on, and the
two CSRs with each other.  The shapes are the smallest that reach the step: batches grouped by key,
int32 values."""
import os

import numpy as np
import pytest

import oracle as O
from kcep import native as N
from kcep import synth, Schema, QueryBuilder, Event

pytestmark = pytest.mark.gpu

I32 = Schema([("value", "i32")])
FIELDS = ("match_record", "match_key", "ent_off", "ent_name", "ent_record")
TILE = 4096
ST_DENSE = 512                         # csrc/kcep_internal.h: a super-tile's first matches lie in the dense region
FIRST_ROUND = 5 * 64                   # csrc/stencil.hip FIN_B x 64: slot words a wave loads before it knows the count
THREADS = min(16, os.cpu_count() or 1)

N_FIRST = 1025 * TILE - 7              # sub = 1, 1025 super-tiles: the first size past SMALL_FINISH; 1025 is no
                                       # multiple of the super-tiles per workgroup, the last tile is partial


def c2_ir():
    return synth.c2_pattern().to_ir(I32)


def nine_ir():
    """C2 with value 9 accepted at every stage (test_stencil_sparse_gpu.test_half_dense_half_selective)."""
    q = QueryBuilder().select("A").where((Event.value() == 0) | (Event.value() == 9))
    q = q.then().select("B").where((Event.value() == 1) | (Event.value() == 9))
    q = q.then().select("C").where((Event.value() == 2) | (Event.value() == 9))
    return q.build().to_ir(I32)


def k_stage_ir(k):
    """test_stencil_gpu.test_k_stages' pattern."""
    q = QueryBuilder().select("s0").where(Event.value() <= (0 if k > 1 else 1))
    for s in range(1, k):
        q = q.then().select(f"s{s}").where((Event.value() == s % 3) | (Event.value() == 2))
    return q.build().to_ir(I32)


def want_csr(ir, key, val):
    return O.baseline_csr(O.OraclePattern(ir), O.BatchArrays(key, [val], [1]), O.MODE_PROCESSOR, THREADS)


def same(got, want, what):
    for f in FIELDS:
        assert got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f]), (what, f, np.flatnonzero(got[f] != want[f])[:5])


def both_ways(monkeypatch, ir, n, push, want):
    """The batch through the one-launch finish and through the two launches: each against the oracle's
    CSR, and against each other."""
    monkeypatch.setenv("KCEP_STENCIL_KEYED", "0")
    monkeypatch.setenv("KCEP_STENCIL_SPARSE_KEYS", "0")
    monkeypatch.setenv("KCEP_STENCIL_DENSE_KEYS", "0")
    outs = []
    for split in ("0", "1"):
        monkeypatch.setenv("KCEP_STENCIL_SPLIT_FINISH", split)
        s = N.Session(N.CompiledPattern(ir), n)
        assert s.path == N.PATH_STENCIL
        push(s)
        outs.append(s.collect())
        same(outs[-1], want, "split" if split == "1" else "fused")
        del s
    same(outs[0], outs[1], "fused against split")
    return outs[0]


def tile_counts(want, n, per):
    """matches per super-tile of ``per`` records: a match belongs to its completing record's super-tile"""
    return np.bincount(np.asarray(want["match_record"]) // per, minlength=(n + per - 1) // per)


def test_first_size_past_small_finish(monkeypatch):
    n = N_FIRST
    key, val, _ = synth.c2_stream_np(n, 40_000)
    want = want_csr(c2_ir(), key, val)
    cnt = tile_counts(want, n, TILE)
    assert len(cnt) == 1025 and 0 < cnt.max() < FIRST_ROUND and len(want["match_record"]) > 50_000
    both_ways(monkeypatch, c2_ir(), n, lambda s: s.push(n, key, [val]), want)


def test_full_empty_and_ordinary_stretches(monkeypatch):
    """Tiles 0-39: value 9 throughout, every record a candidate -- counts far past the first load round
    and past ST_DENSE, so the remainder loop reads the dense region's end and the super-tile's own region.
    Tiles 40-700: a value no stage accepts -- runs of super-tiles without a match.  The rest: C2 values."""
    n = 1031 * TILE + 5
    _, val, _ = synth.c2_stream_np(n, 40_000)
    val = val.copy()
    val[:40 * TILE] = 9
    val[40 * TILE:701 * TILE] = 7
    key = (np.arange(n) // 37).astype(np.int32)
    want = want_csr(nine_ir(), key, val)
    cnt = tile_counts(want, n, TILE)
    assert len(cnt) == 1032
    assert cnt[:40].min() > 3 * ST_DENSE
    assert cnt[40:701].max() == 0
    assert cnt[701:1031].min() > 0 and cnt[701:].max() < FIRST_ROUND
    both_ways(monkeypatch, nine_ir(), n, lambda s: s.push(n, key, [val]), want)


def test_nearly_full_super_tiles_four_tiles_per_workgroup(monkeypatch):
    """8193 tiles, sub = 4, 2049 super-tiles of 16384 records: super-tiles 5-7 hold the always-accepted value
    with keys in runs of 37, so their counts come close to the 16-bit count's bound of 16384.  The full CSR
    is compared (all five arrays)."""
    import torch
    n = 8192 * TILE + 1000
    per = 4 * TILE
    dk, dv, order = synth.c2_stream_torch(n, 1_000_000, "cuda")
    del order
    key, val = dk.cpu().numpy(), dv.cpu().numpy()
    a, b = 5 * per, 8 * per
    val[a:b] = 9
    key[a:b] = key[a] + np.arange(b - a, dtype=np.int32) // 37   # (fewer keys than the stretch had: still grouped)
    assert key[b - 1] <= key[b]
    dk, dv = torch.from_numpy(key).cuda(), torch.from_numpy(val).cuda()
    want = want_csr(nine_ir(), key, val)
    cnt = tile_counts(want, n, per)
    assert len(cnt) == 2049 and cnt[5:8].min() > 15_000 and cnt.max() <= per
    assert cnt[8:2048].min() > 0 and np.delete(cnt, [5, 6, 7]).max() < ST_DENSE
    stream = torch.cuda.current_stream().cuda_stream

    def push(s):
        s.push(n, dk.data_ptr(), [dv.data_ptr()], mem=N.MEM_DEVICE, stream=stream)

    both_ways(monkeypatch, nine_ir(), n, push, want)
    del dk, dv
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k", [1, 7])
def test_k_stages_first_size(k, monkeypatch):
    """k = 1: two records in three match, every super-tile past ST_DENSE; k = 7: seven-int rows."""
    n = N_FIRST
    rng = np.random.default_rng(k)
    key = np.sort(rng.integers(0, 40_000, n)).astype(np.int32)
    val = rng.integers(0, 3, n).astype(np.int32)
    ir = k_stage_ir(k)
    want = want_csr(ir, key, val)
    assert len(want["match_record"]) > 20_000
    got = both_ways(monkeypatch, ir, n, lambda s: s.push(n, key, [val]), want)
    assert len(got["ent_record"]) == k * len(got["match_record"])
