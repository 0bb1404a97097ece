"""Match placement of the runs path (csrc/runs.hip) at every chunk class and on every route of push_runs:
runs_emit (every span below the chunk), runs_order (the longest span at most 1024) and the radix sort.

The interval driver of runs_intervals_lib chooses the set of (start, end) pairs freely; its closed form
(test_runs_intervals_cpu.py holds it against the oracle) gives match_record, match_key, ent_off, ent_name and
ent_record, which are compared whole and exactly.  Each case asserts from the model that its batch is in the
chunk class and on the route it aims at, and that it holds what it is built to hold."""
import functools

import numpy as np
import pytest

from kcep import native as N
import runs_intervals_lib as RI

pytestmark = pytest.mark.gpu

FIELDS = (("match_record", np.int64), ("match_key", np.int32), ("ent_off", np.int64), ("ent_name", np.int32),
          ("ent_record", np.int64))
WAYS = {"natural": ("0", "1"), "no_emit": ("0", "0"), "radix": ("1", "1")}     # KCEP_RUNS_RADIX, KCEP_RUNS_EMIT


@functools.lru_cache(maxsize=None)
def compiled(name):
    cp = N.CompiledPattern(RI.FORMS[name].build().to_ir(RI.SCHEMA))
    assert cp.info.runs_ok == 1
    return cp


def route(keys, form):
    """where push_runs sends the batch when nothing is forced"""
    span, C = RI.longest_span(keys, form), RI.chunk_of(RI.n_records(keys))
    return "emit" if span < C else "order" if span <= 1024 else "radix"


def run(form, keys, way, monkeypatch):
    """one push on the runs path; every array of the result against the model's"""
    monkeypatch.setenv("KCEP_RUNS_RADIX", WAYS[way][0])
    monkeypatch.setenv("KCEP_RUNS_EMIT", WAYS[way][1])
    cp = compiled(form.name)
    key, lim, idx = RI.columns(keys)
    n = len(key)
    want = RI.expected_csr(keys, form, cp.names)
    assert len(want["match_record"]) > 0
    s = N.Session(cp, n, mode=N.MODE_PROCESSOR, force_path=N.PATH_RUNS)
    try:
        assert s.jit
        s.push(n, key, [lim, idx], flags=N.BATCH_OFFSETS_MONOTONE)
        out = s.collect(raise_on_error=False)
        assert out["path"] == N.PATH_RUNS and out["err"] == 0
        C = RI.chunk_of(n)
        for f, dt in FIELDS:
            got, exp = out[f], want[f]
            assert got.dtype == dt and exp.dtype == dt
            assert got.shape == exp.shape, (f, got.shape, exp.shape)
            if not np.array_equal(got, exp):
                i = int(np.flatnonzero(got != exp)[0])
                m = i if f.startswith("match") or f == "ent_off" else int(np.searchsorted(want["ent_off"], i, "right")) - 1
                m = min(m, len(want["match_record"]) - 1)
                e = int(want["match_record"][m])
                pytest.fail(f"{f}[{i}] = {got[i]}, expected {exp[i]}: match {m} ending on record {e} "
                            f"(chunk {e // C} of {C}, slot {e % C}), entry {i - int(want['ent_off'][m])} of the match; "
                            f"{int(np.sum(got != exp))} elements differ")
        assert s.checksum()[0] == len(want["match_record"])
    finally:
        s.close()
    return want


# ---- small batches: chunk 128 ----
@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("tail", [0, 1, 37])
@pytest.mark.parametrize("form", [RI.THREE, RI.SIX], ids=lambda f: f.name)
def test_scenarios_1_to_6(form, tail, way, monkeypatch):
    """chunk edges, a fat bucket, the onion, a chunk of more than two entry windows, the batch's end and random
    keys in one batch whose every span is below the chunk: runs_emit's"""
    C = 128
    keys, at = RI.small_batch(form, tail)
    n = RI.n_records(keys)
    assert n <= 12_000 and n % C == tail and RI.chunk_of(n) == C
    assert RI.longest_span(keys, form) == C - 1 and route(keys, form) == "emit"
    j, e, k = RI.intervals(keys, form)
    # the bucket: its size, and neighbours on both sides
    fat = e[k == at["fat"]]
    Bf = int(np.bincount(fat - fat.min()).argmax() + fat.min())
    assert Bf % C == 5 and np.sum(fat == Bf) == RI.fat_bucket_size(C, form) == C - form.smin
    assert np.sum(fat == Bf - 1) >= 1 and np.sum(fat == Bf + 1) >= 1
    # the onion is fully reversed
    m = RI.onion_size(C, form)
    assert np.sum(k == at["onion"]) == m and RI.inversions([keys[at["onion"]]], form) == m * (m - 1) // 2
    # a chunk of more than 4096 entries, and a run across a multiple of 2048 of them
    ch, a, b = RI.chunk_entries(keys, form, C)
    w = k == at["windows"]
    assert len(set(ch[w].tolist())) == 1 and b[w].max() > 4096 and np.any(a[w] // 2048 != (b[w] - 1) // 2048)
    # runs ending on a chunk's first and last record, and on the batch's last
    assert np.any(e % C == 0) and np.any(e % C == C - 1) and e[-1] == n - 1 and not np.any(j == n - form.smin)
    assert np.any((e - j == C - 1) & (e % C == 0))         # starts exactly C - 1 before the chunk
    assert np.any(j % C == C - 1)
    run(form, keys, way, monkeypatch)


def _one_key(form, builder, *a):
    return RI.single(builder, 128, form, *a)


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("long", [1024, 1025])
@pytest.mark.parametrize("form", [RI.THREE, RI.SIX], ids=lambda f: f.name)
def test_window_edge(form, long, way, monkeypatch):
    """A run of span 1024 -- the widest runs_order takes -- that 1023 - smin later starts overtake: across four
    workgroups of 256, as the batch's first matches (the window's lo clamps at 0), in its middle and as its last
    (hi clamps at nm).  With span 1025 the batch is the radix sort's."""
    keys = _one_key(form, RI.window_edge, long)
    n = RI.n_records(keys)
    assert n <= 12_000 and RI.chunk_of(n) == 128 and RI.longest_span(keys, form) == long
    assert route(keys, form) == ("order" if long == 1024 else "radix")
    j, e, _ = RI.intervals(keys, form)
    start_rank = np.argsort(np.argsort(j, kind="stable"), kind="stable")      # output place -> place in start order
    moved = np.arange(len(j)) - start_rank
    at = np.flatnonzero(e - j == long)
    assert len(at) == 3 and np.all(moved[at] == RI.window_edge_moves(form)) and RI.window_edge_moves(form) > 3 * 256
    assert start_rank[at[0]] == 0 and at[-1] == len(j) - 1 and start_rank[at[1]] >= 1300
    run(form, keys, way, monkeypatch)


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("form", [RI.THREE, RI.SIX], ids=lambda f: f.name)
def test_group_skip(form, way, monkeypatch):
    """runs_order skips groups of 16 window entries by their latest end: long runs at both ends of a group"""
    keys = _one_key(form, RI.group_skip, np.random.default_rng(8))
    n = RI.n_records(keys)
    assert n <= 12_000 and RI.chunk_of(n) == 128 and route(keys, form) == "order"
    j, e, _ = RI.intervals(keys, form)
    assert len(j) == 4000
    rank = np.argsort(np.argsort(j, kind="stable"), kind="stable")
    long = e - j >= 256
    assert 40 <= np.sum(long) <= 140 and np.all((e - j)[~long] == form.smin)
    assert np.any(rank[long] % 16 == 15) and np.any(rank[long] % 16 == 0)
    run(form, keys, way, monkeypatch)


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("form", [RI.THREE, RI.SIX], ids=lambda f: f.name)
def test_ties_over_a_workgroup_boundary(form, way, monkeypatch):
    """700 runs ending on one record, from starts spread over four workgroups, with 200 short runs among them"""
    keys = _one_key(form, RI.ties, np.random.default_rng(9))
    n = RI.n_records(keys)
    assert n <= 12_000 and RI.chunk_of(n) == 128 and route(keys, form) == "order"
    j, e, _ = RI.intervals(keys, form)
    E = int(e.max())
    assert np.sum(e == E) == 700 and np.sum(e < E) == 200 and np.all((e - j)[e < E] == form.smin)
    assert 128 <= RI.longest_span(keys, form) < 1024
    assert j[e == E].max() - j[e == E].min() > 3 * 256 and np.all(np.diff(j[e == E]) > 0)
    run(form, keys, way, monkeypatch)


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("form", [RI.THREE, RI.SIX], ids=lambda f: f.name)
def test_span_equals_chunk_128(form, way, monkeypatch):
    """the first batch runs_emit refuses: the longest span is the chunk"""
    keys = RI.span_chunk_batch(128, None, form)
    assert RI.chunk_of(RI.n_records(keys)) == 128 and RI.longest_span(keys, form) == 128
    assert route(keys, form) == "order"
    run(form, keys, way, monkeypatch)


# ---- large batches: the smallest n of each chunk class (+ 37), and the first n of chunk 1024 itself ----
LARGE = [(256, RI.CHUNK_FROM[256] + 37, "three", "natural"),
         (512, RI.CHUNK_FROM[512] + 37, "three", "natural"),
         (1024, RI.CHUNK_FROM[1024] + 37, "three", "natural"),
         (1024, RI.CHUNK_FROM[1024] + 37, "six", "natural"),
         (1024, RI.CHUNK_FROM[1024] + 37, "three", "no_emit"),
         (1024, RI.CHUNK_FROM[1024], "three", "natural")]


@pytest.mark.parametrize("C,n,form,way", LARGE, ids=[f"{c}-{n}-{f}-{w}" for c, n, f, w in LARGE])
def test_large_batch(C, n, form, way, monkeypatch):
    """Scenarios 1-6 at the front of the batch and 1 and 5 again in its last three chunks, in the chunk classes
    256, 512 and 1024 (there: 2048 window entries, eight per thread, 11-bit start offsets)."""
    form = RI.FORMS[form]
    keys, at = RI.large_batch(C, n, form)
    assert RI.n_records(keys) == n and RI.chunk_of(n) == C and n - RI.CHUNK_FROM[C] in (0, 37)
    assert RI.chunk_of(RI.CHUNK_FROM[C] - 1) == C // 2
    assert RI.longest_span(keys, form) == C - 1 and route(keys, form) == "emit"
    j, e, k = RI.intervals(keys, form)
    assert 0 < len(j) < 20_000 and int(np.sum(e - j + 1)) < 3_000_000
    fat = e[k == at["fat"]]
    assert np.bincount(fat - fat.min()).max() == RI.fat_bucket_size(C, form) == min(C - form.smin, 300)
    m = RI.onion_size(C, form)
    assert np.sum(k == at["onion"]) == m and RI.inversions([keys[at["onion"]]], form) == m * (m - 1) // 2
    ch, a, b = RI.chunk_entries(keys, form, C)
    w = k == at["windows"]
    assert len(set(ch[w].tolist())) == 1 and b[w].max() > 4096 and np.any(a[w] // 2048 != (b[w] - 1) // 2048)
    tail = k >= at["tail_edges"]
    assert np.sum(tail) >= 9 and j[tail].min() >= n - 3 * C - form.smin - 4 and e[-1] == n - 1
    assert np.any(e[tail] % C == 0) and np.any(e[tail] % C == C - 1) and np.any((e - j)[tail] == C - 1)
    run(form, keys, way, monkeypatch)


@pytest.mark.parametrize("C", [256, 512, 1024])
def test_large_span_equals_chunk(C, monkeypatch):
    """the longest span exactly the chunk, in each class: runs_order's"""
    n = RI.CHUNK_FROM[C] + 37
    keys = RI.span_chunk_batch(C, n, RI.THREE)
    assert RI.chunk_of(n) == C and RI.longest_span(keys, RI.THREE) == C and route(keys, RI.THREE) == "order"
    run(RI.THREE, keys, "natural", monkeypatch)
