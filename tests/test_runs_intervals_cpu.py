"""The interval driver of the runs-path placement tests (runs_intervals_lib) without a GPU: both forms of the
pattern are runs-path patterns, the closed form equals the CPU oracle on every scenario at chunk 128 and on 200
seeded random interval sets in both modes, and the numpy-built CSR unpacks to the closed form's list."""
import numpy as np
import pytest

import oracle as O
from kcep import native as N
from gpu_util import oracle_matches
import runs_intervals_lib as RI

FORMS = [RI.THREE, RI.SIX]
C = 128


def _ir(form):
    return form.build().to_ir(RI.SCHEMA)


def _oracle(form, keys, mode):
    key, lim, idx = RI.columns(keys)
    return oracle_matches(_ir(form), key, [lim, idx], RI.COLTYPES, mode)


def _names(form):
    return N.CompiledPattern(_ir(form)).names


def _check(form, keys, modes):
    want = RI.model(keys, form)
    for mode in modes:
        assert _oracle(form, keys, mode) == want
    assert RI.unpack(RI.expected_csr(keys, form, _names(form)), _names(form)) == want
    return want


BOTH = (O.MODE_PROCESSOR, O.MODE_NFA_PER_KEY)


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f.name)
def test_runs_ok(form):
    cp = N.CompiledPattern(_ir(form))
    assert cp.info.runs_ok == 1
    assert set(("first", "mid", "last") + form.pre) <= set(cp.names)


def _scenarios(form):
    rng = np.random.default_rng(7)
    return {
        "chunk_edges": RI.single(RI.chunk_edges, C, form),
        "fat_bucket": RI.single(RI.fat_bucket, C, form),
        "onion": RI.single(RI.onion, C, form),
        "entry_windows": RI.single(RI.entry_windows, C, form),
        "batch_end": RI.single(RI.batch_end, C, form, C + 40),
        "random": RI.single(RI.random_key, C, form, rng, 3 * C),
        "window_edge": RI.single(RI.window_edge, C, form),
        "window_edge_1025": RI.single(RI.window_edge, C, form, 1025),
        "group_skip": RI.single(RI.group_skip, C, form, rng),
        "ties": RI.single(RI.ties, C, form, rng),
        "span_equals_chunk": RI.span_chunk_batch(C, None, form),
    }


SCENARIOS = list(_scenarios(RI.THREE))


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f.name)
@pytest.mark.parametrize("name", SCENARIOS)
def test_scenario_equals_oracle(name, form):
    """every scenario as one key (so MODE_NFA sees what MODE_PROCESSOR sees), and what each is built to hold"""
    keys = _scenarios(form)[name]
    want = _check(form, keys, BOTH)
    assert len(want) > 0
    if name == "fat_bucket":
        B = RI.boundary(C, 0, C + 48)
        assert sum(m[0] == B + 5 for m in want) == RI.fat_bucket_size(C, form) == C - form.smin
        assert sum(m[0] == B + 4 for m in want) >= 1 and sum(m[0] == B + 6 for m in want) >= 1
    if name == "onion":
        m = RI.onion_size(C, form)
        assert len(want) == m and RI.inversions(keys, form) == m * (m - 1) // 2
    if name == "entry_windows":
        ch, a, b = RI.chunk_entries(keys, form, C)
        assert len(set(ch.tolist())) == 1 and b.max() > 4096 and np.any(a // 2048 != (b - 1) // 2048)
    if name.startswith("window_edge"):
        assert RI.longest_span(keys, form) == (1025 if name.endswith("1025") else 1024)


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f.name)
@pytest.mark.parametrize("tail", [0, 1, 37])
def test_small_batch_equals_oracle(tail, form):
    """scenarios 1-6 packed into one batch of several keys, as the GPU test pushes them"""
    keys, at = RI.small_batch(form, tail)
    assert RI.n_records(keys) % C == tail and RI.chunk_of(RI.n_records(keys)) == C
    want = _check(form, keys, (O.MODE_PROCESSOR,))
    n = RI.n_records(keys)
    assert want[-1][0] == n - 1 and RI.longest_span(keys, form) == C - 1


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f.name)
def test_random_interval_sets(form):
    """200 seeded sets of up to 3000 records: several keys in MODE_PROCESSOR, one key in MODE_NFA"""
    rng = np.random.default_rng(100 + form.smin)
    total = opened = 0
    for case in range(200):
        nfa = case % 2 == 1
        n = int(min(3000, 20 * 2 ** (rng.random() * 7.3)))
        nkeys = 1 if nfa else int(rng.integers(1, 6))
        cuts = np.sort(rng.choice(np.arange(1, n), nkeys - 1, replace=False)) if nkeys > 1 else np.zeros(0, np.int64)
        lens = np.diff(np.concatenate([[0], cuts, [n]])).astype(int)
        smax = int(rng.choice([8, 40, 300, 1100]))
        keys = []
        for kid, ln in enumerate(lens.tolist()):
            runs = {int(o): int(rng.integers(1, smax + 1)) for o in np.flatnonzero(rng.random(ln) < 0.15)}
            keys.append((kid, ln, runs))
        want = RI.model(keys, form)
        got = _oracle(form, keys, O.MODE_NFA_PER_KEY if nfa else O.MODE_PROCESSOR)
        assert got == want, (case, keys)
        total += len(want)
        opened += sum(len(k[2]) for k in keys)
    assert total > 2000 and opened > total                 # matches, and starts that die or stay open
    print(form.name, "starts", opened, "matches", total)


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f.name)
def test_negative_cases(form):
    """Spans too short for mid, and ends around a key's last record, in the middle of a batch and at its end:
    on the last record a match, one past it an open run, none on the next key's first record."""
    s = form.smin
    seglen = 40

    def seg(kid):
        runs = {0: s - 1,                                  # dies: mid needs a record
                2: 1,                                      # span 1
                10: seglen - 1 - 10,                       # ends on the key's last record: a match
                11: seglen - 11,                           # would end on the next key's first record / past the batch
                12: seglen - 12 + 3,                       # would end inside the next key
                seglen - 1 - s: s,                         # shortest run onto the last record: a match
                seglen - s: s,                             # open by one record
                20: s}                                     # (a plain match)
        return (kid, seglen, runs)

    keys = [seg(0), seg(1), seg(2)]
    want = _check(form, keys, (O.MODE_PROCESSOR,))
    for kid in range(3):
        base = kid * seglen
        mine = [(m[0] - base, m[0] - base - (len(m[2]) - 1)) for m in want if m[1] == kid]    # (end, start) offsets
        assert mine == [(20 + s, 20), (seglen - 1, 10), (seglen - 1, seglen - 1 - s)]
    # one key, both modes: the same cases at the batch's end only
    want1 = _check(form, [seg(0)], BOTH)
    assert len(want1) == 3
