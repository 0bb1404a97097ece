"""Carry sessions whose pools change owner mid-stream: the general path's carried-state pool moved into a
fresh buffer (carry_gc) and the runs path's tail pool swapped for a larger one (tail_reserve) while it holds
live tails.  Both streams are compared with the oracle's run over the whole stream, as in test_carry_gpu.py."""
import numpy as np
import pytest

import oracle as O
from kcep import native as N
import patterns_lib as PL
from test_carry_gpu import oracle_run, run_carry

pytestmark = pytest.mark.gpu


def test_general_carry_pool_compacted_before_an_attempt():
    """The carried-state pool of a general-path session is compacted into a fresh buffer (carry_gc) when a
    batch's keys may not fit behind the blobs it holds: cpool_used + 64 * segments > cpool_words, with
    cpool_words = max(2^20, 64 * max_keys).  16384 keys of one record each fill that bound exactly, so the
    first batch runs without it (cpool_used is 0) and the second one -- every key now carries a partial
    run -- compacts before its first attempt.  Both batches match the oracle over the whole stream."""
    from kcep import QueryBuilder, Event
    nk = 16384
    ir = (QueryBuilder().select("first").where(Event.value() >= 0).then()
          .select("second").where(Event.value() == 1).build()).to_ir(PL.I32)
    key = np.tile(np.arange(nk, dtype=np.int32), 2)
    val = np.concatenate([np.zeros(nk, np.int32), (np.arange(nk) % 2).astype(np.int32)])
    _, r1, _ = oracle_run(ir, key[:nk], [val[:nk]], [1], O.MODE_PROCESSOR)
    assert all(r1.state(k) == (2, 2) for k in (0, 1, nk // 2, nk - 1))   # a partial run and the begin run
    want, r, oerr = oracle_run(ir, key, [val], [1], O.MODE_PROCESSOR)
    s = N.Session(N.CompiledPattern(ir), nk, carry=True, max_keys=nk, force_path=N.PATH_GENERAL)
    assert s.path == N.PATH_GENERAL
    got, _, gerr = run_carry(ir, key, [val], [0, nk, 2 * nk], sess=s)
    assert oerr is None and gerr is None
    assert len(want) == nk // 2 and got == want
    for k in (0, 1, nk // 2, nk - 1):
        assert s.key_state(k) == r.state(k), k


def test_runs_carry_tail_pool_compacted_with_live_tails():
    """The tail pool of a runs carry session is compacted into a larger buffer (tail_reserve) when the
    batch's bound does not fit: rpool_used + (batch + rpool_used) > rpool_cap, which starts at
    max(2 * max_events, 65536) = 80000 records here.  Every key opens one run with its first record
    (v > 0) and keeps it open with zeros (avg >= 0; a zero starts no run), so its tail is all its records:
    24000 after the first batch, and the second one (33600 records: 2 * 24000 + 33600 > 80000) compacts
    the pool while those tails are live, as does the third, whose last records (avg < 1000) complete
    every key's run over 2402 records."""
    ir = PL.c3_stock().to_ir(PL.I32)
    nk = 24

    def batch(per_key, first, last):
        v = np.zeros((nk, per_key), np.int32)
        v[:, 0], v[:, -1] = first, last
        return np.repeat(np.arange(nk, dtype=np.int32), per_key), v.reshape(-1)

    parts = [batch(1000, 100, 0), batch(1400, 0, 0), batch(2, 0, 1000)]
    key, val = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    bounds = [int(x) for x in np.cumsum([0] + [len(p[0]) for p in parts])]
    want, _, oerr = oracle_run(ir, key, [val], [1], O.MODE_PROCESSOR)
    s = N.Session(N.CompiledPattern(ir), 40000, carry=True, max_keys=nk)
    assert s.path == N.PATH_RUNS
    got, _, gerr = run_carry(ir, key, [val], bounds[:2], sess=s)
    assert gerr is None and got == []
    assert len(N.state_positions(s.state_export())) == 24000            # > 20000 tail records stay open
    got, _, gerr = run_carry(ir, key[bounds[1]:], [val[bounds[1]:]], [b - bounds[1] for b in bounds[1:]], sess=s)
    assert oerr is None and gerr is None
    assert len(want) == nk and all(len(m[2]) == 2402 for m in want)
    assert got == want
