"""The general path's segment, scan and compaction kernels (csrc/scan.hip, csrc/nfa.hip) at the sizes
where their 1024-element block (256 threads x 4) and the scans' 64-lane waves begin and end.

A batch of S key segments of two records each, S around 256, 1024 and 2048, so that the segment count
crosses the 256- and 1024-wide steps and the record count n = 2 S crosses 2048 and 4096.  The pattern is
two strict stages on the record's value, the values are drawn from a fixed seed: about a quarter of the
keys match, so the per-segment match and entry counts that exclusive_scan_pair scans are neither all
zero nor all equal.  Matches, keys and traversals are compared exactly with the oracle, on the wave and
on the lane kernel."""
import functools

import numpy as np
import pytest

import oracle as O
from kcep import native as N, QueryBuilder, Event
from gpu_util import oracle_matches, product_matches
import patterns_lib as PL

pytestmark = pytest.mark.gpu

SEGMENTS = [1, 255, 256, 257, 1023, 1024, 1025, 2049]


@functools.lru_cache(maxsize=None)
def batch(S):
    """(ir, key, value, the oracle's matches) of the S-segment batch; computed once, read by both kernels"""
    rng = np.random.default_rng(20261020 + S)
    key = np.repeat(np.arange(S, dtype=np.int32), 2)
    val = rng.integers(0, 2, 2 * S).astype(np.int32)
    ir = (QueryBuilder().select("first").where(Event.value() == 0).then()
          .select("second").where(Event.value() == 1).build()).to_ir(PL.I32)
    return ir, key, val, oracle_matches(ir, key, [val], [1], O.MODE_PROCESSOR)


@pytest.mark.parametrize("S", SEGMENTS)
@pytest.mark.parametrize("lane_nfa", [False, True], ids=["wave", "lane"])
def test_two_record_segments(lane_nfa, S):
    ir, key, val, want = batch(S)
    if S > 1:
        assert 0 < len(want) < S                   # some keys match, some do not
    s = N.Session(N.CompiledPattern(ir), len(key), force_path=N.PATH_GENERAL, interpret=True, lane_nfa=lane_nfa)
    assert s.path == N.PATH_GENERAL and s.wave == (not lane_nfa)
    s.push(len(key), key, [val])
    assert product_matches(s, s.collect()) == want
