"""CEP_BATCH_STOP_AT_ERROR over the random patterns of tests/fuzz_patterns.py (the default 12 `mixed`
seeds, key-grouped, the general path forced, lane and wave engine): with the flag the collected result,
untrimmed, is the oracle's matches below its error record and the error list is the oracle's single
error; on a seed that raises nothing it is the flag-off result."""
import numpy as np
import pytest

import oracle as O
from kcep import native as N
import fuzz_patterns as F
import patterns_lib as PL

pytestmark = pytest.mark.gpu

SEEDS = range(12)
STOP = N.BATCH_STOP_AT_ERROR if hasattr(N, "BATCH_STOP_AT_ERROR") else 8


def _oracle(ir, mode, key, val, ts):
    p = O.OraclePattern(ir)
    r = O.OracleRun(p, mode)
    err = None
    try:
        r.process(O.BatchArrays(key, [val], [1], ts=ts))
    except O.OracleError as e:
        err = (e.code, e.record)
    return [(m.record, m.key, [(p.names[nm], ev) for nm, ev in m.traversal]) for m in r.matches(with_groups=False)], err


def _device(cp, gmode, key, val, ts, lane, flags):
    s = N.Session(cp, len(key), mode=gmode, force_path=N.PATH_GENERAL, interpret=True, lane_nfa=lane)
    s.push(len(key), key, [val], ts=ts, flags=flags)
    out = s.collect(raise_on_error=False)
    got = []
    for m in range(len(out["match_record"])):
        a, b = out["ent_off"][m], out["ent_off"][m + 1]
        got.append((int(out["match_record"][m]), int(out["match_key"][m]),
                    [(cp.names[out["ent_name"][i]], int(out["ent_record"][i])) for i in range(a, b)]))
    rec, code = s.batch_errors()
    return got, list(zip(code.tolist(), rec.tolist())), s.checksum()


@pytest.mark.parametrize("lane", [True, False], ids=["lane", "wave"])
def test_fuzz_seeds_stop_at_the_oracles_error(lane):
    raised = clean = 0
    for seed in SEEDS:
        pat, desc, _ = F.pattern_for(seed, "mixed")
        ir = pat.to_ir(PL.I32)
        try:
            O.OraclePattern(ir)
        except O.OracleError:
            continue                                     # an invalid pattern (tests/test_fuzz_gpu.py checks the refusal)
        key, val, ts = F.stream_for(seed, "mixed")
        rng = np.random.default_rng(seed)
        omode = O.MODE_PROCESSOR if rng.random() < 0.5 else O.MODE_NFA_PER_KEY
        gmode = N.MODE_PROCESSOR if omode == O.MODE_PROCESSOR else N.MODE_NFA
        want, oerr = _oracle(ir, omode, key, val, ts)
        cp = N.CompiledPattern(ir)
        got, errs, csum = _device(cp, gmode, key, val, ts, lane, STOP)
        ctx = (seed, desc, omode, lane)
        if oerr is not None:
            raised += 1
            assert got == [m for m in want if m[0] < oerr[1]], ctx
            assert errs == [oerr], ctx
            assert csum[0] == len(got), ctx
        else:
            clean += 1
            assert got == want and errs == [], ctx
            assert (got, errs, csum) == _device(cp, gmode, key, val, ts, lane, 0), ctx
    assert raised >= 6 and clean >= 2, (raised, clean)   # (not vacuous: both kinds of seed were met)
