"""CEP_BATCH_FILTER over the rich carry stream of tests/test_fuzz_gpu.py::test_random_rich_carry_parity:
interleaved keys, ~5 % null records, ~5 % re-deliveries of an earlier record of the same key (possibly in a
later batch), stages reading one topic, 2-6 carry batches each grouped by key.  There the stencil / chain /
runs sessions refuse the stream and it runs on the general path forced; here it is pushed with the flag on
the path the product picks, against the oracle's single pass."""
import os

import numpy as np
import pytest

import oracle as O
from kcep import native as N
import fuzz_patterns as F

pytestmark = pytest.mark.gpu

# 12 seeds by default, chosen so that at least 4 of them open a stencil, chain or runs session (27, 30, 34,
# 35, 37, 38: tests/test_filter_cpu.py checks it without a device); KCEP_FUZZ_SEEDS=a:b for a campaign
DEFAULT_SEEDS = range(27, 39)
_env = os.environ.get("KCEP_FUZZ_SEEDS")
SEEDS = range(*map(int, _env.split(":"))) if _env else DEFAULT_SEEDS
_fast = set()


def _stream(seed):
    """test_random_rich_carry_parity's stream, built the same way."""
    key, val, _ = F.random_stream(seed)
    rng = np.random.default_rng(seed + 6)
    perm = rng.permutation(len(key))
    key, val = key[perm], val[perm]
    n = len(key)
    ts = np.cumsum(rng.integers(1, 4, n)).astype(np.int64)
    px = rng.integers(0, 6000, n).astype(np.int64)
    r = rng.random(n)
    topic = rng.integers(0, 2, n).astype(np.int32)
    valid = (rng.random(n) > 0.05).astype(np.uint8)
    off = np.arange(n, dtype=np.int64)
    last = {}
    for i in range(n):                                   # re-delivery: an earlier record of the key again
        k = int(key[i])
        if k in last and rng.random() < 0.05:
            j = int(rng.choice(last[k][-4:]))
            for a in (val, ts, px, r, topic, valid, off):
                a[i] = a[j]
        last.setdefault(k, []).append(i)
    nb = int(rng.integers(2, 7))
    bounds = [0] + sorted(rng.choice(np.arange(1, n), nb - 1, replace=False).tolist()) + [n]
    order = np.concatenate([a + np.argsort(key[a:b], kind="stable") for a, b in zip(bounds[:-1], bounds[1:])])
    key, val, ts, px, r, topic, valid, off = (x[order] for x in (key, val, ts, px, r, topic, valid, off))
    return key, [val, px, r], ts, topic, valid, off, bounds


@pytest.mark.parametrize("seed", SEEDS)
def test_random_rich_carry_filtered(seed):
    pat, desc, _ = F.random_pattern(seed, rich=True)
    ir = pat.to_ir(F.RICH)
    try:
        po = O.OraclePattern(ir)
    except O.OracleError:
        pytest.skip("invalid pattern")
    key, cols, ts, topic, valid, off, bounds = _stream(seed)
    run = O.OracleRun(po, O.MODE_PROCESSOR)
    oerr = None
    try:
        run.process(O.BatchArrays(key, cols, [1, 2, 3], ts=ts, topic=topic, valid=valid, offset=off))
    except O.OracleError as e:
        oerr = (e.code, e.record)
    want = [(m.record, m.key, [(po.names[nm], ev) for nm, ev in m.traversal]) for m in run.matches(with_groups=False)]
    cp = N.CompiledPattern(ir)
    s = N.Session(cp, max(b - a for a, b in zip(bounds[:-1], bounds[1:])), mode=N.MODE_PROCESSOR, carry=True,
                  max_keys=int(key.max()) + 1)
    if s.path != N.PATH_GENERAL:
        _fast.add(seed)
    got, gerr = [], None
    for a, b in zip(bounds[:-1], bounds[1:]):
        sl = lambda x: np.ascontiguousarray(x[a:b])
        s.push(b - a, sl(key), [sl(c) for c in cols], ts=sl(ts), topic=sl(topic), valid=sl(valid), offset=sl(off),
               flags=N.BATCH_FILTER)
        out = s.collect(raise_on_error=False)
        for m in range(len(out["match_record"])):
            x, y = out["ent_off"][m], out["ent_off"][m + 1]
            got.append((int(out["match_record"][m]), int(out["match_key"][m]),
                        [(cp.names[out["ent_name"][i]], int(out["ent_record"][i])) for i in range(x, y)]))
        if out["err"]:
            gerr = (int(out["err"]), int(out["err_record"]))
            break
    ctx = (seed, desc, s.path, len(bounds) - 1)
    if oerr is not None:
        got = [m for m in got if m[0] < oerr[1]]
        want = [m for m in want if m[0] < oerr[1]]
    assert gerr == oerr, ctx
    assert got == want, ctx


def test_default_seeds_reach_the_fast_paths():
    """Of the default seeds at least 4 ran on a stencil, chain or runs session: the flag was not a no-op."""
    if _env:
        pytest.skip("a KCEP_FUZZ_SEEDS campaign")
    assert len(_fast) >= 4, sorted(_fast)
