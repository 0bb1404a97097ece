"""CEP_BATCH_STOP_AT_ERROR: a general-path batch stops at its earliest exception, as the reference's task
fails at the first exception process() throws (CEPProcessor.java:134-149) and evaluates nothing after it.

Pattern R is patterns_lib.any_any() with the first stage's predicate written so that it divides: over
values {0, 2, 3} it selects 0 exactly as before, and a record of value 7 raises ArithmeticException
(CEP_E_ARITHMETIC, 5) on any key at any time.  Keys: k0 raises at its 4th record, k1 is heavy (8 x 32 x 32
= 8192 skip-till-any matches), k2 is light.  With the flag the collected CSR is the reference's forwarded
stream -- the matches before the exception -- with no filtering on the host, whichever keys had already
run past the exception when it became visible; without it k1 runs to its end for matches every
consumer drops.  Everything is compared with oracle/cep_oracle.c."""
import functools

import numpy as np
import pytest

import oracle as O
from kcep import QueryBuilder, Selected, Event
from kcep import native as N
from kcep.ingest import scalar_column
from kcep.processor import GpuCEPProcessor
from gpu_util import product_matches
import patterns_lib as PL

pytestmark = pytest.mark.gpu

K0 = [0, 2, 3, 7, 3]
K1 = [0] * 8 + [2] * 32 + [3] * 32
K2 = [0, 2, 3]
K3 = [0, 7]
ARITH = 5                                                # CEP_E_ARITHMETIC
STOP = N.BATCH_STOP_AT_ERROR if hasattr(N, "BATCH_STOP_AT_ERROR") else 8

# (lane_nfa, interpret): the lane and the wave engine, interpreting and compiled for the pattern
ENGINES = [(True, True), (False, True), (True, False), (False, False)]
ENGINE_IDS = ["lane-interp", "wave-interp", "lane-jit", "wave-jit"]
ENGINES_INTERP = ENGINES[:2]


def pattern_r():
    v = Event.value()
    return (QueryBuilder().select("first").where(v % (v - 7) == 0).then()
            .select("second", Selected.withSkipTilAnyMatch()).where(Event.value() == 2).then()
            .select("latest", Selected.withSkipTilAnyMatch()).where(Event.value() == 3).build())


@functools.lru_cache(maxsize=None)
def ir_r():
    return pattern_r().to_ir(PL.I32)


def grouped(*keys):
    """Key-grouped stream: key i's records contiguous, in the order given."""
    key = np.concatenate([np.full(len(k), i, np.int32) for i, k in enumerate(keys)])
    val = np.concatenate([np.asarray(k, np.int32) for k in keys])
    return key, val


def interleave(plan, keys):
    """Arrival-order stream from `plan`, a list of (key id, count): the next `count` records of that key."""
    at = [0] * len(keys)
    key, val = [], []
    for k, c in plan:
        key += [k] * c
        val += keys[k][at[k]:at[k] + c]
        at[k] += c
    return np.asarray(key, np.int32), np.asarray(val, np.int32), at


def oracle_run(key, val, mode=O.MODE_PROCESSOR):
    p = O.OraclePattern(ir_r())
    r = O.OracleRun(p, mode)
    err = None
    try:
        r.process(O.BatchArrays(key, [val], [1]))
    except O.OracleError as e:
        err = (e.code, e.record)
    return [(m.record, m.key, [(p.names[nm], ev) for nm, ev in m.traversal])
            for m in r.matches(with_groups=False)], err


@functools.lru_cache(maxsize=None)
def oracle_grouped(mode):
    """k0, k1, k2 key-grouped: the reference fails at k0's 7 (record 3) with one match before it."""
    key, val = grouped(K0, K1, K2)
    want, err = oracle_run(key, val, mode)
    assert err == (ARITH, 3)
    want = [m for m in want if m[0] < err[1]]
    assert [m[0] for m in want] == [2]
    return want, err


def session(n, lane, interp, **kw):
    s = N.Session(N.CompiledPattern(ir_r()), n, force_path=N.PATH_GENERAL, lane_nfa=lane, interpret=interp, **kw)
    assert s.path == N.PATH_GENERAL and s.wave == (not lane) and s.jit == (not interp)
    return s


def push_collect(s, key, val, flags=0):
    s.push(len(key), np.ascontiguousarray(key), [np.ascontiguousarray(val)], flags=flags)
    out = s.collect(raise_on_error=False)
    rec, code = s.batch_errors()
    return product_matches(s, out), (int(out["err"]), int(out["err_record"])), list(zip(rec.tolist(), code.tolist()))


# ---- 1. key-grouped, non-carry ----
@pytest.mark.parametrize("mode", [N.MODE_PROCESSOR, N.MODE_NFA], ids=["processor", "nfa"])
@pytest.mark.parametrize("lane,interp", ENGINES, ids=ENGINE_IDS)
def test_grouped_batch_is_the_references_forwarded_stream(lane, interp, mode):
    want, oerr = oracle_grouped(O.MODE_PROCESSOR if mode == N.MODE_PROCESSOR else O.MODE_NFA_PER_KEY)
    key, val = grouped(K0, K1, K2)
    s = session(len(key), lane, interp, mode=mode)
    got, err, errs = push_collect(s, key, val, STOP)
    assert got == want                                   # (no host-side filter: k1's 8192 matches are not there)
    assert err == oerr == (ARITH, 3)
    assert errs == [(3, ARITH)]
    assert s.checksum()[0] == len(want)                  # the device-side count agrees with the trimmed CSR


def test_heavy_key_alone_has_8192_matches():
    """The sizes the cases rely on (checked on the oracle): k1 alone 8192 matches, 4/16/16 1024."""
    for k, n in ((K1, 8192), ([0] * 4 + [2] * 16 + [3] * 16, 1024)):
        want, err = oracle_run(*grouped(k))
        assert err is None and len(want) == n


# ---- 2. two failing keys ----
@pytest.mark.parametrize("lane,interp", ENGINES, ids=ENGINE_IDS)
def test_only_the_first_of_two_failing_keys_is_listed(lane, interp):
    key, val = grouped(K0, K1, K2, K3)
    p3 = len(K0) + len(K1) + len(K2) + 1                 # k3's 7
    want, oerr = oracle_grouped(O.MODE_PROCESSOR)
    s = session(len(key), lane, interp)
    got, err, errs = push_collect(s, key, val, STOP)
    assert (got, err, errs) == (want, oerr, [(3, ARITH)])
    # today's behaviour without the flag, the contrast: every key runs, both failures are listed
    got0, err0, errs0 = push_collect(s, key, val, 0)
    assert err0 == oerr and errs0 == [(3, ARITH), (p3, ARITH)]
    assert len(got0) == 1 + 8192 + 1 and [m for m in got0 if m[0] < 3] == want


# ---- 3. work is saved ----
@pytest.mark.parametrize("lane,interp", ENGINES_INTERP, ids=ENGINE_IDS[:2])
def test_the_heavy_key_stops_early(lane, interp):
    key, val = grouped(K0, K1, K2)
    evals = {}
    for flags in (0, STOP):
        s = session(len(key), lane, interp, profile=True)
        push_collect(s, key, val, flags)
        prof = s.key_profile()
        evals[flags] = int(prof[prof[:, 0] == 1][0, 2])  # k1's run evaluations
        if flags:
            keys, records = s.batch_stopped()
            print("batch_stopped", keys, records, "k1 run evaluations", evals)
            assert keys >= 1 and records >= 1
        else:
            assert s.batch_stopped() == (0, 0)
    assert evals[STOP] < evals[0]


# ---- 4. arrival order, carry, two batches ----
def arrival_two_batches():
    keys = [K0, K1, K2]
    k1a, v1a, at = interleave([(1, 5), (0, 1), (1, 9), (2, 1), (0, 1), (1, 6)], keys)   # clean prefixes: no 7
    assert 7 not in v1a and at == [2, 20, 1]
    rest = [K0[at[0]:], K1[at[1]:], K2[at[2]:]]
    # k0's 7 arrives with part of k1 before it and part after
    k2a, v2a, at2 = interleave([(1, 30), (0, 1), (1, 6), (0, 1), (2, 1), (1, 16), (0, 1), (2, 1)], rest)
    assert at2 == [len(r) for r in rest]
    p = len(k1a) + int(np.flatnonzero(v2a == 7)[0])
    return (k1a, v1a), (k2a, v2a), p


@functools.lru_cache(maxsize=None)
def oracle_arrival():
    (k1a, v1a), (k2a, v2a), p = arrival_two_batches()
    want, err = oracle_run(np.concatenate([k1a, k2a]), np.concatenate([v1a, v2a]))
    assert err == (ARITH, p)
    want = [m for m in want if m[0] < p]
    assert len(want) > 1000 and any(m[1] == 1 and m[0] > len(k1a) for m in want)
    return want, err


ARRIVAL = N.BATCH_ARRIVAL_ORDER | N.BATCH_OFFSETS_MONOTONE


@pytest.mark.parametrize("lane,interp", ENGINES, ids=ENGINE_IDS)
def test_arrival_carry_batch_stops_and_commits_nothing(lane, interp):
    (k1a, v1a), (k2a, v2a), p = arrival_two_batches()
    want, oerr = oracle_arrival()
    s = session(max(len(k1a), len(k2a)), lane, interp, carry=True, max_keys=3)
    got1, err1, errs1 = push_collect(s, k1a, v1a, ARRIVAL | STOP)
    assert err1 == (0, -1) and errs1 == []
    blob = s.state_export()
    states = [s.key_state(k) for k in range(3)]
    assert all(st is not None for st in states)
    got2, err2, errs2 = push_collect(s, k2a, v2a, ARRIVAL | STOP)
    assert got1 + got2 == want                           # element by element, in forward order
    assert err2 == oerr == (ARITH, p) and errs2 == [(p, ARITH)]
    assert s.checksum()[0] == len(got2)
    assert s.state_export() == blob                      # no key's state was committed
    assert [s.key_state(k) for k in range(3)] == states
    assert s.stream_position() == len(k1a) + len(k2a)    # the failed batch's positions stay used


# ---- 5. capacity hand-back ----
CAP_WORDS = 20000                                        # fits k0 and k2, not k1's 8192 matches


@pytest.mark.parametrize("lane,interp", ENGINES, ids=ENGINE_IDS)
def test_capacity_hand_back_before_the_exception_stands(lane, interp):
    keys = [K0, K1, K2]
    # k1 first, then k2, no 7
    ka, va, _ = interleave([(1, len(K1)), (2, len(K2))], keys)
    s = session(len(K0) + len(K1) + len(K2), lane, interp, carry=True, max_keys=3, max_key_words=CAP_WORDS)
    off = push_collect(s, ka, va, ARRIVAL)
    caps = [(r, c) for r, c in off[2] if c == N.E_RUN_CAPACITY]
    assert len(caps) == 1 and off[2] == caps and caps[0][0] < len(K1), off[2]   # the precondition: k1 handed back at q
    q = caps[0][0]
    assert any(m[1] == 2 for m in off[0])                # k2's match
    s = session(len(K0) + len(K1) + len(K2), lane, interp, carry=True, max_keys=3, max_key_words=CAP_WORDS)
    on = push_collect(s, ka, va, ARRIVAL | STOP)
    assert on == off
    assert s.batch_stopped() == (0, 0)                   # a hand-back is no task failure: nothing stops
    # a 7 on another key at p > q
    kb, vb, _ = interleave([(1, len(K1)), (0, len(K0)), (2, len(K2))], keys)
    p = len(K1) + 3
    s = session(len(kb), lane, interp, carry=True, max_keys=3, max_key_words=CAP_WORDS)
    off = push_collect(s, kb, vb, ARRIVAL)
    assert off[2] == [(q, N.E_RUN_CAPACITY), (p, ARITH)]
    s = session(len(kb), lane, interp, carry=True, max_keys=3, max_key_words=CAP_WORDS)
    on = push_collect(s, kb, vb, ARRIVAL | STOP)
    assert on[0] == [m for m in off[0] if m[0] < p] and len(on[0]) > 0
    assert on[2] == [(q, N.E_RUN_CAPACITY), (p, ARITH)] and on[1] == off[1]


# ---- 6. no exception ----
@pytest.mark.parametrize("lane,interp", ENGINES, ids=ENGINE_IDS)
def test_flag_changes_nothing_without_an_exception(lane, interp):
    keys = [[0, 2, 3, 3], K1, K2]
    key, val, _ = interleave([(1, 20), (0, 2), (2, 1), (1, 40), (0, 2), (2, 2), (1, 12)], keys)
    res = {}
    for flags in (0, STOP):
        s = session(len(key), lane, interp, carry=True, max_keys=3)
        s.push(len(key), key, [val], flags=ARRIVAL | flags)
        out = s.collect(raise_on_error=False)
        res[flags] = ({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in out.items()},
                      [x.tolist() for x in s.batch_errors()], s.checksum(), s.state_export(),
                      [s.key_state(k) for k in range(3)], s.stream_position())
        assert s.batch_stopped() == (0, 0)
    assert res[STOP] == res[0]
    assert len(res[0][0]["match_record"]) == 2 + 8192 + 1 and res[0][0]["err"] == 0


# ---- 7. rejections leave the session untouched ----
def test_rejected_pushes_leave_the_session_untouched():
    v = Event.value()
    strict = QueryBuilder().select("a").where(v == 0).then().select("b").where(v == 1).build().to_ir(PL.I32)
    key = np.zeros(6, np.int32)
    val = np.array([0, 1, 2, 0, 1, 1], np.int32)
    s = N.Session(N.CompiledPattern(strict), 6)
    assert s.path == N.PATH_STENCIL
    s.push(6, key, [val])
    bid = s.batch_id()
    with pytest.raises(N.CepError) as e:
        s.push(6, key, [val[::-1].copy()], flags=STOP)
    assert e.value.code == 12 and "stencil" in str(e.value)
    assert s.batch_id() == bid
    assert [m[0] for m in product_matches(s, s.collect())] == [1, 4]   # the batch before, not the rejected one

    key, val = grouped([0, 2, 3, 3], K2)
    s = session(len(key), True, True)
    s.push(len(key), key, [val])
    bid = s.batch_id()
    with pytest.raises(N.CepError) as e:
        s.push(len(key), key, [val[::-1].copy()], flags=N.BATCH_ARRIVAL_ORDER)
    assert e.value.code == 12
    assert s.batch_id() == bid
    assert [m[0] for m in product_matches(s, s.collect())] == [2, 3, 6]


# ---- 8. processor ----
def test_processor_forwards_and_fails_the_same_with_the_option():
    """The two batches of case 4 as one arrival stream, a flush between them."""
    (k1a, v1a), (k2a, v2a), p = arrival_two_batches()
    key = np.concatenate([k1a, k2a]).tolist()
    val = np.concatenate([v1a, v2a]).tolist()
    runs = {}
    for stop in (False, True):
        proc = GpuCEPProcessor("stop", pattern_r(), PL.I32, scalar_column(PL.I32), batch_size=1 << 10, max_keys=8,
                               stop_at_error=stop)
        got = []
        proc.init(lambda k, s: got.append((k, [(g.getStage(), [e.offset for e in g.getEvents()]) for g in s.matched()])))
        assert proc.session.path == N.PATH_GENERAL
        with pytest.raises(N.CepError) as e:
            for i, (k, v) in enumerate(zip(key, val)):
                proc.process(f"K{k}", v, "events", 0, i, 1000 + i)
                if i + 1 == len(k1a):
                    proc.punctuate(0)
            proc.punctuate(0)
        stopped = proc.session.batch_stopped()
        assert stopped == (0, 0) if not stop else stopped[0] >= 0
        runs[stop] = (got, e.value.code, e.value.record)
        proc.session.close()
    assert runs[True] == runs[False]
    want, _ = oracle_arrival()
    assert runs[True][1:] == (ARITH, p) and [g[0] for g in runs[True][0]] == [f"K{m[1]}" for m in want]
