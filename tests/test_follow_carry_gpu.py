"""The follow path on carry sessions (CEP_SESSION_FOLLOW_CARRY, csrc/follow.hip "carried walks"): every
comparison is an exact list, per batch and in order, against the CPU oracle run over every key's whole stream
with its records mapped to stream positions (follow_carry_lib.oracle_batches)."""
import numpy as np
import pytest

import oracle as O
from kcep import native as N, Schema
from kcep.ingest import scalar_column
from kcep.processor import GpuCEPProcessor
from kcep.sequence import Event as Ev, sequence_from_traversal
from gpu_util import product_matches
import filter_util as U
import follow_lib as FL
import follow_carry_lib as FC

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("mode", [N.MODE_PROCESSOR, N.MODE_NFA], ids=["processor", "nfa"])
AB = [FL.stage("a", False, c=0), FL.stage("b", True, c=1)]
K8 = dict((a[0], a[2]) for a in FL.ACCEPTED)["k8_via_times"]


def omode(mode):
    return O.MODE_PROCESSOR if mode == N.MODE_PROCESSOR else O.MODE_NFA_PER_KEY


def open_session(stages, max_events, max_keys, mode=N.MODE_NFA, schema=FL.I32T, **kw):
    cp = N.CompiledPattern(FL.build(stages).to_ir(schema))
    kw.setdefault("follow_carry", True)
    s = N.Session(cp, max(1, max_events), mode=mode, carry=True, max_keys=max_keys, **kw)
    return s


def push(s, b, flags=0):
    s.push(len(b["key"]), np.ascontiguousarray(b["key"], np.int32), [np.ascontiguousarray(b["val"], np.int32)],
           topic=b["topic"], flags=flags)
    out = s.collect()
    assert out["path"] == N.PATH_FOLLOW
    return product_matches(s, out)


def run(stages, batches, mode=N.MODE_NFA, max_keys=None, **kw):
    nk = max_keys or 1 + max([int(b["key"].max()) for b in batches if len(b["key"])] or [0])
    s = open_session(stages, max(len(b["key"]) for b in batches), nk, mode, **kw)
    assert s.path == N.PATH_FOLLOW
    return [push(s, b) for b in batches], s


def check(stages, batches, mode=N.MODE_NFA, min_matches=1, min_carried=0, **kw):
    want = FC.oracle_batches(stages, FL.I32T, batches, omode(mode))
    got, s = run(stages, batches, mode, **kw)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, stages)
    assert sum(len(w) for w in want) >= min_matches
    carried = sum(m[2][-1][1] < b["pos"][0] for b, w in zip(batches, want) for m in w)
    assert carried >= min_carried                        # matches whose start lies in an earlier batch
    return want, s


def open_positions(s):
    return sorted(N.state_positions(s.state_export()).tolist())


# ---- 1. opening ----
def test_opening():
    s = open_session(FL.abc(), 64, 4)
    assert s.path == N.PATH_FOLLOW
    assert open_session(FL.abc(), 64, 4, follow_carry=True, force_path=N.PATH_FOLLOW).path == N.PATH_FOLLOW
    with pytest.raises(N.CepError) as e:                 # without the flag: today's refusal
        open_session(FL.abc(), 64, 4, follow_carry=False, force_path=N.PATH_FOLLOW)
    assert e.value.code == 12 and "CEP_SESSION_CARRY" in str(e.value)
    assert open_session(FL.abc(), 64, 4, follow_carry=False, follow=True, interpret=True).path == N.PATH_GENERAL
    # without carry the flag is CEP_SESSION_FOLLOW
    cp = N.CompiledPattern(FL.build(FL.abc()).to_ir(FL.I32T))
    assert N.Session(cp, 64, follow_carry=True).path == N.PATH_FOLLOW
    # patterns that are not eligible keep their path
    assert open_session(FL.abc((False, False)), 64, 4).path == N.PATH_STENCIL
    for name, schema, mk, _ in FL.REJECTED:
        if name in ("skip_till_any", "one_or_more"):
            a = N.Session(N.CompiledPattern(mk().to_ir(schema)), 64, carry=True, max_keys=4, interpret=True)
            b = N.Session(N.CompiledPattern(mk().to_ir(schema)), 64, carry=True, max_keys=4, interpret=True, follow_carry=True)
            assert a.path == b.path != N.PATH_FOLLOW
    # blobs of the other kinds are refused, a walk blob is taken
    for magic in (b"KCSR", b"KCST", b"KCSH"):
        with pytest.raises(N.CepError) as e:
            s.state_import(FC.walk_blob(3, 10, [(1, [[1, 4]])], magic=magic))
        assert e.value.code == 11
    with pytest.raises(N.CepError):                      # a walk that names more slots than it may hold
        s.state_import(FC.walk_blob(3, 10, [(1, [[3, 4, 5]])]))
    s.state_import(FC.walk_blob(3, 10, [(1, [[1, 4], [2, 5, 6]])]))
    assert s.stream_position() == 10 and open_positions(s) == [4, 5, 6]
    with pytest.raises(N.CepError) as e:
        s.key_state(1)
    assert e.value.code == 12 and "walks" in str(e.value)


# ---- 2. random parity ----
@MODES
@pytest.mark.parametrize("seed", range(30))
def test_random_parity(seed, mode):
    rng = np.random.default_rng(4000 + seed)
    variant = ["plain", "topics", "times"][seed % 3]
    alphabet = int(rng.integers(2, 5))
    stages = FL.random_stages(rng, variant, alphabet, min_next=1)
    batches = FC.split_stream(rng, int(rng.integers(200, 2001)), 120, alphabet, int(rng.integers(2, 6)))
    check(stages, batches, mode, min_matches=10, min_carried=1, force_path=N.PATH_FOLLOW if seed % 2 else 0)


# ---- 3. cuts at the places the kernels can go wrong ----
def test_cut_right_after_a_start():
    want, s = check(FL.abc(), FC.batches_of([[(0, [0])], [(0, [1, 2])]]), min_carried=1)
    assert want[1] == [(2, 0, [("c", 2), ("b", 1), ("a", 0)])] and open_positions(s) == []


@pytest.mark.parametrize("first,n", [(2, 1), (3, 0)], ids=["satisfies", "fails"])
def test_cut_before_a_strict_successor(first, n):
    pat = FL.abc((True, False))                          # a, followedBy b, then strictly c
    want, s = check(pat, FC.batches_of([[(0, [0, 3, 1])], [(0, [first, 2, 2])]]), min_matches=n)
    assert [len(w) for w in want] == [0, n] and open_positions(s) == []


def test_walk_waits_three_batches_and_a_key_is_absent_for_two():
    parts = [[(0, [0, 0]), (1, [0, 1])], [(0, [3, 3])], [(0, [3])], [(0, [1, 3]), (1, [3])], [(0, [2]), (1, [2, 2])]]
    batches = FC.batches_of(parts)
    want, s = check(FL.abc(), batches, min_matches=3, min_carried=3)
    assert want[4] == [(10, 0, [("c", 10), ("b", 7), ("a", 0)]), (10, 0, [("c", 10), ("b", 7), ("a", 1)]),
                       (11, 1, [("c", 11), ("b", 3), ("a", 2)])]
    # key 1 absent from batches 1 and 2: its walk (two slots taken, positions 2 and 3) stands
    got, s2 = run(FL.abc(), batches[:3])
    assert open_positions(s2) == [0, 1, 2, 3]


def with_key(batches, k, pieces):
    """the batches with key k's records (one piece per batch) appended; k is above every key of theirs"""
    return FC.batches_of([[(int(q), b["val"][b["key"] == q]) for q in np.unique(b["key"])] + [(k, p)]
                          for b, p in zip(batches, pieces)])


def test_k2_and_k8():
    rng = np.random.default_rng(31)
    check(AB, FC.split_stream(rng, 150, 60, 3, 4), min_matches=100, min_carried=10)
    # one match at least that takes slots in every batch: a | b b | b c c | c d
    b = with_key(FC.split_stream(rng, 150, 100, 4, 4), 150, [[0], [1, 1], [1, 2, 2], [2, 3]])
    want, _ = check(K8, b, min_matches=1, min_carried=1)
    assert any(m[1] == 150 and len({p for _, p in m[2]}) == 8 for m in want[3])


def test_batch_sizes():
    rng = np.random.default_rng(32)
    sizes = [1, 63, 64, 65, 0, 4095, 4097, 1]
    val = rng.integers(0, 3, sum(sizes)).astype(np.int32)
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    for c, size in zip(cuts[1:-1], sizes[1:]):           # a start right before every cut, its walk completed after it
        val[c - 1] = 0
        if size >= 3:
            val[c:c + 3] = [1, 2, 0]
    for pat in (FL.abc(), [FL.stage("a", False, c=0), FL.stage("b", True, c=1), FL.stage("c", False, c=2),
                           FL.stage("d", True, c=0)]):
        check(pat, FC.batches_of([[(0, val[a:b])] if b > a else [] for a, b in zip(cuts[:-1], cuts[1:])]),
              min_matches=100, min_carried=5)


@pytest.mark.parametrize("edge", [64, 4096])
def test_segment_start_at_an_edge(edge):
    rng = np.random.default_rng(edge)
    mk = lambda n: rng.integers(0, 3, n).astype(np.int32)
    first = [(0, np.concatenate([mk(40), [0, 3, 3]])), (1, np.concatenate([mk(40), [0, 1, 3]])), (2, [0, 0, 3])]
    # key 1's segment starts at the edge, key 2's one record before the next one
    second = [(0, np.concatenate([[1, 2], mk(edge - 2)])), (1, np.concatenate([[2], mk(edge - 2)])), (2, [1, 3, 2, 2])]
    batches = FC.batches_of([first, second])
    assert batches[1]["key"][edge - 1] == 0 and batches[1]["key"][edge] == 1 and batches[1]["key"][2 * edge - 1] == 2
    want, _ = check(FL.abc(), batches, min_carried=4)
    assert (int(batches[1]["pos"][edge]), 1) in [(m[0], m[1]) for m in want[1]]   # completed by the segment's first record


# ---- 4. many waiting walks ----
def test_many_waiting_walks_one_key():
    n = 40_000
    s = open_session(FL.abc(), n, 2)
    a = dict(key=np.zeros(n, np.int32), val=np.zeros(n, np.int32), topic=None)
    assert push(s, a) == [] and push(s, a) == []         # (the pool grows past its first 65536 walks)
    assert open_positions(s) == list(range(2 * n))
    got = push(s, dict(key=np.zeros(2, np.int32), val=np.array([1, 2], np.int32), topic=None))
    assert got == [(2 * n + 1, 0, [("c", 2 * n + 1), ("b", 2 * n), ("a", i)]) for i in range(2 * n)]
    assert open_positions(s) == []


def test_many_waiting_walks_three_keys():
    parts = [[(k, [0] * 100) for k in range(3)], [(k, [3, 1, 3]) for k in range(3)] + [(3, [0, 0, 1, 2])],
             [(0, [3, 0, 0, 2]), (1, [2]), (2, [0, 3])]]
    batches = FC.batches_of(parts)
    want, s = check(FL.abc(), batches, min_matches=200, min_carried=200)
    # (the second batch completes no carried walk, only key 3's own: the ranked order)
    assert [len(w) for w in want] == [0, 2, 200]
    assert len(open_positions(s)) == 2 * 100 + 3


# ---- 5. checkpoints ----
def test_export_import_evict_clear():
    rng = np.random.default_rng(51)
    nk = 40
    batches = FC.split_stream(rng, nk, 80, 3, 5)
    want = FC.oracle_batches(FL.abc(), FL.I32T, batches)
    s = open_session(FL.abc(), max(len(b["key"]) for b in batches), 2 * nk)
    got = [push(s, b) for b in batches[:2]]
    blob = s.state_export()
    assert blob[:4] == b"KCSW" and len(N.state_positions(blob)) > 0
    s2 = open_session(FL.abc(), max(len(b["key"]) for b in batches), 2 * nk)
    s2.state_import(blob)
    assert s2.stream_position() == s.stream_position() and s2.state_export() == blob
    got.append(push(s2, batches[2]))
    # half the keys leave the device and come back under other ids
    moved = list(range(0, nk, 2))
    blobs = s2.state_evict(moved)
    assert sum(len(b) > 0 for b in blobs) > 3
    before = open_positions(s2)
    s2.state_import_keys([b for b in blobs if b], [nk + k for k, b in zip(moved, blobs) if b])
    assert len(before) < len(open_positions(s2))
    orig = {}                                            # stream position as pushed -> as the oracle saw it
    for b in batches[3:]:
        q = dict(b, key=np.where(b["key"] % 2 == 0, b["key"] + nk, b["key"]).astype(np.int32))
        order = np.argsort(q["key"], kind="stable")      # (the renamed keys' segments move to the batch's end)
        res = push(s2, dict(key=q["key"][order], val=q["val"][order], topic=q["topic"][order]))
        orig.update({int(b["pos"][0]) + i: int(b["pos"][0]) + int(o) for i, o in enumerate(order)})
        back = lambda p: orig.get(p, p)
        res = [(back(r), k - nk if k >= nk else k, [(nm, back(p)) for nm, p in tr]) for r, k, tr in res]
        got.append(sorted(res, key=lambda m: (m[0], m[2][-1][1])))
    assert got == want and sum(len(w) for w in want[3:]) > 10
    s2.state_clear()
    assert s2.stream_position() == 0 and open_positions(s2) == []
    assert push(s2, batches[0]) == want[0]


# ---- 6. batch flags ----
def _oracle_stream(ir, st, mode=O.MODE_PROCESSOR):
    p = O.OraclePattern(ir)
    r = O.OracleRun(p, mode)
    r.process(O.BatchArrays(st["key"], [st["val"]], [1], valid=st["valid"], topic=st["topic"], offset=st["off"], ts=st["ts"]))
    return [(m.record, m.key, [(p.names[nm], ev) for nm, ev in m.traversal]) for m in r.matches(with_groups=False)]


def test_arrival_order():
    rng = np.random.default_rng(61)
    n, nk = 3000, 9
    st = U.make_stream(rng, rng.integers(0, nk, n).astype(np.int32), ntopics=2, p_null=0.0, p_re=0.0)
    ir = FL.build(FL.abc()).to_ir(U.SCHEMA)
    want = _oracle_stream(ir, st)
    s = N.Session(N.CompiledPattern(ir), 1000, mode=N.MODE_PROCESSOR, carry=True, max_keys=nk, follow_carry=True)
    parts = [U.take(st, np.arange(a, min(n, a + 1000))) for a in range(0, n, 1000)]
    got = []
    for p in parts:
        U.push(s, p, N.BATCH_ARRIVAL_ORDER | N.BATCH_DELIVER | N.BATCH_OFFSETS_MONOTONE, with_valid=False)
        out = s.collect()
        assert out["path"] == N.PATH_FOLLOW
        got += U.matches(s, out)
    assert got == want and sum(m[0] >= 1000 > m[2][-1][1] for m in want) > 5


@pytest.mark.parametrize("arrival", [False, True], ids=["grouped", "arrival"])
def test_filter(arrival):
    rng = np.random.default_rng(62)
    n, nk = 3000, 9
    st = U.make_stream(rng, rng.integers(0, nk, n).astype(np.int32), ntopics=2, nvals=3)
    assert (st["valid"] == 0).sum() > 50
    parts = [U.take(st, np.arange(a, min(n, a + 750))) for a in range(0, n, 750)]
    if not arrival:
        parts = [U.grouped(p) for p in parts]
    ir = FL.build(FL.abc()).to_ir(U.SCHEMA)
    want = _oracle_stream(ir, U.concat(parts))
    s = N.Session(N.CompiledPattern(ir), 750, mode=N.MODE_PROCESSOR, carry=True, max_keys=nk, follow_carry=True)
    assert s.path == N.PATH_FOLLOW
    fl = N.BATCH_FILTER | (N.BATCH_ARRIVAL_ORDER | N.BATCH_DELIVER if arrival else 0)
    got = []
    for p in parts:
        U.push(s, p, fl)
        out = s.collect()
        assert out["path"] == N.PATH_FOLLOW
        got += U.matches(s, out)
    assert got == want and sum(m[0] >= 750 > m[2][-1][1] for m in want) > 5
    # a batch the session does not take: nulls without the flag
    with pytest.raises(N.CepError) as e:
        U.push(s, parts[0], 0)
    assert e.value.code == 12 and "a follow carry session takes batches" in str(e.value)
    with pytest.raises(N.CepError) as e:
        U.push(s, parts[0], N.BATCH_OFFSETS_MONOTONE | N.BATCH_STOP_AT_ERROR, with_valid=False)
    assert e.value.code == 12 and "follow" in str(e.value)


# ---- 7. a rejected push ----
def test_rejected_push_changes_nothing():
    rng = np.random.default_rng(71)
    batches = FC.split_stream(rng, 30, 60, 3, 3)
    want = FC.oracle_batches(FL.abc(), FL.I32T, batches)
    s = open_session(FL.abc(), max(len(b["key"]) for b in batches) + 8, 30)
    got = [push(s, batches[0])]
    blob, at = s.state_export(), s.stream_position()
    bad = dict(key=np.array([3, 3, 5, 3], np.int32), val=np.array([0, 1, 0, 2], np.int32), topic=None)
    with pytest.raises(N.CepError) as e:                 # a key in two segments
        push(s, bad)
    assert e.value.code == 11 and "two segments" in str(e.value)
    with pytest.raises(N.CepError) as e:                 # a key id out of range
        push(s, dict(bad, key=np.array([3, 3, 5, 30], np.int32)))
    assert e.value.code == 11
    assert s.state_export() == blob and s.stream_position() == at
    got += [push(s, b) for b in batches[1:]]
    assert got == want


# ---- 8. the processor ----
def _view(seq):
    return [(st.getStage(), [(e.topic, e.offset) for e in st.getEvents()]) for st in seq.matched()]


def _records(rng, n, phase):
    """an interleaved stream with nulls and re-deliveries; the keys in use move on every `phase` records (four at
    a time, one shared with the next phase) and the last phase takes the first keys up again"""
    recs, nxt, hist = [], {}, {}
    phases = (n + phase - 1) // phase
    for i in range(n):
        p = i // phase
        p = 0 if p == phases - 1 else p
        k = f"k{3 * p + int(rng.integers(0, 4))}"
        t = f"T{int(rng.integers(0, 2))}"
        if k in hist and rng.random() < 0.1:             # a re-delivery of one of the key's last records
            recs.append(recs[int(rng.choice(hist[k][-3:]))])
        elif rng.random() < 0.05:                        # a null value, its offset far ahead
            recs.append((k, None, t, 0, nxt.get(t, 0) + 5000, 1000 + i))
        else:
            recs.append((k, int(rng.integers(0, 3)), t, 0, nxt.get(t, 0), 1000 + i))
            nxt[t] = nxt.get(t, 0) + 1
        hist.setdefault(k, []).append(i)
    return recs


@pytest.mark.parametrize("device_filter", [False, True], ids=["host_marks", "device_filter"])
@pytest.mark.parametrize("batch,n,phase", [(1, 400, 80), (7, 700, 100), (1000, 5000, 1000)])
def test_processor(batch, n, phase, device_filter):
    rng = np.random.default_rng(81)
    schema = Schema([("value", "i32")], topics=["T0", "T1"])
    pat = FL.build(FL.abc())
    dec = scalar_column(schema)
    recs = _records(rng, n, phase)
    assert len({r[0] for r in recs}) > 8
    # the oracle over the arrival-order stream (nulls as invalid records)
    live = next(r for r in recs if r[1] is not None)
    keys = {}
    kid = np.array([keys.setdefault(r[0], len(keys)) for r in recs], np.int32)
    p = O.OraclePattern(pat.to_ir(schema))
    orun = O.OracleRun(p, O.MODE_PROCESSOR)
    orun.process(O.BatchArrays(kid, dec.columns([dec.row(r[1] if r[1] is not None else live[1]) for r in recs]), [1],
                               valid=np.array([r[1] is not None for r in recs], np.uint8),
                               topic=np.array([schema.topic_id(r[2]) for r in recs], np.int32),
                               offset=np.array([r[4] for r in recs], np.int64), ts=np.array([r[5] for r in recs], np.int64)))
    ev = lambda i: Ev(recs[i][0], recs[i][1], recs[i][5], recs[i][2], recs[i][3], recs[i][4])
    want = [(recs[m.record][0], _view(sequence_from_traversal(m.traversal, p.names, ev)))
            for m in orun.matches(with_groups=False)]
    assert len(want) > 20
    out = []
    proc = GpuCEPProcessor("q", pat, schema, dec, batch_size=batch, max_keys=8, device_filter=device_filter, follow=True,
                           prune_at=64)
    proc.init(lambda k, seq: out.append((k, _view(seq))))
    assert proc.session.path == N.PATH_FOLLOW
    for r in recs:
        proc.process(*r)
    spilled = len(proc._spilled)
    proc.close()
    assert out == want and spilled > 0


# ---- 9. checksum and device match count ----
def test_checksum_and_count():
    import torch
    rng = np.random.default_rng(91)
    batches = FC.split_stream(rng, 60, 80, 3, 3)
    cap = max(len(b["key"]) for b in batches)
    s = open_session(FL.abc(), cap, 60)
    g = open_session(FL.abc(), cap, 60, follow_carry=False, force_path=N.PATH_GENERAL, interpret=True)
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    total = 0
    for b in batches:
        for i, x in enumerate((s, g)):
            x.push(len(b["key"]), b["key"], [b["val"]], topic=b["topic"])
            x.match_count_to(cnt.data_ptr() + 8 * i)
        torch.cuda.synchronize()
        assert s.checksum() == g.checksum()
        assert cnt[0].item() == cnt[1].item() == s.checksum()[0]
        total += int(cnt[0].item())
    assert total > 100
    s.push(0, batches[0]["key"][:0], [batches[0]["val"][:0]])
    s.match_count_to(cnt.data_ptr())
    torch.cuda.synchronize()
    assert cnt[0].item() == 0 and s.checksum()[0] == 0 and s.collect()["path"] == N.PATH_FOLLOW
