"""CEP_BATCH_STOP_AT_ERROR, the host side without a GPU: the ABI's new names, and GpuCEPProcessor's use of
the flag (kcep/processor.py) against a stand-in session."""
import ctypes

import numpy as np

from kcep import Schema
from kcep import native as N
from kcep.ingest import scalar_column
from kcep.processor import GpuCEPProcessor
import patterns_lib as PL


def test_flag_value_and_exported_symbol():
    assert N.BATCH_STOP_AT_ERROR == 8
    assert "cep_batch_stopped" in N.SYMBOLS
    L = ctypes.CDLL(N.LIB_PATH)
    assert hasattr(L, "cep_batch_stopped")
    k, r = ctypes.c_int64(), ctypes.c_int64()
    L.cep_batch_stopped.argtypes = [ctypes.c_void_p] * 3
    assert L.cep_batch_stopped(None, ctypes.byref(k), ctypes.byref(r)) == 11   # CEP_E_ARG: no session


class Stub:
    """Answers each push like the device: a match per record of value 1, CEP_E_NULL_POINTER (4) at a
    key's first record of value 9, CEP_E_RUN_CAPACITY (9) at a key's first record of value 5 while a
    per-key cap is set.  With BATCH_STOP_AT_ERROR it keeps only what lies before the earliest exception."""

    def __init__(self, path=N.PATH_GENERAL):
        self.path = path
        self.pos = 0
        self.cap = 1
        self.pushes = []

    def stream_position(self):
        return self.pos

    def set_max_key_words(self, w):
        self.cap = w

    def push(self, n, key, cols, topic=None, partition=None, offset=None, ts=None, flags=0, **kw):
        self.pushes.append(dict(flags=flags, offset=offset.tolist(), cap=self.cap))
        rec, errs, dead = [], [], set()
        for i in range(n):
            k, v = int(key[i]), int(cols[0][i])
            if k in dead:
                continue
            if v == 9 or (v == 5 and self.cap):
                dead.add(k)
                errs.append((self.pos + i, 4 if v == 9 else 9))
            elif v == 1:
                rec.append(self.pos + i)
        if flags & N.BATCH_STOP_AT_ERROR:
            raising = [r for r, c in errs if c != 9]
            if raising:
                rec = [r for r in rec if r < raising[0]]
                errs = [(r, c) for r, c in errs if r <= raising[0]]
        self.errs = errs
        self.out = dict(match_record=np.asarray(rec, np.int64), match_key=np.asarray([int(key[r - self.pos]) for r in rec], np.int32),
                        ent_off=np.arange(len(rec) + 1, dtype=np.int64), ent_name=np.zeros(len(rec), np.int32),
                        ent_record=np.asarray(rec, np.int64), path=N.PATH_GENERAL,
                        err=errs[0][1] if errs else 0, err_record=errs[0][0] if errs else -1)
        self.pos += n

    def collect(self, raise_on_error=True):
        return self.out

    def batch_errors(self):
        return np.asarray([r for r, _ in self.errs], np.int64), np.asarray([c for _, c in self.errs], np.int32)

    def close(self):
        pass


def run(stub, records, **kw):
    sch = Schema([("value", "i32")])
    p = GpuCEPProcessor("q", PL.any_any(), sch, scalar_column(sch), batch_size=100, max_key_words=1, **kw)
    got = []
    p.init(lambda k, s: got.append((k, [e.offset for g in s.matched() for e in g.getEvents()])), session=stub)
    for o, (k, v) in enumerate(records):
        p.process(k, v, "events", 0, o, o)
    err = None
    try:
        p.flush()
    except N.CepError as e:
        err = (e.code, e.record)
    return got, err


def test_processor_sets_the_flag_only_when_asked_and_on_the_general_path():
    recs = [("a", 1), ("b", 1)]
    for kw, path, want in ((dict(), N.PATH_GENERAL, 0), (dict(stop_at_error=False), N.PATH_GENERAL, 0),
                           (dict(stop_at_error=True), N.PATH_GENERAL, 8), (dict(stop_at_error=True), N.PATH_STENCIL, 0),
                           (dict(stop_at_error=True), N.PATH_RUNS, 0), (dict(stop_at_error=True), N.PATH_CHAIN, 0)):
        stub = Stub(path)
        got, err = run(stub, recs, **kw)
        assert err is None and [g[0] for g in got] == ["a", "b"]
        assert [p["flags"] & N.BATCH_STOP_AT_ERROR for p in stub.pushes] == [want]
        assert all(p["flags"] & N.BATCH_ARRIVAL_ORDER for p in stub.pushes)


# key a is handed back (5) at arrival index 1, key b raises (9) at index 4; a has records on both sides
RECS = [("a", 1), ("a", 5), ("b", 1), ("a", 1), ("b", 9), ("a", 1), ("c", 1), ("a", 1)]


def test_capacity_rerun_stops_at_the_first_failure_with_the_option():
    stub = Stub()
    got, err = run(stub, RECS, stop_at_error=True)
    assert len(stub.pushes) == 2 and stub.pushes[1]["cap"] == 0
    assert stub.pushes[1]["offset"] == [0, 1, 3]         # key a's records before b's exception, not 5 and 7
    assert all(p["flags"] & N.BATCH_STOP_AT_ERROR for p in stub.pushes)
    assert err == (4, 4)
    assert got == [("a", [0]), ("b", [2]), ("a", [3])]


def test_capacity_rerun_is_unchanged_without_the_option():
    stub = Stub()
    got, err = run(stub, RECS)
    assert len(stub.pushes) == 2 and stub.pushes[1]["offset"] == [0, 1, 3, 5, 7]   # all of key a's records
    assert not any(p["flags"] & N.BATCH_STOP_AT_ERROR for p in stub.pushes)
    assert err == (4, 4)
    assert got == [("a", [0]), ("b", [2]), ("a", [3])]   # the same forwards and failure either way
