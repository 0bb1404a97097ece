"""Where a processor flush's fixed cost goes: a C2-shaped stream pushed from host memory through a
CEP_SESSION_CARRY session in batches of `per` records, each collected (GpuCEPProcessor.flush's
cep_push_batch + cep_collect), with the host-side time of the push call and of the collect call
split, for pinned and for pageable (plain numpy) host input.

Usage: flush_probe.py [--filter] [per=65536] [batches=200]
The "C loop" lines run the same loop in C (tools/flush_loop.c, built here with gcc): the C-ABI's own
cost per flush, without Python in the loop, as the JNI shim sees it.
Run under `rocprofv3 --kernel-trace --memory-copy-trace --marker-trace --stats` with KCEP_ROCTX=1
for the device-side split.

--filter: only the C loops over arrival-order flushes from pinned memory, serial and pipelined, with an
offset column -- what CEP_BATCH_FILTER costs.  Per library (KCEP_LIB picks another build, e.g. the parent
commit's) one line per variant:
  monotone   the pre-filtered stream with CEP_BATCH_OFFSETS_MONOTONE (any build)
  filter     the same stream with CEP_BATCH_FILTER: nothing to drop
  dirty      that stream with 5 % re-deliveries and 5 % null records, CEP_BATCH_FILTER
and the host cost the flag removes: kcep/processor.py's mark loop over one flush's records.  A driver that
alternates builds takes the spread; every line names the library's build id."""
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kafkastreams-cep_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from kcep import native as N, synth, Schema  # noqa: E402

FILTER_MODE = "--filter" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--filter"]
per = int(argv[0]) if len(argv) > 0 else 1 << 16
nb = int(argv[1]) if len(argv) > 1 else 200
n = per * nb
K = max(1000, n // 100)
dev = torch.device("cuda", 0)
key, val, order = synth.c2_stream_torch(n, K, dev)
# the same records in arrival (generation) order: keys interleaved, for CEP_BATCH_ARRIVAL_ORDER
akey, aval = torch.empty_like(key), torch.empty_like(val)
akey[order] = key
aval[order] = val
ak, av = akey.cpu().pin_memory(), aval.cpu().pin_memory()
ir = synth.c2_pattern().to_ir(Schema([("value", "i32")]))
pat = N.CompiledPattern(ir)
st = torch.cuda.current_stream(dev)
pk, pv = key.cpu().pin_memory(), val.cpu().pin_memory()
hk, hv = key.cpu().numpy().copy(), val.cpu().numpy().copy()
want = None


def build_flush_loop():
    so = os.path.join("/tmp", "libflush_loop_%d.so" % os.getpid())
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "flush_loop.c"),
                    "-I", os.path.join(ROOT, "include"), "-L", os.path.dirname(N.LIB_PATH), "-l:" + os.path.basename(N.LIB_PATH),
                    "-Wl,-rpath," + os.path.dirname(N.LIB_PATH)], check=True)
    fl = C.CDLL(so)
    for f in (fl.flush_loop, fl.flush_loop_pipelined):
        f.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                      C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
    return so, fl


def filter_mode():
    so, fl = build_flush_loop()
    build = N.lib().cep_version().decode()
    has_filter = hasattr(N.lib(), "cep_filter_tile_records")
    rng = np.random.default_rng(1)
    k_np, v_np = akey.cpu().numpy(), aval.cpu().numpy()
    off = np.arange(n, dtype=np.int64)                   # arrival index: increasing per key
    # the dirty stream: 5 % of the records deliver their key's previous record again, 5 % are null
    order_k = np.argsort(k_np, kind="stable")
    prev = np.full(n, -1, np.int64)
    same = k_np[order_k[1:]] == k_np[order_k[:-1]]
    prev[order_k[1:][same]] = order_k[:-1][same]
    re = np.flatnonzero((rng.random(n) < 0.05) & (prev >= 0))
    dv, do = v_np.copy(), off.copy()
    dv[re], do[re] = v_np[prev[re]], off[prev[re]]
    dvalid = (rng.random(n) >= 0.05).astype(np.uint8)
    pin = lambda a: torch.from_numpy(a).pin_memory()
    p_off, p_dv, p_do, p_dvalid = pin(off), pin(dv), pin(do), pin(dvalid)
    A = N.BATCH_ARRIVAL_ORDER | N.BATCH_DELIVER
    variants = [("monotone", av, p_off, None, A | N.BATCH_OFFSETS_MONOTONE)]
    if has_filter:
        variants += [("filter", av, p_off, None, A | N.BATCH_FILTER), ("dirty", p_dv, p_do, p_dvalid, A | N.BATCH_FILTER)]
    for label, vals, offs, valid, flags in variants:
        for how, loop in (("serial", fl.flush_loop), ("pipelined", fl.flush_loop_pipelined)):
            s = N.Session(pat, per, mode=N.MODE_PROCESSOR, carry=True, max_keys=K)
            s.set_timing(False)
            best = None
            for _ in range(4):                               # (the first pass warms up)
                s.state_clear()
                torch.cuda.synchronize()
                o = (C.c_double * 4)()
                rc = loop(s.h, nb, per, ak.data_ptr(), vals.data_ptr(), flags, st.cuda_stream, o, offs.data_ptr(),
                          valid.data_ptr() if valid is not None else None)
                assert rc == 0, (rc, N.lib().cep_last_error())
                if best is None or o[0] < best[0]:
                    best = list(o)
            dt, tp, tc, tot = best
            print(f"filter-probe build={build} {label:8s} {how:9s} per={per} batches={nb}: {dt / nb:8.1f} us/batch  "
                  f"push {tp / nb:7.1f}  collect {tc / nb:7.1f}  matches {int(tot)}", flush=True)
            s.close()
    os.unlink(so)
    # the host's side of the rule, as GpuCEPProcessor.flush applies it without device_filter: one flush's records
    recs = [(int(k), None, 0, 0, int(o)) for k, o in zip(k_np[:per], do[:per])]
    best = None
    for _ in range(5):
        hwm, kept, arrival = {}, [], []
        t0 = time.perf_counter()
        for i, r in enumerate(recs):
            hk = (r[0], r[2])
            if r[4] < hwm.get(hk, -1):
                continue
            hwm[hk] = r[4] + 1
            kept.append(r)
            arrival.append(i)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    print(f"filter-probe host mark loop (processor.py flush) per={per}: {best * 1e6:9.1f} us/flush  kept {len(kept)}", flush=True)


if FILTER_MODE:
    filter_mode()
    sys.exit(0)


def one_pass(sess, k_ptr, v_ptr):
    tp = tc = 0.0
    tot = 0
    for i in range(nb):
        a = i * per
        t0 = time.perf_counter()
        sess.push(per, k_ptr + 4 * a, [v_ptr + 4 * a], mem=N.MEM_HOST, stream=st.cuda_stream,
                  flags=N.BATCH_OFFSETS_MONOTONE | N.BATCH_DELIVER)
        t1 = time.perf_counter()
        out = sess.collect()
        t2 = time.perf_counter()
        tp += t1 - t0
        tc += t2 - t1
        tot += len(out["match_record"])
    return tp, tc, tot


for label, kp, vp in (("pinned", pk.data_ptr(), pv.data_ptr()), ("pageable", hk.ctypes.data, hv.ctypes.data)):
    s = N.Session(pat, per, mode=N.MODE_PROCESSOR, carry=True, max_keys=K)
    s.set_timing(False)
    one_pass(s, kp, vp)
    best = None
    for _ in range(3):
        s.state_clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tp, tc, tot = one_pass(s, kp, vp)
        dt = time.perf_counter() - t0
        if best is None or dt < best[0]:
            best = (dt, tp, tc, tot)
    dt, tp, tc, tot = best
    want = tot if want is None else want
    print(f"{label:9s} per={per} batches={nb}: {dt / nb * 1e6:8.1f} us/batch  push {tp / nb * 1e6:7.1f}  "
          f"collect {tc / nb * 1e6:7.1f}  {n / dt:.3e} events/s  matches {tot} (same: {tot == want})", flush=True)
    s.close()


so, fl = build_flush_loop()
A = N.BATCH_ARRIVAL_ORDER
for label, kp, vp, xf, loop in (("pinned", pk.data_ptr(), pv.data_ptr(), 0, fl.flush_loop),
                                ("pageable", hk.ctypes.data, hv.ctypes.data, 0, fl.flush_loop),
                                ("pinned arrival", ak.data_ptr(), av.data_ptr(), A, fl.flush_loop),
                                ("pinned arrival pipelined", ak.data_ptr(), av.data_ptr(), A, fl.flush_loop_pipelined),
                                ("pinned grouped pipelined", pk.data_ptr(), pv.data_ptr(), 0, fl.flush_loop_pipelined)):
    s = N.Session(pat, per, mode=N.MODE_PROCESSOR, carry=True, max_keys=K)
    s.set_timing(False)
    best = None
    for _ in range(4):
        s.state_clear()
        torch.cuda.synchronize()
        o = (C.c_double * 4)()
        rc = loop(s.h, nb, per, kp, vp, N.BATCH_OFFSETS_MONOTONE | N.BATCH_DELIVER | xf, st.cuda_stream, o, None, None)
        assert rc == 0, rc
        if best is None or o[0] < best[0]:
            best = list(o)
    dt, tp, tc, tot = best
    print(f"C loop {label:25s} per={per} batches={nb}: {dt / nb:8.1f} us/batch  push {tp / nb:7.1f}  "
          f"collect {tc / nb:7.1f}  {n / (dt * 1e-6):.3e} events/s  matches {int(tot)} (same: {int(tot) == want})",
          flush=True)
    s.close()
os.unlink(so)
