#!/usr/bin/env python3
"""A/B of a two-field strict pattern (P2) with and without CEP_SESSION_MASK_PASS.

Usage: tools/mask_pass_ab.py OLD_SO [--events 10000000] [--big 100000000] [--runs 5]

P2 = three strict stages over (price i64, volume i64), each `where` reading both fields, resident in HBM
(CEP_MEM_DEVICE) with C2's key and order shape (100 events per key).  Alternating in one call, a fresh
process per run (a process loads one libkcep.so): OLD_SO on its automatic path against this tree's
library with the flag, `--runs` runs each of 20 timed pushes after 5 warm-ups at `--events` records; then
the new library with the flag alone at `--big` records.  One JSON line per run, then a summary line with
the medians, ranges and the ratio; match count and cep_checksum must agree between the two libraries.
A run that fails ends the call (nothing more is started on the device)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 20, 5


def p2():
    from kcep import QueryBuilder, Event
    price, volume = Event.field("price"), Event.field("volume")
    return (QueryBuilder().select("s0").where((price >= 0) & (price + volume == 3)).then()
            .select("s1").where((price <= volume) & (volume - price <= 1)).then()
            .select("s2").where((price > 1) | (volume > 1)).build())


def child(n, mask_pass, interpret):
    sys.path[:0] = [os.path.join(ROOT, "kafkastreams-cep_amd")]
    import torch
    from kcep import native as N, synth, Schema
    dev = torch.device("cuda:0")
    K = max(1, n // 100)
    key, pri, _ = synth.c2_stream_torch(n, K, dev)
    _, vol, _ = synth.c2_stream_torch(n, K, dev, val_seed=0xB0B)
    pri, vol = pri.to(torch.int64), vol.to(torch.int64)
    cp = N.CompiledPattern(p2().to_ir(Schema([("price", "i64"), ("volume", "i64")])))
    s = N.Session(cp, n, mask_pass=mask_pass, interpret=interpret)
    stream = torch.cuda.current_stream().cuda_stream

    def step():
        s.push(n, key.data_ptr(), [pri.data_ptr(), vol.data_ptr()], mem=N.MEM_DEVICE, stream=stream)

    for _ in range(WARMUP):
        step()
    torch.cuda.synchronize()
    fast = s.path in (N.PATH_STENCIL, N.PATH_CHAIN)
    if fast:
        s.set_timing(False)                      # no event packets in the timed pushes
    t0 = time.perf_counter()
    for _ in range(STEPS):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / STEPS
    nm, csum = s.checksum()
    line = dict(lib=N.lib().cep_version().decode(), n=n, path=s.path, jit=s.jit, mask_pass=mask_pass,
                ms_per_push=ms, matches=nm, checksum=f"{csum:016x}")
    if fast:                                     # the split under HIP events: batch = pre-pass + stencil, kernel = stencil
        s.set_timing(True)
        kb = []
        for _ in range(STEPS):
            step()
            kb.append((s.last_kernel_ms(), s.last_batch_ms()))
        line["kernel_ms"] = statistics.median(k for k, _ in kb)
        line["batch_ms"] = statistics.median(b for _, b in kb)
    print(json.dumps(line), flush=True)


def spawn(lib, n, mask_pass, interpret=False):
    env = dict(os.environ)
    if lib:
        env["KCEP_LIB"] = lib
    else:
        env.pop("KCEP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n)] + (["--mask-pass"] if mask_pass else []) + \
          (["--interpret"] if interpret else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(f"run failed (rc {r.returncode}): nothing more is started")
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def summary(tag, rows):
    v = [r["ms_per_push"] for r in rows]
    return {f"{tag}_median_ms": statistics.median(v), f"{tag}_range_ms": [min(v), max(v)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old_so", nargs="?")
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--big", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--mask-pass", action="store_true")
    ap.add_argument("--interpret", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.mask_pass, a.interpret)
    if not a.old_so:
        ap.error("OLD_SO is required")
    old, new, big = [], [], []
    for _ in range(a.runs):
        old.append(spawn(os.path.abspath(a.old_so), a.events, False))
        new.append(spawn(None, a.events, True))
        if (old[-1]["matches"], old[-1]["checksum"]) != (new[-1]["matches"], new[-1]["checksum"]):
            sys.exit("match count or checksum differs between the two libraries")
    interp = spawn(None, a.events, True, interpret=True)
    for _ in range(a.runs if a.big else 0):
        big.append(spawn(None, a.big, True))
    s = {"summary": "mask_pass_ab", "events": a.events, **summary("old", old), **summary("new", new),
         "old_path": old[0]["path"], "new_path": new[0]["path"], "matches": new[0]["matches"],
         "checksum": new[0]["checksum"], "interpreted_ms": interp["ms_per_push"]}
    s["ratio_old_over_new"] = s["old_median_ms"] / s["new_median_ms"]
    if big:
        s.update(big_events=a.big, **summary("big", big))
    print(json.dumps(s), flush=True)


if __name__ == "__main__":
    main()
