#!/usr/bin/env python3
"""A/B of a skip-till-next pattern on carry sessions: the follow path (CEP_SESSION_FOLLOW_CARRY) against the
general NFA path.

Usage: tools/follow_carry_ab.py [--events 10000000] [--batches 10] [--runs 5] [--passes 3]

A followedBy(next) B followedBy(next) C over C2's data shape (value = rng % 4, 100 records per key), resident in
HBM (CEP_MEM_DEVICE), pushed as `--batches` carry batches: every batch holds the next 100 / batches records of
every key (the last one the rest), so every key's walks wait across every cut.  One process, one library, two carry sessions on the same
columns: force_path = CEP_PATH_GENERAL and the follow-carry flag.  A pass is the `--batches` pushes from a cleared
state (cep_state_clear, untimed).  The two alternate, `--runs` runs each of `--passes` timed passes after one
warm-up pass.  One JSON line per run, then the ceiling -- one push of all the records on a follow session without
carry -- and a summary line: median and range of ms per pass for both, their ratio, whether the ranges overlap,
and whether match counts and checksums (summed over a pass's batches, one untimed pass each) agree."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tools")]


def main():
    from follow_ab import pattern
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "kafkastreams-cep_amd")]
    import torch
    from kcep import native as N, synth, Schema
    per_key = 100
    nk = max(1, a.events // per_key)
    n = a.events
    dev = torch.device("cuda:0")
    key, val, _ = synth.c2_stream_torch(n, nk, dev)      # grouped by key, ~100 records each
    # batch b: every key's records number [b * piece, (b + 1) * piece) (the last batch: the rest), grouped by key
    piece = per_key // a.batches
    first = torch.searchsorted(key, torch.arange(nk, dtype=torch.int32, device=dev))
    rank = torch.arange(n, device=dev) - first[key.long()]
    bid = torch.clamp(rank // piece, max=a.batches - 1)
    kb = [key[bid == b].contiguous() for b in range(a.batches)]
    vb = [val[bid == b].contiguous() for b in range(a.batches)]
    nb = max(len(k) for k in kb)
    del first, rank, bid
    cp = N.CompiledPattern(pattern().to_ir(Schema([("value", "i32")])))
    assert cp.follow[0], cp.follow[3]
    stream = torch.cuda.current_stream().cuda_stream
    sessions = {"general": N.Session(cp, nb, mode=N.MODE_NFA, carry=True, max_keys=nk, force_path=N.PATH_GENERAL),
                "follow": N.Session(cp, nb, mode=N.MODE_NFA, carry=True, max_keys=nk, follow_carry=True)}
    assert sessions["follow"].path == N.PATH_FOLLOW and sessions["general"].path == N.PATH_GENERAL

    def one_pass(s, check=False):
        s.state_clear()
        torch.cuda.synchronize()
        nm = csum = 0
        t0 = time.perf_counter()
        for b in range(a.batches):
            s.push(len(kb[b]), kb[b].data_ptr(), [vb[b].data_ptr()], mem=N.MEM_DEVICE, stream=stream)
            if check:
                m, c = s.checksum()
                nm, csum = nm + m, (csum + c) & (2 ** 64 - 1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, nm, csum

    rows = {tag: [] for tag in sessions}
    sums = {tag: one_pass(s, check=True)[1:] for tag, s in sessions.items()}   # (also the warm-up pass)
    for run in range(a.runs):
        for tag, s in sessions.items():
            ms = statistics.mean(one_pass(s)[0] for _ in range(a.passes))
            line = dict(run=run, session=tag, lib=N.lib().cep_version().decode(), events=n, batches=a.batches, path=s.path,
                        ms_per_pass=ms, matches=sums[tag][0], checksum=f"{sums[tag][1]:016x}")
            rows[tag].append(line)
            print(json.dumps(line), flush=True)
    # the ceiling: the same records in one push on a follow session without carry
    del sessions
    c = N.Session(cp, n, mode=N.MODE_NFA, follow=True)
    ceil = []
    for i in range(3 + a.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.push(n, key.data_ptr(), [val.data_ptr()], mem=N.MEM_DEVICE, stream=stream)
        torch.cuda.synchronize()
        if i >= 3:
            ceil.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(session="ceiling", events=n, path=c.path, ms_per_push=ceil, matches=c.checksum()[0])), flush=True)
    out = {"summary": "follow_carry_ab", "events": n, "batches": a.batches, "passes": a.passes}
    for tag, r in rows.items():
        v = [x["ms_per_pass"] for x in r]
        out[f"{tag}_median_ms"] = statistics.median(v)
        out[f"{tag}_range_ms"] = [min(v), max(v)]
    out["ceiling_median_ms"] = statistics.median(ceil)
    out["matches"] = sums["follow"][0]
    out["checksums_equal"] = sums["follow"] == sums["general"]
    out["ratio_general_over_follow"] = out["general_median_ms"] / out["follow_median_ms"]
    out["ranges_overlap"] = out["general_range_ms"][0] <= out["follow_range_ms"][1]
    print(json.dumps(out), flush=True)
    if not out["checksums_equal"]:
        sys.exit("match count or checksum differs between the two paths")


if __name__ == "__main__":
    main()
