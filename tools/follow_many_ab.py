#!/usr/bin/env python3
"""A/B of a skip-till-next pattern with a oneOrMore stage on the follow path (CEP_SESSION_FOLLOW_MANY) against
the general NFA path.

Usage: tools/follow_many_ab.py [--events 10000000] [--runs 5] [--steps 20] [--only many|general]

A followedBy(next) B+ followedBy(next) C over C2's data shape (value = rng % 4, 100 records per key), resident in
HBM (CEP_MEM_DEVICE), CEP_MODE_NFA.  One process, one library, two sessions on the same columns: force_path =
CEP_PATH_GENERAL and the follow-many flag.  The two alternate, `--runs` runs each of `--steps` timed pushes after 3
warm-ups.  One JSON line per run, then a summary line: median and range of ms per push for both, their ratio,
whether the ranges overlap, the match and entry counts, and whether the checksums agree.  Where the general path
hands keys back (CEP_E_RUN_CAPACITY in cep_batch_errors) or re-runs a batch with a grown pool
(cep_batch_attempts > 1), the run's line says so and the summary reports that instead of a ratio.  `--only` opens
and times one of the two alone (a profiler run of its kernels)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP = 3


def pattern():
    from kcep import QueryBuilder, Selected, Event
    v = Event.field("value")
    nxt = Selected.withSkipTilNextMatch
    return (QueryBuilder().select("a").where(v == 0).then().select("b", nxt()).oneOrMore().where(v == 1).then()
            .select("c", nxt()).where(v == 2).build())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", choices=["many", "general"])
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "kafkastreams-cep_amd")]
    import torch
    from kcep import native as N, synth, Schema
    n = a.events
    dev = torch.device("cuda:0")
    key, val, _ = synth.c2_stream_torch(n, max(1, n // 100), dev)
    cp = N.CompiledPattern(pattern().to_ir(Schema([("value", "i32")])))
    ok, k, nxt, many, ev, why = cp.follow_many
    assert ok and not ev, why
    stream = torch.cuda.current_stream().cuda_stream
    sessions = {}
    if a.only != "many":
        sessions["general"] = N.Session(cp, n, mode=N.MODE_NFA, force_path=N.PATH_GENERAL)
    if a.only != "general":
        sessions["many"] = N.Session(cp, n, mode=N.MODE_NFA, follow_many=True)
        assert sessions["many"].path == N.PATH_FOLLOW

    def timed(tag, steps):
        s = sessions[tag]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            s.push(n, key.data_ptr(), [val.data_ptr()], mem=N.MEM_DEVICE, stream=stream)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    rows = {tag: [] for tag in sessions}
    for tag in sessions:
        timed(tag, WARMUP)
    for run in range(a.runs):
        for tag, s in sessions.items():
            ms = timed(tag, a.steps)
            line = dict(run=run, session=tag, lib=N.lib().cep_version().decode(), n=n, path=s.path, ms_per_push=ms)
            if tag == "general":
                _, codes = s.batch_errors()
                line["attempts"] = s.attempts()
                line["handed_back"] = int((codes == N.E_RUN_CAPACITY).sum())
            else:
                line["kernel_ms"] = s.last_kernel_ms()
                line["batch_ms"] = s.last_batch_ms()
            if run == a.runs - 1:                        # (the checksum walks the whole CSR on the host: once per session)
                out = s.collect()
                nm, csum = s.checksum()
                line.update(matches=nm, entries=int(out["ent_off"][-1]) if nm else 0, checksum=f"{csum:016x}")
            rows[tag].append(line)
            print(json.dumps(line), flush=True)
    out = {"summary": "follow_many_ab", "events": n, "steps": a.steps, "slots": k}
    for tag, r in rows.items():
        v = [x["ms_per_push"] for x in r]
        out[f"{tag}_median_ms"] = statistics.median(v)
        out[f"{tag}_range_ms"] = [min(v), max(v)]
        out[f"{tag}_matches"] = r[-1]["matches"]
        out[f"{tag}_entries"] = r[-1]["entries"]
    if len(rows) == 2:
        g, f = rows["general"], rows["many"]
        out["checksums_equal"] = (g[-1]["matches"], g[-1]["entries"], g[-1]["checksum"]) == \
                                 (f[-1]["matches"], f[-1]["entries"], f[-1]["checksum"])
        out["general_attempts_max"] = max(x["attempts"] for x in g)
        out["general_handed_back_max"] = max(x["handed_back"] for x in g)
        if out["general_handed_back_max"] == 0:
            out["ratio_general_over_many"] = out["general_median_ms"] / out["many_median_ms"]
            out["ranges_overlap"] = out["general_range_ms"][0] <= out["many_range_ms"][1]
        if not out["checksums_equal"] and out["general_handed_back_max"] == 0:
            print(json.dumps(out), flush=True)
            sys.exit("match count, entry count or checksum differs between the two paths")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
