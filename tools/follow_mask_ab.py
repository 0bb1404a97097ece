#!/usr/bin/env python3
"""Three-way A/B of a skip-till-next pattern over two fields: the general NFA path, the follow path's evaluated
form (CEP_SESSION_MASK_PASS | CEP_SESSION_FOLLOW: one streaming kernel from the columns to the bitmaps), and the
same session split in two launches (KCEP_FOLLOW_MASK_SPLIT=1: the mask pre-pass into a column, follow_bits over it).

Usage: tools/follow_mask_ab.py [--events 10000000] [--runs 5] [--steps 20] [--general-steps N]
                               [--only general|fused|split] [--no-general] [--carry [--batches 10] [--passes 3]]

FM2 -- s0: price >= 0 && price + volume == 3; followedBy s1: price <= volume && volume - price <= 1; followedBy
s2: price > 1 || volume > 1 -- over C2's key shape (100 records per key), two i64 fields uniform in 0..3, resident
in HBM (CEP_MEM_DEVICE), CEP_MODE_NFA.  One process, one library, three sessions on the same columns; they
alternate, `--runs` runs each of `--steps` timed pushes after a warm-up push.  One JSON line per run, then a
summary: median and range of ms per push for each, the ratios general / fused and split / fused, whether the
ranges overlap, and whether match counts and checksums agree (they must).  `--only` opens and times one session
alone (a profiler run of its kernels).  `--carry`: the ten-batch pass of tools/follow_carry_ab.py on carry sessions
(every batch the next tenth of every key's records), ms per pass."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pattern():
    from kcep import QueryBuilder, Selected, Event
    p, v = Event.field("price"), Event.field("volume")
    nxt = Selected.withSkipTilNextMatch
    return (QueryBuilder().select("s0").where((p >= 0) & (p + v == 3)).then()
            .select("s1", nxt()).where((p <= v) & (v - p <= 1)).then()
            .select("s2", nxt()).where((p > 1) | (v > 1)).build())


def bytes_per_record(k=3, widths=(8, 8)):
    """what the fused kernel moves per record: the key, the columns read, (k + 1) / 8 of bitmap"""
    return 4 + sum(widths) + (k + 1) / 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--general-steps", type=int, default=0, help="timed pushes of the general session (default: --steps)")
    ap.add_argument("--only", choices=["general", "fused", "split"])
    ap.add_argument("--no-general", action="store_true", help="the two follow sessions alone (a kernel trace of both)")
    ap.add_argument("--carry", action="store_true")
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "kafkastreams-cep_amd")]
    import torch
    from kcep import native as N, synth, Schema
    n, per_key = a.events, 100
    nk = max(1, n // per_key)
    dev = torch.device("cuda:0")
    key, _, _ = synth.c2_stream_torch(n, nk, dev)        # grouped by key, ~100 records each
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    cols = [torch.randint(0, 4, (n,), dtype=torch.int64, device=dev, generator=g) for _ in range(2)]
    cp = N.CompiledPattern(pattern().to_ir(Schema([("price", "i64"), ("volume", "i64")])))
    assert cp.follow_mask[0], cp.follow_mask[3]
    stream = torch.cuda.current_stream().cuda_stream
    if a.carry:                                          # batch b: every key's records [b * piece, (b + 1) * piece)
        piece = per_key // a.batches
        first = torch.searchsorted(key, torch.arange(nk, dtype=torch.int32, device=dev))
        rank = torch.arange(n, device=dev) - first[key.long()]
        bid = torch.clamp(rank // piece, max=a.batches - 1)
        kb = [key[bid == b].contiguous() for b in range(a.batches)]
        cb = [[c[bid == b].contiguous() for c in cols] for b in range(a.batches)]
        del first, rank, bid
    else:
        kb, cb = [key], [cols]
    cap = max(len(k) for k in kb)
    kw = dict(mode=N.MODE_NFA, **(dict(carry=True, max_keys=nk) if a.carry else {}))
    flag = dict(follow_carry=True) if a.carry else dict(follow=True)

    def open_session(tag):
        if tag == "general":                             # (what the parent commit opens for this pattern)
            return N.Session(cp, cap, force_path=N.PATH_GENERAL, **kw)
        if tag == "split":
            os.environ["KCEP_FOLLOW_MASK_SPLIT"] = "1"   # read at session open
        try:
            s = N.Session(cp, cap, mask_pass=True, **flag, **kw)
        finally:
            os.environ.pop("KCEP_FOLLOW_MASK_SPLIT", None)
        assert s.path == N.PATH_FOLLOW and s.jit
        return s

    sessions = {tag: open_session(tag) for tag in ("general", "fused", "split")
                if a.only in (None, tag) and not (a.no_general and tag == "general")}

    def one_pass(s, check=False):
        """the batches once (from a cleared state on carry sessions): ms, matches and checksum summed over them"""
        if a.carry:
            s.state_clear()
        torch.cuda.synchronize()
        nm = csum = 0
        t0 = time.perf_counter()
        for k, c in zip(kb, cb):
            s.push(len(k), k.data_ptr(), [x.data_ptr() for x in c], mem=N.MEM_DEVICE, stream=stream)
            if check:
                m, h = s.checksum()
                nm, csum = nm + m, (csum + h) & (2 ** 64 - 1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, nm, csum

    sums = {tag: one_pass(s, check=True)[1:] for tag, s in sessions.items()}   # (also the warm-up)
    reps = a.passes if a.carry else a.steps
    rows = {tag: [] for tag in sessions}
    for run in range(a.runs):
        for tag, s in sessions.items():
            r = a.general_steps if tag == "general" and a.general_steps and not a.carry else reps
            ms = statistics.mean(one_pass(s)[0] for _ in range(r))
            line = dict(run=run, session=tag, lib=N.lib().cep_version().decode(), events=n, carry=a.carry,
                        batches=len(kb), path=s.path, ms=ms, matches=sums[tag][0], checksum=f"{sums[tag][1]:016x}")
            if tag != "general":
                line["kernel_ms"] = s.last_kernel_ms()    # (the last batch's bitmap kernel or kernels)
            else:                                         # keys handed back (CEP_E_RUN_CAPACITY) make its result partial
                line["attempts"] = s.attempts()
                line["handed_back"] = int((s.batch_errors()[1] == N.E_RUN_CAPACITY).sum())
            rows[tag].append(line)
            print(json.dumps(line), flush=True)
    out = {"summary": "follow_mask_ab", "events": n, "carry": a.carry, "batches": len(kb), "reps": reps,
           "unit": "ms per pass" if a.carry else "ms per push", "fused_bytes_per_record": bytes_per_record()}
    for tag, r in rows.items():
        v = [x["ms"] for x in r]
        out[f"{tag}_median_ms"] = statistics.median(v)
        out[f"{tag}_range_ms"] = [min(v), max(v)]
        if tag != "general":
            out[f"{tag}_kernel_ms"] = statistics.median(x["kernel_ms"] for x in r)
    handed = max([x["handed_back"] for x in rows.get("general", [])] or [0])
    out["general_handed_back_max"] = handed
    cmp = {tag: v for tag, v in sums.items() if tag != "general" or not handed} or sums
    out["matches"] = next(iter(cmp.values()))[0]
    out["checksums_equal"] = len(set(cmp.values())) == 1
    if "fused" in rows:
        for tag in ("general", "split"):
            if tag in rows:
                out[f"ratio_{tag}_over_fused"] = out[f"{tag}_median_ms"] / out["fused_median_ms"]
                lo = max(out[f"{tag}_range_ms"][0], out["fused_range_ms"][0])
                out[f"{tag}_ranges_overlap"] = lo <= min(out[f"{tag}_range_ms"][1], out["fused_range_ms"][1])
    print(json.dumps(out), flush=True)
    if not out["checksums_equal"]:
        sys.exit("match count or checksum differs between the sessions")


if __name__ == "__main__":
    main()
