"""Selectivity sweep of the plain stencil kernel's key reads (csrc/stencil_kernel.h window_same_keys).

100M events, 1M keys (100 events each, grouped), values uniform in 0..99, the 3-stage strict pattern
value < t: a record is a candidate (three consecutive values below t) with density (t/100)^3.  At each
density the resident batch is pushed --steps times under HIP events, --reps times per mode; the modes
are the launch modes of the library in use (KCEP_STENCIL_SPARSE_KEYS / KCEP_STENCIL_DENSE_KEYS /
neither).  With --modes lib the flags are left alone: that is the row of an older build selected with
KCEP_LIB, which has one mode.  One JSON line per density and mode; the match counts of all lines at a
density must agree (checked within the run, and comparable across runs by "matches").

usage: python tools/stencil_sweep.py [--modes sparse,dense,adaptive | --modes lib] [--tag NAME] [--thresholds 0,25,100]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kafkastreams-cep_amd"))

# t and the density (t/100)^3 it gives: 0, 1e-3, 1/64, ~1/16, 1/8, ~1/4, ~1/2, 1
THRESHOLDS = [0, 10, 25, 40, 50, 63, 79, 100]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=100_000_000)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", default="sparse,dense,adaptive")
    ap.add_argument("--tag", default="new")
    ap.add_argument("--thresholds", type=lambda x: [int(v) for v in x.split(",") if v], default=THRESHOLDS,
                    help="the values of t to run (default: all eight)")
    args = ap.parse_args()

    import torch
    from kcep import native as N
    from kcep import Schema, QueryBuilder, Event

    n = args.events
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    key = (torch.arange(n, device=dev, dtype=torch.int64) // (n // args.keys)).to(torch.int32)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    val = torch.randint(0, 100, (n,), device=dev, dtype=torch.int32, generator=g)
    build = N.lib().cep_version().decode().rsplit(" ", 1)[-1]
    sch = Schema([("value", "i32")])
    for t in args.thresholds:
        q = (QueryBuilder().select("a").where(Event.value() < t).then().select("b").where(Event.value() < t)
             .then().select("c").where(Event.value() < t).build())
        sess = N.Session(N.CompiledPattern(q.to_ir(sch)), n, mode=N.MODE_PROCESSOR)
        assert sess.path == N.PATH_STENCIL
        sess.set_timing(False)
        counts = set()
        for mode in args.modes.split(","):
            if mode != "lib":
                os.environ["KCEP_STENCIL_SPARSE_KEYS"] = "1" if mode == "sparse" else "0"
                os.environ["KCEP_STENCIL_DENSE_KEYS"] = "1" if mode == "dense" else "0"

            def step():
                sess.push(n, key.data_ptr(), [val.data_ptr()], mem=N.MEM_DEVICE, stream=stream.cuda_stream)

            for _ in range(args.warmup):
                step()
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.steps):
                    step()
                e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / args.steps)
            nm, cs = sess.checksum()
            counts.add((nm, cs))
            print(json.dumps({"tag": args.tag, "build": build, "t": t, "density": round((t / 100) ** 3, 6),
                              "mode": mode, "ms_per_step": [round(x, 4) for x in sorted(ms)], "matches": nm,
                              "checksum": f"{cs:016x}"}), flush=True)
        assert len(counts) == 1, f"modes disagree at t={t}: {counts}"
        del sess


if __name__ == "__main__":
    main()
