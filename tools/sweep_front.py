"""The two frame-table fronts (k_scan + k_scan_chunks + k_compact against k_hop) over the shapes
that decide HOP_MAX_FRAMES and HOP_MIN_STREAMS (zflac_amd/csrc/common.h): C5-style streams
(stereo 16-bit mid/side LPC-8, block 4,096), `--inflight` runs in flight as bench.py keeps them.

  frames sweep   frames per stream over --frames at constant total samples (1,250 x 32 frames)
  streams sweep  streams per batch over --streams at 32 frames per stream
  cells          any other --cells STREAMSxFRAMES

Each cell: ms per run of the same batches with the front forced to scan and to hop, alternating,
`--reps` times each, best and median. Prints one JSON object; --out also writes it.
Usage: python tools/sweep_front.py [--steps 40] [--reps 3] [--out profiles/x.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOTAL_FRAMES = 1250 * 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="8,32,128,512")
    ap.add_argument("--streams", default="16,64,256,1250")
    ap.add_argument("--cells", default="", help="further cells, STREAMSxFRAMES, comma-separated")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--out")
    args = ap.parse_args()
    os.environ.setdefault("ZFLAC_RUN_STREAMS", str(args.inflight))
    os.environ["ZFLAC_HOP_MAX_FRAMES"] = "1000000"  # the sweep decides the limits: none while it runs
    import synth
    import zflac_amd
    from zflac_amd import _lib

    def shard(frames, n):
        distinct = min(n, 1250)
        sts = [s.flac for s in synth.generate_many([synth.config_c5(i, n_frames=frames) for i in range(distinct)])]
        return [sts[i % distinct] for i in range(n)]

    def ms_per_run(batches, steps):
        pending = [False] * len(batches)
        t0 = time.perf_counter()
        for i in range(steps):
            j = i % len(batches)
            if pending[j]:
                batches[j].wait()
            batches[j].submit()
            pending[j] = True
        for j, p in enumerate(pending):
            if p:
                batches[j].wait()
        return (time.perf_counter() - t0) / steps * 1e3

    def cell(streams):
        sets = {f: [zflac_amd.Batch(streams, front=f) for _ in range(args.inflight)] for f in ("scan", "hop")}
        want = {"scan": _lib.FRONT_SCAN, "hop": _lib.FRONT_HOP}
        times = {"scan": [], "hop": []}
        for f, bs in sets.items():
            ms_per_run(bs, args.steps)  # warm
            assert all(b.front() == (want[f], want[f]) for b in bs), (f, bs[0].front())
        for _ in range(args.reps):
            for f, bs in sets.items():
                times[f].append(ms_per_run(bs, args.steps))
        for bs in sets.values():
            for b in bs:
                b.close()
        row = {f: {"best": round(min(t), 4), "median": round(statistics.median(t), 4)} for f, t in times.items()}
        row["hop_over_scan"] = round(row["hop"]["median"] / row["scan"]["median"], 4)
        return row

    out = {"build_id": zflac_amd.build_id(), "steps": args.steps, "reps": args.reps, "inflight": args.inflight,
           "unit": "ms per run", "frames_sweep": {}, "streams_sweep": {}, "cells": {}}
    for fr in [int(x) for x in args.frames.split(",") if x]:
        n = max(1, TOTAL_FRAMES // fr)
        out["frames_sweep"][f"{fr} frames x {n} streams"] = cell(shard(fr, n))
        print(fr, out["frames_sweep"][f"{fr} frames x {n} streams"], file=sys.stderr, flush=True)
    base = shard(32, 1250)
    for n in [int(x) for x in args.streams.split(",") if x]:
        out["streams_sweep"][f"{n} streams x 32 frames"] = cell(base[:n])
        print(n, out["streams_sweep"][f"{n} streams x 32 frames"], file=sys.stderr, flush=True)
    for c in [x for x in args.cells.split(",") if x]:  # e.g. 768x64: the corner of the auto rule
        n, fr = (int(v) for v in c.split("x"))
        out["cells"][f"{n} streams x {fr} frames"] = cell(shard(fr, n))
        print(c, out["cells"][f"{n} streams x {fr} frames"], file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
