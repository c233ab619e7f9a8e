"""Speed of the warm-started sequence path on one GPU (seeded weights, 512x512 structured pairs, hipGraph replay, one sequence
in flight unless stated).

    python tools/bench_sequence.py [--rounds 5] [--frames 200] [--json OUT]
        pairs/s of: GraphedForward cold, twice (two objects: their difference is the spread two identical runs show in this very
        call); SequenceStitcher at iters = 12, 8, 6; three SequenceStitcher objects (iters = 12) on three streams.  All variants
        are timed in the same process, alternating round by round after a warm-up; the median round is reported.  The iters = 8 and
        6 rows are THROUGHPUT only: with seeded weights nothing can be said about the flow's quality at fewer iterations.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/bench_sequence.py --kernels-only
        200 launches of the splat kernel on the two low-res flows of one pair ([2,2,64,64]) in each layout, nothing else timed;
    python tools/bench_sequence.py --report-kernels DIR/.../k_kernel_stats.csv [--json OUT]
        the kernel's average duration against the 10 ms host path it replaces and the 12.1 ms of kernels per pair.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOST_PATH_MS = 10.0            # the reference's forward_interpolate for one 64x64 field on the CPU (two scipy griddata calls)
KERNELS_PER_PAIR_MS = 12.1     # sum of kernel durations of one graphed pair (profiles/r6_kernel_summary.txt)
SHIFTS = ((5, -9), (6, -10), (7, -11))


def _model():
    import stitch_amd
    from oracle import spec
    cfg, _ = stitch_amd.load_inference_config("all_img1_with_inpaint_g12_transRef")
    m = stitch_amd.build_model(cfg)
    m.load_state_dict(spec.seeded_state_dict(1234), strict=True)
    return m.cuda().eval()


def bench(rounds, frames):
    import numpy as np
    import torch
    import stitch_amd
    from oracle import inputs
    model = _model()
    pairs = [tuple(t.cuda() for t in inputs.structured_pair(512, 512, seed=7, shift=s)) for s in SHIFTS]
    seq3 = [stitch_amd.SequenceStitcher(model, graphed=True) for _ in range(3)]
    streams = [torch.cuda.Stream() for _ in range(3)]

    def one(fn):
        def run(n):
            for i in range(n):
                fn(*pairs[i % len(pairs)])
            return n
        return run

    def three(n):
        for i in range(n):
            for s, q in zip(streams, seq3):
                with torch.cuda.stream(s):
                    q(*pairs[i % len(pairs)])
        return 3 * n

    variants = {"cold_a": one(model.graphed("test_eval")), "cold_b": one(model.graphed("test_eval"))}
    for it in (12, 8, 6):
        variants[f"sequence_iters{it}"] = one(stitch_amd.SequenceStitcher(model, iters=it, graphed=True))
    variants["sequence_iters12_x3_streams"] = three

    def timed(run, n):
        for s in streams:
            s.wait_stream(torch.cuda.current_stream())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = run(n)
        torch.cuda.synchronize()
        return done / (time.perf_counter() - t0)

    with torch.no_grad():
        for run in variants.values():
            timed(run, 3)                                   # captures
        per = {k: [] for k in variants}
        for _ in range(rounds):
            for k, run in variants.items():
                per[k].append(timed(run, frames if run is not three else max(1, frames // 3)))
    med = {k: float(np.median(v)) for k, v in per.items()}
    ms = {k: 1e3 / v for k, v in med.items()}
    return {"pairs_per_s": med, "ms_per_pair": ms, "rounds_pairs_per_s": per,
            "cold_spread_ms": abs(ms["cold_a"] - ms["cold_b"]),
            "warm12_minus_cold_ms": ms["sequence_iters12"] - min(ms["cold_a"], ms["cold_b"]),
            "device": torch.cuda.get_device_name(0),
            "method": f"median of {rounds} alternating rounds of {frames} frames each after a warm-up, one process; seeded weights, so the "
                      "iters = 8 / 6 rows are throughput only"}


def kernels_only():
    import torch
    import stitch_amd
    ops = stitch_amd.ops
    g = torch.Generator(device="cuda").manual_seed(0)
    flow = (torch.rand(2, 2, 64, 64, device="cuda", generator=g) - 0.5) * 6
    grid = torch.empty(2 * 4096, 2, device="cuda")
    ops.coords_grid(grid, 2, 64, 64)
    rows = (grid + flow.reshape(2, 2, 4096).permute(0, 2, 1).reshape(-1, 2)).contiguous()
    out = torch.empty_like(flow)
    for _ in range(200):
        ops.forward_interpolate(flow, out=out)
    for _ in range(200):
        ops.forward_interpolate(rows, out=out, coords_rows=(2, 64, 64))
    torch.cuda.synchronize()
    print("launched the splat kernel 200 x NCHW + 200 x coords1 rows, [2,2,64,64]")


def report_kernels(stats_csv):
    rep = {}
    for r in csv.DictReader(open(stats_csv)):
        if "flow_forward_interpolate_kernel" not in r["Name"]:
            continue
        layout = "coords1_rows" if "ILb1E" in r["Name"] or "<true>" in r["Name"] else "nchw"
        us = float(r["AverageNs"]) / 1e3
        rep[layout] = dict(calls=int(r["Calls"]), avg_us=us, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3,
                           frac_of_kernels_per_pair=us / (KERNELS_PER_PAIR_MS * 1e3), host_path_over_kernel=HOST_PATH_MS * 1e3 / us)
    return rep


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--report-kernels", default=None)
    args = ap.parse_args()
    if args.report_kernels:
        res = report_kernels(args.report_kernels)
    elif args.kernels_only:
        kernels_only()
        res = None
    else:
        res = bench(args.rounds, args.frames)
    if res is not None:
        print(json.dumps(res, indent=1))
        if args.json:
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
