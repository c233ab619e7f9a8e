"""Speed of FlowHomoAdpater's branches on one GPU (seeded weights, structured pairs).

    python tools/bench_branches.py [--rounds 5] [--iters 20] [--json OUT]
        graphed test_eval pairs/s: shipped, only_homo, use_combine_h_flow (mask off);
        GraphedTestOut launch + finish ms per pair: consistency mask on vs off, at 512x512 and 1024x1024.
        The variants of one table are timed in the same process, alternating round by round after a warm-up; the median
        round is reported.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/bench_branches.py --kernels-only
        200 launches of st_homo_flow_warp (B=1 and B=8 at 512x512) and st_blend_plain (1024x1024 canvas), nothing else timed;
    python tools/bench_branches.py --report-kernels DIR/.../k_kernel_stats.csv
        average kernel time against bytes moved / 6.3 TB/s (MI355X HBM peak): both kernels are HBM-bound, one pixel per lane.
"""
from __future__ import annotations

import argparse
import contextlib
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3
# bytes per pixel: homo_flow_warp reads flow (8) + image 2 (12, the 4 taps mostly hit cache) and writes 6 channels (24) +
# overlap (4); blend_plain reads homo1 / homo2 / fin (3 x 24) and writes output2, mask1, mask2 (3 x 12) + the uint8 blend (3)
BYTES_PER_PX = {"homo_flow_warp_kernel": 48, "blend_plain_kernel": 111}
KERNEL_CASES = (("homo_flow_warp_kernel", 1, 512, 512), ("homo_flow_warp_kernel", 8, 512, 512), ("blend_plain_kernel", 1, 1024, 1024))


@contextlib.contextmanager
def flags(model, **kw):
    old = {k: getattr(model.cfg, k) for k in kw}
    for k, v in kw.items():
        setattr(model.cfg, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(model.cfg, k, v)


def _model():
    import stitch_amd
    from oracle import spec
    cfg, _ = stitch_amd.load_inference_config("all_img1_with_inpaint_g12_transRef")
    m = stitch_amd.build_model(cfg)
    m.load_state_dict(spec.seeded_state_dict(1234), strict=True)
    return m.cuda().eval()


def _time(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def _alternate(variants, rounds, iters):
    """variants: {name: (flag dict, fn)}; warm-up (captures) then `rounds` rounds of `iters` calls each, alternating."""
    import numpy as np
    for name, (kw, fn) in variants.items():
        with flags(MODEL, **kw):
            _time(fn, 3)
    per = {name: [] for name in variants}
    for _ in range(rounds):
        for name, (kw, fn) in variants.items():
            with flags(MODEL, **kw):
                per[name].append(_time(fn, iters))
    return {name: float(np.median(v)) for name, v in per.items()}


def bench(rounds, iters):
    import torch
    from oracle import inputs
    a, b = (t.cuda() for t in inputs.structured_pair(512, 512, seed=7))
    gf = MODEL.graphed("test_eval")
    ev = _alternate({"shipped": ({}, lambda: gf(a, b)),
                     "only_homo": (dict(only_homo=True), lambda: gf(a, b)),
                     "combine_h_flow": (dict(use_combine_h_flow=True, use_fb_consistency_mask=False), lambda: gf(a, b))},
                    rounds, iters)
    res = {"test_eval_graphed_pairs_per_s": {k: 1.0 / v for k, v in ev.items()}}
    out = {}
    for n in (512, 1024):
        a, b = (t.cuda() for t in inputs.structured_pair(n, n, seed=7))
        gt = MODEL.graphed_test_out()
        t = _alternate({"mask": ({}, lambda: gt(a, b)), "no_mask": (dict(use_fb_consistency_mask=False), lambda: gt(a, b))},
                       rounds, max(2, iters // 4))
        out[f"{n}x{n}"] = {k: v * 1e3 for k, v in t.items()}
    res["test_out_graphed_ms_per_pair"] = out
    res["device"] = torch.cuda.get_device_name(0)
    res["method"] = (f"median of {rounds} alternating rounds after a warm-up; test_eval {iters} replays per round, test_out "
                     f"{max(2, iters // 4)} launch + finish per round (finish includes the canvas-size read-back)")
    return res


def kernels_only():
    import torch
    import stitch_amd
    ops = stitch_amd.ops
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, B, h, w in KERNEL_CASES:
        if name == "homo_flow_warp_kernel":
            img = torch.rand(B, 3, h, w, device="cuda", generator=g) * 255
            flow = (torch.rand(B, 2, h, w, device="cuda", generator=g) - 0.5) * 4
            H8 = (torch.eye(3, device="cuda") + 1e-3 * torch.randn(B, 3, 3, device="cuda", generator=g)).contiguous()
            fn = lambda: ops.homo_flow_warp(img, H8, flow)          # noqa: E731
        else:
            homo1, homo2, fin = (torch.rand(1, 6, h, w, device="cuda", generator=g) for _ in range(3))
            fn = lambda: ops.blend_plain(homo1, homo2, fin)         # noqa: E731
        for _ in range(200):
            fn()
        torch.cuda.synchronize()
    print("launched", [f"{n} B={B} {h}x{w} x200" for n, B, h, w in KERNEL_CASES])


def report_kernels(stats_csv):
    rows = {r["Name"]: r for r in csv.DictReader(open(stats_csv))}
    rep = {}
    for name in BYTES_PER_PX:
        hit = [r for n, r in rows.items() if name in n]
        if not hit:
            continue
        r = hit[0]
        # one stats row per kernel name mixes the launch shapes: the average is weighted by the case sizes below
        px = sum(B * h * w for n, B, h, w in KERNEL_CASES if n == name) / sum(1 for n, *_ in KERNEL_CASES if n == name)
        avg_us = float(r["AverageNs"]) / 1e3
        bound_us = px * BYTES_PER_PX[name] / (HBM_TBS * 1e12) * 1e6
        rep[name] = dict(calls=int(r["Calls"]), avg_us=avg_us, mean_px_per_launch=px, bytes_per_px=BYTES_PER_PX[name],
                         hbm_bound_us=bound_us, frac_of_hbm_peak=bound_us / avg_us, bound="HBM")
    return rep


MODEL = None

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
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
        import torch
        MODEL = _model()
        with torch.no_grad():
            res = bench(args.rounds, args.iters)
    if res is not None:
        print(json.dumps(res, indent=1))
        if args.json:
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
