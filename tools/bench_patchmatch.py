"""Time `ops.inpaint_patchmatch` (patchmatch_inpainter's fill) beside `ops.inpaint_telea` (cv_inpainter's) on the masks the real chain hands to
the inpainter, and the out.py loop with the `_pm`, `_cv` and pass-through configs.

    python tools/bench_patchmatch.py [--reps 20] [--pairs 8] [--rounds 2] [--json out.json] [--op-only CASE --calls N]

Cases: those of tools/bench_inpaint.py (demo1 / demo2 of tests/golden/e2e_demo_512.npz through the seeded-weights `test_out` forward, the TPS
post-pipeline and `mix_fn` -- all_img1_with_inpaint: thin border; inpaint_all_area: every hole -- and the thin border of a 1024x1024 canvas) plus
a 1067x1134 canvas with the inpaint_all_area hole of demo1 scaled onto it.  Per case: fill pixels, level-0 targets and sources, levels, launches
per call (2 + levels (6 + 2 iters)), and the time of both ops in the same run (device events around the op, after warm-up; median over
--reps).  The out.py rows run `run_pairs` on --pairs synthetic 512x512 pairs written as JPEGs, the three configs alternated --rounds times each.
`--op-only CASE` runs --calls calls of the one case and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_inpaint as base  # noqa: E402

CONFIGS = ("inpaint_all_area_g12_pm", "inpaint_all_area_g12_cv", "inpaint_all_area_g12_diffusion")


def cases(model):
    out = base.chain_cases(model)
    label, img, mask = next(c for c in out if c[0] == "demo1/inpaint_all_area")
    H, W = 1067, 1134
    ys = (torch.arange(H, device=img.device) * img.shape[0] // H)[:, None]
    xs = (torch.arange(W, device=img.device) * img.shape[1] // W)[None, :]
    out.append(("demo1/inpaint_all_area @1067x1134", img[ys, xs].contiguous(), mask[ys, xs].contiguous()))
    return out


def time_fn(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def out_loop(model, n_pairs, rounds):
    """pairs/s of out.py's run_pairs for CONFIGS, alternated"""
    from PIL import Image
    import stitch_amd
    from stitch_amd.data import structured_pair
    spec_ = importlib.util.spec_from_file_location("stitch_out_bench_pm", os.path.join(ROOT, "out.py"))
    outmod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(outmod)
    res = {c: [] for c in CONFIGS}
    with tempfile.TemporaryDirectory() as td:
        root = os.path.join(td, "demo")
        names = []
        for i in range(n_pairs):
            d = os.path.join(root, f"p{i}")
            os.makedirs(d)
            a, b = structured_pair(512, 512, seed=900 + i, shift=(3 - i % 5, i % 4 - 2))
            for nm, t in (("input1.jpg", a), ("input2.jpg", b)):
                Image.fromarray(t[0].permute(1, 2, 0).numpy().astype(np.uint8)).save(os.path.join(d, nm), quality=95)
            names.append(f"p{i}/")
        with open(os.path.join(root, "demo.txt"), "w") as f:
            f.write("\n".join(names) + "\n")
        comp = stitch_amd.composition.Network().cuda().eval()
        for r in range(rounds + 1):
            for inf_cfg in res:
                cfg = outmod.get_config(["--data_root_path", root + "/", "--inf_cfg", inf_cfg])
                todo = outmod.get_data_dict_list(cfg.data_root_path, cfg.txt_file)
                inp = outmod.load_inpainter(cfg.TPS_PIPELINE_CONFIG.inpainter)
                save = os.path.join(td, f"res_{inf_cfg}_{r}") + "/"
                os.makedirs(save)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outmod.run_pairs(cfg, todo, save, model, comp, inp)
                torch.cuda.synchronize()
                if r > 0:                                    # round 0: warm-up
                    res[inf_cfg].append(n_pairs / (time.perf_counter() - t0))
    return {k: statistics.median(v) for k, v in res.items()}, res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--pairs", type=int, default=8)
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--iters", type=int, default=4)
    p.add_argument("--json", default="")
    p.add_argument("--op-only", default="", metavar="CASE")
    p.add_argument("--calls", type=int, default=5)
    args = p.parse_args()
    import stitch_amd
    ops = stitch_amd.ops
    torch.cuda.set_device(0)
    model = base.seeded_model()
    todo = cases(model)
    if args.op_only:
        label, img, mask = next(c for c in todo if c[0] == args.op_only)
        ws = torch.empty(ops.patchmatch_workspace_bytes(*mask.shape), dtype=torch.uint8, device=img.device)
        for _ in range(args.calls):
            ops.inpaint_patchmatch(img, mask, iters=args.iters, workspace=ws)
        torch.cuda.synchronize()
        print(f"{label}: {args.calls} calls of inpaint_patchmatch, iters {args.iters}")
        return
    rows = []
    print(f"{'case':40} {'canvas':>10} {'fill px':>8} {'targets':>8} {'sources':>8} {'lv':>3} {'launches':>8} {'pm ms':>8} {'telea ms':>9}")
    for label, img, mask in todo:
        H, W = mask.shape
        ws = torch.empty(ops.patchmatch_workspace_bytes(H, W), dtype=torch.uint8, device=img.device)
        _, info = ops.inpaint_patchmatch(img, mask, iters=args.iters, workspace=ws)
        info = info.cpu().tolist()
        levels = ops.patchmatch_levels(H, W)
        launches = 2 + levels * (6 + 2 * args.iters)
        fill = int((mask != 0).sum())
        pm = time_fn(lambda: ops.inpaint_patchmatch(img, mask, iters=args.iters, workspace=ws), args.reps)
        telea = time_fn(lambda: ops.inpaint_telea(img, mask, 64), args.reps)
        rows.append(dict(case=label, canvas=[H, W], fill_pixels=fill, valid=info[0], start_level=info[1], sources=info[2], targets=info[3], levels=levels,
                         iters=args.iters, launches=launches, workspace_bytes=ws.numel(), patchmatch_ms=pm, telea_ms=telea))
        print(f"{label:40} {H:>4}x{W:<5} {fill:8d} {info[3]:8d} {info[2]:8d} {levels:3d} {launches:8d} {pm:8.3f} {telea:9.3f}")
    med, raw = out_loop(model, args.pairs, args.rounds)
    for k, v in med.items():
        print(f"out.py run_pairs {k}: {v:.2f} pairs/s (rounds: {', '.join(f'{x:.2f}' for x in raw[k])})")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(op=rows, out_loop_pairs_per_s=med, out_loop_rounds=raw, pairs=args.pairs), f, indent=1)


if __name__ == "__main__":
    main()
