"""Time `ops.inpaint_telea` (cv_inpainter's fill) on the masks the real chain hands to the inpainter, and the out.py loop with the
`_cv` configs against the pass-through ones.

    python tools/bench_inpaint.py [--reps 20] [--pairs 8] [--rounds 2] [--json out.json]

Cases: demo1 / demo2 of tests/golden/e2e_demo_512.npz through the seeded-weights `test_out` forward, the TPS post-pipeline and
`mix_fn` (all_img1_with_inpaint: thin border; inpaint_all_area: every hole), plus one 1024x1024 `test_out` canvas.  Per case:
fill pixels, rings, disc visits (fill pixels x offsets inside the radius, an upper bound: offsets outside the image or not yet
known are skipped), op time (device events around the op, after warm-up; median over --reps) and visits/s.  The out.py rows run
`run_pairs` on --pairs synthetic 512x512 pairs written as JPEGs, the two configs alternated --rounds times each."""
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


class Recorder:
    """Inpainter that records what `mix_fn` hands over and returns what `inner` returns."""

    def __init__(self, inner):
        self.inner, self.name, self.calls = inner, inner.name, []

    def inpaint(self, init_image_tensor, mask_image_tensor, control_image_tensor=None, prompt="", resize_to_area_limit_before_inpaint=False):
        out = self.inner.inpaint(init_image_tensor, mask_image_tensor, control_image_tensor=control_image_tensor, prompt=prompt,
                                 resize_to_area_limit_before_inpaint=resize_to_area_limit_before_inpaint)
        self.calls.append((init_image_tensor.clone(), mask_image_tensor.clone(), out.clone()))
        return out


def seeded_model():
    import stitch_amd
    from oracle import spec
    cfg, _ = stitch_amd.load_inference_config("all_img1_with_inpaint_g12_transRef")
    m = stitch_amd.build_model(cfg)
    m.load_state_dict(spec.seeded_state_dict(1234), strict=True)
    return m.cuda().eval()


def run_chain(model, a, b, mix_method, inpainter, inf_cfg="all_img1_with_inpaint_g12_cv"):
    """test_out forward + tps_H_warp with `mix_method`'s mix_fn and `inpainter`, as out.py:inference_one_data wires them.
    Returns (mix_fn outputs dict, tps_H_warp result)."""
    import stitch_amd
    _, tpc = stitch_amd.load_inference_config(inf_cfg)
    out = model(a, b, type="test_out", pad_mode="replicate")
    inputs = dict(output1=out["output1"], mask1=out["mask1"], H_warp=out["H_warp"], H_warp_mask=out["H_warp_mask"],
                  final_warp=out["final_warp"], mask2=out["mask2"], residual_flow=out["residual_flow"], valid=None,
                  occlusion_mask=out["occlusion_mask"], border_points_mask=out["occlusion_mask"])
    limit = dict(width_min=out["width_min"], height_min=out["height_min"], out_height=out["out_height"], out_width=out["out_width"])
    mix_fn = importlib.import_module(f"stitch_amd.mix_methods.{mix_method}").mix_fn
    got = {}

    def fn(**kw):
        r = mix_fn(**kw, inpainter=inpainter, use_composition=False, is_plot=False,
                   resize_to_area_limit_before_inpaint=tpc.resize_to_area_limit_before_inpaint)
        got.update(zip(("tfw", "tfwm", "inpaint_img", "inpaint_img_mask", "inpaint_area_mask"), r))
        return r

    new = stitch_amd.tps_pipeline.tps_H_warp(inputs, limit, tpc, inpaint_fn=fn)
    return got, new


def demo_pair(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", "e2e_demo_512.npz"))
    f = lambda k: torch.from_numpy(g[f"{name}_{k}"]).permute(2, 0, 1)[None].float().cuda()   # noqa: E731
    return f("input1"), f("input2")


def chain_cases(model):
    """[(label, img uint8 [H,W,3], mask uint8 [H,W])] of the inputs the chain hands to cv_inpainter."""
    import stitch_amd
    from stitch_amd.data import structured_pair
    from stitch_amd.mix_methods.utils.cv_inpainter import inpainter as cv
    pairs = [("demo1", *demo_pair("demo1")), ("demo2", *demo_pair("demo2"))]
    a, b = structured_pair(1024, 1024, seed=7)
    cases = []
    for label, a_, b_ in pairs + [("synthetic1024", a.cuda(), b.cuda())]:
        for mm in ("all_img1_with_inpaint", "inpaint_all_area"):
            if label == "synthetic1024" and mm == "inpaint_all_area":
                continue
            rec = Recorder(cv)
            run_chain(model, a_, b_, mm, rec)
            init, mask, _ = rec.calls[0]
            img, m = stitch_amd.ops.inpaint_prep(init[0].float().contiguous(), mask[0].float().contiguous())
            cases.append((f"{label}/{mm}", img, m))
    return cases


def time_op(img, mask, reps, radius=64):
    import stitch_amd
    for _ in range(3):
        stitch_amd.ops.inpaint_telea(img, mask, radius)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        stitch_amd.ops.inpaint_telea(img, mask, radius)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def out_loop(model, n_pairs, rounds):
    """pairs/s of out.py's run_pairs for the `_cv` config and the pass-through `_transRef` config, alternated."""
    from PIL import Image
    import stitch_amd
    from stitch_amd.data import structured_pair
    spec_ = importlib.util.spec_from_file_location("stitch_out_bench", os.path.join(ROOT, "out.py"))
    outmod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(outmod)
    res = {"all_img1_with_inpaint_g12_transRef": [], "all_img1_with_inpaint_g12_cv": []}
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
    p.add_argument("--json", default="")
    args = p.parse_args()
    import stitch_amd
    torch.cuda.set_device(0)
    model = seeded_model()
    ndisc = stitch_amd.ops.inpaint_disc_size(64)
    rows = []
    print(f"{'case':40} {'canvas':>10} {'fill px':>8} {'rings':>6} {'visits':>11} {'op ms':>8} {'visits/s':>10}")
    for label, img, mask in chain_cases(model):
        _, d, _ = stitch_amd.ops.inpaint_telea(img, mask, 64, return_fields=True)
        fill = int((mask != 0).sum())
        rings = int(d.max()) if d is not None else 0
        visits = fill * ndisc
        ms = time_op(img, mask, args.reps)
        row = dict(case=label, canvas=list(mask.shape), fill_pixels=fill, rings=rings, disc_visits=visits, op_ms=ms,
                   visits_per_s=visits / (ms * 1e-3))
        rows.append(row)
        print(f"{label:40} {mask.shape[0]:>4}x{mask.shape[1]:<5} {fill:8d} {rings:6d} {visits:11d} {ms:8.3f} {row['visits_per_s']:10.3e}")
    med, raw = out_loop(model, args.pairs, args.rounds)
    for k, v in med.items():
        print(f"out.py run_pairs {k}: {v:.2f} pairs/s (rounds: {', '.join(f'{x:.2f}' for x in raw[k])})")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(op=rows, out_loop_pairs_per_s=med, out_loop_rounds=raw, pairs=args.pairs), f, indent=1)


if __name__ == "__main__":
    main()
