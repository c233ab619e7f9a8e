"""inner_crop on the MI355X: `ops.inner_rect` per call beside `ops.multiband_blend`, its kernels one by one against their traffic floors, and
the out.py loop with `--crop inner` off and on.

    python tools/bench_crop.py [--out profiles/crop_bench.json] [--parent-out PATH/out.py] [--pairs 48] [--rounds 5]

* call: canvases 548x588 and 1067x1134 under two overlapping quadrilateral masks (the canvases and masks of tools/bench_multiband.py), and
  an all-ones 4096x4096 canvas, the worst case of the row search: a single call between HIP events, and 50 calls back to back in one
  workspace; median of the rounds.  `ops.multiband_blend` (5 levels) at the first two sizes, for scale.
* kernels: one `rocprofv3 --kernel-trace --stats` run of a child process of its own per canvas making 20 calls; per kernel name the mean
  duration per call, the bytes the kernel must move (masks read once, the run plane written once and read once, the row records), that
  traffic at 6.3 TB/s, and the ratio.
* loop: the out.py loop (`run_pairs`, depth 2) on synthetic 512x512 pairs: the flags off and `--crop inner`; with `--parent-out` the loop
  of another out.py (the commit before the flag existed) in the same alternation; wall pairs/s, median of the rounds.
"""
import argparse
import contextlib
import csv
import glob
import importlib.util
import io
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CANVASES = ((548, 588), (1067, 1134), (4096, 4096))
LEVELS = 5
HBM_BYTES_PER_S = 6.3e12
KERNELS = ("crop_runs_kernel", "crop_rows_kernel", "crop_pick_kernel")


def floor_bytes(H, W):
    """the bytes each kernel must move: both masks read once and the run plane written; the run plane read and a record per row written; the
    records read and info written"""
    return {"crop_runs_kernel": 8 * H * W + 2 * H * W, "crop_rows_kernel": 2 * H * W + 8 * H, "crop_pick_kernel": 8 * H + 24}


def masks(H, W):
    """two overlapping quadrilateral masks; all ones at 4096 x 4096; device tensors [1,1,H,W]"""
    import torch
    if (H, W) == (4096, 4096):
        return [torch.ones((1, 1, H, W), device="cuda"), torch.ones((1, 1, H, W), device="cuda")]
    y, x = np.mgrid[:H, :W].astype(np.float32)
    m1 = (x < 0.62 * W + 0.1 * y) & (y > 0.08 * H) & (y < 0.93 * H) & (x > 0.04 * W)
    m2 = (x > 0.33 * W + 0.2 * y) & (y > 0.17 * H) & (y < 0.97 * H) & (x < 0.96 * W)
    return [torch.from_numpy(m[None, None].astype(np.float32)).cuda() for m in (m1, m2)]


def images(H, W):
    import torch
    y, x = np.mgrid[:H, :W].astype(np.float32)
    scene = np.stack([128 + 80 * np.sin(x / 37 + y / 53), 128 + 60 * np.cos(x / 29), 100 + 100 * x / W]).astype(np.float32)
    other = scene + ((x * 7 + y * 13) % 5).astype(np.float32)
    return [torch.from_numpy(a)[None].cuda() for a in (scene, other)]


def timed(fn, n=50):
    """median single call between events, and n calls back to back, in microseconds"""
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    single = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        single.append(e0.elapsed_time(e1) * 1e3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return float(np.median(single)), e0.elapsed_time(e1) * 1e3 / n


def call_variants(H, W):
    import torch
    from stitch_amd import ops
    k1, k2 = masks(H, W)
    ws = torch.empty(ops.inner_rect_workspace_bytes(H, W), dtype=torch.uint8, device="cuda")
    out = {"inner_rect": lambda: ops.inner_rect(k1, k2, workspace=ws), "inner_rect_one_mask": lambda: ops.inner_rect(k1, workspace=ws)}
    if H * W < 4096 * 4096:
        img1, img2 = images(H, W)
        wsb = torch.empty(ops.multiband_workspace_bytes(H, W, LEVELS), dtype=torch.uint8, device="cuda")
        out["multiband_blend"] = lambda: ops.multiband_blend(img1, img2, k1, k2, levels=LEVELS, workspace=wsb)
    return out, ops.inner_rect(k1, k2, workspace=ws).tolist()


def inner(n):
    import torch
    from stitch_amd import ops
    for H, W in CANVASES:
        k1, k2 = masks(H, W)
        for _ in range(n):
            ops.inner_rect(k1, k2)
    torch.cuda.synchronize()


def kernel_trace(n=20):
    """per kernel name, launches and mean duration per call, from a traced child process of its own per canvas"""
    res = {}
    for H, W in CANVASES:
        d = tempfile.mkdtemp(prefix="crop_prof_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "crop", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--inner", str(n), "--canvas", f"{H}x{W}"]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        path = (glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) or [None])[0]
        if path is None:
            raise RuntimeError(f"rocprofv3 wrote no kernel_stats.csv under {d}")
        floors = floor_bytes(H, W)
        rows = []
        for r in csv.DictReader(open(path)):
            name = re.sub(r"\(.*", "", re.sub(r"^void ", "", r["Name"]))
            if name in KERNELS:
                us = float(r["TotalDurationNs"]) / n / 1e3
                floor_us = floors[name] / HBM_BYTES_PER_S * 1e6
                rows.append(dict(name=name, launches_per_call=int(r["Calls"]) / n, us_per_call=us, floor_bytes=floors[name], floor_us=floor_us,
                                 ratio_to_floor=us / floor_us))
        shutil.rmtree(d, ignore_errors=True)
        res[f"{H}x{W}"] = dict(launches_per_call=len(KERNELS), kernels=sorted(rows, key=lambda r: KERNELS.index(r["name"])),
                               kernel_us_per_call=sum(r["us_per_call"] for r in rows))
    return res


def load_out(path, tag):
    spec = importlib.util.spec_from_file_location(tag, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def loop_bench(pairs, rounds, parent_path):
    import torch
    import stitch_amd
    from PIL import Image
    from stitch_amd.data import structured_pair
    outmod = load_out(os.path.join(ROOT, "out.py"), "stitch_out_harness_crop")
    root = tempfile.mkdtemp(prefix="crop_loop_")
    names = []
    base = [structured_pair(512, 512, seed=40 + i) for i in range(8)]
    for i in range(pairs):
        d = os.path.join(root, "demo", f"p{i:03d}")
        os.makedirs(d)
        a, b = base[i % 8]
        for n, t in (("input1.jpg", a), ("input2.jpg", b)):
            arr = np.roll(t[0].permute(1, 2, 0).numpy().astype(np.uint8), (3 * (i // 8), -5 * (i // 8)), (0, 1))
            Image.fromarray(arr).save(os.path.join(d, n), quality=95)
        names.append(f"p{i:03d}/")
    open(os.path.join(root, "demo", "demo.txt"), "w").write("\n".join(names) + "\n")
    cfg = outmod.get_config(["--data_root_path", os.path.join(root, "demo") + "/"])
    todo = outmod.get_data_dict_list(cfg.data_root_path, cfg.txt_file)
    torch.manual_seed(1234)
    model = stitch_amd.build_model(cfg).cuda().eval()
    comp = stitch_amd.composition.Network().cuda().eval()
    inp = outmod.load_inpainter("passthrough_inpainter")
    rects = []
    variants = {"flags_off": lambda d_: outmod.run_pairs(cfg, todo, d_, model, comp, inp),
                "crop_inner": lambda d_: outmod.run_pairs(cfg, todo, d_, model, comp, inp, crop="inner", on_done=lambda j, o: rects.append(o["crop_rect"])),
                "crop_inner_gpu_jpeg": lambda d_: outmod.run_pairs(cfg, todo, d_, model, comp, inp, crop="inner", gpu_jpeg=True),
                "flags_off_gpu_jpeg": lambda d_: outmod.run_pairs(cfg, todo, d_, model, comp, inp, gpu_jpeg=True)}
    if parent_path:
        parent = load_out(parent_path, "stitch_out_harness_parent")
        variants = dict({"parent_commit": lambda d_: parent.run_pairs(cfg, todo, d_, model, comp, inp)}, **variants)
    samples, run_id, last_dir = {k: [] for k in variants}, 0, {}
    with contextlib.redirect_stdout(io.StringIO()):
        for rnd in range(rounds + 1):                      # round 0: graph capture, file cache, lazy constants
            for tag, fn in variants.items():
                dst = os.path.join(root, f"run{run_id}") + "/"
                run_id += 1
                os.makedirs(dst)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(dst)
                torch.cuda.synchronize()
                if rnd:
                    samples[tag].append(pairs / (time.perf_counter() - t0))
                if tag in last_dir:
                    shutil.rmtree(last_dir[tag])
                last_dir[tag] = dst
    res = {k: dict(pairs_per_s_median=float(np.median(v)), pairs_per_s_rounds=[round(s, 2) for s in v]) for k, v in samples.items()}
    files = {k: sorted(os.listdir(os.path.join(d, "p000"))) for k, d in last_dir.items()}
    res["files_per_pair"] = {k: len(v) for k, v in files.items()}
    res["crop_rects_of_the_first_pairs"] = [list(r) if r else None for r in rects[:8]]
    ref_tag = "parent_commit" if parent_path else "flags_off"
    res["ten_files_identical_to_" + ref_tag] = all(
        open(os.path.join(last_dir[k], p, f), "rb").read() == open(os.path.join(last_dir[ref_tag], p, f), "rb").read()
        for k in variants for p in sorted(os.listdir(last_dir[ref_tag])) for f in files[ref_tag])
    if parent_path:
        v = samples["parent_commit"]
        res["parent_spread_pairs_per_s"] = max(v) - min(v)
        res["off_within_parent_scatter"] = bool(res["flags_off"]["pairs_per_s_median"] >= float(np.median(v)) - (max(v) - min(v)))
    shutil.rmtree(root, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-out", default="")
    ap.add_argument("--pairs", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--inner", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--canvas", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.inner:
        global CANVASES
        CANVASES = (tuple(int(v) for v in a.canvas.split("x")),)
        inner(a.inner)
        return
    res = {"what": f"ops.inner_rect beside ops.multiband_blend at {LEVELS} levels; times in microseconds; floors at {HBM_BYTES_PER_S / 1e12} TB/s",
           "rounds": a.rounds}
    if not a.no_trace:
        res["kernel_trace"] = kernel_trace()            # before this process opens the GPU: the traced child runs alone
    import stitch_amd  # noqa: F401
    res["call"] = {}
    for H, W in CANVASES:
        variants, info = call_variants(H, W)
        entry = {"info": info}
        for name, fn in variants.items():
            xs = [timed(fn) for _ in range(a.rounds)]
            entry[name] = dict(single_call_us_median=float(np.median([x[0] for x in xs])), single_call_us_rounds=[round(x[0], 1) for x in xs],
                               back_to_back_us_median=float(np.median([x[1] for x in xs])), back_to_back_us_rounds=[round(x[1], 1) for x in xs])
        res["call"][f"{H}x{W}"] = entry
    if not a.no_loop:
        res["out_loop"] = dict(pairs=a.pairs, depth=2, **loop_bench(a.pairs, a.rounds, a.parent_out))
    text = json.dumps(res, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
