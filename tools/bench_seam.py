"""seam_dp on the MI355X: `ops.seam_dp` per call beside the `ops.multiband_blend` it precedes, its kernels one by one, and the out.py loop
with `--seam dp` off and on.

    python tools/bench_seam.py [--out profiles/seam_bench.json] [--parent-out PATH/out.py] [--pairs 48] [--rounds 5]

* call: canvases 548x588 and 1067x1134 (the canvases of tools/bench_multiband.py), two overlapping quadrilateral masks, a smooth pair with a
  texture of a few grey levels between the images.  For the seam (auto, and both orientations fixed), the blend without and with the seam
  (5 levels): a single call between HIP events, and 50 calls back to back in one workspace; median of the rounds.
* kernels: one `rocprofv3 --kernel-trace --stats` run of a child process of its own per canvas making 20 seams (auto); per kernel name the
  summed duration per call; for the DP also per line.
* loop: the out.py loop (`run_pairs`, depth 2) on synthetic 512x512 pairs: the flags off, `--multiband_fusion`, and `--multiband_fusion --seam
  dp`; with `--parent-out` the loop of another out.py (the commit before the flag existed) in the same alternation; wall pairs/s, median of
  the rounds.
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

CANVASES = ((548, 588), (1067, 1134))
LEVELS = 5
KERNELS = ("seam_stats_kernel", "seam_decide_kernel", "seam_cost_kernel", "seam_dp_kernel", "seam_backtrack_kernel", "seam_side_kernel")


def case(H, W):
    """a smooth pair, image 2 with a texture of a few grey levels on top, under two overlapping quadrilateral masks, as device tensors"""
    import torch
    y, x = np.mgrid[:H, :W].astype(np.float32)
    scene = np.stack([128 + 80 * np.sin(x / 37 + y / 53), 128 + 60 * np.cos(x / 29), 100 + 100 * x / W]).astype(np.float32)
    other = scene + ((x * 7 + y * 13) % 5).astype(np.float32)
    m1 = (x < 0.62 * W + 0.1 * y) & (y > 0.08 * H) & (y < 0.93 * H) & (x > 0.04 * W)
    m2 = (x > 0.33 * W + 0.2 * y) & (y > 0.17 * H) & (y < 0.97 * H) & (x < 0.96 * W)
    return [torch.from_numpy(a)[None].cuda() for a in (scene, other, m1[None].astype(np.float32), m2[None].astype(np.float32))]


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
    args = case(H, W)
    ws = torch.empty(ops.seam_workspace_bytes(H, W), dtype=torch.uint8, device="cuda")
    wsb = torch.empty(ops.multiband_workspace_bytes(H, W, LEVELS), dtype=torch.uint8, device="cuda")
    seam = ops.seam_dp(*args, workspace=ws)
    return {"seam_dp_auto": lambda: ops.seam_dp(*args, workspace=ws),
            "seam_dp_vertical": lambda: ops.seam_dp(*args, orientation="vertical", workspace=ws),
            "seam_dp_horizontal": lambda: ops.seam_dp(*args, orientation="horizontal", workspace=ws),
            "multiband_blend": lambda: ops.multiband_blend(*args, levels=LEVELS, workspace=wsb),
            "multiband_blend_seam": lambda: ops.multiband_blend(*args, levels=LEVELS, workspace=wsb, seam=seam),
            "seam_dp_then_blend": lambda: ops.multiband_blend(*args, levels=LEVELS, workspace=wsb, seam=ops.seam_dp(*args, workspace=ws))}


def inner(n):
    import torch
    from stitch_amd import ops
    for H, W in CANVASES:
        args = case(H, W)
        for _ in range(n):
            ops.seam_dp(*args)
    torch.cuda.synchronize()


def kernel_trace(n=20):
    """per kernel name, launches and summed duration per call, from a traced child process of its own per canvas"""
    res = {}
    for H, W in CANVASES:
        d = tempfile.mkdtemp(prefix="seam_prof_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "seam", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--inner", str(n), "--canvas", f"{H}x{W}"]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        path = (glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) or [None])[0]
        if path is None:
            raise RuntimeError(f"rocprofv3 wrote no kernel_stats.csv under {d}")
        rows = []
        for r in csv.DictReader(open(path)):
            name = re.sub(r"\(.*", "", re.sub(r"^void ", "", r["Name"]))
            if name in KERNELS:
                rows.append(dict(name=name, launches_per_call=int(r["Calls"]) / n, us_per_call=float(r["TotalDurationNs"]) / n / 1e3))
        shutil.rmtree(d, ignore_errors=True)
        total = sum(r["us_per_call"] for r in rows)
        dp = sum(r["us_per_call"] for r in rows if r["name"] == "seam_dp_kernel")
        res[f"{H}x{W}"] = dict(launches_per_call=len(KERNELS), kernels=sorted(rows, key=lambda r: -r["us_per_call"]), kernel_us_per_call=total,
                               dp_fraction_of_kernel_time=dp / total if total else None, dp_lines=H, dp_ns_per_line=1e3 * dp / H)      # (these masks: vertical)
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
    outmod = load_out(os.path.join(ROOT, "out.py"), "stitch_out_harness_seam")
    root = tempfile.mkdtemp(prefix="seam_loop_")
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
    variants = {"flags_off": lambda d_: outmod.run_pairs(cfg, todo, d_, model, comp, inp),
                "multiband_on": lambda d_: outmod.run_pairs(cfg, todo, d_, model, comp, inp, multiband=LEVELS),
                "multiband_seam_dp": lambda d_: outmod.run_pairs(cfg, todo, d_, model, comp, inp, multiband=LEVELS, seam="dp")}
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
    res = {"what": f"ops.seam_dp beside ops.multiband_blend at {LEVELS} levels; times in microseconds", "rounds": a.rounds}
    if not a.no_trace:
        res["kernel_trace"] = kernel_trace()            # before this process opens the GPU: the traced child runs alone
    import stitch_amd  # noqa: F401
    res["call"] = {}
    for H, W in CANVASES:
        entry = {}
        for name, fn in call_variants(H, W).items():
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
