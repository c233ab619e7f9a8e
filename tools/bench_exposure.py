"""Exposure compensation on the MI355X: `ops.exposure_compensate` per call, its kernels one by one, and the out.py loop with the switch off
and on.

    python tools/bench_exposure.py [--out profiles/exposure_bench.json] [--parent-out PATH/out.py] [--pairs 48] [--rounds 5]

* call: canvases 548x588 and 1067x1134 (as tools/bench_multiband.py), a smooth pair with image 2 at 0.8 x the gain under two overlapping
  quadrilateral masks, modes "gain" and "blocks" at the defaults (block 32, two smoothing passes).  A single call between HIP events, and
  50 calls back to back in one workspace; median of the rounds.
* kernels: one `rocprofv3 --kernel-trace --stats` run of a child process of its own per canvas and mode making 20 calls; per kernel name
  the summed duration per call beside the bytes it has to move / 6.3 TB/s.
* loop: the out.py loop (`run_pairs`, depth 2) on synthetic 512x512 pairs with `--multiband_fusion` alone ("flag off") and with
  `--exposure_compensation blocks` ("flag on"), and with `--parent-out` the loop of another out.py (the commit before the switch existed)
  with `--multiband_fusion` in the same alternation; wall pairs/s, median of the rounds.
"""
import argparse
import contextlib
import csv
import glob
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_multiband import HBM_BYTES_PER_US, LEVELS, case, load_out  # noqa: E402

CANVASES = ((548, 588), (1067, 1134))
MODES = ("gain", "blocks")
BLOCK, SMOOTH = 32, 2


def call_times(H, W, mode, n=50):
    import torch
    from stitch_amd import ops
    args = case(H, W)
    ws = torch.empty(ops.exposure_workspace_bytes(H, W, BLOCK), dtype=torch.uint8, device="cuda")
    out = (torch.empty_like(args[0]), torch.empty_like(args[1]))
    kw = dict(mode=mode, block=BLOCK, smooth=SMOOTH, workspace=ws, out=out)
    for _ in range(5):
        ops.exposure_compensate(*args, **kw)
    torch.cuda.synchronize()
    single = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.exposure_compensate(*args, **kw)
        e1.record()
        e1.synchronize()
        single.append(e0.elapsed_time(e1) * 1e3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        ops.exposure_compensate(*args, **kw)
    e1.record()
    e1.synchronize()
    return float(np.median(single)), e0.elapsed_time(e1) * 1e3 / n


def floor_bytes(H, W, mode):
    """bytes each kernel name has to move per call (compulsory reads and writes of its arrays once, caches ideal; channels off), and the
    launches of a call.  The statistics read both masks everywhere and the six image planes inside the overlap only."""
    y, x = np.mgrid[:H, :W].astype(np.float32)
    m1 = (x < 0.62 * W + 0.1 * y) & (y > 0.08 * H) & (y < 0.93 * H) & (x > 0.04 * W)
    m2 = (x > 0.33 * W + 0.2 * y) & (y > 0.17 * H) & (y < 0.97 * H) & (x < 0.96 * W)
    n, overlap = H * W, int((m1 & m2).sum())
    tiles = -(-H // BLOCK) * -(-W // BLOCK)
    table = 8 * tiles if mode == "blocks" else 8
    floors = {"ec_stats_kernel": 8 * n + 24 * overlap + 36 * tiles, "ec_global_kernel": 36 * tiles + 32, "ec_apply_kernel": 48 * n + table}
    if mode == "blocks":
        floors.update({"ec_tile_gain_kernel": 12 * tiles + 8 + 8 * tiles, "ec_smooth_kernel": SMOOTH * 16 * tiles})
    return floors, 3 if mode == "gain" else 4 + SMOOTH


def inner(n, H, W, mode):
    import torch
    from stitch_amd import ops
    args = case(H, W)
    for _ in range(n):
        ops.exposure_compensate(*args, mode=mode, block=BLOCK, smooth=SMOOTH)
    torch.cuda.synchronize()


def kernel_trace(n=20):
    """per kernel name, launches and summed duration per call, from a traced child process of its own per canvas and mode"""
    res = {}
    for H, W in CANVASES:
        for mode in MODES:
            d = tempfile.mkdtemp(prefix="ec_prof_")
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "ec", "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--inner", str(n), "--canvas", f"{H}x{W}", "--mode", mode]
            subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL)
            path = (glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) or [None])[0]
            if path is None:
                raise RuntimeError(f"rocprofv3 wrote no kernel_stats.csv under {d}")
            floors, launches = floor_bytes(H, W, mode)
            rows = []
            for r in csv.DictReader(open(path)):
                name = re.sub(r"[<(].*", "", re.sub(r"^void ", "", r["Name"]))
                if name in floors:
                    us, fl = float(r["TotalDurationNs"]) / n / 1e3, floors[name] / HBM_BYTES_PER_US
                    rows.append(dict(name=name, launches_per_call=int(r["Calls"]) / n, us_per_call=us, floor_us_per_call=fl, times_the_floor=us / fl))
            shutil.rmtree(d, ignore_errors=True)
            res[f"{H}x{W} {mode}"] = dict(launches_per_call=launches, kernels=sorted(rows, key=lambda r: -r["us_per_call"]),
                                          kernel_us_per_call=sum(r["us_per_call"] for r in rows))
    return res


def loop_bench(pairs, rounds, parent_path):
    import torch
    import stitch_amd
    from PIL import Image
    from stitch_amd.data import structured_pair
    outmod = load_out(os.path.join(ROOT, "out.py"), "stitch_out_harness_ec")
    root = tempfile.mkdtemp(prefix="ec_loop_")
    names = []
    base = [structured_pair(512, 512, seed=40 + i) for i in range(8)]
    for i in range(pairs):
        d = os.path.join(root, "demo", f"p{i:03d}")
        os.makedirs(d)
        a, b = base[i % 8]
        for n, t in (("input1.jpg", a), ("input2.jpg", b * 0.8)):
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
    variants = {"flag_off": lambda d_: outmod.run_pairs(cfg, todo, d_, model, comp, inp, multiband=LEVELS),
                "flag_on": lambda d_: outmod.run_pairs(cfg, todo, d_, model, comp, inp, multiband=LEVELS, exposure=("blocks", BLOCK))}
    if parent_path:
        parent = load_out(parent_path, "stitch_out_harness_parent")
        variants = dict({"parent_commit": lambda d_: parent.run_pairs(cfg, todo, d_, model, comp, inp, multiband=LEVELS)}, **variants)
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
    ref_tag = "parent_commit" if parent_path else "flag_off"
    same = lambda k, fs: all(open(os.path.join(last_dir[k], p, f), "rb").read() == open(os.path.join(last_dir[ref_tag], p, f), "rb").read()      # noqa: E731
                             for p in sorted(os.listdir(last_dir[ref_tag])) for f in fs)
    ten = [f for f in files[ref_tag] if f != "multiband_fusion.jpg"]
    res["ten_files_identical_to_" + ref_tag] = all(same(k, ten) for k in variants)
    res["flag_off_eleven_files_identical_to_" + ref_tag] = same("flag_off", files[ref_tag])
    if parent_path:
        v = samples["parent_commit"]
        res["parent_spread_pairs_per_s"] = max(v) - min(v)
        res["off_within_parent_scatter"] = bool(res["flag_off"]["pairs_per_s_median"] >= float(np.median(v)) - (max(v) - min(v)))
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
    ap.add_argument("--mode", default="gain", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.inner:
        H, W = (int(v) for v in a.canvas.split("x"))
        inner(a.inner, H, W, a.mode)
        return
    res = {"what": f"ops.exposure_compensate, block {BLOCK}, {SMOOTH} smoothing passes, channels off; times in microseconds", "rounds": a.rounds}
    if not a.no_trace:
        res["kernel_trace"] = kernel_trace()            # before this process opens the GPU: the traced child runs alone
    import stitch_amd  # noqa: F401
    res["call"] = {}
    for H, W in CANVASES:
        for mode in MODES:
            xs = [call_times(H, W, mode) for _ in range(a.rounds)]
            floors, launches = floor_bytes(H, W, mode)
            res["call"][f"{H}x{W} {mode}"] = dict(single_call_us_median=float(np.median([x[0] for x in xs])), single_call_us_rounds=[round(x[0], 1) for x in xs],
                                                 back_to_back_us_median=float(np.median([x[1] for x in xs])),
                                                 back_to_back_us_rounds=[round(x[1], 1) for x in xs],
                                                 floor_us=sum(floors.values()) / HBM_BYTES_PER_US, launches=launches)
    if not a.no_loop:
        res["out_loop"] = dict(pairs=a.pairs, depth=2, multiband_levels=LEVELS, **loop_bench(a.pairs, a.rounds, a.parent_out))
    text = json.dumps(res, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
