"""multiband_fusion on the MI355X: `ops.multiband_blend` per call, its kernels one by one, and the out.py loop with the switch off and on.

    python tools/bench_multiband.py [--out profiles/multiband_bench.json] [--parent-out PATH/out.py] [--pairs 48] [--rounds 5]

* call: canvases 548x588 and 1067x1134 (the result canvases of the 512x512 demo pairs and of a pair twice that size), two overlapping
  quadrilateral masks, 5 levels.  A single call between HIP events, and 50 calls back to back in one workspace; median of the rounds.
* kernels: one `rocprofv3 --kernel-trace --stats` run of a child process of its own making 20 blends of each canvas; per kernel name the
  summed duration per blend beside the bytes it has to move / 6.3 TB/s.
* loop: the out.py loop (`run_pairs`, depth 2) on synthetic 512x512 pairs with `--multiband_fusion` off and on, and with `--parent-out`
  the loop of another out.py (the commit before the switch existed) in the same alternation; wall pairs/s, median of the rounds.
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
HBM_BYTES_PER_US = 6.3e6


def case(H, W):
    """a smooth pair at different gains under two overlapping quadrilateral masks, as device tensors"""
    import torch
    y, x = np.mgrid[:H, :W].astype(np.float32)
    scene = np.stack([128 + 80 * np.sin(x / 37 + y / 53), 128 + 60 * np.cos(x / 29), 100 + 100 * x / W]).astype(np.float32)
    m1 = (x < 0.62 * W + 0.1 * y) & (y > 0.08 * H) & (y < 0.93 * H) & (x > 0.04 * W)
    m2 = (x > 0.33 * W + 0.2 * y) & (y > 0.17 * H) & (y < 0.97 * H) & (x < 0.96 * W)
    return [torch.from_numpy(a)[None].cuda() for a in (scene, 0.8 * scene, m1[None].astype(np.float32), m2[None].astype(np.float32))]


def call_times(H, W, n=50):
    import torch
    from stitch_amd import ops
    args = case(H, W)
    ws = torch.empty(ops.multiband_workspace_bytes(H, W, LEVELS), dtype=torch.uint8, device="cuda")
    for _ in range(5):
        ops.multiband_blend(*args, levels=LEVELS, workspace=ws)
    torch.cuda.synchronize()
    single = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.multiband_blend(*args, levels=LEVELS, workspace=ws)
        e1.record()
        e1.synchronize()
        single.append(e0.elapsed_time(e1) * 1e3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        ops.multiband_blend(*args, levels=LEVELS, workspace=ws)
    e1.record()
    e1.synchronize()
    return float(np.median(single)), e0.elapsed_time(e1) * 1e3 / n


def floor_bytes(H, W):
    """bytes each kernel name has to move per blend (compulsory reads and writes of its arrays once, caches ideal)"""
    hs, ws = [H], [W]
    while len(hs) <= LEVELS and (hs[-1] > 1 or ws[-1] > 1):
        hs.append((hs[-1] + 1) // 2), ws.append((ws[-1] + 1) // 2)
    n = [h * w for h, w in zip(hs, ws)]
    Le = len(n) - 1
    return {"mb_masks_kernel": 11 * n[0], "edt_cols_kernel": 3 * 14 * n[0], "edt_rows_d_kernel": 2 * 8 * n[0], "edt_rows_idx_kernel": 12 * n[0], "mb_fields_kernel": 66 * n[0],
            "mb_reduce_kernel": sum(28 * (n[l] + n[l + 1]) for l in range(Le)), "mb_top_kernel": 40 * n[Le],
            "mb_down_kernel": sum(40 * n[l] + 36 * n[l + 1] for l in range(Le))}, 9 + 2 * Le


def inner(n):
    import torch
    from stitch_amd import ops
    for H, W in CANVASES:
        args = case(H, W)
        for _ in range(n):
            ops.multiband_blend(*args, levels=LEVELS)
    torch.cuda.synchronize()


def kernel_trace(n=20):
    """per kernel name, launches and summed duration per blend, from a traced child process of its own per canvas"""
    res = {}
    for H, W in CANVASES:
        d = tempfile.mkdtemp(prefix="mb_prof_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "mb", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--inner", str(n), "--canvas", f"{H}x{W}"]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        path = (glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) or [None])[0]
        if path is None:
            raise RuntimeError(f"rocprofv3 wrote no kernel_stats.csv under {d}")
        floors, launches = floor_bytes(H, W)
        rows = []
        for r in csv.DictReader(open(path)):
            name = re.sub(r"\(.*", "", re.sub(r"^void ", "", r["Name"]))
            if name in floors:
                rows.append(dict(name=name, launches_per_blend=int(r["Calls"]) / n, us_per_blend=float(r["TotalDurationNs"]) / n / 1e3,
                                 floor_us_per_blend=floors[name] / HBM_BYTES_PER_US))
        shutil.rmtree(d, ignore_errors=True)
        res[f"{H}x{W}"] = dict(launches_per_blend=launches, kernels=sorted(rows, key=lambda r: -r["us_per_blend"]),
                               kernel_us_per_blend=sum(r["us_per_blend"] for r in rows))
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
    outmod = load_out(os.path.join(ROOT, "out.py"), "stitch_out_harness_mb")
    root = tempfile.mkdtemp(prefix="mb_loop_")
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
    variants = {"multiband_off": lambda d_: outmod.run_pairs(cfg, todo, d_, model, comp, inp),
                "multiband_on": lambda d_: outmod.run_pairs(cfg, todo, d_, model, comp, inp, multiband=LEVELS)}
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
    ref_tag = "parent_commit" if parent_path else "multiband_off"
    res["ten_files_identical_to_" + ref_tag] = all(
        open(os.path.join(last_dir[k], p, f), "rb").read() == open(os.path.join(last_dir[ref_tag], p, f), "rb").read()
        for k in variants for p in sorted(os.listdir(last_dir[ref_tag])) for f in files[ref_tag])
    if parent_path:
        v = samples["parent_commit"]
        res["parent_spread_pairs_per_s"] = max(v) - min(v)
        res["off_within_parent_scatter"] = bool(res["multiband_off"]["pairs_per_s_median"] >= float(np.median(v)) - (max(v) - min(v)))
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
    res = {"what": f"ops.multiband_blend at {LEVELS} levels; times in microseconds", "rounds": a.rounds}
    if not a.no_trace:
        res["kernel_trace"] = kernel_trace()            # before this process opens the GPU: the traced child runs alone
    import stitch_amd  # noqa: F401
    res["call"] = {}
    for H, W in CANVASES:
        xs = [call_times(H, W) for _ in range(a.rounds)]
        res["call"][f"{H}x{W}"] = dict(single_call_us_median=float(np.median([x[0] for x in xs])), single_call_us_rounds=[round(x[0], 1) for x in xs],
                                      back_to_back_us_median=float(np.median([x[1] for x in xs])), back_to_back_us_rounds=[round(x[1], 1) for x in xs],
                                      floor_us=sum(floor_bytes(H, W)[0].values()) / HBM_BYTES_PER_US, launches=floor_bytes(H, W)[1])
    if not a.no_loop:
        res["out_loop"] = dict(pairs=a.pairs, depth=2, **loop_bench(a.pairs, a.rounds, a.parent_out))
    text = json.dumps(res, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
