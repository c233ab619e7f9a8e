"""seam_gc on the MI355X: `ops.seam_gc` per call beside `ops.seam_dp` and the `ops.multiband_blend` they precede, its rounds, sweeps and
host reads, its kernels one by one, and the out.py loop with the flags off, `--seam dp` and `--seam gc`.

    python tools/bench_seam_gc.py [--out profiles/seam_gc_bench.json] [--parent-out PATH/out.py] [--pairs 48] [--rounds 5]

* call: the canvases, masks and images of tools/bench_seam.py (548x588 and 1067x1134).  A seam_gc call reads its status record back once per
  round, so it is timed on the host clock between two synchronisations (median and every round); seam_dp and the blend are re-measured the
  same way in the same run.  `rounds_needed` / `sweeps` / `host_reads` are the call's own statistics; `rounds_needed_max` over the
  canvases and the scenes of the tests is what `ops.SEAM_GC_MAX_ROUNDS` is set from (at least 8 x).
* kernels: one `rocprofv3 --kernel-trace --stats` run of a child process of its own per canvas making 3 cuts; per kernel name the launches
  and the summed duration per call.
* loop: the out.py loop (`run_pairs`, depth 2) on synthetic 512x512 pairs: the flags off, `--multiband_fusion --seam dp` and
  `--multiband_fusion --seam gc`; with `--parent-out` the loop of another out.py (the commit before the flag existed) in the same
  alternation; wall pairs/s, median of the rounds.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench_seam  # noqa: E402

CANVASES = bench_seam.CANVASES
LEVELS = bench_seam.LEVELS
KERNELS = ("gc_class_kernel", "gc_setup_kernel", "gc_begin_kernel", "gc_push_kernel", "gc_gather_kernel", "gc_bfs_kernel", "gc_status_kernel",
           "gc_side_kernel", "gc_info_kernel")


def wall(fn, n):
    """n calls, each between two synchronisations, on the host clock; microseconds"""
    import torch
    fn()
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return dict(us_median=float(np.median(out)), us_rounds=[round(v, 1) for v in out])


def call_bench(H, W, rounds):
    import torch
    from stitch_amd import ops
    args = bench_seam.case(H, W)
    ws = torch.empty(ops.seam_workspace_bytes(H, W), dtype=torch.uint8, device="cuda")
    wsg = torch.empty(ops.seam_gc_workspace_bytes(H, W), dtype=torch.uint8, device="cuda")
    wsb = torch.empty(ops.multiband_workspace_bytes(H, W, LEVELS), dtype=torch.uint8, device="cuda")
    side, info, stats = ops.seam_gc(*args, workspace=wsg, return_stats=True)
    dp = ops.seam_dp(*args, workspace=ws)
    k1, k2 = args[2][0, 0] > 0.5, args[3][0, 0] > 0.5
    overlap = k1 & k2
    entry = dict(stats, info=info.tolist(), overlap_pixels=int(overlap.sum()), workspace_bytes=wsg.numel(),
                 image1_share_of_overlap=float((side[overlap] == 1).float().mean()),
                 image1_share_of_overlap_seam_dp=float((dp[0][overlap] == 1).float().mean()) if int(dp[1][0]) else None)
    entry["seam_gc"] = wall(lambda: ops.seam_gc(*args, workspace=wsg), rounds)
    entry["seam_dp"] = wall(lambda: ops.seam_dp(*args, workspace=ws), 5 * rounds)
    entry["multiband_blend"] = wall(lambda: ops.multiband_blend(*args, levels=LEVELS, workspace=wsb), 5 * rounds)
    entry["multiband_blend_seam_gc"] = wall(lambda: ops.multiband_blend(*args, levels=LEVELS, workspace=wsb, seam=(side, info)), 5 * rounds)
    return entry


def scene_rounds():
    """rounds the scenes of tests/test_seam_gc_gpu.py need"""
    import torch
    from stitch_amd import ops
    import _seam_gc_ref as ref
    import _seam_ref as dpref
    from _multiband_cases import noise_pair, quads
    scenes = {f"ghost framed={f}": dpref.ghost_scene(framed=f)[:4] for f in (False, True)}
    scenes.update({f"serpentine {o}": ref.serpentine_scene(o)[:4] for o in ("vertical", "horizontal")})
    scenes["L with hole"] = ref.l_hole_scene()
    scenes["noise quads 40x40"] = noise_pair(40, 40, 73) + quads(40, 40)
    scenes["noise bands 128x129"] = noise_pair(128, 129, 75) + ref.bands(128, 129)
    scenes["smooth + texture bands 256x257"] = ref.smooth_texture_pair(256, 257, 77) + ref.bands(256, 257)
    out = {}
    for name, s in scenes.items():
        t = [torch.from_numpy(np.ascontiguousarray(a))[None].cuda() for a in s]
        out[name] = ops.seam_gc(*t, return_stats=True)[2]
    return out


def inner(n):
    import torch
    from stitch_amd import ops
    for H, W in CANVASES:
        args = bench_seam.case(H, W)
        for _ in range(n):
            ops.seam_gc(*args)
    torch.cuda.synchronize()


def kernel_trace(n=3):
    res = {}
    for H, W in CANVASES:
        d = tempfile.mkdtemp(prefix="seam_gc_prof_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "seam_gc", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--inner", str(n), "--canvas", f"{H}x{W}"]
        subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
        path = (glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) or [None])[0]
        if path is None:
            raise RuntimeError(f"rocprofv3 wrote no kernel_stats.csv under {d}")
        rows = []
        for r in csv.DictReader(open(path)):
            name = re.sub(r"\(.*", "", re.sub(r"^void ", "", r["Name"]))
            if name in KERNELS:
                rows.append(dict(name=name, launches_per_call=int(r["Calls"]) / n, us_per_call=float(r["TotalDurationNs"]) / n / 1e3,
                                 us_per_launch=float(r["TotalDurationNs"]) / int(r["Calls"]) / 1e3))
        shutil.rmtree(d, ignore_errors=True)
        res[f"{H}x{W}"] = dict(kernels=sorted(rows, key=lambda r: -r["us_per_call"]), kernel_us_per_call=sum(r["us_per_call"] for r in rows),
                               launches_per_call=sum(r["launches_per_call"] for r in rows))
    return res


def loop_bench(pairs, rounds, parent_path):
    import torch
    import stitch_amd
    from PIL import Image
    from stitch_amd.data import structured_pair
    outmod = bench_seam.load_out(os.path.join(ROOT, "out.py"), "stitch_out_harness_seam_gc")
    root = tempfile.mkdtemp(prefix="seam_gc_loop_")
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
                "multiband_seam_dp": lambda d_: outmod.run_pairs(cfg, todo, d_, model, comp, inp, multiband=LEVELS, seam="dp"),
                "multiband_seam_gc": lambda d_: outmod.run_pairs(cfg, todo, d_, model, comp, inp, multiband=LEVELS, seam="gc")}
    if parent_path:
        parent = bench_seam.load_out(parent_path, "stitch_out_harness_parent")
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
    ref_tag = "parent_commit" if parent_path else "flags_off"
    files = sorted(os.listdir(os.path.join(last_dir[ref_tag], "p000")))
    res["ten_files_identical_to_" + ref_tag] = all(
        open(os.path.join(last_dir[k], p, f), "rb").read() == open(os.path.join(last_dir[ref_tag], p, f), "rb").read()
        for k in variants for p in sorted(os.listdir(last_dir[ref_tag])) for f in files)
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
    res = {"what": "ops.seam_gc beside ops.seam_dp and ops.multiband_blend at 5 levels; host-clock times in microseconds", "rounds": a.rounds,
           "not_measured": [k for k, off in (("kernel_trace", a.no_trace), ("out_loop", a.no_loop), ("out_loop against the parent commit", not a.parent_out)) if off]}
    if not a.no_trace:
        res["kernel_trace"] = kernel_trace()            # before this process opens the GPU: the traced child runs alone
    from stitch_amd import ops
    res["call"] = {f"{H}x{W}": call_bench(H, W, a.rounds) for H, W in CANVASES}
    res["scenes"] = scene_rounds()
    seen = [v["rounds"] for v in res["scenes"].values()] + [v["rounds"] for v in res["call"].values()]
    res["rounds_needed_max"] = max(seen)
    res["max_rounds_default"] = ops.SEAM_GC_MAX_ROUNDS
    res["sweeps_per_round"] = ops.SEAM_GC_PUSH_SWEEPS
    if not a.no_loop:
        res["out_loop"] = dict(pairs=a.pairs, depth=2, **loop_bench(a.pairs, a.rounds, a.parent_out))
    text = json.dumps(res, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
