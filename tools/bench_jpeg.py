"""The GPU JPEG encoder (csrc/jpeg.hip, `ops.jpeg_encode`) against Pillow, and what it does to the out.py loop.

    python tools/bench_jpeg.py [--out profiles/jpeg_bench.json] [--parent-out PATH/out.py] [--pairs 48] [--rounds 5]

* per image: HIP-event time of one encode (median of single calls, and back-to-back throughput) for a 548x588 and a 1067x1134 RGB
  canvas and a 548x588 0/255 mask, against Pillow's encode of the same arrays on one thread of this box;
* per kernel: one `rocprofv3 --kernel-trace --stats` child making 200 encodes of the 548x588 canvas;
* the loop: `run_pairs` on 48 synthetic 512x512 pairs (10 files per pair) with `gpu_jpeg` off and on, at depth 2 and 3, the variants
  alternating, median of the rounds; wall pairs/s and host CPU seconds per pair (`time.process_time`: all threads of the process).
  `--parent-out` adds the loop of another out.py (the commit before the switch existed) to the same alternation.

    python tools/bench_jpeg.py --options [--out profiles/jpeg_opts_bench.json]

* the option rows (csrc/jpeg_opts.hip), in one run: per image Pillow on one thread with the same keywords, the encoder of the defaults
  (`st_jpeg_encode_u8`), the option entry at the defaults (quality 75, 4:2:0, Annex K tables: the same bytes) and at quality 95, 4:4:4,
  optimised tables; per kernel one traced child making 200 encodes of the 548x588 canvas at (95, 4:4:4, optimised).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def images():
    import _jpeg_ref as ref
    canvas = ref._smooth(548, 588, 3, 5)
    return {"rgb_548x588": canvas, "rgb_1067x1134": ref._smooth(1067, 1134, 3, 6),
            "mask_548x588": ((ref._smooth(548, 588, 0, 7) > 127) * 255).astype(np.uint8)}


def pillow_ms(u8, n=20, **kw):
    from PIL import Image
    ts = []
    for _ in range(n):
        buf = io.BytesIO()
        t0 = time.perf_counter()
        Image.fromarray(u8).save(buf, format="JPEG", **kw)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), len(buf.getvalue())


def encode_times(u8, n=50, **kw):
    import torch
    from stitch_amd import ops
    x = torch.from_numpy(u8).cuda()
    for _ in range(5):
        r = ops.jpeg_encode(x, **kw)
    torch.cuda.synchronize()
    single = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = ops.jpeg_encode(x, **kw)
        e1.record()
        e1.synchronize()
        single.append(e0.elapsed_time(e1))
    ws = torch.empty((ops.jpeg_workspace_bytes(u8.shape[0], u8.shape[1], 3 if u8.ndim == 3 else 1, **kw),), dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        r = ops.jpeg_encode(x, workspace=ws, **kw)
    e1.record()
    e1.synchronize()
    return float(np.median(single)), e0.elapsed_time(e1) / n, len(ops.jpeg_bytes(*r))


OPTION_ROWS = {"defaults_old_entry": {}, "defaults_new_entry": dict(quality=75, subsampling=2), "q95_444_optimised": dict(quality=95, subsampling=0, optimize=True)}


def option_keywords(kw, u8):
    return {k: v for k, v in kw.items() if not (k == "subsampling" and u8.ndim == 2)}        # an L file has one component


def profile_child(n, options=False):
    """per-kernel stand-alone durations (us per encode) from a traced child making n encodes of the 548x588 canvas (`options`: at
    quality 95, 4:4:4, optimised tables)"""
    d = tempfile.mkdtemp(prefix="jpeg_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "jpeg", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--inner", str(n)] + (["--options"] if options else [])
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    path = (glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) or [None])[0]
    if path is None:
        raise RuntimeError(f"rocprofv3 wrote no kernel_stats.csv under {d}")
    rows = []
    for r in csv.DictReader(open(path)):
        if "jpeg_" in r["Name"] or "jpego_" in r["Name"]:
            name = re.sub(r"\(.*", "", re.sub(r"^void ", "", r["Name"]).replace("(anonymous namespace)::", ""))
            rows.append(dict(name=name, calls_per_encode=int(r["Calls"]) / n, us_per_encode=float(r["TotalDurationNs"]) / n / 1e3))
    return sorted(rows, key=lambda r: -r["us_per_encode"])


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
    outmod = load_out(os.path.join(ROOT, "out.py"), "stitch_out_harness_jb")
    root = tempfile.mkdtemp(prefix="jpeg_loop_")
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
    variants = {"gpu_jpeg_off": lambda d_, depth: outmod.run_pairs(cfg, todo, d_, model, comp, inp, depth=depth),
                "gpu_jpeg_on": lambda d_, depth: outmod.run_pairs(cfg, todo, d_, model, comp, inp, depth=depth, gpu_jpeg=True)}
    if parent_path:
        parent = load_out(parent_path, "stitch_out_harness_parent")
        variants = dict({"parent_commit": lambda d_, depth: parent.run_pairs(cfg, todo, d_, model, comp, inp, depth=depth)}, **variants)
    res, run_id, last_dir = {}, 0, {}
    with contextlib.redirect_stdout(io.StringIO()):
        for depth in (2, 3):
            samples = {k: [] for k in variants}
            for rnd in range(rounds + 1):                  # round 0: graph capture, file cache, lazy constants
                for tag, fn in variants.items():
                    dst = os.path.join(root, f"run{run_id}") + "/"
                    run_id += 1
                    os.makedirs(dst)
                    torch.cuda.synchronize()
                    t0, c0 = time.perf_counter(), time.process_time()
                    fn(dst, depth)
                    torch.cuda.synchronize()
                    wall, cpu = time.perf_counter() - t0, time.process_time() - c0
                    if rnd:
                        samples[tag].append((pairs / wall, cpu / pairs))
                    if tag in last_dir:
                        shutil.rmtree(last_dir[tag])
                    last_dir[tag] = dst
            res[f"depth{depth}"] = {k: dict(pairs_per_s_median=float(np.median([s[0] for s in v])), pairs_per_s_rounds=[round(s[0], 2) for s in v],
                                            host_cpu_s_per_pair_median=float(np.median([s[1] for s in v]))) for k, v in samples.items()}
    # the files are the same bytes, and what crosses to the host per pair
    same, raw, enc = True, 0, 0
    d_off, d_on = last_dir["gpu_jpeg_off"], last_dir["gpu_jpeg_on"]
    for p in sorted(os.listdir(d_off)):
        for f in sorted(os.listdir(os.path.join(d_off, p))):
            a = open(os.path.join(d_off, p, f), "rb").read()
            same = same and a == open(os.path.join(d_on, p, f), "rb").read()
            im = Image.open(io.BytesIO(a))
            raw += im.size[0] * im.size[1] * len(im.getbands())
            enc += len(a) + 4
    res["files_identical_off_vs_on"] = same
    res["device_to_host_bytes_per_pair"] = dict(gpu_jpeg_off=raw / pairs, gpu_jpeg_on=enc / pairs)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--options", action="store_true", help="the option rows of csrc/jpeg_opts.hip -> profiles/jpeg_opts_bench.json")
    ap.add_argument("--parent-out", default="")
    ap.add_argument("--pairs", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--inner", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "jpeg_opts_bench.json" if a.options else "jpeg_bench.json")
    imgs = images()
    if a.inner:                                            # the traced child
        import torch
        from stitch_amd import ops
        x = torch.from_numpy(imgs["rgb_548x588"]).cuda()
        for _ in range(a.inner):
            ops.jpeg_encode(x, **(OPTION_ROWS["q95_444_optimised"] if a.options else {}))
        torch.cuda.synchronize()
        return
    if a.options:
        res = {"what": "GPU JPEG encoder options (csrc/jpeg_opts.hip) vs Pillow (one thread, same keywords) and vs the encoder of the defaults "
                       "(csrc/jpeg.hip), same run, one MI355X"}
        rows = profile_child(a.launches, options=True)
        res["kernels_rgb_548x588_q95_444_optimised"] = dict(source=f"rocprofv3 --kernel-trace --stats, {a.launches} encodes (stand-alone kernel durations)", rows=rows,
                                                            us_per_encode_total=sum(r["us_per_encode"] for r in rows),
                                                            table_kernel_us_per_encode=sum(r["us_per_encode"] for r in rows if "table" in r["name"]))
        import torch
        assert torch.cuda.is_available(), "needs the GPU"
        per = {}
        for name, u8 in imgs.items():
            per[name] = {}
            for row, kw in OPTION_ROWS.items():
                kw = option_keywords(kw, u8)
                p_ms, p_bytes = pillow_ms(u8, **kw)
                single, b2b, g_bytes = encode_times(u8, **kw)
                assert g_bytes == p_bytes
                per[name][row] = dict(keywords=kw, pillow_ms_one_thread=p_ms, gpu_ms_single_call_hip_events=single, gpu_ms_back_to_back=b2b, file_bytes=g_bytes)
        res["per_image"] = per
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    res = {"what": "GPU baseline JPEG encoder (csrc/jpeg.hip) vs Pillow (one thread) on the same arrays, one MI355X; the out.py loop with gpu_jpeg off / on"}
    res["kernels_rgb_548x588"] = dict(source=f"rocprofv3 --kernel-trace --stats, {a.launches} encodes (stand-alone kernel durations)",
                                      rows=profile_child(a.launches))
    res["kernels_rgb_548x588"]["us_per_encode_total"] = sum(r["us_per_encode"] for r in res["kernels_rgb_548x588"]["rows"])
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    per = {}
    for name, u8 in imgs.items():
        p_ms, p_bytes = pillow_ms(u8)
        single, b2b, g_bytes = encode_times(u8)
        assert g_bytes == p_bytes
        per[name] = dict(pillow_ms_one_thread=p_ms, gpu_ms_single_call_hip_events=single, gpu_ms_back_to_back=b2b, file_bytes=g_bytes,
                         raw_bytes=int(u8.size))
    res["per_image"] = per
    if not a.no_loop:
        res["out_loop"] = dict(pairs=a.pairs, rounds=a.rounds, **loop_bench(a.pairs, a.rounds, a.parent_out))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
