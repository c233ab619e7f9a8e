"""The GPU JPEG encoder (csrc/jpeg.hip, `ops.jpeg_encode`) against Pillow, and what it does to the out.py loop.

    python tools/bench_jpeg.py [--out profiles/jpeg_bench.json] [--parent-out PATH/out.py] [--pairs 48] [--rounds 5]

* per image: HIP-event time of one encode (median of single calls, and back-to-back throughput) for a 548x588 and a 1067x1134 RGB
  canvas and a 548x588 0/255 mask, against Pillow's encode of the same arrays on one thread of this box;
* per kernel: one `rocprofv3 --kernel-trace --stats` child making 200 encodes of the 548x588 canvas;
* the loop: `run_pairs` on 48 synthetic 512x512 pairs (10 files per pair) with `gpu_jpeg` off and on, at depth 2 and 3, the variants
  alternating, median of the rounds; wall pairs/s and host CPU seconds per pair (`time.process_time`: all threads of the process).
  `--parent-out` adds the loop of another out.py (the commit before the switch existed) to the same alternation.

    python tools/bench_jpeg.py --options [--out profiles/jpeg_opts_bench.json]

* the option rows, in one run: per image Pillow on one thread with the same keywords, `st_jpeg_encode_u8` (`defaults_old_entry`),
  `st_jpeg_encode_u8_ex` at the defaults (`defaults_new_entry`: quality 75, 4:2:0, Annex K tables) -- the first entry calls the second, so
  the two rows time one code path and are kept as a check of each other -- and quality 95, 4:4:4, optimised tables; per kernel one traced
  child making 200 encodes of the 548x588 canvas at (95, 4:4:4, optimised).

    python tools/bench_jpeg.py --against OTHER_ROOT [--rounds 7] [--out profiles/jpeg_unify_bench.json]

* this tree's library against the one built in another checkout (OTHER_ROOT: an exported commit with its library built), per image at the
  defaults and at (95, 4:4:4, optimised): every sample is a fresh child process that imports one of the two trees, the two alternate for
  `--rounds` rounds; per row both versions' medians over the rounds and each version's min-max, and whether this tree's median stays within
  the other's median plus the other's own min-max spread; then one traced child per version (200 default encodes of the 548x588 canvas).

    python tools/bench_jpeg.py --restart [--out profiles/jpeg_rst_enc_bench.json]

* restart intervals (the jpegr_enc_* kernels of csrc/jpeg.hip): per image Pillow on one thread and the GPU at the defaults and with `restart_marker_rows=1`, in
  one run (the defaults against a parent checkout are `--against`'s business).
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


VERSION_ROWS = {"defaults": {}, "q95_444_optimised": OPTION_ROWS["q95_444_optimised"]}


def version_sample(root):
    """one child: the timings of `encode_times` for every image and row of VERSION_ROWS, with the package of the checkout at `root`"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sample", "--root", root], check=True, timeout=300, stdout=subprocess.PIPE, text=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def versions_bench(other_root, rounds):
    roots = {"other": os.path.abspath(other_root), "this": ROOT}
    samples = {v: [] for v in roots}
    for _ in range(rounds):
        for v, root in roots.items():
            samples[v].append(version_sample(root))
    res = {}
    for name in samples["this"][0]:
        res[name] = {}
        for row in VERSION_ROWS:
            entry = {}
            for v in roots:
                assert len({s_[name][row]["file_bytes"] for s_ in samples["this"] + samples["other"]}) == 1
                for key in ("single_call_us", "back_to_back_us"):
                    xs = [s_[name][row][key] for s_ in samples[v]]
                    entry.setdefault(key, {})[v] = dict(median=float(np.median(xs)), min=min(xs), max=max(xs))
            for key in ("single_call_us", "back_to_back_us"):
                o, t = entry[key]["other"], entry[key]["this"]
                entry[key]["other_spread"] = o["max"] - o["min"]
                entry[key]["this_within_other_median_plus_spread"] = bool(t["median"] <= o["median"] + (o["max"] - o["min"]))
            res[name][row] = entry
    return res


def profile_child(n, options=False, root=""):
    """per-kernel stand-alone durations (us per encode) from a traced child making n encodes of the 548x588 canvas (`options`: at
    quality 95, 4:4:4, optimised tables; `root`: with the package of another checkout)"""
    d = tempfile.mkdtemp(prefix="jpeg_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "jpeg", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--inner", str(n)] + (["--options"] if options else []) + (["--root", root] if root else [])
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    path = (glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) or [None])[0]
    if path is None:
        raise RuntimeError(f"rocprofv3 wrote no kernel_stats.csv under {d}")
    rows = []
    for r in csv.DictReader(open(path)):
        if "jpeg_" in r["Name"]:
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
    ap.add_argument("--options", action="store_true", help="the option rows -> profiles/jpeg_opts_bench.json")
    ap.add_argument("--restart", action="store_true", help="the defaults and restart_marker_rows=1 -> profiles/jpeg_rst_enc_bench.json")
    ap.add_argument("--against", default="", help="another checkout with its library built -> profiles/jpeg_unify_bench.json")
    ap.add_argument("--against-label", default="", help="how the result file names the other checkout (default: its path)")
    ap.add_argument("--sample", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default="", help=argparse.SUPPRESS)
    ap.add_argument("--parent-out", default="")
    ap.add_argument("--pairs", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--inner", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "jpeg_rst_enc_bench.json" if a.restart else "jpeg_unify_bench.json" if a.against else "jpeg_opts_bench.json" if a.options else "jpeg_bench.json")
    imgs = images()
    if a.root:                                             # a child of --against: the package of the checkout at a.root
        sys.path.insert(0, a.root)
        from stitch_amd import _lib
        assert os.path.dirname(os.path.dirname(_lib.LIB_PATH)) == a.root, _lib.LIB_PATH
    if a.sample:
        out = {}
        for name, u8 in imgs.items():
            out[name] = {}
            for row, kw in VERSION_ROWS.items():
                single, b2b, nbytes = encode_times(u8, **option_keywords(kw, u8))
                out[name][row] = dict(single_call_us=single * 1e3, back_to_back_us=b2b * 1e3, file_bytes=nbytes)
        print(json.dumps(out))
        return
    if a.against:
        res = {"what": "ops.jpeg_encode of this tree against the library of another checkout, one MI355X: HIP-event median of 50 single calls and "
                       "50 calls back to back per sample, every sample a fresh process, the two versions alternating",
               "other": a.against_label or a.against, "rounds": a.rounds, "per_image": versions_bench(a.against, a.rounds)}
        res["kernels_rgb_548x588_defaults"] = dict(source=f"rocprofv3 --kernel-trace --stats, {a.launches} encodes per version, each traced child a run of its own",
                                                   other=profile_child(a.launches, root=os.path.abspath(a.against)), this=profile_child(a.launches))
        res["every_row_within_margin"] = all(e[k]["this_within_other_median_plus_spread"] for im in res["per_image"].values() for e in im.values()
                                             for k in ("single_call_us", "back_to_back_us"))
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    if a.inner:                                            # the traced child
        import torch
        from stitch_amd import ops
        x = torch.from_numpy(imgs["rgb_548x588"]).cuda()
        for _ in range(a.inner):
            ops.jpeg_encode(x, **(OPTION_ROWS["q95_444_optimised"] if a.options else {}))
        torch.cuda.synchronize()
        return
    if a.restart:
        res = {"what": "GPU JPEG encoder at the defaults and with restart_marker_rows=1 (the jpegr_enc_* kernels of csrc/jpeg.hip) vs Pillow (one thread, same keywords), same run, one MI355X",
               "per_image": {}}
        for name, u8 in imgs.items():
            res["per_image"][name] = {}
            for row, kw in (("defaults", {}), ("restart_marker_rows_1", dict(restart_marker_rows=1))):
                p_ms, p_bytes = pillow_ms(u8, **kw)
                single, b2b, g_bytes = encode_times(u8, **kw)
                assert g_bytes == p_bytes
                res["per_image"][name][row] = dict(pillow_ms_one_thread=p_ms, gpu_ms_single_call_hip_events=single, gpu_ms_back_to_back=b2b, file_bytes=g_bytes)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    if a.options:
        res = {"what": "GPU JPEG encoder (csrc/jpeg.hip) with options vs Pillow (one thread, same keywords), same run, one MI355X; defaults_old_entry "
                       "(st_jpeg_encode_u8) and defaults_new_entry (st_jpeg_encode_u8_ex at the defaults) are one code path, timed twice"}
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
