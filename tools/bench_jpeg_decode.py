"""The GPU JPEG decoder (csrc/jpeg_dec.hip, `ops.jpeg_decode`) against Pillow, and what it does to the evaluation loop.

    python tools/bench_jpeg_decode.py [--out profiles/jpeg_decode_bench.json] [--parent-root PATH] [--pairs 48] [--rounds 5] [--no-profile]

* per file: HIP-event time of one decode of device-resident bytes (median of single calls, and back-to-back throughput with one
  workspace) for a 512x512 4:2:0 file at quality 75 and 95, a 1024x1024 file and a 512x512 0/255 mask (L), against Pillow's decode of
  the same bytes on one thread of this box; the launches of the synchronise stage and the rounds its fixpoint needs (CPU model);
* per kernel: one `rocprofv3 --kernel-trace --stats` child making 200 decodes of the 512x512 quality-75 file;
* the loop: `validate_with_model` on synthetic 512x512 JPEG pairs with `gpu_decode` off and on, each run a child process, the variants
  alternating, median of the rounds: pairs/s, host CPU seconds per pair (`time.process_time`: all threads) and host-to-device bytes
  per pair.  `--parent-root` adds the loop of another checkout (the commit before the switch existed, built) to the alternation.

    python tools/bench_jpeg_decode.py --restart [--out profiles/jpeg_rst_bench.json] [--no-profile]

* restart intervals (the jpegr_* kernels of csrc/jpeg_dec.hip): the same four images written without DRI, with `restart_marker_rows=1` and with
  `restart_marker_blocks=4`: Pillow on one thread, single call and back to back, the intervals and subsequences of each file; per kernel one
  `rocprofv3 --kernel-trace --stats` child making 200 decodes of the 512x512 quality-75 file with a row per interval, with the synchronise
  launches that did work counted from the trace (a launch that returns at once takes a few microseconds); the evaluation loop on `--pairs`
  synthetic pairs written with `restart_marker_rows=1`, `gpu_decode` off against on (`--pairs 0`: not run).

    python tools/bench_jpeg_decode.py --against OTHER_ROOT [--rounds 7] [--out profiles/jpeg_rst_unify_bench.json]

* this tree's library against the one built in another checkout (OTHER_ROOT: an exported commit with its library built), per file of the
  three restart variants: every sample is a fresh child process that imports one of the two trees, the two alternate for `--rounds`
  rounds; per row both versions' medians over the rounds and each version's min-max, and whether this tree's median lies inside the
  other's own min-max.
"""
import argparse
import csv
import glob
import io
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def files(**restart):
    """the four files; `restart`: Pillow's restart_marker_blocks / restart_marker_rows for all of them"""
    import _jpeg_ref as eref
    from PIL import Image

    def pil(u8, **kw):
        buf = io.BytesIO()
        Image.fromarray(u8).save(buf, format="JPEG", **kw, **restart)
        return buf.getvalue()
    return {"rgb_512_q75": pil(eref._smooth(512, 512, 3, 5)), "rgb_512_q95": pil(eref._smooth(512, 512, 3, 5), quality=95),
            "rgb_1024_q75": pil(eref._smooth(1024, 1024, 3, 6)), "mask_512": pil(((eref._smooth(512, 512, 0, 7) > 127) * 255).astype(np.uint8))}


def pillow_ms(data, n=20):
    from PIL import Image
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        np.array(Image.open(io.BytesIO(data)))
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def decode_times(data, n=50):
    import torch
    from stitch_amd import ops
    info = ops.jpeg_probe(data, restart=True)
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    ws = torch.empty((ops.jpeg_dec_workspace_bytes(info),), dtype=torch.uint8, device="cuda")
    out = torch.empty((info.H, info.W, info.ncomp), dtype=torch.uint8, device="cuda")
    for _ in range(5):
        ops.jpeg_decode(dev, info=info, out=out, workspace=ws)
    torch.cuda.synchronize()
    single = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.jpeg_decode(dev, info=info, out=out, workspace=ws)
        e1.record()
        e1.synchronize()
        single.append(e0.elapsed_time(e1))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        ops.jpeg_decode(dev, info=info, out=out, workspace=ws)
    e1.record()
    e1.synchronize()
    return float(np.median(single)), e0.elapsed_time(e1) / n


def profile_child(n, restart=False):
    d = tempfile.mkdtemp(prefix="jpegd_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "jpegd", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--inner-profile", str(n)] + (["--restart"] if restart else [])
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    path = (glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) or [None])[0]
    if path is None:
        raise RuntimeError(f"rocprofv3 wrote no kernel_stats.csv under {d}")
    rows = []
    for r in csv.DictReader(open(path)):
        if "jpeg" in r["Name"]:
            name = re.sub(r"\(.*", "", re.sub(r"^void ", "", r["Name"]).replace("(anonymous namespace)::", ""))
            rows.append(dict(name=name, calls_per_decode=int(r["Calls"]) / n, us_per_decode=float(r["TotalDurationNs"]) / n / 1e3))
    rows = sorted(rows, key=lambda r: -r["us_per_decode"])
    if restart:                                                   # synchronise launches that did work: the others return at once, in a few us
        trace = (glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True) or [None])[0]
        durs = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in csv.DictReader(open(trace)) if "jpegr_sync_kernel" in r.get("Kernel_Name", "")] if trace else []
        if durs:
            rows.append(dict(name="jpegr_sync_kernel launches above 20 us (did work)", calls_per_decode=sum(v > 20.0 for v in durs) / n,
                             us_per_decode=sum(v for v in durs if v > 20.0) / n))
            rows.append(dict(name="jpegr_sync_kernel launches below 20 us (returned at once)", calls_per_decode=sum(v <= 20.0 for v in durs) / n,
                             us_per_decode=sum(v for v in durs if v <= 20.0) / n))
    return rows


def write_dataset(root, pairs, **save_kw):
    from PIL import Image
    sys.path.insert(0, ROOT)
    from stitch_amd.data import structured_pair
    for d in ("input1", "input2"):
        os.makedirs(os.path.join(root, "testing", d), exist_ok=True)
    base = [structured_pair(512, 512, seed=40 + i) for i in range(8)]
    nbytes = 0
    for i in range(pairs):
        for d, t in zip(("input1", "input2"), base[i % 8]):
            path = os.path.join(root, "testing", d, f"{i:06d}.jpg")
            Image.fromarray(t[0].permute(1, 2, 0).numpy().astype(np.uint8)).save(path, quality=95, **save_kw)
            nbytes += os.path.getsize(path)
    return nbytes / pairs


def inner_eval(root, data_dir, gpu_decode, rounds):
    """child: `rounds` timed runs of the loop of the checkout at `root` (after one untimed run that captures the graphs)"""
    sys.path.insert(0, root)
    import torch
    import stitch_amd
    from stitch_amd import evaluate as ev
    from oracle import spec
    cfg, _ = stitch_amd.load_inference_config("all_img1_with_inpaint_g12_transRef")
    model = stitch_amd.build_model(cfg)
    model.load_state_dict(spec.seeded_state_dict(1234), strict=True)
    model = model.cuda().eval()
    ds = ev.UDISDataset(data_dir, phase="testing")
    kw = dict(gpu_decode=True) if gpu_decode else {}
    ev.validate_with_model(model, ds, batch_size=1, **kw)
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0, c0 = time.perf_counter(), time.process_time()
        ev.validate_with_model(model, ds, batch_size=1, **kw)
        torch.cuda.synchronize()
        out.append(dict(pairs_per_s=len(ds) / (time.perf_counter() - t0), cpu_s_per_pair=(time.process_time() - c0) / len(ds)))
    print("RESULT " + json.dumps(out), flush=True)


def loop_bench(pairs, rounds, parent_root, **save_kw):
    data_dir = tempfile.mkdtemp(prefix="jpegd_loop_") + "/"
    file_bytes = write_dataset(data_dir, pairs, **save_kw)
    variants = [("gpu_decode_off", ROOT, 0), ("gpu_decode_on", ROOT, 1)] + ([("parent", parent_root, 0)] if parent_root else [])
    runs = {name: [] for name, _, _ in variants}
    for _ in range(rounds):                                       # alternating: one timed run per child, the variants in turn
        for name, root, on in variants:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--inner-eval", root, data_dir, str(on)], check=True, timeout=900,
                               stdout=subprocess.PIPE, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
            runs[name].extend(json.loads(line[7:]))
    res = {"pairs": pairs, "rounds": rounds, "h2d_bytes_per_pair": {"gpu_decode_off": 2 * 512 * 512 * 3, "gpu_decode_on": file_bytes}}
    for name, rs in runs.items():
        res[name] = dict(pairs_per_s_median=float(np.median([r["pairs_per_s"] for r in rs])), pairs_per_s=[round(r["pairs_per_s"], 2) for r in rs],
                         cpu_s_per_pair_median=float(np.median([r["cpu_s_per_pair"] for r in rs])))
    return res


RESTART_VARIANTS = {"no_dri": {}, "rows_1": dict(restart_marker_rows=1), "blocks_4": dict(restart_marker_blocks=4)}


def restart_bench(no_profile, pairs, rounds):
    import torch
    import _jpeg_rst_ref as rst
    res = {"device": torch.cuda.get_device_name(0), "per_file": {}}
    for variant, kw in RESTART_VARIANTS.items():
        for name, data in files(**kw).items():
            single, b2b = decode_times(data)
            info = rst.probe(data)
            parts = rst.intervals(data, info)
            nsub = sum(max(1, -(-n * 8 // 1024)) for _, n in parts)       # (stuffed bytes: the device cuts the unstuffed ones, a few less)
            longest = max(-(-n * 8 // 1024) for _, n in parts)
            enqueued = -(-(-(-info["scan_len"] * 8 // 1024) + (len(parts) if kw else 0)) // 256)          # the host's bound
            res["per_file"][f"{name}/{variant}"] = dict(file_bytes=len(data), pillow_ms=pillow_ms(data), gpu_single_ms=single, gpu_back_to_back_ms=b2b,
                                                        intervals=len(parts), subsequences_about=nsub, longest_interval_subsequences=longest,
                                                        sync_launches_enqueued=enqueued, sync_launches_needed_at_most=min(enqueued, -(-longest // 256) + 1))
            print(name, variant, res["per_file"][f"{name}/{variant}"], flush=True)
    if not no_profile:
        res["kernels_rgb_512_q75_rows_1"] = profile_child(200, restart=True)
    if pairs:                                                     # the evaluation loop on inputs written with a row per interval
        res["eval_loop_rows_1"] = loop_bench(pairs, rounds, "", restart_marker_rows=1)
        print(json.dumps(res["eval_loop_rows_1"]), flush=True)
    return res


def versions_bench(other_root, rounds):
    roots = {"other": os.path.abspath(other_root), "this": ROOT}
    samples = {v: [] for v in roots}
    for _ in range(rounds):
        for v, root in roots.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sample", "--root", root], check=True, timeout=300, stdout=subprocess.PIPE, text=True)
            samples[v].append(json.loads(r.stdout.strip().splitlines()[-1]))
    res = {}
    for row in samples["this"][0]:
        res[row] = {}
        for key in ("single_call_us", "back_to_back_us"):
            e = {v: dict(median=float(np.median(xs)), min=min(xs), max=max(xs)) for v in roots for xs in [[s_[row][key] for s_ in samples[v]]]}
            e["this_median_inside_other_min_max"] = bool(e["other"]["min"] <= e["this"]["median"] <= e["other"]["max"])
            e["this_median_not_above_other_max"] = bool(e["this"]["median"] <= e["other"]["max"])
            res[row][key] = e
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="")
    p.add_argument("--restart", action="store_true")
    p.add_argument("--parent-root", default="")
    p.add_argument("--pairs", type=int, default=48)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--no-profile", action="store_true")
    p.add_argument("--inner-profile", type=int, default=0)
    p.add_argument("--inner-eval", nargs=3, default=None)
    p.add_argument("--against", default="", help="another checkout with its library built -> profiles/jpeg_rst_unify_bench.json")
    p.add_argument("--against-label", default="", help="how the result file names the other checkout (default: its path)")
    p.add_argument("--sample", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--root", default="", help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.inner_eval:
        return inner_eval(args.inner_eval[0], args.inner_eval[1], int(args.inner_eval[2]), 1)
    args.out = args.out or os.path.join(ROOT, "profiles", "jpeg_rst_unify_bench.json" if args.against else "jpeg_rst_bench.json" if args.restart else "jpeg_decode_bench.json")
    if args.against:
        res = {"what": "ops.jpeg_decode of this tree against the library of another checkout, one MI355X: HIP-event median of 50 single calls and 50 calls "
                       "back to back per sample, every sample a fresh process, the two versions alternating",
               "other": args.against_label or args.against, "rounds": args.rounds, "per_file": versions_bench(args.against, args.rounds)}
        res["every_row_not_above_other_max"] = all(e[k]["this_median_not_above_other_max"] for e in res["per_file"].values() for k in e)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return None
    sys.path.insert(0, args.root or ROOT)
    import torch
    from stitch_amd import ops
    if args.sample:                                                # a child of --against: the package of the checkout at args.root
        from stitch_amd import _lib
        assert os.path.dirname(os.path.dirname(_lib.LIB_PATH)) == args.root, _lib.LIB_PATH
        out = {}
        for variant, kw in RESTART_VARIANTS.items():
            for name, data in files(**kw).items():
                single, b2b = decode_times(data)
                out[f"{name}/{variant}"] = dict(single_call_us=single * 1e3, back_to_back_us=b2b * 1e3)
        print(json.dumps(out))
        return None
    if args.inner_profile:
        data = files(**(RESTART_VARIANTS["rows_1"] if args.restart else {}))["rgb_512_q75"]
        info = ops.jpeg_probe(data, restart=True)
        dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        for _ in range(args.inner_profile):
            ops.jpeg_decode(dev, info=info)
        torch.cuda.synchronize()
        return None
    if args.restart:
        res = restart_bench(args.no_profile, args.pairs, args.rounds)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", args.out)
        return None
    import _jpeg_dec_ref as dref
    res = {"device": torch.cuda.get_device_name(0), "per_file": {}}
    for name, data in files().items():
        single, b2b = decode_times(data)
        info = ops.jpeg_probe(data)
        model = dref.sync_model(data, 1024)
        res["per_file"][name] = dict(file_bytes=len(data), pillow_ms=pillow_ms(data), gpu_single_ms=single, gpu_back_to_back_ms=b2b,
                                     subsequences=len(model["states"]), sync_launches=-(-len(model["states"]) // 256), fixpoint_rounds=model["rounds"])
        print(name, res["per_file"][name], flush=True)
    if not args.no_profile:
        res["kernels_rgb_512_q75"] = profile_child(200)
    res["eval_loop"] = loop_bench(args.pairs, args.rounds, args.parent_root)
    print(json.dumps(res["eval_loop"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
