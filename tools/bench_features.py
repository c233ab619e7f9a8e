"""feature_align on the MI355X: `ops.feature_homography` per call beside `predict_homo` with the homography network, its kernels one by one,
evaluate.py's loop under `last_config_features` and `last_config_only_homo`, and out.py's loop with the default config against another
checkout's (the parent commit's).

    python tools/bench_features.py [--out profiles/features_bench.json] [--parent-root PATH] [--pairs 24] [--rounds 5]

* call: procedural 512x512 pairs with a known homography (tests/_features_ref.py), B = 1 and 8.  `feature_homography` (2048 hypotheses) in
  its own workspace and `predict_homo` of a seeded model, alternating inside every round: a single call between HIP events (median of 30)
  and 30 calls back to back; median of the rounds.
* kernels: one `rocprofv3 --kernel-trace --stats` run of a child process of its own making 20 calls at B = 1; per kernel the summed duration
  per call.
* evaluate: `validate_with_model` (the pipelined loop of evaluate.py) on 64 of those pairs held in memory, batch 4, the two configs
  alternating; wall pairs/s, median of the rounds.
* out: `run_pairs` of out.py with the default config in a child process per checkout and round, this tree and `--parent-root` alternating;
  every child captures, then times three passes; wall pairs/s.
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
KERNELS = ("ft_detect_kernel", "ft_describe_kernel", "ft_match_kernel", "ft_compact_kernel", "ft_norm_kernel", "ft_hyp_kernel", "ft_refit_kernel")


def scenes(n, B=1):
    """n batches [B,3,512,512] of procedural pairs, as device tensors"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _features_ref as ref
    out = []
    for i in range(n):
        items = [ref.pair(512, 512, ref.MOTIONS[(i * B + k) % len(ref.MOTIONS)], seed=50 + i * B + k)[:2] for k in range(B)]
        out.append(tuple(torch.from_numpy(np.concatenate([it[j] for it in items])).cuda() for j in (0, 1)))
    return out


def timed(fn, n=30):
    """median single call between events, and n calls back to back, in microseconds"""
    import torch
    for _ in range(3):
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


def seeded_model(model_config_name="last_config"):
    import stitch_amd
    from oracle import spec
    cfg, _ = stitch_amd.load_inference_config("all_img1_with_inpaint_g12_transRef", model_config_name=model_config_name)
    model = stitch_amd.build_model(cfg)
    model.load_state_dict(spec.seeded_state_dict(1234), strict=True)
    return model.cuda().eval()


def call_bench(rounds):
    import torch
    from stitch_amd import ops
    model = seeded_model()
    res = {}
    for B in (1, 8):
        a, b = scenes(1, B)[0]
        ws = torch.empty(ops.feature_workspace_bytes(B, 512, 512), dtype=torch.uint8, device="cuda")
        info = ops.feature_homography(a, b, workspace=ws)[2].cpu().numpy()
        variants = {"feature_homography": lambda: ops.feature_homography(a, b, workspace=ws), "predict_homo_network": lambda: model.predict_homo(a, b)}
        xs = {k: [] for k in variants}
        with torch.no_grad():
            for _ in range(rounds):
                for k, fn in variants.items():
                    xs[k].append(timed(fn))
        res[f"B{B}"] = dict(info=info.tolist(), **{k: dict(single_call_us_median=float(np.median([x[0] for x in v])), single_call_us_rounds=[round(x[0], 1) for x in v],
                                                       back_to_back_us_median=float(np.median([x[1] for x in v])), back_to_back_us_rounds=[round(x[1], 1) for x in v])
                                                   for k, v in xs.items()})
    return res


def inner(n):
    import torch
    from stitch_amd import ops
    a, b = scenes(1)[0]
    for _ in range(n):
        ops.feature_homography(a, b)
    torch.cuda.synchronize()


def kernel_trace(n=20):
    """per kernel name, launches and summed duration per call, from a traced child process of its own"""
    d = tempfile.mkdtemp(prefix="features_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "features", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--inner", str(n)]
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    path = (glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) or [None])[0]
    if path is None:
        raise RuntimeError(f"rocprofv3 wrote no kernel_stats.csv under {d}")
    rows = []
    for r in csv.DictReader(open(path)):
        name = re.sub(r"\(.*", "", re.sub(r"^void ", "", r["Name"]))
        name = re.sub(r"<.*", "", name)
        if name in KERNELS:
            rows.append(dict(name=name, launches_per_call=int(r["Calls"]) / n, us_per_call=float(r["TotalDurationNs"]) / n / 1e3))
    shutil.rmtree(d, ignore_errors=True)
    return dict(shape="1x3x512x512", calls=n, kernels=sorted(rows, key=lambda r: -r["us_per_call"]), kernel_us_per_call=sum(r["us_per_call"] for r in rows))


class _Pairs:
    """pairs held in memory as float [3,H,W] CPU tensors: the generic dataset of validate_with_model"""

    def __init__(self, n):
        self.items = [(a[0].cpu(), b[0].cpu()) for a, b in scenes(n)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def eval_bench(rounds, n=64):
    import torch
    from stitch_amd import evaluate as sev
    data = _Pairs(n)
    models = {k: seeded_model(k) for k in ("last_config_features", "last_config_only_homo")}
    samples, results, same = {k: [] for k in models}, {}, {k: True for k in models}
    with contextlib.redirect_stdout(io.StringIO()):
        for rnd in range(rounds + 1):                      # round 0: graph capture
            for k, m in models.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = sev.validate_with_model(m, data, batch_size=4)[0]
                same[k] = same[k] and (k not in results or repr(res) == repr(results[k]))
                results[k] = res
                torch.cuda.synchronize()
                if rnd:
                    samples[k].append(n / (time.perf_counter() - t0))
    return {k: dict(pairs_per_s_median=float(np.median(v)), pairs_per_s_rounds=[round(s, 1) for s in v], result_same_every_round=same[k], result={a: float(b) if isinstance(b, (int, float, np.floating)) else str(b) for a, b in results[k].items()})
            for k, v in samples.items()}


def out_child(pairs, passes=3):
    """this checkout's out.py loop with the default config: prints one JSON line of pairs/s per pass"""
    import torch
    import stitch_amd
    from PIL import Image
    from stitch_amd.data import structured_pair
    spec = importlib.util.spec_from_file_location("stitch_out_harness_features_bench", os.path.join(ROOT, "out.py"))
    outmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(outmod)
    root = tempfile.mkdtemp(prefix="features_loop_")
    names = []
    base = [structured_pair(512, 512, seed=40 + i) for i in range(8)]
    for i in range(pairs):
        d = os.path.join(root, "demo", f"p{i:03d}")
        os.makedirs(d)
        for n, t in zip(("input1.jpg", "input2.jpg"), base[i % 8]):
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
    rates = []
    with contextlib.redirect_stdout(io.StringIO()):
        for p in range(passes + 1):                        # pass 0: graph capture, file cache, lazy constants
            dst = os.path.join(root, f"run{p}") + "/"
            os.makedirs(dst)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outmod.run_pairs(cfg, todo, dst, model, comp, inp)
            torch.cuda.synchronize()
            if p:
                rates.append(pairs / (time.perf_counter() - t0))
            shutil.rmtree(dst)
    shutil.rmtree(root, ignore_errors=True)
    print("OUT_CHILD " + json.dumps(rates))


def out_bench(pairs, rounds, parent_root):
    roots = {"this_tree": ROOT}
    if parent_root:
        roots = dict({"parent_commit": os.path.abspath(parent_root)}, **roots)
    samples = {k: [] for k in roots}
    for _ in range(rounds):
        for k, r in roots.items():
            here = os.path.abspath(__file__) if r == ROOT else os.path.join(r, "tools", "_bench_features_child.py")
            if r != ROOT:
                shutil.copyfile(os.path.abspath(__file__), here)           # the parent checkout does not have this tool: the same child, its tree
            try:
                p = subprocess.run([sys.executable, here, "--out-child", str(pairs)], check=True, timeout=900, stdout=subprocess.PIPE, text=True, cwd=r)
            finally:
                if r != ROOT:
                    os.remove(here)
            line, = [ln for ln in p.stdout.splitlines() if ln.startswith("OUT_CHILD ")]
            samples[k] += json.loads(line[len("OUT_CHILD "):])
    res = {k: dict(pairs_per_s_median=float(np.median(v)), pairs_per_s_passes=[round(s, 2) for s in v]) for k, v in samples.items()}
    if parent_root:
        v = samples["parent_commit"]
        res["parent_spread_pairs_per_s"] = max(v) - min(v)
        res["this_tree_within_parent_scatter"] = bool(res["this_tree"]["pairs_per_s_median"] >= float(np.median(v)) - (max(v) - min(v)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit, for the out.py loop")
    ap.add_argument("--pairs", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-loops", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--inner", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out-child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.inner:
        return inner(a.inner)
    if a.out_child:
        return out_child(a.out_child)
    res = {"what": "ops.feature_homography (2048 hypotheses) beside predict_homo with the homography network at 512x512; times in microseconds", "rounds": a.rounds}
    if not a.no_trace:
        res["kernel_trace"] = kernel_trace()               # before this process opens the GPU: the traced child runs alone
    if not a.no_loops:
        res["out_loop_default_config"] = dict(pairs=a.pairs, depth=2, **out_bench(a.pairs, max(1, a.rounds // 2), a.parent_root))
    import stitch_amd  # noqa: F401
    res["call"] = call_bench(a.rounds)
    if not a.no_loops:
        res["evaluate_loop"] = dict(pairs=64, batch_size=4, **eval_bench(a.rounds))
    text = json.dumps(res, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
