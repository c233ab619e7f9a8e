"""dense_flow on the MI355X: `ops.dense_flow` per call beside `predict_flow_pair` with FlowFormer++ on seeded weights, its kernels one by one
with their traffic floors, evaluate.py's loop under `last_config_classical` and `last_config_features`, and out.py's loop with the default
config against another checkout's (the parent commit's).

    python tools/bench_dense_flow.py [--out profiles/dense_flow_bench.json] [--parent-root PATH] [--pairs 24] [--rounds 5]

* call: procedural 512x512 pairs (tests/_dense_flow_ref.py: a homography plus a smooth 3 px residual; image 2's right fifth masked), B = 1
  and 2, the defaults (5 levels, 4 iterations, radius 4).  `dense_flow` in its own workspace and `predict_flow_pair` of a seeded model (both
  directions, as the consistency mask needs them; `DenseFlow.flow_pair` is the like-for-like call and is timed too), alternating inside
  every round: a single call between HIP events (median of 30) and 30 calls back to back; median of the rounds.
* kernels: one `rocprofv3 --kernel-trace --stats` run of a child process of its own (no counters) making 20 calls at B = 1; per kernel the
  launches and the summed duration per call, beside the bytes every launch must move at least and the time they take at 6.3 TB/s.
* evaluate: `validate_with_model` (the pipelined loop of evaluate.py) on 64 pairs held in memory, batch 4, the two configs alternating; wall
  pairs/s and the metric, median of the rounds.
* out: tools/bench_features.py's `out_bench`: out.py's default loop in a child process per checkout and round.
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
KERNELS = ("df_luma_kernel", "df_down_kernel", "df_init_kernel", "df_iterate_kernel", "df_median_kernel")
HBM_BYTES_PER_S = 6.3e12


def _features_bench():
    spec = importlib.util.spec_from_file_location("_bench_features", os.path.join(ROOT, "tools", "bench_features.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def scenes(n, B=1):
    """n batches of procedural pairs as device tensors: (img1, img2 [B,3,512,512], mask2 [B,1,512,512])"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _dense_flow_ref as ref
    out = []
    for i in range(n):
        items = [ref.homography_residual_pair(512, 512, seed=50 + i * B + k, motion=(0, 0, 0, 0, 0)) for k in range(B)]
        a, b = (np.concatenate([it[j] for it in items]) for j in (0, 1))
        m2 = np.ones((B, 1, 512, 512), np.float32)
        m2[:, :, :, 410:] = 0
        out.append(tuple(torch.from_numpy(t).cuda() for t in (a, b * m2, m2)))
    return out


def traffic_floor(B=1, H=512, W=512, levels=5, iters=4):
    """{kernel: bytes per call every launch must at least read and write}: each operand once"""
    from stitch_amd import ops
    sizes = ops.dense_flow_level_sizes(H, W, levels)
    px = [B * h * w for h, w in sizes]
    return {"df_luma_kernel": px[0] * (12 + 12 + 4 + 6),                                                   # two images, one mask; V and m of both
            "df_down_kernel": sum(6 * px[l] + 6 * px[l + 1] for l in range(len(px) - 1)),
            "df_init_kernel": 8 * px[-1] + sum(8 * px[l + 1] + 8 * px[l] for l in range(len(px) - 1)),
            "df_iterate_kernel": iters * sum((2 + 2 + 1 + 1 + 8 + 8 + 1) * p for p in px),                 # V1, V2, m1, m2, U in; U, support out
            "df_median_kernel": iters * sum(16 * p for p in px) + 8 * px[0]}                               # + the fp32 flow once


def call_bench(rounds):
    import torch
    import stitch_amd
    from stitch_amd import ops
    bf = _features_bench()
    model = bf.seeded_model()
    lk = stitch_amd.DenseFlow()
    res = {}
    for B in (1, 2):
        a, b, m2 = scenes(1, B)[0]
        ws = torch.empty(ops.dense_flow_workspace_bytes(B, 512, 512), dtype=torch.uint8, device="cuda")
        flow, support = ops.dense_flow(a, b, mask2=m2, workspace=ws)
        variants = {"dense_flow": lambda: ops.dense_flow(a, b, mask2=m2, workspace=ws), "dense_flow_pair": lambda: lk.flow_pair(a, b, m2),
                    "predict_flow_pair_network": lambda: model.predict_flow_pair(a, b)}
        xs = {k: [] for k in variants}
        with torch.no_grad():
            for _ in range(rounds):
                for k, fn in variants.items():
                    xs[k].append(bf.timed(fn))
        res[f"B{B}"] = dict(supported_fraction=float(support.float().mean()), mean_flow_px=float(flow.abs().mean()),
                            **{k: dict(single_call_us_median=float(np.median([x[0] for x in v])), single_call_us_rounds=[round(x[0], 1) for x in v],
                                       back_to_back_us_median=float(np.median([x[1] for x in v])), back_to_back_us_rounds=[round(x[1], 1) for x in v])
                               for k, v in xs.items()})
    return res


def inner(n):
    import torch
    from stitch_amd import ops
    a, b, m2 = scenes(1)[0]
    for _ in range(n):
        ops.dense_flow(a, b, mask2=m2)
    torch.cuda.synchronize()


def kernel_trace(n=20):
    """per kernel name, launches and summed duration per call, from a traced child process of its own"""
    d = tempfile.mkdtemp(prefix="dense_flow_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "dense_flow", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--inner", str(n)]
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
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import torch
        import _dense_flow_ref as ref
        import _features_ref as fref
        self.items = []
        for i in range(n):
            a, b = ref.homography_residual_pair(512, 512, seed=50 + i, motion=fref.MOTIONS[i % 3])
            self.items.append((torch.from_numpy(a[0]), torch.from_numpy(b[0])))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def eval_bench(rounds, n=64):
    import torch
    from stitch_amd import evaluate as sev
    bf = _features_bench()
    data = _Pairs(n)
    models = {k: bf.seeded_model(k) for k in ("last_config_classical", "last_config_features")}
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
    return {k: dict(pairs_per_s_median=float(np.median(v)), pairs_per_s_rounds=[round(s, 1) for s in v], result_same_every_round=same[k],
                    result={a: float(b) if isinstance(b, (int, float, np.floating)) else str(b) for a, b in results[k].items()})
            for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit, for the out.py loop")
    ap.add_argument("--pairs", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-loops", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--inner", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.inner:
        return inner(a.inner)
    res = {"what": "ops.dense_flow (5 levels, 4 iterations, radius 4) beside predict_flow_pair with FlowFormer++ on seeded weights at 512x512; times in microseconds",
           "rounds": a.rounds}
    if not a.no_trace:
        res["kernel_trace"] = kernel_trace()               # before this process opens the GPU: the traced child runs alone
    if not a.no_loops:
        res["out_loop_default_config"] = dict(pairs=a.pairs, depth=2, **_features_bench().out_bench(a.pairs, max(1, a.rounds // 2), a.parent_root))
    import stitch_amd  # noqa: F401
    if "kernel_trace" in res:
        floor = traffic_floor()
        for r in res["kernel_trace"]["kernels"]:
            r["floor_bytes_per_call"] = floor[r["name"]]
            r["floor_us_at_6.3TBps"] = floor[r["name"]] / HBM_BYTES_PER_S * 1e6
    res["call"] = call_bench(a.rounds)
    if not a.no_loops:
        res["evaluate_loop"] = dict(pairs=64, batch_size=4, **eval_bench(a.rounds))
    text = json.dumps(res, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
