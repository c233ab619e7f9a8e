"""feature_align_ms on the MI355X: `ops.feature_homography_ms` per call beside `ops.feature_homography`, and its kernels one by one.

    python tools/bench_features_ms.py [--out profiles/features_ms_bench.json] [--rounds 4]

* call: procedural 512x512 pairs with a known homography (tests/_features_ref.py), B = 1 and 8, 2048 hypotheses, 6 levels, oriented.  The
  multi-scale call and the single-scale call, each in its own workspace, alternating inside every round: a single call between HIP events
  (median of 30) and 30 calls back to back; median of the rounds.
* kernels: one `rocprofv3 --kernel-trace --stats` run of a child process of its own making 20 calls at B = 1; per kernel the launches and the
  summed duration per call.
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("ftms_luma_kernel", "ftms_down_kernel", "ftms_detect_kernel", "ftms_describe_kernel", "ft_match_kernel", "ft_compact_kernel", "ftms_norm_kernel",
           "ft_hyp_kernel", "ftms_refit_kernel")


def _bench_features():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_features
    return bench_features


def call_bench(rounds):
    import torch
    from stitch_amd import ops
    bf = _bench_features()
    res = {}
    for B in (1, 8):
        a, b = bf.scenes(1, B)[0]
        ws_ms = torch.empty(ops.feature_ms_workspace_bytes(B, 512, 512), dtype=torch.uint8, device="cuda")
        ws = torch.empty(ops.feature_workspace_bytes(B, 512, 512), dtype=torch.uint8, device="cuda")
        info_ms = ops.feature_homography_ms(a, b, workspace=ws_ms)[2].cpu().numpy()
        info = ops.feature_homography(a, b, workspace=ws)[2].cpu().numpy()
        variants = {"feature_homography_ms": lambda: ops.feature_homography_ms(a, b, workspace=ws_ms), "feature_homography": lambda: ops.feature_homography(a, b, workspace=ws)}
        xs = {k: [] for k in variants}
        for _ in range(rounds):
            for k, fn in variants.items():
                xs[k].append(bf.timed(fn))
        res[f"B{B}"] = dict(info_ms=info_ms.tolist(), info=info.tolist(), slots_ms=ops.feature_ms_slots(512, 512), slots=ops.feature_slots(512, 512),
                            workspace_bytes_ms=ws_ms.numel(), workspace_bytes=ws.numel(),
                            **{k: dict(single_call_us_median=float(np.median([x[0] for x in v])), single_call_us_rounds=[round(x[0], 1) for x in v],
                                       back_to_back_us_median=float(np.median([x[1] for x in v])), back_to_back_us_rounds=[round(x[1], 1) for x in v])
                               for k, v in xs.items()})
    return res


def inner(n):
    import torch
    from stitch_amd import ops
    a, b = _bench_features().scenes(1)[0]
    for _ in range(n):
        ops.feature_homography_ms(a, b)
    torch.cuda.synchronize()


def kernel_trace(n=20):
    """per kernel name, launches and summed duration per call, from a traced child process of its own"""
    d = tempfile.mkdtemp(prefix="features_ms_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "features_ms", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--inner", str(n)]
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
    return dict(shape="1x3x512x512", levels=6, calls=n, kernels=sorted(rows, key=lambda r: -r["us_per_call"]), kernel_us_per_call=sum(r["us_per_call"] for r in rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--inner", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.inner:
        return inner(a.inner)
    res = {"what": "ops.feature_homography_ms (6 levels, oriented, 2048 hypotheses) beside ops.feature_homography at 512x512; times in microseconds", "rounds": a.rounds}
    if not a.no_trace:
        res["kernel_trace"] = kernel_trace()               # before this process opens the GPU: the traced child runs alone
    import stitch_amd  # noqa: F401
    res["call"] = call_bench(a.rounds)
    text = json.dumps(res, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
