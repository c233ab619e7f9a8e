"""TransRef inpainter timing: median wall time of ``Inpainter.inpaint`` (hipGraph replay and eager launches) on a seeded network and
the golden's synthetic inputs, FLOP of the attention and GEMM families of one forward, and (``--profile``) a per-kernel table from
``rocprofv3 --kernel-trace --stats`` run on a child process of this tool, with the fraction of the fp32 matrix peak each family reaches.

    python tools/bench_transref.py [--iters 30] [--profile] [--out bench_transref.json]
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_FP32_MATRIX = 157.3e12          # MI355X, v_mfma_f32_32x32x2_f32 (spec)
ATT = ("tr_attention_kernel",)
GEMM = ("conv_gemm", "rowstream_gemm", "splitk_reduce", "narrow_conv", "skinny_gemm")


def inputs():
    g = np.load(os.path.join(ROOT, "tests", "golden", "transref_512.npz"))
    f = lambda a: torch.from_numpy(a.astype(np.float32))[None].cuda()   # noqa: E731
    mask = torch.from_numpy(g["mask"].astype(np.float32))[None, None].expand(1, 3, -1, -1).contiguous().cuda()
    return f(g["init"]), mask, f(g["control"])


def flops(inp):
    """(attention FLOP, GEMM FLOP) of one forward, counted at the ops layer"""
    import stitch_amd
    ops = stitch_amd.ops
    cnt = dict(att=0, gemm=0)
    oa, og = ops.tr_attention, ops.conv_gemm

    def att(q, k, v, out, heads, D, scale):
        cnt["att"] += 4 * q.shape[0] * k.shape[0] * D * heads
        return oa(q, k, v, out, heads, D, scale)

    def gemm(x, w, out, **kw):
        M = out.shape[0]
        cnt["gemm"] += 2 * M * w.shape[0] * w.shape[1]
        return og(x, w, out, **kw)

    ops.tr_attention, ops.conv_gemm = att, gemm
    try:
        x6, ref3, _, _, _ = inp.prepare(*inputs())
        inp.forward_eager(x6, ref3)
        torch.cuda.synchronize()
    finally:
        ops.tr_attention, ops.conv_gemm = oa, og
    return cnt["att"], cnt["gemm"]


def timed(fn, iters):
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def profile(n_calls):
    """(forwards, per-kernel time per network forward) of a rocprofv3 child that makes ``n_calls`` graph-replayed inpaint() calls
    (stand-alone kernel durations: tracing serialises the dispatches; the wrapper's own kernels are spread over the forwards)"""
    d = tempfile.mkdtemp(prefix="tr_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "tr", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--inner", str(n_calls)]
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    path = (glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) or [None])[0]
    if path is None:
        raise RuntimeError(f"rocprofv3 wrote no kernel_stats.csv under {d}")
    raw = [(re.sub(r"\(.*", "", re.sub(r"^void ", "", r["Name"]))[:90], int(r["Calls"]), float(r["TotalDurationNs"]))
           for r in csv.DictReader(open(path))]
    # network forwards traced (the capture's eager warm-up included): patch_block3's attention (D = 256) runs once per forward
    fw = sum(c for n, c, _ in raw if "tr_attention_kernel<256>" in n)
    rows = [dict(name=n, calls=c / fw, ms=t / fw / 1e6) for n, c, t in raw]
    return fw, sorted(rows, key=lambda r: -r["ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--inner", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import stitch_amd.transref as tr
    inp = tr.Inpainter(seed=0, device="cuda")
    x = inputs()
    if a.inner:                                      # profiled child: warm up (capture), then the measured calls
        inp.inpaint(*x[:2], control_image_tensor=x[2])
        for _ in range(a.inner):
            inp.inpaint(*x[:2], control_image_tensor=x[2])
        torch.cuda.synchronize()
        return
    inp.inpaint(*x[:2], control_image_tensor=x[2])
    t_graph = timed(lambda: inp.inpaint(*x[:2], control_image_tensor=x[2]), a.iters)
    inp.graph = False
    inp.inpaint(*x[:2], control_image_tensor=x[2])
    t_eager = timed(lambda: inp.inpaint(*x[:2], control_image_tensor=x[2]), a.iters)
    inp.graph = True
    f_att, f_gemm = flops(inp)
    res = dict(inpaint_ms_graph=t_graph, inpaint_ms_eager=t_eager, attention_gflop=f_att / 1e9, gemm_gflop=f_gemm / 1e9,
               origin_hw=list(x[0].shape[2:]))
    print(f"inpaint() {tuple(x[0].shape[2:])}: graph {t_graph:.2f} ms, eager {t_eager:.2f} ms (median of {a.iters}); "
          f"attention {f_att / 1e9:.2f} GFLOP, GEMM {f_gemm / 1e9:.2f} GFLOP per forward")
    if a.profile:
        fw, rows = profile(10)
        tot = sum(r["ms"] for r in rows)
        att = sum(r["ms"] for r in rows if any(k in r["name"] for k in ATT))
        gemm = sum(r["ms"] for r in rows if any(k in r["name"] for k in GEMM))
        print(f"kernel time per forward ({fw} traced) {tot:.3f} ms: attention {att:.3f} ms ({f_att / (att * 1e-3) / PEAK_FP32_MATRIX * 100:.1f} % of the fp32 "
              f"matrix peak), GEMM family {gemm:.3f} ms ({f_gemm / (gemm * 1e-3) / PEAK_FP32_MATRIX * 100:.1f} %)")
        for r in rows[:15]:
            print(f"{r['ms']:8.3f} ms  x{r['calls']:6.1f}  {r['name']}")
        res.update(kernel_ms=tot, attention_kernel_ms=att, gemm_kernel_ms=gemm,
                   attention_peak_frac=f_att / (att * 1e-3) / PEAK_FP32_MATRIX, gemm_peak_frac=f_gemm / (gemm * 1e-3) / PEAK_FP32_MATRIX,
                   top_kernels=rows[:15])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
