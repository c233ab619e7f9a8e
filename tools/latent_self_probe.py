"""st_latent_self_attn_split3 against the two launches it replaces (GPU box): python tools/latent_self_probe.py [--rows 65536] [--launches 50]

Stand-alone timing at the benchmark's shape (65 536 rows = 8 192 cost maps of 8 latents): a hipGraph of `launches` launches, HIP events around
`reps` replays, the median per launch.  Prints the three kernels alone, the pair, the fused launch, the bytes each moves and whether the results
are the same bits.  The gate of the fused path: fused < rowlin + attention_small."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stitch_amd  # noqa: E402

ops = stitch_amd.ops


def graph_us(fn, launches, reps):
    """median microseconds per call of fn: `launches` calls captured into one hipGraph, replayed `reps` times between HIP events"""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(launches):
                fn()
        g.replay()
        s.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            g.replay()
            b.record(s)
            s.synchronize()
            ts.append(a.elapsed_time(b) / launches * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    M = a.rows
    assert M % 8 == 0
    g = torch.Generator().manual_seed(7)
    x = torch.randn(M, 128, generator=g).cuda()
    w = (torch.randn(384, 128, generator=g) / 128 ** 0.5).cuda()
    b = (0.1 * torch.randn(384, generator=g)).cuda()
    lin, fused = ops.rowlin128_split3_pack(w, b), ops.latent_self_attn_split3_pack(w, b)
    qkv = torch.empty(M, 384, device="cuda")
    att, out = torch.empty(M, 128, device="cuda"), torch.empty(M, 128, device="cuda")

    def rowlin():
        ops.rowlin128_split3(x, qkv, lin, ln_eps=1e-5)

    def attn():
        ops.attention_small(qkv[:, :128], (8 * 384, 384), qkv[:, 128:256], (8 * 384, 384), qkv[:, 256:], (8 * 384, 384), att, (8 * 128, 128),
                            M // 8, 8, 8, 8, 16, 16 ** -0.5)

    def pair():
        rowlin()
        attn()

    def one():
        ops.latent_self_attn_split3(x, out, fused, ln_eps=1e-5)

    pair()
    one()
    torch.cuda.synchronize()
    same = torch.equal(att, out)
    res = {}
    for name, fn in (("rowlin128_split3", rowlin), ("attention_small", attn), ("pair", pair), ("fused", one), ("pair_again", pair), ("fused_again", one)):
        res[name] = graph_us(fn, a.launches, a.reps)
        print(f"{name:18s} {res[name][0]:8.2f} us per launch (min {res[name][1]:.2f}, max {res[name][2]:.2f}; {a.launches} launches per graph, {a.reps} replays)", flush=True)
    mb = M * 128 * 4 / 1e6
    p, f = min(res["pair"][0], res["pair_again"][0]), max(res["fused"][0], res["fused_again"][0])
    print(f"{M} rows: rows in {mb:.1f} MB; pair moves {mb * (1 + 3 + 3 + 1):.1f} MB in {p:.2f} us, fused {mb * 2:.1f} MB in {f:.2f} us "
          f"({mb * 2 / f:.2f} TB/s): x{p / f:.2f}; same bits: {same}")
    print("GATE (slower fused run < faster pair run):", "pass" if f < p else "FAIL")


if __name__ == "__main__":
    main()
