"""Shared inputs of tests/test_multiband_cpu.py and tests/test_multiband_gpu.py: masks for the distance transform, mask pairs and image pairs
for the blend.  Everything is seeded."""
import numpy as np


def edt_cases():
    """(name, bool mask): 1x1, 1x7, 7x1, 13x17, 32x33 at densities 0.05 / 0.5 / 0.95, all ones, all zeros, a single zero"""
    rng = np.random.default_rng(20260101)
    out = []
    for H, W in ((1, 1), (1, 7), (7, 1), (13, 17), (32, 33)):
        for dens in (0.05, 0.5, 0.95):
            out.append((f"{H}x{W}@{dens}", rng.random((H, W)) < dens))
        out.append((f"{H}x{W}@ones", np.ones((H, W), bool)))
        out.append((f"{H}x{W}@zeros", np.zeros((H, W), bool)))
        m = np.ones((H, W), bool)
        m[rng.integers(H), rng.integers(W)] = False
        out.append((f"{H}x{W}@single", m))
    return out


def quads(H, W):
    """two overlapping quadrilateral masks [1,H,W] float32"""
    y, x = np.mgrid[:H, :W]
    m1 = (x < 0.62 * W + 0.1 * y) & (y > 0.08 * H) & (y < 0.93 * H) & (x > 0.04 * W)
    m2 = (x > 0.33 * W + 0.2 * y) & (y > 0.17 * H) & (y < 0.97 * H) & (x < 0.96 * W)
    return m1[None].astype(np.float32), m2[None].astype(np.float32)


def mask_cases(H, W):
    y, x = np.mgrid[:H, :W]
    f = lambda b: b[None].astype(np.float32)                                # noqa: E731
    q1, q2 = quads(H, W)
    full = np.ones((H, W), bool)
    centre = (abs(y - H // 2) <= H // 5) & (abs(x - W // 2) <= W // 5)
    pinhole = full.copy()
    pinhole[0, 0] = False                      # image 1 misses one corner pixel: only the canvas ring keeps image 2 from owning everything
    return {"quads": (q1, q2), "disjoint": (f(x < W // 3), f(x > W - 1 - W // 3)), "nested": (f(full), f(centre)), "identical": (q1, q1.copy()),
            "m2_empty": (q1, f(~full)), "both_empty": (f(~full), f(~full)), "pinhole": (f(pinhole), f(full))}


def noise_pair(H, W, seed, lo=-30.0, hi=290.0):
    rng = np.random.default_rng(seed)
    return (rng.random((3, H, W)) * (hi - lo) + lo).astype(np.float32), (rng.random((3, H, W)) * (hi - lo) + lo).astype(np.float32)
