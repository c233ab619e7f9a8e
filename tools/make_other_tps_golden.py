"""Golden vectors of tps_method="other" from the REFERENCE's own code (build container only; writes tests/golden/other_tps.npz).

    python tools/make_other_tps_golden.py

Imports core/inference/tps_methods/other_tps.py and core/inference/tps_pipline.py from the reference tree on CPU, with the
third-party stand-ins of oracle.ref_harness (imported, not edited).  cv2.remap is stood in for by the INTER_CUBIC restatement
(tests/_other_tps_ref.py with the package's coefficient table), so the warp output pins everything the reference itself does
(normalisation, to_pillow_fn, the float32 sgesv fit, the float64 grid and maps, the layout) around an unpinned cv2.remap.
Stored per point set: theta (reduced, [n+2, 2] float32 from numpy's sgesv) and mapx / mapy (float32) of
tps_theta_from_points / tps_grid / tps_grid_to_remap; on a seeded synthetic canvas also warp_by_tps(..., "other").
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "other_tps.npz")

WELL = dict(seed=11, out_h=140, out_w=180)          # synthetic canvas and well-conditioned point set
CHAIN_GRID = (267, 284)                             # the 533 x 567 chain canvas sampled on a half-size grid (same normalised spline)


def well_points():
    rng = np.random.default_rng(WELL["seed"])
    h, w = WELL["out_h"], WELL["out_w"]
    gx, gy = np.meshgrid(np.linspace(8, w - 9, 5), np.linspace(6, h - 7, 4))
    src = np.stack([gx.ravel(), gy.ravel()], 1) + rng.integers(-3, 4, (20, 2))
    dst = src + rng.normal(0, 2.0, src.shape)
    return src.astype(np.int64), dst.astype(np.float32)


def main():
    from oracle.ref_harness.make_tps_goldens import install_inference_stubs
    from oracle import tps_pipeline as otp
    import _other_tps_ref as R
    import stitch_amd
    table = stitch_amd.ops.cubic_remap_table()
    install_inference_stubs()
    cv2 = sys.modules["cv2"]
    cv2.INTER_CUBIC = 2

    def remap(img, mapx, mapy, interpolation):
        assert interpolation == cv2.INTER_CUBIC and img.dtype == np.uint8 and img.ndim == 3
        return R.remap_cubic(img.transpose(2, 0, 1).astype(np.int32), mapx, mapy, table).transpose(1, 2, 0).astype(np.uint8)
    cv2.remap = remap
    from core.inference.tps_methods import other_tps as ref_o
    from core.inference import tps_pipline as ref_tp

    out = {}

    def spline(name, ps, pd, out_h, out_w, grid_hw):
        c_src, c_dst = R.normalise(ps, out_h, out_w), R.normalise(pd, out_h, out_w)
        theta = ref_o.tps_theta_from_points(c_src, c_dst, reduced=True)
        grid = ref_o.tps_grid(theta, c_dst, grid_hw)
        mx, my = ref_o.tps_grid_to_remap(grid, grid_hw)
        assert theta.dtype == np.float32 and mx.dtype == np.float32
        out.update({f"{name}_points_src": np.asarray(ps), f"{name}_points_dst": np.asarray(pd, np.float32),
                    f"{name}_out_hw": np.array([out_h, out_w]), f"{name}_grid_hw": np.array(grid_hw),
                    f"{name}_theta": theta, f"{name}_mapx": mx, f"{name}_mapy": my})
        print(f"{name}: n {len(ps)}, |theta| max {np.abs(theta).max():.3e}, mapx {mx.min():.2f}..{mx.max():.2f}")

    ps, pd = well_points()
    spline("well", ps, pd, WELL["out_h"], WELL["out_w"], (WELL["out_h"], WELL["out_w"]))
    ch = np.load(os.path.join(ROOT, "tests", "golden", "tps_illcond_points.npz"))
    oh, ow = (int(v) for v in ch["out_hw"])
    spline("chain", ch["points_src"][0], ch["points_dst"][0], oh, ow, CHAIN_GRID)

    case = otp.synthetic_case(WELL["seed"], 120, 160, -9, -7, WELL["out_h"], WELL["out_w"])
    Hw, Hm = case["H_warp"], case["H_warp_mask"]
    res = ref_tp.warp_by_tps(Hw, Hm, torch.from_numpy(ps)[None], torch.from_numpy(pd)[None], WELL["out_h"], WELL["out_w"],
                             "other", 1.0, 1.0)
    assert res.shape == (1, 6, WELL["out_h"], WELL["out_w"]) and res.dtype == torch.float32
    out["warp_case"] = np.array([WELL["seed"], 120, 160, -9, -7, WELL["out_h"], WELL["out_w"]])
    out["warp_out"] = res[0].numpy().astype(np.uint8)
    out["note"] = np.array("tools/make_other_tps_golden.py: the reference's other_tps.py (theta by float32 sgesv, float64 maps) and "
                           "warp_by_tps(..., 'other') with cv2.remap stood in for by tests/_other_tps_ref.py")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
