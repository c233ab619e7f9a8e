"""The branch configs and goldens of tests/test_branches_gpu.py, checked without a GPU."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _cfg(name):
    import importlib
    return importlib.import_module(f"configs.{name}").config_dict


def test_branch_configs_differ_from_last_config_only_in_named_keys():
    base = _cfg("last_config")
    for name, changed in (("last_config_only_homo", {"only_homo": True}),
                          ("last_config_combine_h_flow", {"use_combine_h_flow": True, "use_fb_consistency_mask": False})):
        cfg = _cfg(name)
        assert set(cfg) == set(base)
        assert {k: cfg[k] for k in cfg if cfg[k] != base[k]} == changed, name
    assert base["only_homo"] is False and base["use_combine_h_flow"] is False and base["use_fb_consistency_mask"] is True


def test_branch_goldens_hold_every_array_the_gpu_tests_read():
    need = {
        "branches_eval_512.npz": ["oh_keys", "oh_H", "oh_output_H_sub", "cb_keys", "cb_H", "cb_flow_sub", "cb_final_sub",
                                  "cb_overlap_bits", "cb_floor_overlap_flips", "cb_sens_offsets_final_max"],
        "branches_kernel.npz": ["k_H", "k_Hi", "k_flow", "k_image2", "k_final4", "k_overlap"],
        "branches_out.npz": [f"out{h}x{w}_{k}" for (h, w) in ((512, 512), (320, 480))
                             for k in ("keys", "ints", "H", "blend_sub")],
    }
    for f, keys in need.items():
        path = os.path.join(GOLDEN, f)
        assert os.path.getsize(path) < 1 << 20
        g = np.load(path)
        missing = [k for k in keys if k not in g.files]
        assert not missing, (f, missing)
    g = np.load(os.path.join(GOLDEN, "branches_eval_512.npz"))
    assert g["oh_output_H_sub"].shape == (1, 4, 128, 128) and g["cb_final_sub"].shape == (1, 4, 128, 128)
    assert "origin_occlusion_mask" not in set(g["cb_keys"]) and "origin_occlusion_mask" not in set(g["oh_keys"])
    o = np.load(os.path.join(GOLDEN, "branches_out.npz"))
    assert "occlusion_mask" not in set(o["out512x512_keys"])


# ---- the combined branch's arithmetic, restated in numpy (csrc/geom.hip: mat3_inv_cm and homo_flow_warp_kernel) -----------
from oracle.mat3 import F32, inv3_column_major  # noqa: E402


def _golden(name):
    return np.load(os.path.join(GOLDEN, name))


def test_column_major_inverse_restatement_matches_torch_bit_for_bit():
    g = _golden("branches_kernel.npz")
    got = np.stack([inv3_column_major(m) for m in g["k_cm_in"]])
    assert np.array_equal(got.view(np.uint32), g["k_cm_inv"].view(np.uint32))


def test_combined_branch_mesh_and_flow_restatement_matches_reference():
    """H2Mesh's projection of the per-pixel rigid mesh through inverse(Hi) and final_flow = (mesh - grid) + flow, as
    homo_flow_warp_kernel computes them: x, 1, y summed in that order, unfused; reproduces the reference's final_flow bit for bit."""
    import torch
    g = _golden("branches_kernel.npz")
    B, _, h, w = g["k_flow"].shape
    x = torch.linspace(0.0, float(w), w).numpy()[None, :].repeat(h, 0)       # get_rigid_mesh(grid_w = w - 1)
    y = torch.linspace(0.0, float(h), h).numpy()[:, None].repeat(w, 1)
    for b in range(B):
        p = inv3_column_major(g["k_Hi"][b]).reshape(-1)
        t = [((p[3 * r] * x).astype(F32) + p[3 * r + 2]).astype(F32) + (p[3 * r + 1] * y).astype(F32) for r in range(3)]
        fx = ((t[0] / t[2]).astype(F32) - x).astype(F32) + g["k_flow"][b, 0]
        fy = ((t[1] / t[2]).astype(F32) - y).astype(F32) + g["k_flow"][b, 1]
        assert np.array_equal(fx.view(np.uint32), g["k_final_flow"][b, 0].view(np.uint32))
        assert np.array_equal(fy.view(np.uint32), g["k_final_flow"][b, 1].view(np.uint32))
