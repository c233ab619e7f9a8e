"""Golden vectors of FlowHomoAdpater's homography-only, H+flow and no-mask branches from the REFERENCE's own code (CPU only;
writes tests/golden/branches_*.npz).

    python tools/make_branch_goldens.py

The reference is built by oracle.ref_harness.stubs.build_reference (imported, not edited) with a cfg overlay per branch:
  only_homo=True                                        test_eval (core/flowHomoAdpater.py:115-118), seeded weights
  use_combine_h_flow=True, use_fb_consistency_mask=False test_eval (:144-164), damped weights
  use_fb_consistency_mask=False                          test_out (:347-353,374-376), damped weights, 512x512 and 320x480
Every recorded run is repeated with 1 instead of 8 CPU threads; the spread between the two is stored as ``*_floor_*``.

branches_kernel.npz holds the combined branch's geometric tail on its own (get_rigid_mesh / H2Mesh / warp of core/warp_utils.py:10-80
at per-pixel resolution, then the overlap test), B=2 x 96x128, given a DLT homography, a smooth residual flow and a uint8-valued
image 2: the input of the st_homo_flow_warp kernel test.  It also holds torch.inverse of 483 column-major 3x3 matrices (the layout
in which H2Mesh receives the first inverse), the pin of the second inverse's operation order.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import inputs, spec  # noqa: E402
from oracle.ref_harness import stubs  # noqa: E402
from oracle.ref_harness.make_goldens import OUT, checksum, packbits, sub  # noqa: E402

SHIPPED = dict(test_not_use_combine_h_flow=True, use_forward=False, use_fb_consistency_mask=True, use_whole_resolution=False)
OUT_SIZES = ((512, 512), (320, 480))


def _both(model, a, b, type):
    with torch.no_grad():
        torch.set_num_threads(8)
        o8 = model(a, b, type=type)
        torch.set_num_threads(1)
        o1 = model(a, b, type=type)
        torch.set_num_threads(8)
    return o8, o1


def _mx(x, y):
    return np.array(float((x - y).abs().max()))


def eval_branches(rec):
    a, b = inputs.structured_pair(512, 512, seed=7)
    # ---- only_homo (seeded weights: the homography network is the same in both weight sets) --------------------------------
    model, _ = stubs.build_reference(spec.seeded_state_dict(1234), overlay=dict(SHIPPED, only_homo=True))
    o8, o1 = _both(model, a, b, "test_eval")
    assert o8["flow_predictions"] is None and o8["overlap"] is None and o8["final_warp_output"] is o8["output_H"]
    rec["oh_keys"] = np.array(sorted(o8.keys()))
    rec["oh_H"] = o8["H"].numpy()
    rec["oh_output_H_sub"] = sub(o8["output_H"][:, 0:4], 4)
    rec["oh_output_H_cs"] = checksum(o8["output_H"])
    rec["oh_output_H_inv_cs"] = checksum(o8["output_H_inv"])
    rec["oh_floor_H_max"] = _mx(o8["H"], o1["H"])
    rec["oh_floor_output_H_max"] = _mx(o8["output_H"], o1["output_H"])
    # ---- use_combine_h_flow without the consistency mask (damped weights) ----------------------------------------------------
    model, _ = stubs.build_reference(spec.damped_state_dict(1234),
                                     overlay=dict(SHIPPED, use_combine_h_flow=True, use_fb_consistency_mask=False))
    o8, o1 = _both(model, a, b, "test_eval")
    assert len(o8["flow_predictions"]) == 1 and "origin_occlusion_mask" not in o8
    fin = o8["final_warp_output"]
    assert torch.equal(fin[:, 3], fin[:, 4]) and torch.equal(fin[:, 3], fin[:, 5])
    rec["cb_keys"] = np.array(sorted(o8.keys()))
    rec["cb_H"] = o8["H"].numpy()                                # the INVERSE of the DLT homography (reassigned at :150)
    rec["cb_flow_sub"] = sub(o8["flow_predictions"][0], 4)
    rec["cb_flow_cs"] = checksum(o8["flow_predictions"][0])
    rec["cb_final_sub"] = sub(fin[:, 0:4], 4)                   # channels 3..5 are equal: one mask channel is kept
    rec["cb_final_cs"] = checksum(fin)
    rec["cb_output_H_sub"] = sub(o8["output_H"][:, 0:4], 4)
    rec["cb_overlap_bits"] = packbits(o8["overlap"])
    rec["cb_floor_H_max"] = _mx(o8["H"], o1["H"])
    rec["cb_floor_flow_max_px"] = _mx(o8["flow_predictions"][0], o1["flow_predictions"][0])
    rec["cb_floor_final_max"] = _mx(fin, o1["final_warp_output"])
    rec["cb_floor_overlap_flips"] = np.array(int((o8["overlap"] != o1["overlap"]).sum()))
    # the branch's sensitivity to the homography network: the same run with the corner offsets moved by uniform noise of
    # +-1.5e-5 px (the size of the GPU network's offset difference, tests/test_model_gpu.py::test_homography_offsets_512),
    # six draws; final_warp_output's max difference where the mask channels agree
    sens = []
    predict_homo = model.predict_homo
    for seed in range(6):
        gen = torch.Generator().manual_seed(seed)
        model.predict_homo = lambda x, y: (lambda off: off + 1.5e-5 * (2 * torch.rand(off.shape, generator=gen) - 1))(predict_homo(x, y))
        with torch.no_grad():
            o = model(a, b, type="test_eval")
        got, want = sub(o["final_warp_output"][:, 0:4], 4), rec["cb_final_sub"]
        sens.append(float((np.abs(got[:, 0:3] - want[:, 0:3]) * (got[:, 3:4] == want[:, 3:4])).max()))
    model.predict_homo = predict_homo
    rec["cb_sens_offsets_final_max"] = np.array(sens)
    print("eval branches:", {k: v.tolist() for k, v in rec.items() if "_floor_" in k}, flush=True)


def out_nomask(rec):
    model, _ = stubs.build_reference(spec.damped_state_dict(1234), overlay=dict(SHIPPED, use_fb_consistency_mask=False))
    for (h, w) in OUT_SIZES:
        p = f"out{h}x{w}_"
        a, b = inputs.structured_pair(h, w, seed=7)
        o8, o1 = _both(model, a, b, "test_out")
        assert "occlusion_mask" not in o8 and "origin_occlusion_mask" not in o8
        rec[p + "keys"] = np.array(sorted(o8.keys()))
        rec[p + "ints"] = np.array([o8["width_min"], o8["height_min"], o8["out_height"], o8["out_width"]])
        rec[p + "H"] = o8["H"].numpy()
        rec[p + "I_mat"] = o8["I_mat"].numpy()
        rec[p + "blend_sub"] = o8["blend_image"][..., ::2, ::2].contiguous().numpy()
        rec[p + "blend_cs"] = checksum(o8["blend_image"])
        rec[p + "mask1_bits"], rec[p + "mask2_bits"] = packbits(o8["mask1"]), packbits(o8["mask2"])
        rec[p + "warp_mask_bits"] = packbits(o8["warp_input2_mask"])
        rec[p + "residual_flow_sub"] = sub(o8["residual_flow"], 8)
        rec[p + "final_warp_cs"] = checksum(o8["final_warp"])
        rec[p + "output2_cs"] = checksum(o8["output2"])
        same = [o1[k] == o8[k] for k in ("width_min", "height_min", "out_height", "out_width")]
        assert all(same), "the reference's canvas size moved with the thread count"
        d = (o8["blend_image"].int() - o1["blend_image"].int()).abs()
        rec[p + "floor_blend_gt2_frac"] = np.array(float((d > 2).double().mean()))
        rec[p + "floor_H_max"] = _mx(o8["H"], o1["H"])
        rec[p + "floor_residual_flow_max_px"] = _mx(o8["residual_flow"], o1["residual_flow"])
        print(p, {k: v.tolist() for k, v in rec.items() if k.startswith(p) and ("floor" in k or k.endswith("ints"))}, flush=True)


def kernel_case(rec):
    stubs.install()
    import core.udis_utils.torch_DLT as torch_DLT
    from core.warp_utils import H2Mesh, get_rigid_mesh, warp
    g = torch.Generator().manual_seed(11)
    B, h, w = 2, 96, 128
    src = torch.tensor([[0., 0.], [w, 0.], [0., h], [w, h]]).unsqueeze(0).expand(B, -1, -1)
    motion = (torch.rand(B, 4, 2, generator=g) - 0.5) * 24.0
    H = torch_DLT.tensor_DLT(src / 8, (src + motion) / 8)                        # flowHomoAdpater.py:96
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    amp = (torch.rand(B, 2, 1, 1, generator=g) - 0.5) * 6.0
    flow = (amp * torch.stack([torch.sin(xx / 17.0 + yy / 29.0), torch.cos(yy / 13.0 - xx / 23.0)])).contiguous()
    image2 = torch.randint(0, 256, (B, 3, h, w), generator=g).float()
    with torch.no_grad():                                                       # flowHomoAdpater.py:150-164
        Hi = torch.inverse(H)
        rigid = get_rigid_mesh(batch_size=B, height=h, width=w, grid_h=h - 1, grid_w=w - 1)
        mesh = H2Mesh(Hi, rigid, grid_h=h - 1, grid_w=w - 1)
        final_flow = (mesh - rigid).permute(0, 3, 1, 2) + flow
        fin = warp(torch.cat((image2, torch.ones_like(image2)), 1), final_flow)
        ov = fin[:, 3:6].mean(dim=1)
        overlap = torch.where(ov < 0.9, torch.ones_like(ov), torch.zeros_like(ov))
    assert torch.equal(fin[:, 3], fin[:, 4]) and torch.equal(fin[:, 3], fin[:, 5])
    rec.update(k_H=H.numpy(), k_Hi=Hi.numpy(), k_flow=flow.numpy(), k_image2=image2.numpy().astype(np.uint8),
               k_final4=fin[:, 0:4].contiguous().numpy(), k_final_cs=checksum(fin), k_overlap=overlap.numpy().astype(np.uint8),
               k_final_flow=final_flow.numpy())
    # torch.inverse of column-major 3x3s (the layout of a torch.inverse result, as H2Mesh receives Hi): the pin of mat3_inv_cm
    A = torch.cat([torch.eye(3) + s * torch.randn(96, 3, 3, generator=g) for s in (0.01, 0.1, 0.4, 1.0, 3.0)]
                  + [Hi, torch.inverse(torch.tensor([[1.0, 0.2, 3.0], [0.1, 0.9, -2.0], [1e-3, 2e-3, 1.0]]))[None]])
    cm = A.mT.contiguous().mT
    assert not cm.is_contiguous() and torch.equal(cm, A)
    rec.update(k_cm_in=A.contiguous().numpy(), k_cm_inv=torch.inverse(cm).contiguous().numpy())
    print("kernel case: overlap px", int(overlap.sum()), "final_flow absmax", float(final_flow.abs().max()), flush=True)


def main():
    torch.manual_seed(0)
    rec = {}
    kernel_case(rec)
    np.savez_compressed(os.path.join(OUT, "branches_kernel.npz"), **rec)
    rec = {}
    eval_branches(rec)
    np.savez_compressed(os.path.join(OUT, "branches_eval_512.npz"), **rec)
    rec = {}
    out_nomask(rec)
    np.savez_compressed(os.path.join(OUT, "branches_out.npz"), **rec)
    for f in ("branches_kernel.npz", "branches_eval_512.npz", "branches_out.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
