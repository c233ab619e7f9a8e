"""Time the out.py stages after the forward on one 512x512 pair (HIP events): test_out forward, TPS post-pipeline with the
configured mix_fn (pass-through inpainter), composition.  Random-init weights, structured synthetic pair."""
import importlib, sys, time, torch
sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import stitch_amd
from stitch_amd.data import structured_pair
cfg, tpc = stitch_amd.load_inference_config("all_img1_with_inpaint_g12_transRef")
from oracle import spec            # seeded weights (bounded scales): random init drives the flow past the pipeline's flow limit
model = stitch_amd.build_model(cfg)
model.load_state_dict(spec.seeded_state_dict(1234), strict=True)
model = model.cuda().eval()
comp = stitch_amd.composition.Network().cuda().eval()
a, b = (t.cuda() for t in structured_pair(512, 512, seed=7))
mix_fn = importlib.import_module(f"stitch_amd.mix_methods.{tpc.mix_method}").mix_fn
inp = importlib.import_module("stitch_amd.mix_methods.utils.passthrough_inpainter").inpainter
fn = lambda **kw: mix_fn(**kw, inpainter=inp, use_composition=False, is_plot=False, resize_to_area_limit_before_inpaint=750 * 750)
def run(tps_method):
    tpc.tps_method = tps_method
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t0 = time.perf_counter()
    ev[0].record()
    out = model(a, b, type="test_out")
    ev[1].record()
    inputs = dict(output1=out["output1"], mask1=out["mask1"], H_warp=out["H_warp"], H_warp_mask=out["H_warp_mask"], final_warp=out["final_warp"],
                  mask2=out["mask2"], residual_flow=out["residual_flow"], valid=None, occlusion_mask=out["occlusion_mask"],
                  border_points_mask=out["occlusion_mask"])
    limit = dict(width_min=out["width_min"], height_min=out["height_min"], out_height=out["out_height"], out_width=out["out_width"])
    new = stitch_amd.tps_pipeline.tps_H_warp(inputs, limit, tpc, inpaint_fn=fn)
    ev[2].record()
    m1, m2 = (out["mask1"] > 0.5).float(), (new["mask2"].repeat(1, 3, 1, 1) > 0.5).float()
    c = stitch_amd.composition.compose(comp, out["output1"], new["output2"], m1, m2)
    ev[3].record(); torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(3)], wall, new["points_src"].shape[1], (out["out_height"], out["out_width"])
for m in ("kornia", "opencv", "other"):
    run(m)
    ts, wall, n, canvas = run(m)
    print(f"tps_method={m}: canvas {canvas}, {n} control points: forward {ts[0]:.2f} ms, post-pipeline {ts[1]:.2f} ms, composition {ts[2]:.2f} ms; wall {1e3*wall:.1f} ms")

# the network above leaves no control point on this pair; time the post-pipeline alone on a synthetic test_out-shaped case
from types import SimpleNamespace
from oracle import tps_pipeline as otp
case = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in otp.synthetic_case(5, 512, 544, -21, -13, 548, 588).items()}
limit = dict(width_min=-21, height_min=-13, out_height=548, out_width=588)
for m in ("kornia", "opencv", "other"):
    tpc.tps_method = m
    for rep in range(2):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        new = stitch_amd.tps_pipeline.tps_H_warp(case, SimpleNamespace(**limit), tpc, inpaint_fn=fn)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    pts_a, pts_b = new["points_dst"][0].float().cuda(), new["points_src"][0].float().cuda()
    e0.record()
    if m == "other":
        stitch_amd.ops.tps_other_solve(pts_b / torch.tensor([588.0, 548.0], device="cuda"), pts_a / torch.tensor([588.0, 548.0], device="cuda"))
    else:
        stitch_amd.ops.tps2_solve(pts_a, pts_b if m == "kornia" else pts_a, pts_b, mode=0 if m == "kornia" else 1)
    e1.record(); torch.cuda.synchronize()
    print(f"synthetic 548x588 canvas, tps_method={m}: {new['points_src'].shape[1]} control points, tps_H_warp + mix_fn wall {1e3*dt:.2f} ms (TPS solve alone {e0.elapsed_time(e1):.2f} ms)")

# warp_by_tps alone, "opencv" (pixel-unit spline sampled bilinearly, mode 3) next to "other" (per-axis splines, fp64 maps, bicubic
# remap): on the synthetic canvas above and on the 533 x 567 chain canvas with its 101 control points (tests/golden/tps_illcond_points.npz)
import os
import numpy as np
def time_warp(m, Hw, Hm, ps, pd, oh, ow, reps=20):
    for _ in range(3):
        stitch_amd.tps_pipeline.warp_by_tps(Hw, Hm, ps, pd, oh, ow, m, 1.0, 1.0)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        stitch_amd.tps_pipeline.warp_by_tps(Hw, Hm, ps, pd, oh, ow, m, 1.0, 1.0)
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))
ch = np.load(os.path.join(__file__.rsplit("/tools/", 1)[0], "tests", "golden", "tps_illcond_points.npz"))
coh, cow = (int(v) for v in ch["out_hw"])
chain = otp.synthetic_case(3, 512, 512, -(cow - 512) // 2, -(coh - 512) // 2, coh, cow)
cases = [("synthetic 548x588", case["H_warp"], case["H_warp_mask"], new["points_src"], new["points_dst"], 548, 588),
         (f"chain {coh}x{cow}", chain["H_warp"].cuda(), chain["H_warp_mask"].cuda(), torch.from_numpy(ch["points_src"]),
          torch.from_numpy(ch["points_dst"]), coh, cow)]
for label, Hw, Hm, ps, pd, oh, ow in cases:
    line = [f"{m} {time_warp(m, Hw, Hm, ps, pd, oh, ow):.3f} ms" for m in ("opencv", "other")]
    # the two "other" kernels alone (HIP events, weights fitted once)
    cs = torch.stack([ps[0, :, 0].double() / ow, ps[0, :, 1].double() / oh], 1).float().cuda()
    cd = torch.stack([pd[0, :, 0].double() / ow, pd[0, :, 1].double() / oh], 1).float().cuda()
    w = stitch_amd.ops.tps_other_solve(cs, cd)
    x = torch.cat((Hw, Hm), 1).float().contiguous()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for rep in range(5):
        ev[0].record(); mx, my = stitch_amd.ops.tps_other_maps(cs, cd, oh, ow, weights=w); ev[1].record()
        stitch_amd.ops.remap_cubic(x, mx, my); ev[2].record(); torch.cuda.synchronize()
    print(f"warp_by_tps {label}, {ps.shape[1]} control points (median of 20, wall incl. host sync): " + ", ".join(line)
          + f"; other kernels: maps {ev[0].elapsed_time(ev[1]):.3f} ms, remap {ev[1].elapsed_time(ev[2]):.3f} ms")
