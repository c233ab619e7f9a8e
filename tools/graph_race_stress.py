"""Repeats tests/test_model_gpu.py::test_graphed_test_out_matches_eager's scenario (two test_out graphs replayed concurrently vs the eager forward)
and counts bitwise mismatches per output key:  ST_SPLIT3=0|1 python tools/graph_race_stress.py [reps]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import stitch_amd
from oracle import inputs, spec
cfg, _ = stitch_amd.load_inference_config("all_img1_with_inpaint_g12_transRef")
m = stitch_amd.build_model(cfg)
m.load_state_dict(spec.seeded_state_dict(1234), strict=True)
m = m.cuda().eval()
pairs = [inputs.structured_pair(320, 416, seed=70 + i, shift=(4 - 3 * i, 2 * i - 5)) for i in range(2)]
eager = [m(a.cuda(), b.cuda(), type="test_out") for a, b in pairs]
eager2 = [m(a.cuda(), b.cuda(), type="test_out") for a, b in pairs]
keys = ("blend_image", "output2", "mask2", "residual_flow", "occlusion_mask", "H")
print("eager vs eager:", {k: all(torch.equal(e[k], f[k]) for e, f in zip(eager, eager2)) for k in keys})
cpu_ref = [{k: e[k].cpu().clone() for k in keys} for e in eager]
gs = [m.graphed_test_out() for _ in range(2)]
streams = [torch.cuda.Stream() for _ in range(2)]
bad = {k: 0 for k in keys}
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
for rep in range(reps):
    handles = []
    for i, (a, b) in enumerate(pairs):
        streams[i].wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(streams[i]):
            handles.append(gs[i].launch(a.cuda(), b.cuda()))
        if os.environ.get("SERIAL") == "1":
            torch.cuda.synchronize()
    outs = [gs[i].finish(h) for i, h in enumerate(handles)]
    torch.cuda.synchronize()
    for i, (e, o) in enumerate(zip(eager, outs)):
        for k in keys:
            if not torch.equal(e[k], o[k]):
                bad[k] += 1
                if bad[k] <= 3:
                    d = (e[k].float() - o[k].float()).abs()
                    print(f"rep {rep} pair {i} {k}: {int((d > 0).sum())} of {d.numel()} differ, max {d.max().item():.3e}", flush=True)
                    print("   eager copy still equals its CPU snapshot:", torch.equal(e[k].cpu(), cpu_ref[i][k]), "| graph output equals the snapshot:", torch.equal(o[k].cpu(), cpu_ref[i][k]), flush=True)
                    idx = (d > 0).nonzero()
                    if k == "residual_flow" and bad[k] <= 3:
                        c, r, x0 = idx[0, 1].item(), idx[0, 2].item(), idx[0, 3].item()
                        gv = o[k][0, c, r, x0:x0 + 16].cpu()
                        print("   graph :", [round(v, 3) for v in gv.tolist()])
                        print("   eager :", [round(v, 3) for v in e[k][0, c, r, x0:x0 + 16].cpu().tolist()])
                        # is it a copy of something nearby / of the other pair / of the other channel?
                        cands = {}
                        for nm, t in (("eager same pair", e[k]), ("eager other pair", eager[1 - i][k]), ("graph other pair", outs[1 - i][k])):
                            tt = t[0].cpu()
                            best = None
                            for cc in range(2):
                                for rr in range(max(0, r - 3), min(tt.shape[1], r + 4)):
                                    for xx in range(max(0, x0 - 32), min(tt.shape[2] - 16, x0 + 33)):
                                        dd = (tt[cc, rr, xx:xx + 16] - gv).abs().max().item()
                                        if best is None or dd < best[0]:
                                            best = (dd, cc, rr, xx)
                            cands[nm] = best
                        print("   nearest 16-run (max abs diff, channel, row, col):", cands, "at", (c, r, x0), flush=True)
                    print("   where:", idx[:, 1].unique().tolist(), "rows", idx[:, 2].unique().tolist(), "cols", idx[:, 3].min().item(), "..", idx[:, 3].max().item(),
                          "graph values", o[k][tuple(idx[0].tolist())].item(), o[k][tuple(idx[-1].tolist())].item(), "eager", e[k][tuple(idx[0].tolist())].item(),
                          "| re-read after sync equal:", torch.equal(e[k], o[k]), flush=True)
print("SPLIT3 =", os.environ.get("ST_SPLIT3", "1"), "mismatches over", reps, "reps x 2 pairs:", bad)
