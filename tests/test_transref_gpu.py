"""TransRef inpainter on the MI355X: the new kernels (csrc/transref.hip, the LeakyReLU epilogue) against float64, the network and the
wrapper against the reference's own fp64 run (tests/golden/transref_512.npz, tools/make_transref_golden.py), graph replay against
eager, and the plug-in through mix_fn and out.py.  Bounds fixed from the reference's own spread before the first GPU run:
attention error <= 2x torch-CPU fp32's error against fp64; network output <= max(3 x the reference's fp32 spread, 2e-5)."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _deform_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "transref_512.npz")


def _ops():
    import stitch_amd
    return stitch_amd.ops


def _attn64(q, k, v, heads, D, scale):
    out = []
    for h in range(heads):
        s = slice(h * D, (h + 1) * D)
        a = torch.softmax((q[:, s] @ k[:, s].T) * scale, dim=-1)
        out.append(a @ v[:, s])
    return torch.cat(out, 1)


ATT_CASES = [  # (Nq, Nk, heads, D, scale): every Block / Block_Ref / Block_dec / non-local shape of the network, ragged key counts
    (16384, 1024, 1, 64, None), (4096, 1024, 2, 64, None), (1024, 256, 4, 80, None), (256, 256, 4, 128, None),
    (4096, 256, 1, 128, None), (1024, 256, 2, 160, None), (256, 64, 2, 256, None), (64, 64, 8, 64, None),
    (4096, 1024, 1, 32, 1.0), (1024, 256, 1, 32, 1.0), (256, 64, 1, 32, 1.0), (16, 4, 1, 32, 1.0),
    (100, 1, 2, 80, None), (77, 17, 1, 64, None), (300, 1000, 2, 160, None), (33, 1000, 1, 256, 1.0),
]


@pytest.mark.parametrize("Nq,Nk,heads,D,scale", ATT_CASES)
def test_attention_vs_fp64(Nq, Nk, heads, D, scale):
    ops = _ops()
    g = torch.Generator().manual_seed(Nq + 7 * Nk + D)
    C = heads * D
    scale = D ** -0.5 if scale is None else scale
    # strided views: q a column slice of a wider buffer, k / v the two halves of one kv buffer (as the network lays them out)
    qb = torch.randn((Nq, C + 16), generator=g)
    kv = torch.randn((Nk, 2 * C), generator=g)
    q, k, v = qb[:, 8:8 + C], kv[:, :C], kv[:, C:]
    ref = _attn64(q.double(), k.double(), v.double(), heads, D, scale)
    cpu32 = _attn64(q, k, v, heads, D, scale)
    err32 = (cpu32.double() - ref).abs().max().item()
    qd, kvd = qb.cuda(), kv.cuda()
    ob = torch.full((Nq, C + 4), float("nan"), device="cuda")
    ops.tr_attention(qd[:, 8:8 + C], kvd[:, :C], kvd[:, C:], ob[:, :C], heads, D, scale)
    got = ob[:, :C].cpu().double()
    assert torch.isnan(ob[:, C:].cpu()).all()                      # nothing written past the view
    err = (got - ref).abs().max().item()
    print(f"attention Nq {Nq} Nk {Nk} heads {heads} D {D}: err {err:.2e} (torch fp32 {err32:.2e})")
    assert err <= 2 * err32 if err32 > 0 else err <= 1e-7


def test_attention_rejects_unsupported_head_dim():
    ops = _ops()
    x = torch.zeros((4, 48), device="cuda")
    with pytest.raises(ops.StitchErrorBase):
        ops.tr_attention(x, x, x, torch.empty_like(x), 1, 48, 1.0)


def test_deform_im2col_and_conv_vs_fp64():
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    C, H, W = 64, 24, 20
    x = torch.randn((1, C, H, W), generator=g)
    off = torch.randn((1, 18, H, W), generator=g) * 2.5                  # fractional
    off[:, :, :4] *= 12                                                   # large: far outside the image
    off[:, 0::2, :, -3:] = torch.tensor(float(H))                         # h >= H: zero
    off[:, 1::2, 5, :] = -0.999                                           # w just above -1 near column 0: partial corners
    w = torch.randn((C, C, 3, 3), generator=g) / (9 * C) ** 0.5
    ref_cols = _deform_ref.deform_im2col(x.double(), off.double())        # [1, 9, C, H, W]
    ref = _deform_ref.deform_conv2d(x.double(), off.double(), w.double())
    xd = x[0].permute(1, 2, 0).reshape(H * W, C).contiguous().cuda()
    od = off[0].permute(1, 2, 0).reshape(H * W, 18).contiguous().cuda()
    cols = ops.tr_deform_im2col(xd, od, torch.empty((H * W, 9 * C), device="cuda"), H, W)
    c_ref = ref_cols[0].permute(2, 3, 0, 1).reshape(H * W, 9 * C)
    assert (cols.cpu().double() - c_ref).abs().max().item() <= 2e-6 * (1 + c_ref.abs().max().item())
    out = ops.conv_gemm(cols, w.permute(0, 2, 3, 1).reshape(C, 9 * C).contiguous().cuda(), torch.empty((H * W, C), device="cuda"))
    o_ref = ref[0].permute(1, 2, 0).reshape(H * W, C)
    err = (out.cpu().double() - o_ref).abs().max().item()
    assert err <= 1e-5 * (1 + o_ref.abs().max().item()), err


@pytest.mark.parametrize("k,act,res", [(3, "lrelu", False), (4, "none", True), (4, "none", False)])
def test_transposed_conv_vs_fp64(k, act, res):
    from stitch_amd import transref as tr
    g = torch.Generator().manual_seed(k)
    cin, cout, H, W = 64, 48 if k == 3 else 32, 12, 10
    name = "Tenc.RefPA1.PA.offset_estimator.upblock1.0" if k == 3 else "convtail.convd8x.conv2d"
    w = torch.randn((cin, cout, k, k), generator=g) / (cin * k * k / 4) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    x = torch.randn((1, cin, H, W), generator=g)
    r = torch.randn((1, cout, 2 * H, 2 * W), generator=g)
    y = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1, output_padding=1 if k == 3 else 0)
    if act == "lrelu":
        y = F.leaky_relu(y, 0.01)
    if res:
        y = y + r.double()
    net = tr.TransRefNet(tr.pack({name + ".weight": w, name + ".bias": b}, "cuda"), "cuda")
    cl = lambda t: t[0].permute(1, 2, 0).reshape(-1, t.shape[1]).contiguous()   # noqa: E731
    got = net.convT(cl(x).cuda(), name, H, W, act=act, res=cl(r).cuda() if res else None)
    err = (got.cpu().double() - cl(y)).abs().max().item()
    assert err <= 1e-5 * (1 + y.abs().max().item()), err


def test_dwconv3x3_gelu_vs_fp64():
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    C, H, W = 256, 17, 23
    x = torch.randn((1, C, H, W), generator=g)
    w = torch.randn((C, 1, 3, 3), generator=g) / 3
    b = torch.randn((C,), generator=g) * 0.1
    ref = F.gelu(F.conv2d(x.double(), w.double(), b.double(), padding=1, groups=C))
    xd = x[0].permute(1, 2, 0).reshape(H * W, C).contiguous().cuda()
    got = ops.tr_dwconv3x3_gelu(xd, w.reshape(C, 9).t().contiguous().cuda(), b.cuda(), torch.empty_like(xd), H, W)
    err = (got.cpu().double() - ref[0].permute(1, 2, 0).reshape(H * W, C)).abs().max().item()
    assert err <= 2e-6, err


@pytest.mark.parametrize("M,N,K", [(4, 64, 64), (4096, 3, 32), (1000, 64, 96), (16384, 64, 128)])
def test_leaky_relu_epilogue(M, N, K):
    ops = _ops()
    g = torch.Generator().manual_seed(M + N)
    a, w, b = torch.randn((M, K), generator=g), torch.randn((N, K), generator=g) / K ** 0.5, torch.randn((N,), generator=g)
    ref = F.leaky_relu(a.double() @ w.double().T + b.double(), 0.01)
    got = ops.conv_gemm(a.cuda(), w.cuda(), torch.empty((M, N), device="cuda"), bias=b.cuda(), act="lrelu").cpu().double()
    assert (got - ref).abs().max().item() <= 1e-5 * (1 + ref.abs().max().item())
    assert bool(((got < 0) == (ref < 0)).all())


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def inp(gold):
    from stitch_amd import transref as tr
    return tr.Inpainter(seed=int(gold["seed"]), device="cuda")


def _golden_inputs(gold):
    f = lambda a: torch.from_numpy(a.astype(np.float32))[None].cuda()   # noqa: E731
    init = f(gold["init"]) + 0.7                          # to_pillow_fn truncates: the fraction must not survive
    ctl = f(gold["control"]) + 0.3
    mask = torch.from_numpy(gold["mask"].astype(np.float32))[None, None].expand(1, 3, -1, -1).contiguous().cuda()
    return init, mask, ctl


def test_network_vs_fp64_golden(gold, inp):
    init, mask, ctl = _golden_inputs(gold)
    x6, ref3, _, _, _ = inp.prepare(init, mask, ctl)
    taps = {}
    out = inp.forward_eager(x6, ref3, taps)
    torch.cuda.synchronize()
    gs = int(gold["grid"])
    got = out.view(512, 512, 3).permute(2, 0, 1)[:, gs // 2::gs, gs // 2::gs].cpu().double()
    err = (got - torch.from_numpy(gold["net_out64"]).double()).abs().max().item()
    bound = max(3 * float(gold["spread_max"]), 2e-5)
    t4 = taps["tenc"][3].view(16, 16, 512).permute(2, 0, 1).cpu().double()
    td = taps["tdec"].view(8, 8, 512).permute(2, 0, 1).cpu().double()
    e4 = (t4 - torch.from_numpy(gold["tenc4"]).double()).abs().max().item()
    ed = (td - torch.from_numpy(gold["tdec"]).double()).abs().max().item()
    print(f"network vs fp64: {err:.2e} (bound {bound:.2e}; reference fp32 spread {float(gold['spread_max']):.2e}); "
          f"Tenc stage 4 {e4:.2e}, Tdec {ed:.2e}")
    assert err <= bound
    assert e4 <= 1e-3 and ed <= 1e-3


def test_graph_replay_equals_eager(gold, inp):
    init, mask, ctl = _golden_inputs(gold)
    x6, ref3, _, _, _ = inp.prepare(init, mask, ctl)
    eager = inp.forward_eager(x6, ref3).clone()
    g1 = inp.forward_graph(x6, ref3).clone()
    g2 = inp.forward_graph(x6 * 1.0, ref3).clone()
    assert torch.equal(eager, g1) and torch.equal(g1, g2)


def test_inpaint_uint8_vs_golden(gold, inp):
    init, mask, ctl = _golden_inputs(gold)
    got = inp.inpaint(init, mask, control_image_tensor=ctl)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 3) + tuple(gold["init"].shape[1:]) and got.device == init.device
    u = got[0].cpu().numpy().astype(np.int32)
    ref = gold["u8_64"].astype(np.int32)
    d = np.abs(u - ref)
    assert d.max() <= 1
    diff = np.flatnonzero(d.ravel())
    tol = 3 * float(gold["spread_max"]) * 127.5
    near = dict(zip(gold["near_half_idx"].tolist(), gold["near_half_dist"].tolist()))
    bad = [i for i in diff if near.get(int(i), 1.0) > tol]
    print(f"inpaint uint8: {len(diff)} bytes differ from the fp64 golden, all within {tol:.1e} of a .5 boundary: {not bad}; "
          f"reference fp32 vs fp64: {int((gold['u8_32'] != gold['u8_64']).sum())}")
    assert not bad


def test_inpaint_rejects_batches_and_missing_control(inp):
    with pytest.raises(ValueError):
        inp.inpaint(torch.zeros(2, 3, 8, 8, device="cuda"), torch.ones(2, 1, 8, 8, device="cuda"), torch.zeros(2, 3, 8, 8, device="cuda"))
    with pytest.raises(ValueError):
        inp.inpaint(torch.zeros(1, 3, 8, 8, device="cuda"), torch.ones(1, 1, 8, 8, device="cuda"))


def test_cpu_device_raises():
    from stitch_amd import transref as tr
    with pytest.raises(RuntimeError):
        tr.Inpainter(seed=0, device="cpu")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_inpaint", os.path.join(ROOT, "tools", "bench_inpaint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def model():
    return _bench().seeded_model()


class _Rec:
    """records what mix_fn hands the inpainter (control included) and returns what `inner` returns"""

    def __init__(self, inner):
        self.inner, self.name, self.calls = inner, inner.name, []

    def inpaint(self, init_image_tensor, mask_image_tensor, control_image_tensor=None, prompt="", resize_to_area_limit_before_inpaint=False):
        out = self.inner.inpaint(init_image_tensor, mask_image_tensor, control_image_tensor=control_image_tensor, prompt=prompt,
                                 resize_to_area_limit_before_inpaint=resize_to_area_limit_before_inpaint)
        ctl = None if control_image_tensor is None else control_image_tensor.clone()
        self.calls.append((init_image_tensor.clone(), mask_image_tensor.clone(), ctl, out.clone()))
        return out


@pytest.mark.parametrize("mm", ["all_img1_with_inpaint", "inpaint_all_area"])
def test_mix_fn_transref_branch_on_demo1(model, inp, mm):
    from stitch_amd.mix_methods.utils.passthrough_inpainter import inpainter as pt
    b = _bench()
    a_, b_ = b.demo_pair("demo1")
    rt, rp = _Rec(inp), _Rec(pt)
    got_t, _ = b.run_chain(model, a_, b_, mm, rt)
    got_p, _ = b.run_chain(model, a_, b_, mm, rp)
    assert len(rt.calls) == 1 and rt.calls[0][2] is not None        # the transref branch: a control image is handed over
    init, mask, ctl, res = rt.calls[0]
    assert res.dtype == torch.uint8 and tuple(res.shape) == (1, 3) + tuple(init.shape[2:])
    assert torch.equal(inp.inpaint(init, mask, control_image_tensor=ctl), res)
    # what mix_fn derives from the masks alone is the pass-through's
    for key in ("inpaint_img_mask", "inpaint_area_mask"):
        assert torch.equal(got_t[key], got_p[key]), key
    m = mask[:, :1] > 0.5
    assert int(m.sum()) > 0
    hole = got_t["inpaint_img"][m.expand_as(got_t["inpaint_img"])]
    print(f"[{mm}] hole px {int(m.sum())}, mean filled value {hole.float().mean():.1f}")


def test_out_py_chain_with_seeded_transref(tmp_path, model, inp):
    sys.path.insert(0, ROOT)
    import out as out_py
    from PIL import Image
    g = np.load(os.path.join(ROOT, "tests", "golden", "e2e_demo_512.npz"))
    d = tmp_path / "demo" / "pair"
    d.mkdir(parents=True)
    Image.fromarray(g["demo1_input1"]).save(str(d / "input1.jpg"), quality=95)
    Image.fromarray(g["demo1_input2"]).save(str(d / "input2.jpg"), quality=95)
    (tmp_path / "demo" / "demo.txt").write_text("pair/\n")
    cfg = out_py.get_config(["--data_root_path", str(tmp_path / "demo") + "/"])
    assert cfg.TPS_PIPELINE_CONFIG.inpainter == "transref_inpainter"
    dd = out_py.get_data_dict_list(cfg.data_root_path, cfg.txt_file)[0]
    rec = _Rec(inp)
    save = tmp_path / "results"
    save.mkdir()
    out_py.inference_one_data(cfg, dd, str(save) + "/", model, inpainter=rec)
    assert len(rec.calls) == 1
    files = sorted(p.name for p in save.rglob("*") if p.is_file())
    print("out.py files:", files)
    assert len(files) >= 5, files
