"""cv_inpainter on the MI355X: the Telea kernels (csrc/inpaint.hip) against the CPU restatement of the contract (tests/_telea_ref.py).
d and T must be bit-equal.  The fill is checked teacher-forced: for a ring-k pixel the float64 restatement is evaluated on the GPU's
own output for the rings below k (those values are in the final image and are exactly what ring k read), and the GPU byte must be
round-half-up of it; where the restatement lies within 1e-3 of a .5 boundary either neighbour is accepted (counted, reported).
Then the plug-in through tps_H_warp / mix_fn on the demo pair and out.py with the `_cv` config."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _telea_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_inpaint", os.path.join(ROOT, "tools", "bench_inpaint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Truncating:
    """test-local inpainter: the truncated uint8 input, nothing filled (cv_inpainter's result type without the fill)"""
    name = "truncating_inpainter"

    def inpaint(self, init_image_tensor, mask_image_tensor, control_image_tensor=None, prompt="", resize_to_area_limit_before_inpaint=False):
        return init_image_tensor[:1].clamp(0, 255).to(torch.uint8)


@pytest.fixture(scope="module")
def model(seeded_sd):
    import stitch_amd
    cfg, _ = stitch_amd.load_inference_config("all_img1_with_inpaint_g12_transRef")
    m = stitch_amd.build_model(cfg)
    m.load_state_dict(seeded_sd, strict=True)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def demo1_masks(model):
    """(img uint8 [H,W,3], mask uint8 [H,W]) that demo1's chain hands to cv_inpainter, per mix method"""
    import stitch_amd
    from stitch_amd.mix_methods.utils.cv_inpainter import inpainter as cv
    b = _bench()
    a_, b_ = b.demo_pair("demo1")
    out = {}
    for mm in ("all_img1_with_inpaint", "inpaint_all_area"):
        rec = b.Recorder(cv)
        b.run_chain(model, a_, b_, mm, rec)
        init, mask, _ = rec.calls[0]
        out[mm] = stitch_amd.ops.inpaint_prep(init[0].float().contiguous(), mask[0].float().contiguous())
    return out


def _run(img, mask, radius):
    import stitch_amd
    out, d, T = stitch_amd.ops.inpaint_telea(img, mask, radius, return_fields=True)
    return out.cpu().numpy(), d.cpu().numpy(), T.cpu().numpy()


def _check_fields(img, mask, radius):
    """d, T bit-equal; known pixels untouched; returns (out, d, T) on the host"""
    out, d, T = _run(img, mask, radius)
    fill = mask.cpu().numpy() != 0
    d_ref = R.ring_distance(fill)
    T_ref = R.arrival_time(d_ref)
    assert np.array_equal(d, d_ref)
    assert np.array_equal(T.view(np.int32), T_ref.view(np.int32)), np.abs(T - T_ref).max()
    assert np.array_equal(out[~fill], img.cpu().numpy()[~fill])
    return out, d, T


def _teacher_forced(out, d, T, radius, per_ring, seed=0):
    rng = np.random.default_rng(seed)
    offs = R.disc(radius)
    checked = ambiguous = 0
    for k in range(1, int(d.max()) + 1):
        ys, xs = np.nonzero(d == k)
        pick = rng.choice(len(ys), min(per_ring, len(ys)), replace=False)
        for i in pick:
            y, x = ys[i], xs[i]
            ref = R.fill_value(out, d, T, y, x, radius, offs)
            got = out[y, x].astype(np.int64)
            exp = R.round_u8(ref).astype(np.int64)
            frac = ref - np.floor(ref)
            near = np.abs(frac - 0.5) < 1e-3
            ok = (got == exp) | (near & (np.abs(got - exp) <= 1))
            assert ok.all(), (k, y, x, ref, got)
            ambiguous += int((near & (got != exp)).sum())
            checked += 1
    return checked, ambiguous


def _synthetic(H, W, kind, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([(xx * 3 + yy) % 256, (yy * 5 + 40) % 256, (128 + 60 * np.sin(xx / 7.0) * np.cos(yy / 5.0))], -1)
    img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
    fill = np.zeros((H, W), bool)
    if kind == "rect":
        fill[H // 4:3 * H // 4, W // 5:W // 2] = True
    elif kind == "border":
        fill[:3] = fill[-4:] = True
        fill[:, :2] = fill[:, -5:] = True
        fill[H // 2 - 6:H // 2 + 6, W // 2 - 20:W // 2 + 20] = True
    elif kind == "blobs":
        for _ in range(6):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(3, 14)
            fill |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    img[fill] = 0
    return torch.from_numpy(img).cuda(), torch.from_numpy(fill.astype(np.uint8) * 255).cuda()


def test_prep_matches_the_restatement():
    import stitch_amd
    rng = np.random.default_rng(3)
    img = (rng.random((3, 45, 67), np.float32) * 300 - 20).astype(np.float32)
    for mask in (rng.integers(0, 2, (1, 45, 67)).astype(np.float32), rng.random((3, 45, 67), np.float32) * np.float32(0.012),
                 rng.random((3, 45, 67), np.float32) * 255):
        a, m = stitch_amd.ops.inpaint_prep(torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda())
        assert np.array_equal(a.cpu().numpy(), R.prep_image(img))
        assert np.array_equal(m.cpu().numpy(), R.prep_mask(mask))


@pytest.mark.parametrize("kind,radius", [("rect", 5), ("border", 7), ("blobs", 64), ("rect", 88)])
def test_synthetic_holes_fields_bit_equal_and_fill_teacher_forced(kind, radius):
    img, mask = _synthetic(72, 96, kind, seed=11)
    out, d, T = _check_fields(img, mask, radius)
    checked, amb = _teacher_forced(out, d, T, radius, per_ring=40)
    print(f"[{kind} r={radius}] rings {d.max()}, {checked} pixels checked, {amb} channel values within 1e-3 of .5 rounded the other way")


def test_demo1_thin_border_radius64(demo1_masks):
    img, mask = demo1_masks["all_img1_with_inpaint"]
    out, d, T = _check_fields(img, mask, 64)
    assert d.max() >= 1
    checked, amb = _teacher_forced(out, d, T, 64, per_ring=48)
    fill = mask.cpu().numpy() != 0
    assert (out[fill].sum(-1) > 0).mean() > 0.5               # the border is filled from the image, not left black
    print(f"[demo1 thin border r=64] {int(fill.sum())} fill px, rings {d.max()}, {checked} checked, {amb} ambiguous")


def test_demo1_inpaint_all_area_small_radius_many_rings(demo1_masks):
    img, mask = demo1_masks["inpaint_all_area"]
    out, d, T = _check_fields(img, mask, 5)
    checked, amb = _teacher_forced(out, d, T, 5, per_ring=24)
    print(f"[demo1 inpaint_all_area r=5] {int((mask != 0).sum())} fill px, rings {d.max()}, {checked} checked, {amb} ambiguous")


def test_nothing_to_fill_and_nothing_known():
    import stitch_amd
    img, _ = _synthetic(20, 30, "rect", seed=2)
    out, d, T = stitch_amd.ops.inpaint_telea(img, torch.zeros((20, 30), dtype=torch.uint8, device="cuda"), return_fields=True)
    assert torch.equal(out, img) and d is None and T is None
    out = stitch_amd.ops.inpaint_telea(img, torch.full((20, 30), 255, dtype=torch.uint8, device="cuda"))
    assert torch.equal(out, img)


def test_plugin_rejects_batches():
    from stitch_amd.mix_methods.utils.cv_inpainter import inpainter
    with pytest.raises(ValueError):
        inpainter.inpaint(torch.zeros(2, 3, 8, 8, device="cuda"), torch.ones(2, 1, 8, 8, device="cuda"))


@pytest.mark.parametrize("mm", ["all_img1_with_inpaint", "inpaint_all_area"])
def test_plugin_through_tps_H_warp_on_demo1(model, mm):
    import stitch_amd
    from stitch_amd.mix_methods.utils.cv_inpainter import inpainter as cv
    b = _bench()
    a_, b_ = b.demo_pair("demo1")
    rc, rt = b.Recorder(cv), b.Recorder(Truncating())
    got_cv, _ = b.run_chain(model, a_, b_, mm, rc)
    got_tr, _ = b.run_chain(model, a_, b_, mm, rt)
    (init, mask, res), (init_t, mask_t, _) = rc.calls[0], rt.calls[0]
    assert torch.equal(init, init_t) and torch.equal(mask, mask_t)
    assert res.dtype == torch.uint8 and tuple(res.shape) == (1, 3) + tuple(init.shape[2:]) and res.device == init.device
    img, m = stitch_amd.ops.inpaint_prep(init[0].float().contiguous(), mask[0].float().contiguous())
    fill = m != 0
    assert int(fill.sum()) > 0
    direct = stitch_amd.ops.inpaint_telea(img, m).permute(2, 0, 1)[None]
    assert torch.equal(res, direct)                              # inside the mask: the op itself
    outside = ~fill
    for key in ("tfw", "tfwm", "inpaint_img", "inpaint_img_mask", "inpaint_area_mask"):
        x, y = got_cv[key], got_tr[key]
        assert x.shape == y.shape, key
        sel = outside[None, None].expand_as(x)
        assert torch.equal(x[sel], y[sel]), key
    filled = got_cv["inpaint_img"][fill.expand(3, -1, -1)[None].expand_as(got_cv["inpaint_img"])]
    print(f"[{mm}] fill px {int(fill.sum())}, nonzero filled values {(filled > 0).float().mean():.3f}")


def test_out_py_cv_config_writes_all_files(tmp_path):
    from PIL import Image
    g = np.load(os.path.join(ROOT, "tests", "golden", "e2e_demo_512.npz"))
    d = tmp_path / "demo" / "pair"
    d.mkdir(parents=True)
    Image.fromarray(g["demo1_input1"]).save(str(d / "input1.jpg"), quality=95)
    Image.fromarray(g["demo1_input2"]).save(str(d / "input2.jpg"), quality=95)
    (tmp_path / "demo" / "demo.txt").write_text("pair/\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "out.py"), "--data_root_path", str(tmp_path / "demo") + "/",
                        "--inf_cfg", "all_img1_with_inpaint_g12_cv"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "not available here" not in r.stdout
    res = [p for p in (tmp_path / "results").rglob("pair") if p.is_dir()]
    assert len(res) == 1
    files = sorted(os.listdir(res[0]))
    assert len(files) == 10, files
