"""tps_method="other" on the GPU (csrc/tps_other.hip through the C-ABI): the maps against the CPU restatement
(tests/_other_tps_ref.py) teacher-forced on the GPU's own fp64-fitted theta, the fixed-point remap bit for bit on adversarial
maps and edge sizes, the whole branch against the restatement and the reference golden (tests/golden/other_tps.npz), the
degenerate-set policies, tps_H_warp and out.py with the `_other` config."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
import _other_tps_ref as R  # noqa: E402
from _measure import check  # noqa: E402

from oracle import tps_pipeline as otp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    import stitch_amd
    return stitch_amd.ops


@pytest.fixture(scope="module")
def tp():
    import stitch_amd
    return stitch_amd.tps_pipeline


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "other_tps.npz"))


@pytest.fixture(scope="module")
def table(ops):
    return ops.cubic_remap_table()


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def point_set(gold, name):
    """-> (c_src, c_dst) normalised float32, (H, W) of the canvas"""
    if name == "random":
        rng = np.random.default_rng(21)
        H, W = 200, 260
        dst = np.stack([rng.uniform(0, W - 1, 40), rng.uniform(0, H - 1, 40)], 1).astype(np.float32)
        src = (dst + rng.normal(0, 3, dst.shape)).astype(np.float32)
        return R.normalise(src, H, W), R.normalise(dst, H, W), (H, W)
    oh, ow = (int(v) for v in gold[f"{name}_out_hw"])
    return R.normalise(gold[f"{name}_points_src"], oh, ow), R.normalise(gold[f"{name}_points_dst"], oh, ow), (oh, ow)


@pytest.mark.parametrize("name", ["well", "chain", "random"])
def test_maps_match_the_restatement(ops, gold, name):
    c_src, c_dst, (H, W) = point_set(gold, name)
    cs, cd = torch.from_numpy(c_src).cuda(), torch.from_numpy(c_dst).cuda()
    kw, aw = ops.tps_other_solve(cs, cd)
    mx, my = ops.tps_other_maps(cs, cd, H, W)
    kw_h, aw_h = kw.cpu().numpy(), aw.cpu().numpy()
    rx, ry = R.maps(kw_h, aw_h, c_dst, H, W)
    rk, ra = R.fit(c_src, c_dst)
    gap = max(np.abs(rk[1:] - kw_h[1:]).max(), np.abs(ra - aw_h).max()) / np.abs(rk).max()
    for axis, got, ref in (("x", mx, rx), ("y", my, ry)):
        u = ulps(got.cpu().numpy(), ref)
        print(f"[{name} {H}x{W}] map{axis}: ulps max {u.max()}, bit-equal {np.mean(u == 0):.6f}; theta vs numpy fp64 solve {gap:.2e}")
        assert u.max() <= 1
        check(f"other_maps_{name}_{axis}_differs_frac", np.mean(u != 0), 1e-4, inclusive=True)
    if name != "chain":
        check(f"other_theta_{name}_rel_gap", gap, 1e-6)


def _adversarial_maps(H, W, rng, Hs=None, Ws=None):
    """maps [H,W] over a source Hs x Ws (default H x W): a margin past every edge, specials, huge values and half-quantum ties"""
    Hs, Ws = Hs or H, Ws or W
    mx = rng.uniform(-4, Ws + 3, (H, W)).astype(np.float32)
    my = rng.uniform(-4, Hs + 3, (H, W)).astype(np.float32)
    flat = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 2.0 ** 26, -2.0 ** 26, 2.0 ** 27 + 64, -3e9, 1e30, 67108860.0,
                     -1.5 / 32, 0.5 / 32, 1.5 / 32, 2.5 / 32, 3.5 / 32, -0.5 / 32, -2.5 / 32, Ws - 0.5 / 32, Ws + 0.5 / 32,
                     Ws - 1 + 31.5 / 32, -1.0, -2.0, -3.0, Ws + 1.0, Ws + 2.0, -1 + 0.5 / 32], np.float32)
    n = min(flat.size, H * W)
    ix = rng.choice(H * W, n, replace=False)
    mx.reshape(-1)[ix] = flat[:n]
    iy = rng.choice(H * W, n, replace=False)
    my.reshape(-1)[iy] = rng.permutation(flat)[:n]
    ties = rng.random((H, W)) < 0.3                                # exact half-quanta everywhere else
    mx[ties] = (np.floor(mx[ties] * 32) + 0.5).astype(np.float32) / np.float32(32)
    return mx, my


def _planes(P, H, W, rng):
    p = rng.uniform(-20, 280, (P, H, W)).astype(np.float32)
    p[:, ::3] = np.floor(p[:, ::3])
    return p


def _remap_both(ops, planes, mx, my, table):
    got = ops.remap_cubic(torch.from_numpy(planes).cuda(), torch.from_numpy(mx).cuda(), torch.from_numpy(my).cuda()).cpu().numpy()
    ref = R.remap_cubic(R.quantise(planes), mx, my, table).astype(np.float32)
    return got, ref


def test_remap_bit_exact_on_adversarial_maps(ops, table):
    rng = np.random.default_rng(5)
    planes = _planes(6, 37, 53, rng)
    mx, my = _adversarial_maps(41, 47, rng, 37, 53)
    got, ref = _remap_both(ops, planes, mx, my, table)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    assert (got > 0).mean() > 0.3 and (got == 0).any()


@pytest.mark.parametrize("H", [1, 3, 4, 5, 567])
@pytest.mark.parametrize("W", [1, 3, 4, 5, 567])
def test_remap_bit_exact_on_edge_sizes(ops, table, H, W):
    rng = np.random.default_rng(H * 1000 + W)
    planes = _planes(6, H, W, rng)
    mx, my = _adversarial_maps(H, W, rng)
    got, ref = _remap_both(ops, planes, mx, my, table)
    assert got.shape == (6, H, W) and np.array_equal(got, ref)


def _warp_case(gold):
    seed, ih, iw, wmin, hmin, oh, ow = (int(v) for v in gold["warp_case"])
    return otp.synthetic_case(seed, ih, iw, wmin, hmin, oh, ow), oh, ow


def test_branch_is_the_restated_remap_of_its_own_maps(ops, tp, gold, table):
    case, oh, ow = _warp_case(gold)
    ps, pd = torch.from_numpy(gold["well_points_src"])[None], torch.from_numpy(gold["well_points_dst"])[None]
    Hw, Hm = case["H_warp"], case["H_warp_mask"]
    got = tp.warp_by_tps(Hw.cuda(), Hm.cuda(), ps, pd, oh, ow, "other", 3.0, 5.0).cpu().numpy()      # scales unused
    c_src, c_dst = R.normalise(ps[0].numpy(), oh, ow), R.normalise(pd[0].numpy(), oh, ow)
    mx, my = ops.tps_other_maps(torch.from_numpy(c_src).cuda(), torch.from_numpy(c_dst).cuda(), oh, ow)
    planes = R.quantise(np.concatenate([Hw[0].numpy(), Hm[0].numpy()]))
    ref = R.remap_cubic(planes, mx.cpu().numpy(), my.cpu().numpy(), table).astype(np.float32)
    assert got.shape == (1, 6, oh, ow) and got.dtype == np.float32
    assert np.array_equal(got[0], ref)


def test_branch_against_the_reference_golden(ops, tp, gold):
    """the GPU (fp64 fit) against the reference (float32 sgesv): bytes may differ only where the quantised map coordinates do"""
    case, oh, ow = _warp_case(gold)
    ps, pd = gold["well_points_src"], gold["well_points_dst"]
    got = tp.warp_by_tps(case["H_warp"].cuda(), case["H_warp_mask"].cuda(), torch.from_numpy(ps)[None], torch.from_numpy(pd)[None],
                         oh, ow, "other", 1.0, 1.0).cpu().numpy()[0]
    c_src, c_dst = R.normalise(ps, oh, ow), R.normalise(pd, oh, ow)
    mx, my = (m.cpu().numpy() for m in ops.tps_other_maps(torch.from_numpy(c_src).cuda(), torch.from_numpy(c_dst).cuda(), oh, ow))
    rx, ry = gold["well_mapx"], gold["well_mapy"]
    same_q = (np.rint(mx * 32) == np.rint(rx * 32)) & (np.rint(my * 32) == np.rint(ry * 32))
    d = np.abs(got - gold["warp_out"].astype(np.float32))
    print(f"[other vs reference golden] quantised (X, Y) differ at {np.mean(~same_q):.2e} of pixels; bytes differ at "
          f"{np.mean(d > 0):.2e}, max {d.max():.0f} levels; map |d| max {np.abs(mx - rx).max():.2e} px")
    assert not (d[:, same_q] > 0).any()
    check("other_golden_quantised_xy_differs_frac", np.mean(~same_q), 1e-2)


def test_duplicate_points_keep_the_first(ops, tp, table):
    case = otp.synthetic_case(9, 120, 160, -9, -7, 140, 180)
    Hw, Hm = case["H_warp"], case["H_warp_mask"]
    g = torch.Generator().manual_seed(4)
    src = torch.stack([torch.randint(10, 170, (1, 30), generator=g), torch.randint(10, 130, (1, 30), generator=g)], -1).float()
    dst = src + torch.randint(-3, 4, src.shape, generator=g).float()
    src = torch.cat([src, src[:, :3] + 2], 1)                  # three coincident points_dst with other sources
    dst = torch.cat([dst, dst[:, :3]], 1)
    got = tp.warp_by_tps(Hw.cuda(), Hm.cuda(), src, dst, 140, 180, "other", 1.0, 1.0).cpu()
    c_src, c_dst = R.dedup_first(R.normalise(src[0].numpy(), 140, 180), R.normalise(dst[0].numpy(), 140, 180))
    assert len(c_dst) == 30
    mx, my = ops.tps_other_maps(torch.from_numpy(c_src).cuda(), torch.from_numpy(c_dst).cuda(), 140, 180)
    ref = R.remap_cubic(R.quantise(np.concatenate([Hw[0].numpy(), Hm[0].numpy()])), mx.cpu().numpy(), my.cpu().numpy(), table)
    assert torch.isfinite(got).all() and np.array_equal(got[0].numpy(), ref.astype(np.float32))


def test_collinear_points_leave_the_homography_warp(ops, tp):
    img = torch.rand(1, 6, 64, 80).cuda() * 255
    line = torch.tensor([[[5.0, 5.0], [10.0, 10.0], [20.0, 20.0], [40.0, 40.0], [50.0, 50.0]]])
    with pytest.raises(ops.SingularTPSError):
        ops.tps_other_solve((line[0] / 80).cuda(), (line[0] / 80).cuda() + 0.01)
    out = tp.warp_by_tps(img[:, :3], img[:, 3:], line + 1, line, 64, 80, "other", 1.0, 1.0)
    assert torch.equal(out, img) and torch.isfinite(out).all()


def test_tps_H_warp_other_matches_opencv_layout_and_points(tp):
    ih, iw, wmin, hmin, oh, ow = 200, 264, -21, -13, 236, 300
    case = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in otp.synthetic_case(5, ih, iw, wmin, hmin, oh, ow).items()}
    limit = SimpleNamespace(width_min=wmin, height_min=hmin, out_height=oh, out_width=ow)
    base = dict(grid_h=12, grid_w=12, pad_num=4, residual_flow_use_forward=False, flow_limit=-1, add_corner=False,
                get_pt_methods=["advanced_uniform_multi"], affine_scale=1.0, kernel_scale=1.0, use_boundary_limit=False,
                output2_is_only_tps=True, do_avg_pooling=True)
    a = tp.tps_H_warp(case, limit, SimpleNamespace(tps_method="opencv", **base))
    b = tp.tps_H_warp(case, limit, SimpleNamespace(tps_method="other", **base))
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
    assert torch.equal(a["points_src"], b["points_src"]) and torch.equal(a["points_dst"], b["points_dst"])
    assert b["points_src"].shape[1] >= 3
    t = b["tps_output"]
    assert torch.equal(t, t.round()) and t.min() >= 0 and t.max() <= 255 and t.max() > 0


def test_out_py_other_config_writes_all_files(tmp_path):
    from PIL import Image
    g = np.load(os.path.join(ROOT, "tests", "golden", "e2e_demo_512.npz"))
    d = tmp_path / "demo" / "pair"
    d.mkdir(parents=True)
    Image.fromarray(g["demo1_input1"]).save(str(d / "input1.jpg"), quality=95)
    Image.fromarray(g["demo1_input2"]).save(str(d / "input2.jpg"), quality=95)
    (tmp_path / "demo" / "demo.txt").write_text("pair/\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "out.py"), "--data_root_path", str(tmp_path / "demo") + "/",
                        "--inf_cfg", "all_img1_with_inpaint_g12_other"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "NotImplementedError" not in r.stdout + r.stderr
    res = [p for p in (tmp_path / "results").rglob("pair") if p.is_dir()]
    assert len(res) == 1
    files = sorted(os.listdir(res[0]))
    assert len(files) == 10, files
