"""tps_method="other" without a GPU: the CPU restatement (tests/_other_tps_ref.py) against the reference's own numpy code
(tests/golden/other_tps.npz, written by tools/make_other_tps_golden.py), the coefficient table, the fixed-point remap's
properties, the C-ABI's host-side argument checks and an ISA guard on the built kernels."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import _other_tps_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "seamless-through-breaking-rethinking-image-stitching-for-optimal-alignment_amd")
LLVM = "/opt/rocm/llvm/bin"


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "other_tps.npz"))


@pytest.fixture(scope="module")
def table():
    import stitch_amd
    return stitch_amd.ops.cubic_remap_table()


def _points(gold, name):
    oh, ow = (int(v) for v in gold[f"{name}_out_hw"])
    return R.normalise(gold[f"{name}_points_src"], oh, ow), R.normalise(gold[f"{name}_points_dst"], oh, ow)


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("name", ["well", "chain"])
def test_maps_from_the_reference_theta_match_the_reference_maps(gold, name):
    """teacher-forced on the reference's own float32 theta: the fp64 index-order maps (w_0 as numpy's float32 np.sum) are the
    reference's maps (BLAS dot) to 1 ulp, bit-equal almost everywhere (measured: everywhere, both sets)"""
    _, c_dst = _points(gold, name)
    H, W = (int(v) for v in gold[f"{name}_grid_hw"])
    kw, aw = R.from_reduced(gold[f"{name}_theta"], len(c_dst))
    mx, my = R.maps(kw, aw, c_dst, H, W)
    for got, ref in ((mx, gold[f"{name}_mapx"]), (my, gold[f"{name}_mapy"])):
        u = ulps(got, ref)
        print(f"[{name}] map ulps max {u.max()}, bit-equal {np.mean(u == 0):.6f}")
        assert u.max() <= 1 and np.mean(u == 0) >= 0.9999


def test_w0_is_numpys_float32_sum():
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 8, 9, 100, 128, 129, 300, 1031, 4095):
        a = (rng.standard_normal((n, 2)) * rng.choice([1e-3, 1.0, 50.0])).astype(np.float32)
        for k in range(2):
            assert R.f32_sum(a[:, k]) == np.sum(a[:, k], keepdims=True)[0], (n, k)


@pytest.mark.parametrize("n", R.N_TABLE)
def test_matrix_case_w0_is_numpys_float32_sum(n):
    """the inputs of tests/test_other_tps_matrix_gpu.py: the restated sum of w_1..w_{n-1} is numpy's, on the strided column itself"""
    kw = R.case(n)[0]
    assert kw.shape == (n, 2) and kw.dtype == np.float32
    for a in range(2):
        col = kw[1:, a]
        assert col.strides == (8,)
        assert R.f32_sum(col).tobytes() == np.sum(col, keepdims=True)[0].tobytes(), (n, a)
        assert R.reduce_w0(kw)[0, a].tobytes() == (-np.sum(col, keepdims=True)[0]).tobytes(), (n, a)


WRONG_SUMS = {"in_order": (R.sum_in_order, lambda m: m >= 8),
              "leaf_no_split": (R.sum_leaf_no_split, lambda m: m > 128),
              "halves_unrounded": (R.sum_halves_unrounded, R.unrounded_halves_differ)}


@pytest.mark.parametrize("wrong", sorted(WRONG_SUMS))
@pytest.mark.parametrize("n", [n for n in R.N_TABLE if n >= 130])
def test_matrix_case_tells_a_wrong_sum_from_numpys(n, wrong):
    """a kernel that sums w_1..w_{n-1} in one of the three wrong ways gets another w_0 on at least one axis, at every n of the table
    past the 128-element block, wherever the wrong way is a different sequence of additions at that length (the unrounded halves
    are the same additions at 129, 256 and 512 elements: n = 130, 257, 513)"""
    fn, defined_differently = WRONG_SUMS[wrong]
    kw = R.case(n)[0]
    if not defined_differently(n - 1):
        assert wrong == "halves_unrounded" and n in (130, 257, 513)
        assert all(fn(kw[1:, a]) == R.f32_sum(kw[1:, a]) for a in range(2))
        return
    assert any(fn(kw[1:, a]) != R.f32_sum(kw[1:, a]) for a in range(2)), (n, wrong)
    # ... and the 1 x 1 probe, float32(U(3) * w_0), shows it: the product does not round the two w_0 onto one float32
    u3 = R.u(np.float64(R.PROBE_R))
    probe = lambda s: np.float32(u3 * np.float64(-s))                                                       # noqa: E731
    assert any(probe(fn(kw[1:, a])) != probe(R.f32_sum(kw[1:, a])) for a in range(2)), (n, wrong)


def test_in_order_sum_differs_from_numpys_from_eight_elements_on():
    """below the 128-element block only the in-order sum is a different sequence; the matrix cases see it from n = 9 on"""
    for n in R.N_TABLE:
        kw = R.case(n)[0]
        same = all(R.sum_in_order(kw[1:, a]) == R.f32_sum(kw[1:, a]) for a in range(2))
        assert same == (n - 1 < 8), n


@pytest.mark.parametrize("n", [257, 264, 300, 513])
def test_matrix_case_sees_a_dropped_last_chunk(n):
    """centres are staged 256 at a time: what the centres of a partial last chunk add to the 37 x 130 maps is far above the 1 ulp
    that the GPU test allows, at most pixels, so a kernel that drops them fails there"""
    H, W = 37, 130
    kw, aw, centres = R.case(n)
    mx, my = R.maps(kw, aw, centres, H, W)
    xs, ys = R.grid_axes(H, W)
    x, y = xs.astype(np.float64)[None, :], ys.astype(np.float64)[:, None]
    c, w = centres.astype(np.float64), kw.astype(np.float64)
    last = np.zeros((2, H, W))
    for k in range(n - n % 256, n):
        uk = R.u(np.sqrt((x - c[k, 0]) ** 2 + (y - c[k, 1]) ** 2))
        last[0] += uk * w[k, 0] * W
        last[1] += uk * w[k, 1] * H
    for part, m in zip(last, (mx, my)):
        assert np.mean(np.abs(part) > 4 * np.spacing(np.abs(m))) > 0.9, n


@pytest.mark.parametrize("n", R.N_TABLE)
def test_w0_probe_does_not_sit_on_a_float32_rounding_boundary(n):
    """the probe's maps are float32(U(3) * w_0) and are compared bit for bit, while the GPU's log may differ from the host's in the
    last place: 9 * (log(3 + 1e-6) +- 1 ulp) rounds to U(3) moved by up to 2 fp64 ulps, and no such move may change the float32"""
    kw, aw, centres = R.probe_case(n)
    w0 = R.reduce_w0(kw)[0].astype(np.float64)
    u3 = R.u(np.float64(R.PROBE_R))
    mx, my = R.maps(kw, aw, centres, 1, 1)
    want = (0.0 + u3 * w0).astype(np.float32)                      # the spline sum starts from +0.0
    assert mx.shape == (1, 1) and mx[0, 0].tobytes() == want[0].tobytes() and my[0, 0].tobytes() == want[1].tobytes()
    if n == 1:
        assert np.signbit(R.reduce_w0(kw)[0]).all() and not np.signbit(want).any() and (want == 0).all()      # w_0 = -0.0, maps +0.0
    else:
        assert (want != 0).all()
    for k in (-2, -1, 1, 2):
        moved = u3
        for _ in range(abs(k)):
            moved = np.nextafter(moved, np.inf if k > 0 else -np.inf)
        assert (0.0 + moved * w0).astype(np.float32).tobytes() == want.tobytes(), (n, k)


@pytest.mark.parametrize("name", ["well", "chain"])
def test_fp64_fit_against_the_reference_sgesv(gold, name):
    """the documented deviation: the fit is solved in fp64 (the reference: float32 sgesv).  Reported on both sets, bounded on the
    well-conditioned one (measured 1.5e-6 of max |theta| there; the 101-point chain set is ill-conditioned: 1.6e-3)."""
    c_src, c_dst = _points(gold, name)
    n = len(c_dst)
    kw, aw = R.fit(c_src, c_dst)
    th = gold[f"{name}_theta"]
    gap = max(np.abs(kw[1:] - th[:n - 1]).max(), np.abs(aw - th[n - 1:]).max()) / np.abs(th).max()
    print(f"[{name}] fp64 theta vs sgesv theta: {gap:.3e} of max |theta|")
    if name == "well":
        assert gap < 5e-6


def test_table_invariants(table):
    t = table.astype(np.int64)
    assert table.dtype == np.int16 and t.shape == (1024, 16)
    assert (t.sum(1) == 32768).all()
    # fraction (0, 0): the unit tap at (1, 1), saturated to int16 (32767) with the sum correction's 1 on (2, 2)
    unit = np.zeros(16, np.int64)
    unit[5], unit[10] = 32767, 1
    assert np.array_equal(t[0], unit)
    f = np.float32
    tt = np.arange(32, dtype=f) * f(1 / 32)
    A = f(-0.75)
    c0 = ((A * (tt + 1) - 5 * A) * (tt + 1) + 8 * A) * (tt + 1) - 4 * A
    c1 = ((A + 2) * tt - (A + 3)) * tt * tt + 1
    c2 = ((A + 2) * (1 - tt) - (A + 3)) * (1 - tt) * (1 - tt) + 1
    c = np.stack([c0, c1, c2, 1 - c0 - c1 - c2], 1).astype(np.float64)
    exact = (c[:, None, :, None] * c[None, :, None, :]).reshape(1024, 16) * 32768
    # every entry is within 1 of cy * cx * 32768, except the one entry per row that absorbs the sum correction (centre 2 x 2)
    off = np.abs(t - exact) > 1.0 + 1e-3
    assert (off.sum(1) <= 1).all()
    assert not off[:, [k for k in range(16) if k not in (10, 11, 14, 15)]].any()
    print(f"rows corrected: {(off.sum(1) > 0).sum()}, largest correction {np.abs(t - exact)[off].max():.2f}")


def _rng_img(P, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (P, H, W)).astype(np.int32)


def test_remap_constant_image_stays_constant_inside(table):
    H, W = 23, 31
    img = np.full((2, H, W), 173, np.int32)
    img[1] = 9
    rng = np.random.default_rng(1)
    mx = rng.uniform(-3, W + 2, (40, 50)).astype(np.float32)
    my = rng.uniform(-3, H + 2, (40, 50)).astype(np.float32)
    out = R.remap_cubic(img, mx, my, table)
    sx, _, _ = R.quantise_map(mx)
    sy, _, _ = R.quantise_map(my)
    inside = (sx >= 1) & (sx + 2 < W) & (sy >= 1) & (sy + 2 < H)
    assert inside.sum() > 500
    assert (out[0][inside] == 173).all() and (out[1][inside] == 9).all()


def test_remap_integer_maps_copy_and_outside_gives_zero(table):
    img = _rng_img(3, 17, 29)
    yy, xx = np.meshgrid(np.arange(17, dtype=np.float32), np.arange(29, dtype=np.float32), indexing="ij")
    assert np.array_equal(R.remap_cubic(img, xx, yy, table), img)
    far = np.full((5, 6), -2.6, np.float32)                      # sx = -3: taps -4..-1
    assert (R.remap_cubic(img, far, far * 0 + 3, table) == 0).all()
    assert (R.remap_cubic(img, far * 0 + 30.6, far * 0 + 3, table) == 0).all()      # sx = 30 > W: taps 29..32
    bad = np.array([[np.nan, np.inf, -np.inf, 3e8]], np.float32)
    assert (R.remap_cubic(img, bad, np.full_like(bad, 3), table) == 0).all()


def test_remap_rounds_half_quanta_to_even(table):
    k = np.arange(-40, 40)
    m = ((k + 0.5) / 32).astype(np.float32)
    X = np.rint(m.astype(np.float64) * 32).astype(np.int64)
    sx, fx, ok = R.quantise_map(m)
    assert ok.all() and np.array_equal(sx * 32 + fx, X) and (X % 2 == 0).all()
    # on an image: 2.5/32 past pixel 4 is fraction 2 (to even), not 3
    img = _rng_img(1, 4, 12, seed=2)
    a = R.remap_cubic(img, np.float32([[4 + 2.5 / 32]]), np.float32([[1.0]]), table)
    b = R.remap_cubic(img, np.float32([[4 + 2 / 32]]), np.float32([[1.0]]), table)
    c = R.remap_cubic(img, np.float32([[4 + 3.5 / 32]]), np.float32([[1.0]]), table)
    d = R.remap_cubic(img, np.float32([[4 + 4 / 32]]), np.float32([[1.0]]), table)
    assert a == b and c == d


def test_restatement_warp_vs_reference_golden(gold, table):
    """the whole branch restated (fp64 fit) against the reference's warp_by_tps(..., 'other') around the same remap: bytes differ
    only where the fp64-vs-sgesv theta moves a quantised map coordinate"""
    import torch
    from oracle import tps_pipeline as otp
    seed, ih, iw, wmin, hmin, oh, ow = (int(v) for v in gold["warp_case"])
    case = otp.synthetic_case(seed, ih, iw, wmin, hmin, oh, ow)
    ps, pd = gold["well_points_src"], gold["well_points_dst"]
    got, (mx, my), _ = R.warp_other(case["H_warp"].numpy(), case["H_warp_mask"].numpy(), ps, pd, oh, ow, table)
    ref = gold["warp_out"].astype(np.float32)
    kw, aw = R.from_reduced(gold["well_theta"], len(pd))
    rx, ry = R.maps(kw, aw, R.normalise(pd, oh, ow), oh, ow)
    same_q = (np.rint(mx * 32) == np.rint(rx * 32)) & (np.rint(my * 32) == np.rint(ry * 32))
    diff = got[0] != ref
    print(f"[restated warp] quantised coordinates differ at {np.mean(~same_q):.2e} of pixels; bytes differ {np.mean(diff):.2e}")
    assert not diff[:, same_q].any()
    teacher = R.remap_cubic(R.quantise(np.concatenate([case["H_warp"][0].numpy(), case["H_warp_mask"][0].numpy()])), rx, ry, table)
    assert np.array_equal(teacher, ref)                           # the golden IS the restated remap of the reference's maps
    del torch


def test_capi_rejects_bad_arguments_on_the_host():
    from stitch_amd._lib import lib
    dp = C.c_void_p(256)            # never dereferenced: every call below is rejected on the host
    assert lib.st_tps_other_solve(None, dp, dp, dp, dp, 10, dp, None) == 1001
    assert lib.st_tps_other_solve(dp, dp, dp, dp, dp, 2, dp, None) == 1001
    assert lib.st_tps_other_solve(dp, dp, dp, dp, dp, 4097, dp, None) == 1001
    assert lib.st_tps_other_solve(dp, dp, dp, dp, dp, 10, None, None) == 1001
    assert lib.st_tps_other_maps(dp, dp, None, 10, 8, 8, dp, dp, None) == 1001
    assert lib.st_tps_other_maps(dp, dp, dp, 0, 8, 8, dp, dp, None) == 1001
    assert lib.st_tps_other_maps(dp, dp, dp, 10, 0, 8, dp, dp, None) == 1001
    assert lib.st_tps_other_maps(dp, dp, dp, 10, 8, 8, dp, None, None) == 1001
    assert lib.st_tps_other_maps(dp, dp, dp, 10, 8, 8, None, dp, None) == 1001
    assert lib.st_tps_other_maps(dp, dp, dp, 4097, 8, 8, dp, dp, None) == 1001
    assert lib.st_tps_other_maps(dp, dp, dp, 10, 8, 0, dp, dp, None) == 1001
    assert lib.st_tps_other_maps(dp, dp, dp, 10, 8, -1, dp, dp, None) == 1001
    assert lib.st_tps_other_maps(dp, dp, dp, 10, 65536, 32768, dp, dp, None) == 1001              # h w = 2^31
    assert lib.st_remap_cubic_u8(dp, 6, 8, 8, dp, dp, 8, 8, dp, None, None) == 1001
    assert lib.st_remap_cubic_u8(dp, 0, 8, 8, dp, dp, 8, 8, dp, dp, None) == 1001
    assert lib.st_remap_cubic_u8(dp, 6, 32761, 8, dp, dp, 8, 8, dp, dp, None) == 1001
    assert lib.st_remap_cubic_u8(dp, 6, 8, 8, dp, dp, 8, 8, C.c_void_p(258), dp, None) == 1001     # misaligned table
    assert lib.st_remap_cubic_u8(dp, 6, 8, 8, dp, dp, 8, -1, dp, dp, None) == 1001


def _code_object(tmp_path, marker):
    lib = os.path.join(PKG, "libstitch_gfx950.so")
    fb = str(tmp_path / "fatbin")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fb}", lib, str(tmp_path / "lib_copy.so")])
    data = open(fb, "rb").read()
    for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data):
        s = m.start()
        (n,) = struct.unpack_from("<Q", data, s + 24)
        p = s + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            co = data[s + off:s + off + size]
            if triple.endswith("gfx950") and marker in co:
                path = tmp_path / "tps_other.co"
                path.write_bytes(co)
                return str(path)
    raise AssertionError("no gfx950 code object with the tps_other kernels in the library")


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-objdump"), reason="needs the ROCm LLVM tools")
def test_tps_other_kernels_isa_no_packed_fp32_no_scratch(tmp_path):
    co = _code_object(tmp_path, b"remap_cubic_u8_kernel")
    asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", co], capture_output=True, text=True, check=True).stdout
    bodies = dict((m.group(1), m.group(2)) for m in re.finditer(r"^[0-9a-f]+ <(\S+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", asm, re.S | re.M))
    names = [k for k in bodies if any(s in k for s in ("tps_other_solve_kernel", "tps_other_maps_kernel", "remap_cubic_u8_kernel"))]
    assert len(names) == 3, sorted(bodies)
    for k in names:
        assert not re.search(r"v_pk_(mul|add|fma)_f32", bodies[k]), k
        assert "scratch_" not in bodies[k], k
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    seen = 0
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", notes, re.S):
        if not any(s in m.group(1) for s in ("tps_other", "remap_cubic")):
            continue
        seen += 1
        body = m.group(2)
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", body), m.group(1)
        spill = re.search(r"\.vgpr_spill_count:\s+(\d+)", body)
        assert spill is None or int(spill.group(1)) == 0, m.group(1)
    assert seen == 3
