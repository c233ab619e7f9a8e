"""The refusal matrix of the classical-path C entries (csrc/features.hip, features_ms.hip, dense_flow.hip, patchmatch.hip, seam_gc.hip,
crop.hip), host logic only: every refused variant of tests/_classical_cases.py returns its refusal code on fabricated addresses, which
nothing dereferences because every case must return before a launch.  Only variants are called, never a base record of an entry that
launches, and the calls are skipped where a device is visible: there a case accepted by mistake would launch on those addresses (the same
table runs on live buffers in tests/test_classical_matrix_gpu.py).  Also here: the table's own coverage, the wrappers of stitch_amd/ops.py
that raise before any pointer is taken, and the properties the inputs of the GPU file are chosen for."""
import ctypes as C

import numpy as np
import pytest
import torch

import _classical_cases as cc
import _dense_flow_ref as dfref
import _features_ref as ftref

FAKE = 0x7F0000000000


def _device_visible():
    return torch.cuda.is_available()


def _addresses(entry):
    host = {a.name: (C.c_int64 * 2048)() for a in cc.entries()[entry] if a.role == "host"}           # (real memory: an accepted helper writes there)
    order = [a.name for a in cc.entries()[entry]]
    return lambda op: C.addressof(host[op]) if op in host else FAKE + ((order.index(op) + 1) << 32)


# ---- the table itself --------------------------------------------------------------------------------------------------------------------------
def test_the_table_covers_every_entry_of_the_six_files():
    import re
    from stitch_amd import _lib
    names = set(cc.entries())
    assert len(names) == 34 and names <= set(_lib.declared_functions())
    for src, prefix in (("features.hip", "st_feature_"), ("features_ms.hip", "st_feature_ms_"), ("dense_flow.hip", "st_dense_flow"), ("seam_gc.hip", "st_seam_gc_"),
                        ("crop.hip", "st_inner_rect"), ("patchmatch.hip", "st_patchmatch_")):
        text = open(f"{_lib.HERE}/csrc/{src}").read()
        defined = set(re.findall(r'extern "C" int (st_\w+)\(', text))
        assert defined and defined <= names and all(n.startswith(prefix) for n in defined), src
        names -= defined
    assert not names, names


@pytest.mark.parametrize("entry", sorted(cc.entries()))
def test_every_field_of_an_entry_is_violated_and_every_pair_three_times(entry):
    rows = cc.refusals(entry)
    fields = {a.name for a in cc.entries()[entry]}
    assert {c.field for c in rows} == fields - cc.no_refusal(entry), (entry, fields - {c.field for c in rows})
    b = cc.base(entry)
    for c in cc.table():
        if c.entry == entry:
            rec = cc.record(c)
            assert [k for k in b if not cc._same(rec[k], b[k])] == [c.field]                        # exactly one field differs from the base
    count = {}
    for c in rows:
        if c.kind.startswith("overlap:"):
            pair = frozenset(c.kind.split(":")[1].split("|"))
            count[pair] = count.get(pair, 0) + 1
    assert set(count) == {frozenset(p) for p in cc.pairs(entry)} and set(count.values()) <= {3}, (entry, count)
    lim = cc.LIMITS[cc.family(entry)]
    for a in cc.entries()[entry]:                                                                   # each category of the issue, per field kind
        kinds = {c.kind for c in rows if c.field == a.name}
        if a.role == "scalar" and a.name in lim:
            assert {"below"} | ({"above"} if lim[a.name][1] is not None else set()) <= kinds, a.name
        if a.name == "thr":
            assert len([c for c in rows if c.field == "thr"]) == 4
        if a.name.endswith("_channels"):
            assert sorted(c.value for c in rows if c.field == a.name) == [0, 2, 4]
        if a.role == "ws":
            assert {"null", "misaligned4", "misaligned8"} <= kinds
        if a.name == "workspace_bytes":
            assert kinds == {"short"}
        if a.role in ("in", "out", "host") and (entry, a.name) not in cc.OPTIONAL:
            assert "null" in kinds, a.name
    ins = [a.name for a in cc.entries()[entry] if a.role == "in"]
    assert len([c for c in cc.accepted(entry) if c.kind.startswith("alias:")]) == len(ins) * (len(ins) - 1) // 2


def test_the_issues_scalar_cases_are_in_the_table():
    have = {(c.entry, c.field, c.value) for c in cc.refusals() if not isinstance(c.value, (cc.Ptr, float)) and c.value is not None}
    for entry, field, values in (("st_feature_ransac", "max_hyp", (0, 65537)), ("st_feature_homography", "min_inliers", (-1,)), ("st_feature_ms_homography", "levels", (0, 9)),
                                 ("st_feature_ms_detect", "oriented", (2, -1)), ("st_dense_flow", "iters", (0, 17)), ("st_patchmatch_fill", "iters", (-1, 65)),
                                 ("st_dense_flow_iterate", "radius", (0, 8)), ("st_dense_flow", "damping", (-1, (1 << 24) + 1)), ("st_dense_flow_pyramid", "mask2_channels", (0, 2, 4)),
                                 ("st_feature_homography", "B", (0, 65)), ("st_feature_detect", "H", (63, 1025)), ("st_dense_flow", "W", (15, 1025)),
                                 ("st_seam_gc_begin", "H", (0, 4097)), ("st_inner_rect", "W", (0, 4097)), ("st_patchmatch_fill", "H", (14, 4097))):
        for v in values:
            assert (entry, field, v) in have, (entry, field, v)
    thr = [c.value for c in cc.refusals("st_feature_ms_ransac") if c.field == "thr"]
    assert 0.0 in thr and -1.0 in thr and float("inf") in thr and any(v != v for v in thr)


# ---- the refusals --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.refusals(), ids=cc.case_id)
def test_refused_before_any_launch(case):
    if _device_visible() and case.entry not in cc.HOST_ONLY:
        pytest.skip("a device is visible: this case runs on live buffers in test_classical_matrix_gpu.py")
    want = cc.REFUSAL.get(case.entry, cc.EINVAL)
    assert cc.call(case.entry, cc.record(case), _addresses(case.entry)) == want


@pytest.mark.parametrize("case", [c for c in cc.accepted() if c.entry in cc.HOST_ONLY], ids=cc.case_id)
def test_helpers_accept_each_limit_and_a_null_optional_pointer(case):
    rc = cc.call(case.entry, cc.record(case), _addresses(case.entry))
    assert rc > 0 if case.entry in cc.REFUSAL else rc == 0


@pytest.mark.parametrize("entry", sorted(cc.HOST_ONLY))
def test_helpers_accept_their_base_record(entry):
    rc = cc.call(entry, cc.base(entry), _addresses(entry))
    assert rc > 0 if entry in cc.REFUSAL else rc == 0


# ---- the wrappers of ops.py, before any pointer is taken --------------------------------------------------------------------------------------
def _img(B=1, H=64, W=64, dtype=torch.float32):
    return torch.zeros((B, 3, H, W), dtype=dtype)


def test_wrappers_refuse_scalars_outside_the_contract():
    from stitch_amd import ops
    a = _img()
    for kw in (dict(max_hyp=0), dict(max_hyp=65537), dict(thr=0.0), dict(thr=-1.0), dict(thr=float("nan")), dict(thr=float("inf")), dict(min_inliers=-1)):
        with pytest.raises(ValueError):
            ops.feature_homography(a, a, **kw)
        with pytest.raises(ValueError):
            ops.feature_homography_ms(a, a, **kw)
        N = ops.feature_slots(64, 64)
        kp, mt, ct = torch.zeros((1, N, 2), dtype=torch.int32), torch.zeros((1, N, 2), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
        with pytest.raises(ValueError):
            ops.feature_ransac(kp, kp, mt, ct, 64, 64, **kw)
        with pytest.raises(ValueError):
            ops.feature_ms_ransac(kp, kp, mt, ct, 64, 64, 1, **kw)
    for levels in (0, 9, 1.5):
        with pytest.raises(ValueError):
            ops.feature_homography_ms(a, a, levels=levels)
        with pytest.raises(ValueError):
            ops.feature_ms_pyramid(a, levels=levels)
    f = _img(1, 16, 16)
    for kw in (dict(levels=0), dict(levels=9), dict(iters=0), dict(iters=17), dict(radius=0), dict(radius=8), dict(damping=-1), dict(damping=(1 << 24) + 1), dict(radius=1.5)):
        with pytest.raises(ValueError):
            ops.dense_flow(f, f, **kw)
    v, m, u = torch.zeros((1, 16, 16), dtype=torch.int16), torch.zeros((1, 16, 16), dtype=torch.uint8), torch.zeros((1, 2, 16, 16), dtype=torch.int32)
    for kw in (dict(radius=0), dict(radius=8), dict(damping=-1), dict(damping=(1 << 24) + 1)):
        with pytest.raises(ValueError):
            ops.dense_flow_iterate(v, v, m, m, u, **kw)
    img, mask = torch.zeros((15, 15, 3), dtype=torch.uint8), torch.zeros((15, 15), dtype=torch.uint8)
    for kw in (dict(iters=-1), dict(iters=65), dict(levels=0), dict(levels=9)):
        with pytest.raises(ValueError):
            ops.inpaint_patchmatch(img, mask, **kw)
    k = torch.ones((1, 1, 8, 8))
    with pytest.raises(ValueError):
        ops.seam_gc(torch.zeros((1, 3, 8, 8)), torch.zeros((1, 3, 8, 8)), k, k, max_rounds=-1)


def test_wrappers_refuse_shapes_outside_the_contract():
    from stitch_amd import ops
    for B, H, W in ((0, 64, 64), (65, 64, 64), (1, 63, 64), (1, 64, 63), (1, 1025, 64), (1, 64, 1025)):
        a = torch.zeros((B, 3, H, W)) if B else torch.zeros((0, 3, H, W))
        for fn in (lambda: ops.feature_homography(a, a), lambda: ops.feature_homography_ms(a, a), lambda: ops.feature_detect(a), lambda: ops.feature_ms_pyramid(a)):
            with pytest.raises(ValueError):
                fn()
    for B, H, W in ((0, 16, 16), (65, 16, 16), (1, 15, 16), (1, 16, 15), (1, 1025, 16), (1, 16, 1025)):
        a = torch.zeros((B, 3, H, W))
        with pytest.raises(ValueError):
            ops.dense_flow(a, a)
        with pytest.raises(ValueError):
            ops.dense_flow_pyramid(a, a)
    for H, W in ((14, 15), (15, 14), (4097, 15), (15, 4097)):
        with pytest.raises(ValueError):
            ops.inpaint_patchmatch(torch.zeros((H, W, 3), dtype=torch.uint8), torch.zeros((H, W), dtype=torch.uint8))
    for H, W in ((4097, 1), (1, 4097)):
        with pytest.raises(ValueError):
            ops.inner_rect(torch.zeros((1, 1, H, W)))


def test_wrappers_refuse_dtype_rank_mismatch_and_strides():
    from stitch_amd import ops
    a = _img()
    wrong = [(_img(dtype=torch.float64), a), (a[0], a), (torch.zeros((1, 1, 64, 64)), a), (a, _img(1, 64, 96)), (a, _img(2)), (a, _img(dtype=torch.float16))]
    for x, y in wrong:
        with pytest.raises(ValueError):
            ops.feature_homography(x, y)
        with pytest.raises(ValueError):
            ops.feature_homography_ms(x, y)
    f = _img(1, 16, 16)
    for x, y in ((_img(1, 16, 16, torch.float64), f), (f[0], f), (f, _img(1, 16, 32)), (f, _img(2, 16, 16))):
        with pytest.raises(ValueError):
            ops.dense_flow(x, y)
    for mask in (torch.ones((1, 2, 16, 16)), torch.ones((1, 1, 16, 17)), torch.ones((1, 1, 16, 16), dtype=torch.float64), torch.ones((2, 1, 16, 16)), torch.ones((1, 16, 16))):
        with pytest.raises(ValueError):
            ops.dense_flow(f, f, mask1=mask)
        with pytest.raises(ValueError):
            ops.dense_flow_pyramid(f, f, mask2=mask)
    strided = torch.zeros((1, 3, 64, 128))[:, :, :, ::2]
    assert strided.shape == a.shape and not strided.is_contiguous()
    for fn in (lambda: ops.feature_homography(strided, a), lambda: ops.feature_detect(strided), lambda: ops.feature_homography_ms(strided, a),
               lambda: ops.feature_ms_pyramid(strided)):
        with pytest.raises(ValueError, match="contiguous"):
            fn()
    N = ops.feature_slots(64, 64)
    box, kp = torch.zeros((1, 64, 64), dtype=torch.int16), torch.zeros((1, N, 2), dtype=torch.int32)
    for b, k in ((box.to(torch.int32), kp), (box, kp.to(torch.int64)), (box, kp[:, :-1]), (box, kp[0]), (torch.zeros((1, 64, 96), dtype=torch.int16), kp)):
        with pytest.raises(ValueError):
            ops.feature_describe(b, k)
    with pytest.raises(ValueError, match="contiguous"):
        ops.feature_describe(torch.zeros((1, 64, 128), dtype=torch.int16)[:, :, ::2], kp)
    desc = torch.zeros((1, N, 8), dtype=torch.int32)
    for k1, d1 in ((kp, desc[:, :, :4]), (kp.to(torch.int16), desc), (kp[:, :4], desc)):
        with pytest.raises(ValueError):
            ops.feature_match(k1, d1, kp, desc, 64, 64)
        with pytest.raises(ValueError):
            ops.feature_ms_match(k1, d1, kp, desc, 64, 64, 1)
    v, m, u = torch.zeros((1, 16, 16), dtype=torch.int16), torch.zeros((1, 16, 16), dtype=torch.uint8), torch.zeros((1, 2, 16, 16), dtype=torch.int32)
    for args in ((v.to(torch.int32), v, m, m, u), (v, v[:, :8], m, m, u), (v, v, m.to(torch.int16), m, u), (v, v, m, m, u[:, :1]), (v[0], v, m, m, u)):
        with pytest.raises(ValueError):
            ops.dense_flow_iterate(*args)
    img, mask = torch.zeros((15, 15, 3), dtype=torch.uint8), torch.zeros((15, 15), dtype=torch.uint8)
    for i, k in ((img.to(torch.float32), mask), (img[:, :, :2], mask), (img, mask[:14]), (img, mask.to(torch.int32)), (img[0], mask)):
        with pytest.raises(ValueError):
            ops.inpaint_patchmatch(i, k)
    for k1, k2 in ((torch.ones((1, 2, 8, 8)), None), (torch.ones((8, 8)), None), (torch.ones((1, 1, 8, 8)), torch.ones((1, 1, 8, 9))),
                   (torch.ones((1, 1, 8, 8), dtype=torch.float64), None), (torch.ones((2, 1, 8, 8)), None)):
        with pytest.raises(ValueError):
            ops.inner_rect(k1, k2)


# ---- the guards restated: what the GPU file's expectations rest on ---------------------------------------------------------------------------
def test_the_restated_index_clamp_decides_the_expectation():
    """the mutation check for ft_norm_kernel's clamp, on the CPU side: without the index rule the restatement gives other bits for the hostile
    lists of part B, so the expectations the kernel is compared with do depend on it"""
    H, W = 96, 128
    N = ftref.slots(H, W)
    hit = 0
    for bad in cc.HOSTILE_INDICES:
        kp1, kp2, mt, m = cc.hostile_matches(H, W, bad)
        with_rule = cc.ransac_guarded(kp1, kp2, mt, m, H, W, max_hyp=256, thr=3.0, min_inliers=6, seed=7)
        try:
            without = cc.ransac_guarded(kp1, kp2, mt, m, H, W, clamp=False, max_hyp=256, thr=3.0, min_inliers=6, seed=7)
        except IndexError:                                                                          # (numpy refuses what the kernel would have read)
            hit += 1
            continue
        hit += not all(np.array_equal(a, b) for a, b in zip(with_rule, without))
    assert hit == len(cc.HOSTILE_INDICES)
    matches = cc.hostile_matches(H, W, -1)[2]
    mt, mm = cc.clamp_list(matches, -5, N)
    assert mm == 0 and cc.clamp_list(matches, cc.I32_MAX, N)[1] == N and cc.clamp_list(matches, N + 1, N)[1] == N


def test_the_restated_describe_guard():
    H, W = 65, 97
    rng = np.random.default_rng(2)
    box = rng.integers(0, 6376, (H, W)).astype(np.int64)
    kp = cc.hostile_keypoints(H, W, ftref.BORDER, ftref.slots(H, W))
    d = cc.describe_guarded(box, kp)
    inside = (kp[:, 0] >= 16) & (kp[:, 0] < W - 16) & (kp[:, 1] >= 16) & (kp[:, 1] < H - 16)
    assert inside.sum() == 5 and (d[~inside] == 0).all() and (d[inside] != 0).any(1).all()
    assert np.array_equal(d[inside], ftref.describe(box, kp[inside]))


# ---- the saturated inputs reach the extremes they are chosen for ---------------------------------------------------------------------------------
def test_saturated_inputs_reach_the_extremes_of_the_intermediates():
    """flow: max |gx| = max |It| = 4080 = 16 * 255, the largest values the int16 planes of df_iterate_kernel hold; features: a Sobel response
    of +-1020 = 4 * 255, the largest gradient of ft_detect_kernel.  The restatements hold all of these as int64."""
    for name in ("checker", "steps", "steps_swapped"):
        a, b = cc.saturated_pair(name)
        V1, m1 = dfref.level0(a[0], None)
        V2, m2 = dfref.level0(b[0], None)
        assert V1.dtype == np.int64 and V1.max() == 4080 and V1.min() == 0
        gx, gy, w = dfref.gradients(V1, m1)
        J, w2 = dfref.sample(V2, m2, np.zeros_like(V1), np.zeros_like(V1))
        It = J - V1
        assert gx.dtype == np.int64 and It.dtype == np.int64 and dfref.window_sum(gx * gx, 7).dtype == np.int64
        assert np.abs(It).max() == 4080 and np.abs(It[8:-8, 8:-8]).max() == 4080, name
        assert max(np.abs(gx).max(), np.abs(gy).max()) == 4080, name                                # (at the clamped border for every pattern)
        if name == "steps_swapped":
            assert gx[8:-8, 8:-8].max() == 4080 and gx[8:-8, 8:-8].min() == -4080                   # and away from it for period 3
            assert dfref.window_sum(gx * gx, 7).max() >= 150 * 4080 ** 2 > 2 ** 31                      # 10 of the 15 columns of a window, 15 rows: past int32
        for img in (a, b):
            Y = ftref.luma(img[0])
            ix, iy = ftref.sobel(Y)
            assert ix.dtype == np.int64 and ftref.harris(Y).dtype == np.int64
            assert max(np.abs(ix).max(), np.abs(iy).max()) == (510 if name == "checker" else 1020), name       # (the checkerboard cancels inside 1 2 1)
    ix, _ = ftref.sobel(ftref.luma(cc.saturated_pair("steps")[1][0]))
    assert ix[8:-8, 8:-8].max() == 1020 and ix[8:-8, 8:-8].min() == -1020
    a, b = cc.saturated_pair("nonfinite")
    assert np.isinf(a).sum() == 200 and (np.abs(a[np.isfinite(a)]) == np.float32(1e30)).sum() == 200
    p = ftref.pixels(a[0])
    assert p.min() == 0 and p.max() == 255
