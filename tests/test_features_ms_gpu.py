"""csrc/features_ms.hip on the GPU: `ops.feature_homography_ms` equals the CPU restatement (tests/_features_ms_ref.py) bit for bit -- pyramids,
keypoints, bins, descriptors, the best / second-best planes, the match list, the level-0 coordinates, the inlier mask, H, motion and info --
over the sizes, level counts, batches, hypothesis counts and planted match lists below; the result does not depend on the stream, the
workspace's history or a hipGraph replay and nothing is written outside the operands; each stage op, fed the restatement's intermediate
data, equals its stage."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _features_ms_ref as ms
import _features_ref as ref

pytestmark = pytest.mark.gpu

# one level; the level switch; ragged cells on two and three levels; five levels
SIZES = [(64, 64), (79, 64), (80, 80), (81, 100), (100, 125), (96, 130), (130, 96), (192, 256)]
FIELDS = ("kp1", "kp2", "bins1", "bins2", "desc1", "desc2", "nn", "matches", "count", "mask", "xy")


@functools.lru_cache(maxsize=None)
def _pair(h, w):
    return ref.small_pair(h, w)


@functools.lru_cache(maxsize=None)
def _want(h, w, levels=6, oriented=True, max_hyp=2048, seed=1, min_inliers=12):
    return ms.homography(*_pair(h, w), levels=levels, oriented=oriented, max_hyp=max_hyp, seed=seed, min_inliers=min_inliers)


def _same(got, want, tag=""):
    motion, Hm, info, fields = got
    assert motion.dtype == torch.float32 and Hm.dtype == torch.float32 and info.dtype == torch.int32, tag
    for k in ("pyr1", "pyr2"):
        assert len(fields[k]) == len(want[k]), (tag, k)
        for l, (g, w) in enumerate(zip(fields[k], want[k])):
            g = g.cpu().numpy()
            assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w), (tag, k, l, int((g != w).sum()))
    for k in FIELDS:
        g = fields[k].cpu().numpy()
        w = want[k]
        if k.startswith("desc"):
            g = g.view(np.uint32)
        if k == "xy":
            g, w = g.view(np.uint64), np.ascontiguousarray(w).view(np.uint64)
        assert g.shape == w.shape and np.array_equal(g, w), (tag, k, int((g != w).sum()))
    assert np.array_equal(info.cpu().numpy(), want["info"]), (tag, info.cpu().numpy(), want["info"])
    assert np.array_equal(Hm.cpu().numpy().view(np.uint32), want["H"].view(np.uint32)), (tag, Hm.cpu().numpy(), want["H"])
    assert np.array_equal(motion.cpu().numpy().view(np.uint32), want["motion"].view(np.uint32)), (tag, motion.cpu().numpy(), want["motion"])
    return True


def _run(a, b, **kw):
    from stitch_amd import ops
    return ops.feature_homography_ms(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), return_fields=True, **kw)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_equals_the_restatement_bit_for_bit(size):
    from stitch_amd import ops
    h, w = size
    want = _want(h, w)
    assert ops.feature_ms_level_sizes(h, w, 6) == ms.level_sizes(h, w, 6)
    assert ops.feature_ms_slots(h, w, 6) == ms.slots(h, w, 6) == want["kp1"].shape[1]
    assert _same(_run(*_pair(h, w)), want, f"{h}x{w}")
    bare = ops.feature_homography_ms(*(torch.from_numpy(t).cuda() for t in _pair(h, w)))
    assert len(bare) == 3 and np.array_equal(bare[0].cpu().numpy(), want["motion"]) and np.array_equal(bare[2].cpu().numpy(), want["info"])


def test_512_rotated_by_45_degrees_once():
    a, b, Hgt = ref.pair(512, 512, (20, 10, 45, 1e-4, 0), 3)
    want = ms.homography(a, b)
    assert want["info"][0, 0] == 1 and want["kp1"].shape[1] == 2848
    got = _run(a, b)
    assert _same(got, want, "512x512")
    assert ref.corner_error(got[1][0].cpu().numpy(), Hgt, 512, 512) < 3 * 0.754          # (tests/test_features_ms_cpu.py, MEASURED)


def test_a_quarter_turn_at_100x125():
    a, b, Hgt = ref.pair(100, 125, (3, -2, 90, 0, 0), 3)
    want = ms.homography(a, b, min_inliers=8)
    print(want["info"][0], ref.corner_error(want["H"][0], Hgt, 100, 125))
    assert want["info"][0, 0] == 1 and ref.homography(a, b, min_inliers=8)["info"][0, 0] == 0
    assert len(set(want["bins1"][0].tolist())) > 8                                       # the bins are in use
    assert _same(_run(a, b, min_inliers=8), want, "quarter turn")


@pytest.mark.parametrize("levels,oriented", [(1, True), (2, True), (8, True), (6, False), (1, False)])
def test_level_counts_and_upright_mode(levels, oriented):
    h, w = 100, 125
    want = _want(h, w, levels, oriented)
    assert len(want["pyr1"]) == min(levels, 3) and bool(want["bins1"].any()) == oriented
    assert _same(_run(*_pair(h, w), levels=levels, oriented=oriented), want, f"levels {levels} oriented {oriented}")


@pytest.mark.parametrize("B", (1, 2, 3))
def test_batches_with_a_constant_item(B):
    h, w = 81, 100
    items = [_pair(h, w), ref.degenerate("constant", h, w), ref.degenerate("identical", h, w)][:B] if B > 1 else [ref.degenerate("constant", h, w)]
    a, b = np.concatenate([i[0] for i in items]), np.concatenate([i[1] for i in items])
    want = ms.homography(a, b)
    assert _same(_run(a, b), want, f"B={B}")
    assert want["info"][min(1, B - 1), 0] == 0                      # the constant item: not valid, zero motion, identity
    if B > 1:
        assert np.array_equal(want["info"][0], _want(h, w)["info"][0]) and np.array_equal(want["H"][0], _want(h, w)["H"][0])      # items are independent


@pytest.mark.parametrize("name", ref.DEGENERATE)
def test_degenerate_images(name):
    a, b = ref.degenerate(name)
    assert _same(_run(a, b), ms.homography(a, b), name)


@pytest.mark.parametrize("max_hyp", (1, 64, 65, 2048))
def test_hypothesis_counts_and_seeds(max_hyp):
    h, w = 100, 125
    winners = set()
    for seed in (1, 0x9E3779B9):
        want = _want(h, w, 6, True, max_hyp, seed, 6)
        assert _same(_run(*_pair(h, w), max_hyp=max_hyp, seed=seed, min_inliers=6), want, f"max_hyp {max_hyp} seed {seed}")
        winners.add(int(want["info"][0, 4]))
    if max_hyp == 2048:
        assert len(winners) == 2 and -1 not in winners               # the seed reaches the result


def _dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def test_stage_ops_on_the_restatements_intermediate_data():
    from stitch_amd import ops
    h, w = 100, 125
    a, b = _pair(h, w)
    want = _want(h, w)
    for img, n in ((a, "1"), (b, "2")):
        pyr = ops.feature_ms_pyramid(torch.from_numpy(img).cuda())
        assert len(pyr) == 3 and all(np.array_equal(g.cpu().numpy(), x) for g, x in zip(pyr, want["pyr" + n]))
        kp, bins, box = ops.feature_ms_detect(_dev([p.astype(np.uint8) for p in want["pyr" + n]]))
        assert np.array_equal(kp.cpu().numpy(), want["kp" + n]) and np.array_equal(bins.cpu().numpy(), want["bins" + n])
        assert all(np.array_equal(g.cpu().numpy().astype(np.int64), x) for g, x in zip(box, want["box" + n]))
        upright = ops.feature_ms_detect(_dev([p.astype(np.uint8) for p in want["pyr" + n]]), oriented=False)
        assert np.array_equal(upright[0].cpu().numpy(), want["kp" + n]) and not upright[1].any()
        desc = ops.feature_ms_describe(_dev([p.astype(np.int16) for p in want["box" + n]]), *_dev([want["kp" + n], want["bins" + n]]))
        assert np.array_equal(desc.cpu().numpy().view(np.uint32), want["desc" + n])
    nn, matches, count = ops.feature_ms_match(*_dev([want["kp1"], want["desc1"].view(np.int32), want["kp2"], want["desc2"].view(np.int32)]), h, w)
    assert np.array_equal(nn.cpu().numpy(), want["nn"]) and np.array_equal(matches.cpu().numpy(), want["matches"])
    assert np.array_equal(count.cpu().numpy(), want["count"])
    motion, Hm, info, mask, xy = ops.feature_ms_ransac(*_dev([want["kp1"], want["kp2"], want["matches"], want["count"]]), h, w)
    assert np.array_equal(info.cpu().numpy(), want["info"]) and np.array_equal(mask.cpu().numpy(), want["mask"]) and np.array_equal(xy.cpu().numpy(), want["xy"])
    assert np.array_equal(Hm.cpu().numpy(), want["H"]) and np.array_equal(motion.cpu().numpy(), want["motion"])


def _ransac_equals(kp1, kp2, matches, m, H, W, levels, **kw):
    from stitch_amd import ops
    want = ms.ransac(kp1, kp2, matches, m, H, W, levels, **kw)
    got = ops.feature_ms_ransac(*_dev([kp1[None], kp2[None], matches[None], np.array([m], np.int32)]), H, W, levels, **kw)
    for g, x, name in zip(got, want, ("motion", "H", "info", "mask", "xy")):
        g = g.cpu().numpy()
        g = g[:, 0] if name == "xy" else g[0]
        assert np.array_equal(g, x), (name, g, x)
    return want


@pytest.mark.parametrize("name", ref.PLANTED)
def test_ransac_on_planted_matches(name):
    """m = 8 (most hypotheses repeat an index), a line (every system singular), seven matches, a third outliers; one level: feature_align's slots"""
    H, W = 96, 128
    kp1, kp2, matches, m = ref.planted_matches(name, H, W)
    want = _ransac_equals(kp1, kp2, matches, m, H, W, 1, max_hyp=256, thr=3.0, min_inliers=6, seed=7)
    plain = ref.ransac(kp1, kp2, matches, m, H, W, 256, 3.0, 6, 7)
    assert all(np.array_equal(a, b) for a, b in zip(want[:4], plain))                     # level 0 alone: the very numbers of feature_align
    assert want[2][0] == (name in ("m8", "outliers"))


def _long_list(m, tail_only):
    """synthetic keypoints in all N = 4548 slots of 640x640 at 8 levels and a list of m matches (a slot of image 1 with a slot of the same level of
    image 2), the last slot first: the list positions from 4096 on hold slots of level 0.  An inlier's partner is the image under a homography,
    rounded in its level: 0.5 px per axis off at level 0, 0.5 x 1.25^7 = 2.4 px at level 7.  tail_only: inliers at list positions >= 4096 alone,
    everything before them displaced by 12 px or more -- a refit that stops at 4096 entries finds nothing."""
    H = W = 640
    rng = np.random.default_rng(m)
    levels, start, sizes = ms.slot_levels(H, W, 8), ms.slot_starts(H, W, 8), ms.level_sizes(H, W, 8)
    N = len(levels)
    assert N == 4548
    kp1 = np.stack([[rng.integers(20, sizes[l][1] - 20), rng.integers(20, sizes[l][0] - 20)] for l in levels]).astype(np.int32)
    Hm = ref.homography_matrix(H, W, 7, -5, 3.0, 2e-5, -1e-5)
    p0 = ms.level0(kp1, H, W, 8)
    q0 = np.c_[p0, np.ones(N)] @ Hm.T
    q0 = q0[:, :2] / q0[:, 2:]
    scale = (0.8 ** levels)[:, None]
    kp2_at = np.rint((q0 + 0.5) * scale - 0.5).astype(np.int64)                          # back into the level of the slot
    lim = np.array([[sizes[l][1] - 1, sizes[l][0] - 1] for l in levels])
    partner = np.concatenate([start[l] + rng.permutation(start[l + 1] - start[l]) for l in range(len(sizes))])
    out = np.arange(N) > N - 1 - 4096 if tail_only else np.arange(N) % 5 == 0
    kp2_at[out] += rng.integers(12, 40, (int(out.sum()), 2))
    kp2 = np.full((N, 2), -1, np.int32)
    kp2[partner] = np.clip(kp2_at, 0, lim)
    matches = np.full((N, 2), -1, np.int32)
    matches[:m] = np.stack([np.arange(N)[::-1][:m], partner[::-1][:m]], 1)
    return kp1, kp2, matches, m


@pytest.mark.parametrize("m,tail_only", [(4096, False), (4097, False), (4500, True)])
def test_ransac_on_lists_longer_than_4096(m, tail_only):
    kp1, kp2, matches, m = _long_list(m, tail_only)
    seed = 1
    if tail_only:                                               # a seed under which one of the 2048 hypotheses draws its four matches from the tail
        seed = next(s for s in range(1, 200) if (ref.draws(s, np.arange(2048), m) >= 4096).all(1).any())
    want = _ransac_equals(kp1, kp2, matches, m, 640, 640, 8, max_hyp=2048, thr=3.0, min_inliers=12, seed=seed)
    info, mask = want[2], want[3]
    print(m, tail_only, seed, info)
    assert info[0] == 1 and info[3] == m
    if tail_only:
        assert not mask[:4096].any() and info[5] == mask[4096:m].sum() > 300 and not mask[m:].any()
    else:
        assert info[5] > 0.7 * m and mask[4000:m].any()


@pytest.fixture(scope="module")
def two_cases():
    return _pair(100, 125), _want(100, 125), _pair(81, 100), _want(81, 100)


def test_streams_and_workspace_history(two_cases):
    from stitch_amd import ops
    big, want_big, small, want_small = two_cases
    tb, ts = _dev(big), _dev(small)
    need = ops.feature_ms_workspace_bytes(1, 100, 125)
    assert need > ops.feature_ms_workspace_bytes(1, 81, 100) > 0 and need % 16 == 0
    ws1 = torch.full((need,), 255, dtype=torch.uint8).cuda()
    ws2 = torch.full((need,), 255, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):                                                     # two calls in flight in separate workspaces
        r1 = ops.feature_homography_ms(*tb, workspace=ws1, return_fields=True)
    with torch.cuda.stream(s2):
        r2 = ops.feature_homography_ms(*ts, workspace=ws2, return_fields=True)
    with torch.cuda.stream(s1):                                                     # the workspace just held the larger canvas
        r3 = ops.feature_homography_ms(*ts, workspace=ws1, return_fields=True)
    s1.synchronize(), s2.synchronize()
    assert _same(r1, want_big) and _same(r2, want_small) and _same(r3, want_small)
    with pytest.raises(ops.StitchErrorBase):
        ops.feature_homography_ms(*tb, workspace=ws1[:4096])


def test_captured_into_a_graph_and_replayed_on_other_pixels(two_cases):
    from stitch_amd import ops
    big, want_big, _, _ = two_cases
    other = [np.ascontiguousarray(t[:, :, ::-1, ::-1]) for t in big]
    static = _dev(big)
    ws = torch.empty(ops.feature_ms_workspace_bytes(1, 100, 125), dtype=torch.uint8).cuda()
    side_stream = torch.cuda.Stream()
    side_stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side_stream):
        ops.feature_homography_ms(*static, workspace=ws)
    torch.cuda.current_stream().wait_stream(side_stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = ops.feature_homography_ms(*static, workspace=ws)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(res[0].cpu().numpy(), want_big["motion"]) and np.array_equal(res[2].cpu().numpy(), want_big["info"])
    for t, a in zip(static, other):
        t.copy_(torch.from_numpy(a))
    graph.replay()
    torch.cuda.synchronize()
    want = ms.homography(*other)
    assert not np.array_equal(want["motion"], want_big["motion"])
    assert np.array_equal(res[0].cpu().numpy(), want["motion"]) and np.array_equal(res[1].cpu().numpy(), want["H"]) and np.array_equal(res[2].cpu().numpy(), want["info"])
    assert _same(ops.feature_homography_ms(*static, return_fields=True), want)         # eager on the same pixels


def test_every_operand_inside_a_frame_that_stays_intact():
    """the images in 0x5A frames; the outputs and a workspace of exactly st_feature_ms_workspace_bytes in sentinel frames"""
    from stitch_amd import ops
    from stitch_amd._lib import lib
    B, h, w, pad = 2, 81, 100, 64
    a = np.concatenate([_pair(h, w)[0], ref.degenerate("identical", h, w)[0]])
    b = np.concatenate([_pair(h, w)[1], ref.degenerate("identical", h, w)[1]])
    want = ms.homography(a, b, max_hyp=100, min_inliers=6)
    need = ops.feature_ms_workspace_bytes(B, h, w, 6, 100)
    L, N = ops.feature_ms_workspace_layout(B, h, w, 6, 100), ms.slots(h, w, 6)
    assert L["total"] == need

    def framed(count, dtype, fill, values=None):
        buf = torch.full((pad + count + pad,), fill, dtype=dtype, device="cuda")
        if values is not None:
            buf[pad:pad + count] = torch.from_numpy(np.ascontiguousarray(values).reshape(-1)).cuda()
        return buf
    fa, fb = framed(a.size, torch.float32, 90.0, a), framed(b.size, torch.float32, 90.0, b)
    motion, Hm, info, ws = framed(8 * B, torch.float32, -77.0), framed(9 * B, torch.float32, -77.0), framed(8 * B, torch.int32, -77), framed(need, torch.uint8, 0xA5)
    assert (ws.data_ptr() + pad) % 16 == 0
    ptr = lambda t: C.c_void_p(t.data_ptr() + pad * t.element_size())                # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.st_feature_ms_homography(ptr(fa), ptr(fb), B, h, w, 6, 1, 100, 3.0, 6, 1, ptr(motion), ptr(Hm), ptr(info), ptr(ws), need, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(motion[pad:pad + 8 * B].cpu().numpy().reshape(B, 4, 2), want["motion"]) and np.array_equal(Hm[pad:pad + 9 * B].cpu().numpy().reshape(B, 3, 3), want["H"])
    assert np.array_equal(info[pad:pad + 8 * B].cpu().numpy().reshape(B, 8), want["info"]) and want["info"][:, 0].tolist() == [1, 1]
    raw = ws[pad:pad + need].cpu().numpy()
    assert np.array_equal(raw[L["mask"]:L["mask"] + B * N].reshape(B, N), want["mask"])
    assert np.array_equal(raw[L["matches"]:L["matches"] + 8 * B * N].view(np.int32).reshape(B, N, 2), want["matches"])
    assert np.array_equal(raw[L["bins"]:L["bins"] + 2 * B * N].reshape(2, B, N), np.stack([want["bins1"], want["bins2"]]))
    assert np.array_equal(fa[pad:pad + a.size].cpu().numpy(), a.reshape(-1)) and np.array_equal(fb[pad:pad + b.size].cpu().numpy(), b.reshape(-1))
    for buf, count, fill in ((fa, a.size, 90.0), (fb, b.size, 90.0), (motion, 8 * B, -77.0), (Hm, 9 * B, -77.0), (info, 8 * B, -77), (ws, need, 0xA5)):
        assert (buf[:pad] == fill).all() and (buf[pad + count:] == fill).all()
