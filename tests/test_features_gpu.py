"""csrc/features.hip on the GPU: `ops.feature_homography` equals the CPU restatement (tests/_features_ref.py) bit for bit -- keypoints,
descriptors, the best / second-best planes, the match list, the winner, the inlier mask, H, motion and info -- over the sizes, batches,
degenerate inputs, hypothesis counts and seeds below; the result does not depend on the stream, the workspace's history or a hipGraph
replay and nothing is written outside the operands; each stage op, fed the restatement's intermediate data, equals its stage."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _features_ref as ref

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (64, 65), (65, 97), (96, 128), (160, 127), (160, 128), (160, 129), (127, 160), (128, 160), (129, 160), (192, 256)]
FIELDS = ("kp1", "kp2", "desc1", "desc2", "nn", "matches", "count", "mask")


@functools.lru_cache(maxsize=None)
def _pair(h, w):
    return ref.small_pair(h, w)


@functools.lru_cache(maxsize=None)
def _want(h, w, max_hyp=2048, seed=1, min_inliers=12):
    return ref.homography(*_pair(h, w), max_hyp=max_hyp, seed=seed, min_inliers=min_inliers)


def _same(got, want, tag=""):
    motion, Hm, info, fields = got
    assert motion.dtype == torch.float32 and Hm.dtype == torch.float32 and info.dtype == torch.int32, tag
    for k in FIELDS:
        g = fields[k].cpu().numpy()
        w = want[k]
        if k.startswith("desc"):
            g = g.view(np.uint32)
        assert g.shape == w.shape and np.array_equal(g, w), (tag, k, int((g != w).sum()))
    assert np.array_equal(info.cpu().numpy(), want["info"]), (tag, info.cpu().numpy(), want["info"])
    assert np.array_equal(Hm.cpu().numpy().view(np.uint32), want["H"].view(np.uint32)), (tag, Hm.cpu().numpy(), want["H"])
    assert np.array_equal(motion.cpu().numpy().view(np.uint32), want["motion"].view(np.uint32)), (tag, motion.cpu().numpy(), want["motion"])
    return True


def _run(a, b, **kw):
    from stitch_amd import ops
    return ops.feature_homography(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), return_fields=True, **kw)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_equals_the_restatement_bit_for_bit(size):
    """ragged cells, the wave edge of the match (N = 80 at five cells by four), the tile edge of the corner kernel"""
    from stitch_amd import ops
    h, w = size
    want = _want(h, w)
    assert ops.feature_slots(h, w) == ref.slots(h, w) == want["kp1"].shape[1]
    assert _same(_run(*_pair(h, w)), want, f"{h}x{w}")
    bare = ops.feature_homography(*(torch.from_numpy(t).cuda() for t in _pair(h, w)))
    assert len(bare) == 3 and np.array_equal(bare[0].cpu().numpy(), want["motion"]) and np.array_equal(bare[2].cpu().numpy(), want["info"])


def test_512_once():
    a, b, Hgt = ref.pair(512, 512, ref.MOTIONS[1], seed=4)
    want = ref.homography(a, b)
    assert want["info"][0, 0] == 1 and want["kp1"].shape[1] == 1024
    got = _run(a, b)
    assert _same(got, want, "512x512")
    assert ref.corner_error(got[1][0].cpu().numpy(), Hgt, 512, 512) < 1.0


@pytest.mark.parametrize("B", (1, 2, 3))
def test_batches_with_a_constant_item(B):
    h, w = 96, 128
    items = [_pair(h, w), ref.degenerate("constant", h, w), ref.degenerate("identical", h, w)][:B] if B > 1 else [ref.degenerate("constant", h, w)]
    a, b = np.concatenate([i[0] for i in items]), np.concatenate([i[1] for i in items])
    want = ref.homography(a, b)
    assert _same(_run(a, b), want, f"B={B}")
    assert want["info"][min(1, B - 1), 0] == 0                      # the constant item: not valid, zero motion, identity
    for k in range(B):                                               # items are independent
        solo = ref.homography(a[k:k + 1], b[k:k + 1])
        assert np.array_equal(solo["info"][0], want["info"][k]) and np.array_equal(solo["H"][0], want["H"][k])


@pytest.mark.parametrize("name", ref.DEGENERATE)
def test_degenerate_images(name):
    a, b = ref.degenerate(name)
    want = ref.homography(a, b)
    assert _same(_run(a, b), want, name)


@pytest.mark.parametrize("max_hyp", (1, 63, 64, 65, 2048))
def test_hypothesis_counts_and_seeds(max_hyp):
    h, w = 96, 128
    winners = set()
    for seed in (1, 0x9E3779B9):
        want = _want(h, w, max_hyp, seed, 6)
        assert _same(_run(*_pair(h, w), max_hyp=max_hyp, seed=seed, min_inliers=6), want, f"max_hyp {max_hyp} seed {seed}")
        winners.add(int(want["info"][0, 4]))
    if max_hyp == 2048:
        assert len(winners) == 2 and -1 not in winners               # the seed reaches the result


def _dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def test_stage_ops_on_the_restatements_intermediate_data():
    from stitch_amd import ops
    h, w = 160, 129
    a, b = _pair(h, w)
    want = _want(h, w)
    for img, kpw, boxw, dw in ((a, want["kp1"], want["box1"], want["desc1"]), (b, want["kp2"], want["box2"], want["desc2"])):
        kp, box = ops.feature_detect(torch.from_numpy(img).cuda())
        assert np.array_equal(kp.cpu().numpy(), kpw) and np.array_equal(box.cpu().numpy().astype(np.int64), boxw)
        desc = ops.feature_describe(*_dev([boxw.astype(np.int16), kpw]))
        assert np.array_equal(desc.cpu().numpy().view(np.uint32), dw)
    nn, matches, count = ops.feature_match(*_dev([want["kp1"], want["desc1"].view(np.int32), want["kp2"], want["desc2"].view(np.int32)]), h, w)
    assert np.array_equal(nn.cpu().numpy(), want["nn"]) and np.array_equal(matches.cpu().numpy(), want["matches"])
    assert np.array_equal(count.cpu().numpy(), want["count"])
    motion, Hm, info, mask = ops.feature_ransac(*_dev([want["kp1"], want["kp2"], want["matches"], want["count"]]), h, w)
    assert np.array_equal(info.cpu().numpy(), want["info"]) and np.array_equal(mask.cpu().numpy(), want["mask"])
    assert np.array_equal(Hm.cpu().numpy(), want["H"]) and np.array_equal(motion.cpu().numpy(), want["motion"])


@pytest.mark.parametrize("name", ref.PLANTED)
def test_ransac_on_planted_matches(name):
    """m = 8 (most hypotheses repeat an index), a line (every system singular), seven matches, a third outliers"""
    from stitch_amd import ops
    H, W = 96, 128
    kp1, kp2, matches, m = ref.planted_matches(name, H, W)
    want = ref.ransac(kp1, kp2, matches, m, H, W, 256, 3.0, 6, 7)
    got = ops.feature_ransac(*_dev([kp1[None], kp2[None], matches[None], np.array([m], np.int32)]), H, W, max_hyp=256, thr=3.0, min_inliers=6, seed=7)
    for g, x in zip(got, want):
        assert np.array_equal(g[0].cpu().numpy(), x), (name, g[0].cpu().numpy(), x)
    assert want[2][0] == (name in ("m8", "outliers"))


@functools.lru_cache(maxsize=None)
def _full_list():
    """synthetic keypoints in all N = 4096 slots of 1024x1024 and a list over every slot, the last slot first (built like _long_list of
    test_features_ms_gpu.py): a slot's partner is its image under a homography, rounded to the pixel, every fifth one displaced by 12 px or more.
    List position 4095, the last inlier flag the refit kernel holds, is slot 0: an inlier."""
    H = W = 1024
    rng = np.random.default_rng(4096)
    N = ref.slots(H, W)
    assert N == 4096
    kp1 = np.stack([rng.integers(16, W - 16, N), rng.integers(16, H - 16, N)], 1).astype(np.int32)
    q = np.c_[kp1, np.ones(N)] @ ref.homography_matrix(H, W, 7, -5, 3.0, 2e-5, -1e-5).T
    q = np.rint(q[:, :2] / q[:, 2:]).astype(np.int64)
    out = np.arange(N) % 5 == 2
    q[out] += rng.integers(12, 40, (int(out.sum()), 2))
    partner = rng.permutation(N)
    kp2 = np.full((N, 2), -1, np.int32)
    kp2[partner] = np.clip(q, 0, [W - 1, H - 1])
    return kp1, kp2, np.stack([np.arange(N)[::-1], partner[::-1]], 1).astype(np.int32)


@pytest.mark.parametrize("m", (4096, 4095))
def test_ransac_on_a_list_that_fills_every_slot(m):
    """N = 4096, the most a single-scale call has: the inlier flags fill the refit kernel's array to its last byte, and to one before it"""
    from stitch_amd import ops
    H = W = 1024
    kp1, kp2, matches = _full_list()
    matches = matches.copy()
    matches[m:] = -1
    kw = dict(max_hyp=2048, thr=3.0, min_inliers=12, seed=1)
    want = ref.ransac(kp1, kp2, matches, m, H, W, **kw)
    got = ops.feature_ransac(*_dev([kp1[None], kp2[None], matches[None], np.array([m], np.int32)]), H, W, **kw)
    for g, x, name in zip(got, want, ("motion", "H", "info", "mask")):
        g = g[0].cpu().numpy()
        assert g.dtype == x.dtype and g.shape == x.shape and np.array_equal(g.view(np.uint8), x.view(np.uint8)), (name, g, x)
    info, mask = want[2], want[3]
    assert info[0] == 1 and info[1] == info[2] == 4096 and info[3] == m and info[5] == mask[:m].sum() > 0.7 * m
    assert mask[4094] == 1 and mask[4095] == (m == 4096)


@pytest.fixture(scope="module")
def two_cases():
    return _pair(160, 129), _want(160, 129), _pair(96, 128), _want(96, 128)


def test_streams_and_workspace_history(two_cases):
    from stitch_amd import ops
    big, want_big, small, want_small = two_cases
    tb, ts = _dev(big), _dev(small)
    need = ops.feature_workspace_bytes(1, 160, 129)
    assert need > ops.feature_workspace_bytes(1, 96, 128) > 0 and need % 16 == 0
    ws1 = torch.full((need,), 255, dtype=torch.uint8).cuda()
    ws2 = torch.full((need,), 255, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):                                                     # two calls in flight in separate workspaces
        r1 = ops.feature_homography(*tb, workspace=ws1, return_fields=True)
    with torch.cuda.stream(s2):
        r2 = ops.feature_homography(*ts, workspace=ws2, return_fields=True)
    with torch.cuda.stream(s1):                                                     # the workspace just held the larger canvas
        r3 = ops.feature_homography(*ts, workspace=ws1, return_fields=True)
    s1.synchronize(), s2.synchronize()
    assert _same(r1, want_big) and _same(r2, want_small) and _same(r3, want_small)
    with pytest.raises(ops.StitchErrorBase):
        ops.feature_homography(*tb, workspace=ws1[:4096])


def test_captured_into_a_graph_and_replayed_on_other_pixels(two_cases):
    from stitch_amd import ops
    big, want_big, _, _ = two_cases
    other = [np.ascontiguousarray(t[:, :, ::-1, ::-1]) for t in big]
    static = _dev(big)
    ws = torch.empty(ops.feature_workspace_bytes(1, 160, 129), dtype=torch.uint8).cuda()
    side_stream = torch.cuda.Stream()
    side_stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side_stream):
        ops.feature_homography(*static, workspace=ws)
    torch.cuda.current_stream().wait_stream(side_stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = ops.feature_homography(*static, workspace=ws)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(res[0].cpu().numpy(), want_big["motion"]) and np.array_equal(res[2].cpu().numpy(), want_big["info"])
    for t, a in zip(static, other):
        t.copy_(torch.from_numpy(a))
    graph.replay()
    torch.cuda.synchronize()
    want = ref.homography(*other)
    assert not np.array_equal(want["motion"], want_big["motion"])
    assert np.array_equal(res[0].cpu().numpy(), want["motion"]) and np.array_equal(res[1].cpu().numpy(), want["H"]) and np.array_equal(res[2].cpu().numpy(), want["info"])
    assert _same(ops.feature_homography(*static, return_fields=True), want)         # eager on the same pixels


def test_every_operand_inside_a_frame_that_stays_intact():
    """the images in 0x5A frames; the outputs and a workspace of exactly st_feature_workspace_bytes in sentinel frames"""
    from stitch_amd import ops
    from stitch_amd._lib import lib
    B, h, w, pad = 2, 65, 97, 64
    a = np.concatenate([_pair(h, w)[0], ref.degenerate("identical", h, w)[0]])
    b = np.concatenate([_pair(h, w)[1], ref.degenerate("identical", h, w)[1]])
    want = ref.homography(a, b, max_hyp=100, min_inliers=6)
    need = ops.feature_workspace_bytes(B, h, w, 100)
    L, N = ops.feature_workspace_layout(B, h, w, 100), ref.slots(h, w)
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
    assert lib.st_feature_homography(ptr(fa), ptr(fb), B, h, w, 100, 3.0, 6, 1, ptr(motion), ptr(Hm), ptr(info), ptr(ws), need, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(motion[pad:pad + 8 * B].cpu().numpy().reshape(B, 4, 2), want["motion"]) and np.array_equal(Hm[pad:pad + 9 * B].cpu().numpy().reshape(B, 3, 3), want["H"])
    assert np.array_equal(info[pad:pad + 8 * B].cpu().numpy().reshape(B, 8), want["info"]) and want["info"][:, 0].tolist() == [1, 1]
    raw = ws[pad:pad + need].cpu().numpy()
    assert np.array_equal(raw[L["mask"]:L["mask"] + B * N].reshape(B, N), want["mask"])
    assert np.array_equal(raw[L["matches"]:L["matches"] + 8 * B * N].view(np.int32).reshape(B, N, 2), want["matches"])
    assert np.array_equal(fa[pad:pad + a.size].cpu().numpy(), a.reshape(-1)) and np.array_equal(fb[pad:pad + b.size].cpu().numpy(), b.reshape(-1))
    for buf, count, fill in ((fa, a.size, 90.0), (fb, b.size, 90.0), (motion, 8 * B, -77.0), (Hm, 9 * B, -77.0), (info, 8 * B, -77), (ws, need, 0xA5)):
        assert (buf[:pad] == fill).all() and (buf[pad + count:] == fill).all()
