"""csrc/dense_flow.hip on the GPU: `ops.dense_flow` equals the CPU restatement (tests/_dense_flow_ref.py) bit for bit -- flow, support, both
pyramids and the final flow of every level -- over the sizes, batches, arguments and masks below; the result does not depend on the stream,
the workspace's history or a hipGraph replay and nothing is written outside the operands; each stage op, fed the restatement's intermediate
data, equals its stage."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _dense_flow_ref as ref

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 32, 16                   # df_iterate_kernel's tile
AROUND_TILES = (TILE_W - 1, TILE_W, TILE_W + 1, 2 * TILE_W - 1, 2 * TILE_W, 2 * TILE_W + 1)
SIZES = [(16, 16), (31, 33), (32, 32), (33, 65)] + [(40, w) for w in AROUND_TILES] + [(h, 40) for h in AROUND_TILES] + [(TILE_H + 1, 48), (96, 128), (192, 256)]


@functools.lru_cache(maxsize=None)
def _pair(h, w, seed=3, holes=True):
    """(img1, img2 fp32 [1,3,h,w], mask1, mask2 fp32 [1,1,h,w]): a smooth flow of 2 px (6 px from 96 rows on), image 2 with gain, bias, noise and its right
    fifth masked out; holes in both masks that cross the tile edges at x = 32 and y = 16"""
    a, b, m2, _ = ref.flow_pair(h, w, 6 if h >= 96 else 2, seed)
    m1 = np.ones((1, h, w), np.float32)
    if holes:
        m1[:, 12:min(20, h - 2), max(w - 40, 2):max(w - 30, 6)] = 0
        m2[:, max(h - 20, 1):max(h - 12, 4), 3:9] = 0.5                            # 0.5 is unset
        if w > 36:
            m1[:, 2:5, 28:36] = np.nan
    return a[None], b[None], m1[None], m2[None]


def _want_items(a, b, m1, m2, **kw):
    """the restatement per item -> (flow [B,2,H,W], support [B,1,H,W], fields with [B,...] arrays per level)"""
    res = [ref.dense_flow(a[k], b[k], None if m1 is None else m1[k], None if m2 is None else m2[k], **kw) for k in range(a.shape[0])]
    L = len(res[0][2]["u"])
    fields = {n: [np.stack([r[2][n][l] for r in res]) for l in range(L)] for n in ("v1", "v2", "m1", "m2", "u")}
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])[:, None], fields


@functools.lru_cache(maxsize=None)
def _want(h, w, seed=3):
    return _want_items(*_pair(h, w, seed))


def _same(got, want, tag=""):
    flow, support, fields = got
    wflow, wsup, wf = want
    assert flow.dtype == torch.float32 and support.dtype == torch.uint8 and tuple(support.shape) == wsup.shape, tag
    for n in ("v1", "v2", "m1", "m2", "u"):
        assert len(fields[n]) == len(wf[n]), (tag, n)
        for l, (g, x) in enumerate(zip(fields[n], wf[n])):
            g = g.cpu().numpy().astype(np.int64)
            assert g.shape == x.shape and np.array_equal(g, x), (tag, n, l, int((g != x).sum()))
    assert np.array_equal(support.cpu().numpy(), wsup), (tag, "support", int((support.cpu().numpy() != wsup).sum()))
    assert np.array_equal(flow.cpu().numpy().view(np.uint32), wflow.view(np.uint32)), (tag, "flow")
    return True


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _run(a, b, m1=None, m2=None, **kw):
    from stitch_amd import ops
    return ops.dense_flow(_t(a), _t(b), _t(m1), _t(m2), return_fields=True, **kw)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_equals_the_restatement_bit_for_bit(size):
    """one level, the level threshold at 32, one below / at / above one and two tile widths and heights, ragged coarse levels"""
    from stitch_amd import ops
    h, w = size
    want = _want(h, w)
    assert len(want[2]["u"]) == len(ops.dense_flow_level_sizes(h, w)) == len(ref.level_sizes(h, w, 5))
    assert _same(_run(*_pair(h, w)), want, f"{h}x{w}")
    bare = ops.dense_flow(*(_t(t) for t in _pair(h, w)))
    assert len(bare) == 2 and np.array_equal(bare[0].cpu().numpy(), want[0]) and np.array_equal(bare[1].cpu().numpy(), want[1])
    if h >= 96:
        assert np.abs(want[0]).max() > 2 and 0.3 < want[1].mean() < 1


def test_512_once():
    a, b, m2, f = ref.flow_pair(512, 512, 8, seed=3)
    want = _want_items(a[None], b[None], None, m2[None])
    got = _run(a[None], b[None], None, m2[None])
    assert _same(got, want, "512x512") and len(want[2]["u"]) == 5
    mean, p99, zero, n = ref.endpoint_error(got[0][0].cpu().numpy(), got[1][0, 0].cpu().numpy(), f, m2[None], 8)
    assert mean < zero / 3


def test_direction_through_flow_warp():
    """img1(p) ~ img2(p + flow(p)): warping image 2 by the flow lands on image 1"""
    from stitch_amd import ops
    a, b, m2, f = ref.flow_pair(192, 256, 6, seed=3, masked=False)
    ta, tb = _t(a[None]), _t(b[None])
    flow, support = ops.dense_flow(ta, tb)
    warped = ops.flow_warp(tb, flow)
    sel = (support[0, 0] > 0).cpu().numpy()
    sel[:16], sel[-16:], sel[:, :16], sel[:, -16:] = False, False, False, False
    adj = lambda g: (g - 10.0) / 0.85                                               # noqa: E731  (the known gain and bias of image 2)
    after = np.abs(adj(warped[0, 0].cpu().numpy()) - a[0])[sel].mean()
    before = np.abs(adj(b[0]) - a[0])[sel].mean()
    assert sel.mean() > 0.5 and after < before / 2, (before, after)
    assert (np.hypot(*(flow[0].cpu().numpy() - f))[sel]).mean() < np.hypot(*f)[sel].mean() / 3


@pytest.mark.parametrize("B", (1, 2, 3))
def test_batches_with_a_constant_item(B):
    h, w = 48, 65
    const = (np.full((1, 3, h, w), 90.0, np.float32), np.full((1, 3, h, w), 45.0, np.float32), np.ones((1, 1, h, w), np.float32), np.ones((1, 1, h, w), np.float32))
    items = [_pair(h, w), const, _pair(h, w, 7)][:B] if B > 1 else [const]
    a, b, m1, m2 = (np.concatenate([i[k] for i in items]) for k in range(4))
    want = _want_items(a, b, m1, m2)
    assert _same(_run(a, b, m1, m2), want, f"B={B}")
    k = min(1, B - 1)                                                                # the constant item: zero flow, supported but for the corner
    assert not want[0][k].any() and want[1][k].sum() == h * w - 1
    if B > 1:
        assert want[0][0].any() and _same(_run(a[:1], b[:1], m1[:1], m2[:1]), _want(h, w), "solo")      # items are independent


ARGS = [dict(radius=1), dict(radius=7), dict(iters=1), dict(iters=1, radius=7, levels=1), dict(levels=1), dict(levels=3), dict(levels=8), dict(damping=0),
        dict(damping=1 << 24, iters=2)]


@pytest.mark.parametrize("kw", ARGS, ids=lambda k: "_".join(f"{n}{v}" for n, v in k.items()))
def test_arguments(kw):
    h, w = 96, 130
    args = _pair(h, w)
    want = _want_items(*args, **kw)
    assert len(want[2]["u"]) == min(kw.get("levels", 5), 3)                         # 96x130 -> 48x65 -> 24x33: capped at three levels
    assert _same(_run(*args, **kw), want, str(kw))


@pytest.mark.parametrize("masks", ("none", "one_channel", "three_channels", "mixed"))
def test_mask_layouts(masks):
    h, w = 64, 96
    a, b, m1, m2 = _pair(h, w)
    junk = np.zeros((1, 2, h, w), np.float32)                                       # channels 1 and 2 are not read
    three = lambda m: np.concatenate([m, junk], 1)                                  # noqa: E731
    g1, g2 = dict(none=(None, None), one_channel=(m1, m2), three_channels=(three(m1), three(m2)), mixed=(None, three(m2)))[masks]
    r1, r2 = (None, None) if masks == "none" else (None, m2) if masks == "mixed" else (m1, m2)
    assert _same(_run(a, b, g1, g2), _want_items(a, b, r1, r2), masks)


def test_stage_ops_on_the_restatements_intermediate_data():
    from stitch_amd import ops
    h, w = 65, 97
    a, b, m1, m2 = _pair(h, w)
    want = _want(h, w)[2]
    pyr = ops.dense_flow_pyramid(_t(a), _t(b), _t(m1), _t(m2))
    for n in ("v1", "v2", "m1", "m2"):
        assert len(pyr[n]) == 3
        for g, x in zip(pyr[n], want[n]):
            assert np.array_equal(g.cpu().numpy().astype(np.int64), x), n
    rng = np.random.default_rng(2)
    for l, r, damping in ((2, 4, 65536), (1, 7, 0), (0, 1, 4096), (0, 4, 65536)):
        hl, wl = want["v1"][l].shape[1:]
        U = np.zeros((1, 2, hl, wl), np.int64) if l == 2 else ref.upscale(want["u"][l + 1][0], hl, wl)[None]
        U = U + rng.integers(-300, 300, U.shape)                                    # fractions, negative coordinates, samples outside
        U[0, :, 0, 0], U[0, :, 5, wl - 2], U[0, :, 6, wl - 2], U[0, :, hl - 2, 3], U[0, :, hl - 2, 4] = (-300, -257), (0, 17), (256, 0), (5, 255), (5, 256)
        wu, wok = ref.iterate(want["v1"][l][0], want["v2"][l][0], want["m1"][l][0], want["m2"][l][0], U[0], r, damping)
        gu, gok = ops.dense_flow_iterate(_t(want["v1"][l].astype(np.int16)), _t(want["v2"][l].astype(np.int16)), _t(want["m1"][l].astype(np.uint8)),
                                         _t(want["m2"][l].astype(np.uint8)), _t(U.astype(np.int32)), radius=r, damping=damping)
        assert np.array_equal(gu[0].cpu().numpy(), wu) and np.array_equal(gok[0].cpu().numpy(), wok), (l, r, damping)
        assert 0 < wok.mean() < 1


@pytest.fixture(scope="module")
def two_cases():
    return _pair(96, 128), _want(96, 128), _pair(40, 65), _want(40, 65)


def test_streams_and_workspace_history(two_cases):
    from stitch_amd import ops
    big, want_big, small, want_small = two_cases
    tb, ts = [_t(x) for x in big], [_t(x) for x in small]
    need = ops.dense_flow_workspace_bytes(1, 96, 128)
    assert need > ops.dense_flow_workspace_bytes(1, 40, 65) > 0 and need % 16 == 0
    ws1 = torch.full((need,), 255, dtype=torch.uint8).cuda()
    ws2 = torch.full((need,), 255, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):                                                     # two calls in flight in separate workspaces
        r1 = ops.dense_flow(*tb, workspace=ws1, return_fields=True)
    with torch.cuda.stream(s2):
        r2 = ops.dense_flow(*ts, workspace=ws2, return_fields=True)
    with torch.cuda.stream(s1):                                                     # the workspace just held the larger canvas
        r3 = ops.dense_flow(*ts, workspace=ws1, return_fields=True)
    s1.synchronize(), s2.synchronize()
    assert _same(r1, want_big) and _same(r2, want_small) and _same(r3, want_small)
    with pytest.raises(ops.StitchErrorBase):
        ops.dense_flow(*tb, workspace=ws1[:4096])
    with pytest.raises(ValueError):
        ops.dense_flow(*tb, radius=8)


def test_captured_into_a_graph_and_replayed_on_other_pixels(two_cases):
    from stitch_amd import ops
    big, want_big, _, _ = two_cases
    other = [np.ascontiguousarray(t[:, :, ::-1, ::-1]) for t in big]
    static = [_t(x) for x in big]
    ws = torch.empty(ops.dense_flow_workspace_bytes(1, 96, 128), dtype=torch.uint8).cuda()
    side_stream = torch.cuda.Stream()
    side_stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side_stream):
        ops.dense_flow(*static, workspace=ws)
    torch.cuda.current_stream().wait_stream(side_stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = ops.dense_flow(*static, workspace=ws)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(res[0].cpu().numpy(), want_big[0]) and np.array_equal(res[1].cpu().numpy(), want_big[1])
    for t, x in zip(static, other):
        t.copy_(torch.from_numpy(x))
    graph.replay()
    torch.cuda.synchronize()
    want = _want_items(*other)
    assert not np.array_equal(want[0], want_big[0])
    assert np.array_equal(res[0].cpu().numpy(), want[0]) and np.array_equal(res[1].cpu().numpy(), want[1])
    assert _same(ops.dense_flow(*static, return_fields=True), want)                  # eager on the same pixels


def test_every_operand_inside_a_frame_that_stays_intact():
    """the images and masks in sentinel frames; the outputs and a workspace of exactly st_dense_flow_workspace_bytes in sentinel frames"""
    from stitch_amd import ops
    from stitch_amd._lib import lib
    B, h, w, pad = 2, 33, 65, 64
    p1, p2 = _pair(h, w), _pair(h, w, 7)
    a, b, m1, m2 = (np.concatenate([p1[k], p2[k]]) for k in range(4))
    m2 = np.concatenate([m2, np.zeros((B, 2, h, w), np.float32)], 1)                # three channels
    want = _want_items(a, b, m1, m2, levels=3, iters=2, radius=7)
    need = ops.dense_flow_workspace_bytes(B, h, w, 3)
    L = ops.dense_flow_workspace_layout(B, h, w, 3)
    assert L["total"] == need and L["levels"] == 2

    def framed(count, dtype, fill, values=None):
        buf = torch.full((pad + count + pad,), fill, dtype=dtype, device="cuda")
        if values is not None:
            buf[pad:pad + count] = torch.from_numpy(np.ascontiguousarray(values).reshape(-1)).cuda()
        return buf
    ins = [framed(x.size, torch.float32, 90.0, x) for x in (a, b, m1, m2)]
    flow, sup, ws = framed(2 * B * h * w, torch.float32, -77.0), framed(B * h * w, torch.uint8, 0xA5), framed(need, torch.uint8, 0xA5)
    assert (ws.data_ptr() + pad) % 16 == 0
    ptr = lambda t: C.c_void_p(t.data_ptr() + pad * t.element_size())                # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.st_dense_flow(ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), 1, ptr(ins[3]), 3, B, h, w, 3, 2, 7, 65536, ptr(flow), ptr(sup), ptr(ws), need, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(flow[pad:pad + 2 * B * h * w].cpu().numpy().reshape(B, 2, h, w), want[0]) and want[0].any()
    assert np.array_equal(sup[pad:pad + B * h * w].cpu().numpy().reshape(B, 1, h, w), want[1])
    raw = ws[pad:pad + need].cpu().numpy()
    for l, (hl, wl) in enumerate(((33, 65), (17, 33))):
        assert np.array_equal(raw[L["u"][l]:L["u"][l] + 8 * B * hl * wl].view(np.int32).reshape(B, 2, hl, wl), want[2]["u"][l])
    for buf, x in zip(ins, (a, b, m1, m2)):
        assert np.array_equal(buf[pad:pad + x.size].cpu().numpy(), x.reshape(-1), equal_nan=True)
    for buf, count, fill in [(i, x.size, 90.0) for i, x in zip(ins, (a, b, m1, m2))] + [(flow, 2 * B * h * w, -77.0), (sup, B * h * w, 0xA5), (ws, need, 0xA5)]:
        assert (buf[:pad] == fill).all() and (buf[pad + count:] == fill).all()
