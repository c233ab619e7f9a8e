"""Per-stage gate of the flow network against fp64, at the shapes the product runs (bench.py / evaluate.py: a 512 x 512 pair).

Each HIP stage of FlowFormer++ is traced inside one real forward (``flow_rows_pair`` / ``flow_rows`` with ``trace=``).  Stage k's HIP input
(an fp32 tensor from the same trace) is fed to the oracle's stage (oracle/nets.py) twice: in fp32 (``o32``, the reference's arithmetic)
and in fp64 (``o64``, weights of ``damped_state_dict`` cast to double).  So every stage is judged on its own, on real activations, against
the exact answer of the inputs it was given, whatever happened upstream.  With Y64 = o64:

    e_rms(X) = |X - Y64|_2 / |Y64|_2        e_max(X) = max|X - Y64| / max|Y64|

Bounds (fixed multiples of a control measured in the same run; none is derived from a HIP measurement):
  (a) both builds:  e_rms(HIP) <= 2 x max(e_rms(o32), 2^-24),  e_max(HIP) <= 4 x max(e_max(o32), 2^-24);
  (b) per stage:    e_rms(split3 build) <= 1.25 x e_rms(all-fp32 build)  (the operator tests' criterion, tests/test_split3_gpu.py);
  (c) a stage whose kernel and weights are the same in both builds gives the same bits when fed the other build's input.
Both builds live in one process: the module global ``flowformer.SPLIT3`` is read at pack and at state-allocation time only.

Where a stage's rows are independent the oracle runs on a seeded sample of them that holds the first and last rows and both rows of every
64-row (hence every 128-row) tile boundary; the HIP stage always runs at full size.  The ``_update_block`` plane images of the split3 build
are also checked bit for bit against their fp32 twins after iterations 1 and 7 (every channel the next iteration reads)."""
import time

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _measure import check  # noqa: E402

from oracle import nets, spec  # noqa: E402

FLOOR = 2.0 ** -24
PREFIX = "flow_backbone."
ITERS_GATED = (1, 7)             # iteration 1: coords1 is the integer grid (degenerate bilinear weights); 7: fractional coords, evolved state
SHAPES = {"512pair": (512, 512, True), "512single": (512, 512, False), "480x512pair": (480, 512, True)}


def unpack(planes):
    """Planes -> fp64 [rows, ncols] = hi + mid + lo (exact in fp64)"""
    t = planes.t[:, planes.c0 // 32:(planes.c0 + planes.ncols + 31) // 32].double().sum(0)
    return t.permute(1, 0, 2).reshape(planes.rows, -1)[:, :planes.ncols]


# ---------------------------------------------------------------------------------------------------- both builds, one traced forward each
@pytest.fixture(scope="module")
def sd():
    return spec.damped_state_dict(1234)


@pytest.fixture(scope="module")
def W(sd):
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    return nets.W(sd, PREFIX), nets.W(sd64, PREFIX)


class Build:
    """one FlowFormer instance packed and run under a given value of flowformer.SPLIT3"""

    def __init__(self, sd, split3):
        import stitch_amd
        from stitch_amd import flowformer
        self.ff, self.split3 = flowformer, split3
        m = flowformer.FlowFormer()
        m.load_state_dict({k[len(PREFIX):]: v for k, v in sd.items() if k.startswith(PREFIX)}, strict=True)
        self.m = m.cuda().eval()
        self.ops = stitch_amd.ops
        with self:
            self.m.pack()

    def __enter__(self):
        self._saved = self.ff.SPLIT3
        self.ff.SPLIT3 = self.split3
        return self

    def __exit__(self, *a):
        self.ff.SPLIT3 = self._saved


@pytest.fixture(scope="module")
def builds(sd):
    from stitch_amd import flowformer
    assert flowformer.SPLIT3, "the shipped build is the split3 one (ST_SPLIT3 unset)"
    return {"s3": Build(sd, True), "fp32": Build(sd, False)}


_TRACES = {}


def traced(builds, name, shape):
    key = (name, shape)
    if key not in _TRACES:
        from stitch_amd import data
        H, Wd, pair = SHAPES[shape]
        a, b = data.structured_pair(H, Wd, seed=7)
        tr = []
        with builds[name] as bd, torch.no_grad():
            fn = bd.m.flow_rows_pair if pair else bd.m.flow_rows
            _, _, (B, H1, W1) = fn(a.cuda(), b.cuda(), trace=tr)
        torch.cuda.synchronize()
        assert len(tr) == 1 + 12
        assert (tr[1]["planes"] is not None) if name == "s3" else ("planes" not in tr[1])
        _TRACES[key] = dict(tr=tr, B=B, H1=H1, W1=W1, pair=pair)
    return _TRACES[key]


# ---------------------------------------------------------------------------------------------------- oracle in fp32 and fp64
def oracle(fn, W, *args):
    """fn(w, *args) with the reference's fp32 arithmetic and in fp64 (args cast exactly; the default dtype makes the oracle's own
    constants -- linspace / coords_grid -- fp64 too)"""
    w32, w64 = W
    with torch.no_grad():
        o32 = fn(w32, *[a.float() if torch.is_tensor(a) and a.is_floating_point() else a for a in args])
        torch.set_default_dtype(torch.float64)
        try:
            o64 = fn(w64, *[a.double() if torch.is_tensor(a) and a.is_floating_point() else a for a in args])
        finally:
            torch.set_default_dtype(torch.float32)
    return o32, o64


def errs(x, y64):
    x, y64 = x.detach().cpu().double().reshape(-1), y64.detach().cpu().double().reshape(-1)
    assert x.shape == y64.shape and bool(torch.isfinite(x).all())
    if not bool(y64.any()):                      # an exactly zero answer (the flow of iteration 1): only an exact zero is right
        e = 0.0 if not bool(x.any()) else float("inf")
        return e, e
    return ((x - y64).norm() / y64.norm()).item(), ((x - y64).abs().max() / y64.abs().max()).item()


def sample_units(n, rows_per_unit, seed, extra=(), k=48):
    """unit indices (a pixel, a cost map, ...): first, last, the units holding both rows of every 64-row tile boundary, `extra`, and k seeded
    random ones"""
    s = {0, n - 1, *extra}
    for r in range(64, n * rows_per_unit, 64):
        s.update({(r - 1) // rows_per_unit, r // rows_per_unit})
    s.update(torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:k].tolist())
    return torch.tensor(sorted(u for u in s if 0 <= u < n))


def nchw(rows, B, H, W):
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def grid(B, H1, W1):
    ys, xs = torch.meshgrid(torch.arange(H1), torch.arange(W1), indexing="ij")
    return torch.stack([xs, ys], -1).reshape(1, H1 * W1, 2).expand(B, -1, -1).reshape(B * H1 * W1, 2).double()


# ---------------------------------------------------------------------------------------------------- the stages
def twins_stages(rec_list, w, img, B, prefix):
    """(stage name, hip output, o32, o64) of the LSA / PEG / GSA blocks of both Twins stages for image `img` (images are independent)"""
    out = []
    dims, heads, srs = (128, 256), (4, 8), (8, 4)
    for s, r in enumerate(rec_list):
        H, Wd, C = r["H"], r["W"], dims[s]
        N = H * Wd
        sl = slice(img * N, (img + 1) * N)
        tw = lambda ww: ww.sub(prefix)                                                   # noqa: E731

        def lsa(ww, x):
            b0 = tw(ww).sub(f"blocks.{s}.0.")
            x = x + nets._lsa(b0.sub("attn."), nets.lnorm(b0, "norm1", x, 1e-6), (H, Wd), heads[s])
            return x + nets.mlp(b0, "mlp", nets.lnorm(b0, "norm2", x, 1e-6))

        def peg(ww, x):
            t = x.transpose(1, 2).reshape(1, C, H, Wd)
            t = nets.conv(tw(ww), f"pos_block.{s}.proj.0", t, padding=1, groups=C) + t
            return t.flatten(2).transpose(1, 2)

        def gsa(ww, x):
            b1 = tw(ww).sub(f"blocks.{s}.1.")
            x = x + nets._gsa(b1.sub("attn."), nets.lnorm(b1, "norm1", x, 1e-6), (H, Wd), heads[s], srs[s])
            return x + nets.mlp(b1, "mlp", nets.lnorm(b1, "norm2", x, 1e-6))

        for name, fn, src, dst in (("lsa", lsa, "pe", "lsa"), ("peg", peg, "lsa", "peg"), ("gsa", gsa, "peg", "gsa")):
            x = r[src][sl].cpu().view(1, N, C)
            o32, o64 = oracle(fn, w, x)
            out.append((f"{name}{s + 1}", r[dst][sl].view(1, N, C), o32, o64))
    return out


def encoder_stages(T, w, seed):
    tr0, B, H1, W1 = T["tr"][0], T["B"], T["H1"], T["W1"]
    e = tr0["encoder"]
    M, N = B * H1 * W1, H1 * W1
    cpe = lambda ww: ww.sub("memory_encoder.cost_perceiver_encoder.")                  # noqa: E731
    out = []
    # all-pairs volume: rows sampled; the pair shape writes the forward volume and its transpose (the reverse direction) from one product
    f = tr0["feats"].cpu()                                                               # [2, B', N, 256]
    rows = sample_units(N, 1, seed)
    Bp = f.shape[1]
    for d in range(2 if T["pair"] else 1):
        for b in range(Bp):
            fa, fb = (f[0, b], f[1, b]) if d == 0 else (f[1, b], f[0, b])
            o32, o64 = oracle(lambda ww, x, y: x @ y.t(), w, fa[rows], fb)
            out.append((f"corr_volume{'_rev' if d else ''}", tr0["cost_maps"][(d * Bp + b) * N + rows.cuda()], o32, o64))
    # PatchEmbed: cost maps sampled
    maps = sample_units(M, 64, seed + 1, k=24)
    cm = tr0["cost_maps"][maps.cuda()].cpu().view(-1, 1, H1, W1)
    o32, o64 = oracle(lambda ww, x: nets.patch_embed(cpe(ww).sub("patch_embed."), x)[0], w, cm)
    P = o64.shape[1]
    out.append(("patch_embed", e["tokens"].view(M, P, 128)[maps.cuda()], o32, o64))
    # latent layers: pixels sampled (8 rows each)
    px = sample_units(M, 8, seed + 2, k=48)
    tok = e["tokens"].view(M, P, 128)[px.cuda()].cpu()
    o32, o64 = oracle(lambda ww, t: nets.latent_cross_attn(cpe(ww).sub("input_layer."), cpe(ww)("latent_tokens"), t), w, tok)
    out.append(("latent_in", e["latent_in"].view(M, 8, 128)[px.cuda()], o32, o64))
    ctx = nchw(tr0["context"].cpu(), B, H1, W1)
    short = e["latent_in"].view(B, N, 8, 128).permute(0, 2, 1, 3).cpu()
    for i in range(3):
        src = e["latent_in"] if i == 0 else e["vert"][i - 1]
        x = src.view(M, 8, 128)[px.cuda()].cpu()
        o32, o64 = oracle(lambda ww, t: nets.latent_self_attn(cpe(ww).sub(f"encoder_layers.{i}."), t), w, x)
        out.append((f"latent_self{i}", e["self"][i].view(M, 8, 128)[px.cuda()], o32, o64))
        # vertical layer: the whole tensor of every batch item (rows (latent, pixel) of one item attend to each other)
        for b in range(B):
            xv = e["self"][i].view(B, N, 8, 128)[b].permute(1, 0, 2).cpu()              # [8 latents, N, 128]

            def vert(ww, t, c, r):
                y = nets.vert_layer(cpe(ww).sub(f"vertical_encoder_layers.{i}."), t, (H1, W1), c)
                return y + r if i == 2 else y                                            # cost_encoder_res: + short-cut after the last one
            o32, o64 = oracle(vert, w, xv, ctx[b:b + 1], short[b])
            out.append((f"vertical{i}", e["vert"][i].view(B, N, 8, 128)[b].permute(1, 0, 2), o32, o64))
    return out


def prologue_stages(T, w, seed):
    tr0, B, H1, W1 = T["tr"][0], T["B"], T["H1"], T["W1"]
    pr = tr0["prologue"]
    N = H1 * W1
    dec = lambda ww: ww.sub("memory_decoder.")                                          # noqa: E731
    out = []
    ctx = nchw(tr0["context"].cpu(), B, H1, W1)
    o32, o64 = oracle(lambda ww, c: torch.tanh(nets.conv(dec(ww), "proj", c)[:, :128]), w, ctx)
    out.append(("proj_net", nchw(pr["net"], B, H1, W1), o32, o64))
    o32, o64 = oracle(lambda ww, c: F.relu(nets.conv(dec(ww), "proj", c)[:, 128:]), w, ctx)
    out.append(("proj_inp", nchw(pr["inp"], B, H1, W1), o32, o64))
    inp = nchw(pr["inp"].cpu(), B, H1, W1)
    for sfx, pad in (("1", (0, 2)), ("2", (2, 0))):
        def tab(ww, x):
            g = dec(ww).sub("update_block.gru.")
            return torch.cat([F.conv2d(x, g(f"conv{k}{sfx}.weight")[:, 128:256], g(f"conv{k}{sfx}.bias"), padding=pad) for k in "zrq"], 1)
        o32, o64 = oracle(tab, w, inp)
        out.append((f"gru_table{sfx}", nchw(pr["gru_tab"][sfx], B, H1, W1), o32, o64))
    rows = sample_units(N, 1, seed + 3, k=32)

    def attn_rows(ww, x):
        qk = nets.conv(dec(ww).sub("att."), "to_qk", x)
        q = qk[:, :128].reshape(B, 128, -1).transpose(1, 2)[:, rows] * (128 ** -0.5)
        return torch.softmax(torch.matmul(q, qk[:, 128:].reshape(B, 128, -1)), -1)
    o32, o64 = oracle(attn_rows, w, inp)
    out.append(("gma_attention", pr["attn"][:, rows.cuda()], o32, o64))
    px = sample_units(B * N, 8, seed + 4, k=48)
    mem = tr0["mem"].view(B * N, 8, 128)[px.cuda()].cpu()
    ca = lambda ww: dec(ww).sub("decoder_layer.cross_attend.")                           # noqa: E731
    o32, o64 = oracle(lambda ww, m: torch.cat([nets.linear(ca(ww), "k", m), nets.linear(ca(ww), "v", m)], -1), w, mem)
    out.append(("memory_kv", pr["kv"].view(B * N, 8, 128)[px.cuda()], o32, o64))
    return out


def iteration_stages(T, w, it, seed):
    """the 9x9 lookup, the token chain and every sub-stage of the update block of iteration `it` (1-based), each from its HIP input"""
    tr, B, H1, W1 = T["tr"], T["B"], T["H1"], T["W1"]
    N, R = H1 * W1, B * H1 * W1
    r, pr = tr[it], tr[0]["prologue"]
    dec = lambda ww: ww.sub("memory_decoder.")                                          # noqa: E731
    ub = lambda ww: dec(ww).sub("update_block.")                                        # noqa: E731
    out = []
    g0 = grid(B, H1, W1)
    coords_in = r["coords_in"].cpu()
    # 9x9 lookup and the token chain, pixels sampled
    px = sample_units(R, 1, seed + 10 * it, k=48)
    cm = tr[0]["cost_maps"][px.cuda()].cpu().view(-1, 1, H1, W1)
    c_s = coords_in[px].view(-1, 2, 1, 1)
    o32, o64 = oracle(lambda ww, m, c: nets.cost_lookup(m, c).reshape(-1, 81), w, cm, c_s)
    out.append(("cost_lookup", r["corr"][px.cuda(), :81], o32, o64))

    def chain(ww, cf, c, kv):
        qy = nets.conv(dec(ww), "flow_token_encoder.2", F.gelu(nets.conv(dec(ww), "flow_token_encoder.0", cf.view(-1, 81, 1, 1))))
        qy = qy.reshape(-1, 1, qy.shape[1])
        return nets.decoder_cross_attn(dec(ww).sub("decoder_layer.cross_attend."), qy, kv[..., :64], kv[..., 64:], c).reshape(-1, 64)
    o32, o64 = oracle(chain, w, r["corr"][px.cuda(), :81].cpu(), c_s, pr["kv"].view(R, 8, 128)[px.cuda()].cpu())
    out.append(("token_chain", r["corr"][px.cuda(), 84:148], o32, o64))
    # the update block, full tensors
    corr = r["corr"].cpu()
    corr_nchw = nchw(torch.cat([corr[:, 84:148], corr[:, :81]], 1), B, H1, W1)
    o32, o64 = oracle(lambda ww, x: F.relu(nets.conv(ub(ww).sub("encoder."), "convc1", x)), w, corr_nchw)
    out.append(("convc1", nchw(r["cor1"], B, H1, W1), o32, o64))
    flow = nchw(coords_in.double() - g0, B, H1, W1)                                       # exact: small integers subtracted from fp32
    out.append(("flow", nchw(r["flow"], B, H1, W1), flow.float(), flow))
    o32, o64 = oracle(lambda ww, x: F.relu(nets.conv(ub(ww).sub("encoder."), "convf1", x, padding=3)), w, flow)
    out.append(("flow_encoder", nchw(r["flo1"], B, H1, W1), o32, o64))
    cf = unpack(r["corflo_p"]) if "corflo_p" in r else r["corflo"]
    o32, o64 = oracle(lambda ww, a, b: torch.cat([F.relu(nets.conv(ub(ww).sub("encoder."), "convc2", a, padding=1)),
                                                   F.relu(nets.conv(ub(ww).sub("encoder."), "convf2", b, padding=1))], 1),
                      w, nchw(r["cor1"].cpu(), B, H1, W1), nchw(r["flo1"].cpu(), B, H1, W1))
    out.append(("convc2_convf2", nchw(cf, B, H1, W1), o32, o64))
    o32, o64 = oracle(lambda ww, x: F.relu(nets.conv(ub(ww).sub("encoder."), "conv", x, padding=1)), w, nchw(cf.float().cpu(), B, H1, W1))
    out.append(("conv", nchw(r["motion"], B, H1, W1), o32, o64))
    mf = nchw(torch.cat([r["motion"], r["flow"]], 1).cpu(), B, H1, W1)
    o32, o64 = oracle(lambda ww, a, m: nets.gma_aggregate(ub(ww).sub("aggregator."), a, m), w, pr["attn"].cpu(), mf)
    out.append(("gma_aggregate", nchw(r["aggregate"], B, H1, W1), o32, o64))
    x_gru = torch.cat([nchw(pr["inp"].cpu(), B, H1, W1), mf, nchw(r["aggregate"].cpu(), B, H1, W1)], 1)
    o32, o64 = oracle(lambda ww, h, x: nets.sepconv_gru(ub(ww).sub("gru."), h, x), w, nchw(r["net_in"].cpu(), B, H1, W1), x_gru)
    out.append(("sepconv_gru", nchw(r["gru"], B, H1, W1), o32, o64))
    o32, o64 = oracle(lambda ww, h: F.relu(nets.conv(ub(ww), "flow_head.conv1", h, padding=1)), w, nchw(r["gru"].cpu(), B, H1, W1))
    out.append(("flow_head1", nchw(r["fh"], B, H1, W1), o32, o64))
    # flow head conv2 + the coordinate update in its epilogue (decoder.py:329, an fp32 add in the reference too), compared as the increment
    # it made to coords1.  The exact answer is the exact increment rounded by that same fp32 add: against the unrounded one, the add's own
    # rounding (~ulp(coords) / 2, 3e-5 of the increment) would hide any error of the convolution.
    ci = nchw(coords_in, B, H1, W1)
    d32, d64 = oracle(lambda ww, f: nets.conv(ub(ww), "flow_head.conv2", f, padding=1), w, nchw(r["fh"].cpu(), B, H1, W1))
    y64 = (ci.double() + d64).float().double() - ci.double()
    out.append(("flow_head2", nchw(r["coords_out"].cpu().double() - coords_in.double(), B, H1, W1), (ci + d32).double() - ci.double(), y64))
    return out


def final_stages(T, w):
    tr, B, H1, W1 = T["tr"], T["B"], T["H1"], T["W1"]
    r = tr[-1]
    ub = lambda ww: ww.sub("memory_decoder.update_block.")                              # noqa: E731
    out = []
    o32, o64 = oracle(lambda ww, h: F.relu(nets.conv(ub(ww), "mask.0", h, padding=1)), w, nchw(r["gru"].cpu(), B, H1, W1))
    out.append(("mask_head1", nchw(r["mask_hidden"], B, H1, W1), o32, o64))
    o32, o64 = oracle(lambda ww, h: 0.25 * nets.conv(ub(ww), "mask.2", h), w, nchw(r["mask_hidden"].cpu(), B, H1, W1))
    out.append(("mask_head2", nchw(r["mask"], B, H1, W1), o32, o64))
    flow = nchw(r["coords_out"].cpu().double() - grid(B, H1, W1), B, H1, W1)
    o32, o64 = oracle(lambda ww, f, m: nets.convex_upsample(f, m), w, flow, nchw(r["mask"].cpu(), B, H1, W1))
    out.append(("convex_upsample", r["flow_up"], o32, o64))
    return out


def all_stages(T, w, seed=0):
    tr0, B = T["tr"][0], T["B"]
    out = []
    for net, img in (("cnet", 0), ("fnet", tr0["feats"].shape[0] * tr0["feats"].shape[1] - 1)):
        prefix = "context_encoder.svt." if net == "cnet" else "memory_encoder.feat_encoder.svt."
        out += [(f"{net}_{n}", h, a, b) for n, h, a, b in twins_stages(tr0[net], w, img, B, prefix)]
    out += encoder_stages(T, w, seed)
    out += prologue_stages(T, w, seed)
    for it in ITERS_GATED:
        out += [(f"it{it}_{n}", h, a, b) for n, h, a, b in iteration_stages(T, w, it, seed)]
    out += final_stages(T, w)
    # several entries of one stage (batch items, directions) are one measurement: pooled into one error pair
    pooled = {}
    for name, h, o32, o64 in out:
        pooled.setdefault(name, []).append((h.detach().cpu().double().reshape(-1), o32.double().reshape(-1), o64.double().reshape(-1)))
    return {n: tuple(torch.cat([p[i] for p in v]) for i in range(3)) for n, v in pooled.items()}


def gate(results, shape):
    """results[build][stage] = (hip, o32, o64) -> bounds (a) and (b); every value goes through check() (parity_measured.json)"""
    fails, table = [], []
    ratio = {}
    for bname, stages in results.items():
        for st, (h, o32, o64) in stages.items():
            eh, eo = errs(h, o64), errs(o32, o64)
            ratio[(bname, st)] = (eh[0], max(eo[0], FLOOR))
            for k, which in ((0, "rms"), (1, "max")):
                mult = 2.0 if which == "rms" else 4.0
                try:
                    check(f"stage64_{st}_{bname}_{shape}_{which}", eh[k], mult * max(eo[k], FLOOR), inclusive=True,
                          note=f"{mult:g} x e_{which}(o32) = {eo[k]:.3g} (fp32 reference arithmetic vs fp64, same inputs)")
                except AssertionError as e:
                    fails.append(str(e))
            table.append((st, bname, eh[0], eo[0], eh[1], eo[1]))
    if "s3" in results and "fp32" in results:
        for st in results["s3"]:
            if st.endswith("flow_head2"):
                # both builds run this stage on the same fp32 kernel, and what it is judged by is the handful of pixels (tens of 16 384)
                # where the fp32 coordinate add rounds the other way: a count that small has no 1.25x resolution between two inputs
                continue
            try:
                check(f"stage64_{st}_s3_over_fp32_{shape}_rms", ratio[("s3", st)][0], 1.25 * max(ratio[("fp32", st)][0], FLOOR), inclusive=True,
                      note="1.25 x e_rms of the all-fp32 build at the same stage")
            except AssertionError as e:
                fails.append(str(e))
    print(f"\n# stage gate {shape}: e_rms / e_max of HIP and of the fp32 oracle against fp64 (same inputs)")
    print(f"# {'stage':28s} {'build':5s} {'rms hip':>10s} {'rms o32':>10s} {'hip/o32':>8s} {'max hip':>10s} {'max o32':>10s}")
    for st, bname, rh, ro, mh, mo in sorted(table):
        print(f"  {st:28s} {bname:5s} {rh:10.3e} {ro:10.3e} {rh / max(ro, FLOOR):8.3f} {mh:10.3e} {mo:10.3e}")
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("shape", list(SHAPES))
def test_stage_gate(builds, W, shape):
    t0 = time.time()
    results = {}
    for bname in ("s3", "fp32"):
        T = traced(builds, bname, shape)
        results[bname] = all_stages(T, W)
        if shape != "512pair":                   # the 512 pair is reused by the coherence / same-bits tests below
            _TRACES.pop((bname, shape))
    print(f"\n# {shape}: traced forwards + oracle in {time.time() - t0:.1f} s")
    gate(results, shape)


def test_stage_gate_patch_embed_three_pairs(builds, W):
    """PatchEmbed alone over 3 pairs' cost maps (M = 24 576): the split3 launch loops over chunks of 16 384 maps, the second one ragged"""
    T = traced(builds, "s3", "512pair")
    cm0 = T["tr"][0]["cost_maps"]
    H1, W1 = T["H1"], T["W1"]
    cm = torch.cat([cm0, cm0.flip(0), cm0.roll(1, 1)]).contiguous()            # real cost maps, a different map on each side of every seam
    M = cm.shape[0]
    assert M == 24576
    maps = sample_units(M, 64, 5, extra=(16383, 16384, 8191, 8192), k=24)
    o32, o64 = oracle(lambda ww, x: nets.patch_embed(ww.sub("memory_encoder.cost_perceiver_encoder.patch_embed."), x)[0], W,
                      cm[maps.cuda()].cpu().view(-1, 1, H1, W1))
    results = {}
    for bname in ("s3", "fp32"):
        with builds[bname] as bd, torch.no_grad():
            tok, P = bd.m._patch_embed(cm, M, H1, W1)
        results[bname] = {"patch_embed": (tok.view(M, P, 128)[maps.cuda()].cpu().double().reshape(-1), o32.double().reshape(-1),
                                          o64.double().reshape(-1))}
    gate(results, "3pairs")


@pytest.mark.parametrize("it", ITERS_GATED)
def test_plane_coherence(builds, it):
    """split3 build, 512 pair: after iteration `it` every plane image the next iteration reads equals its fp32 twin bit for bit"""
    r = traced(builds, "s3", "512pair")["tr"][it]
    p = r["planes"]
    hxA = r["hxA"].double()
    assert p["hxA_p"].ncols == 384
    got = unpack(p["hxA_p"])
    bad = {f"{what} (channels {c0}-{c1 - 1})": (got[:, c0:c1] != hxA[:, c0:c1]).sum().item()
           for c0, c1, what in ((0, 128, "net"), (128, 254, "motion"), (254, 256, "flow"), (256, 384, "aggregate"))}
    assert not any(bad.values()), f"hxA planes: values that differ from the fp32 tensor, per channel group: {bad}"
    assert torch.equal(unpack(p["cor1_p"]), r["cor1"].double()), "cor1 planes differ from cor1"
    assert torch.equal(unpack(p["flo1_p"]), r["flo1"].double()), "flo1 planes differ from flo1"
    # corflo exists only as planes in this build (no_f32): its fp32 twin is the unpack the conv stage is gated on; the copy taken when the
    # iteration ended must still be the one `conv` read
    assert torch.equal(unpack(p["corflo_p"]), unpack(r["corflo_p"]))


def test_same_bits_in_both_builds(builds):
    """the lookup, the token chain, the GMA attention and the upsampling are the same kernels with the same weights in both builds: fed the
    split3 build's input, the all-fp32 build gives the split3 build's bits"""
    T = traced(builds, "s3", "512pair")
    tr, B, H1, W1 = T["tr"], T["B"], T["H1"], T["W1"]
    R, N = B * H1 * W1, H1 * W1
    bd = builds["fp32"]
    ops, pk = bd.ops, bd.m._pk
    with bd, torch.no_grad():
        for it in ITERS_GATED:
            r = tr[it]
            corr = torch.zeros(R, 160, device="cuda")
            ops.cost_lookup9x9(tr[0]["cost_maps"], r["coords_in"].clone(), corr, R, H1, W1)
            assert torch.equal(corr[:, :81], r["corr"][:, :81]), f"cost_lookup9x9, iteration {it}"
            ops.decoder_token_chain(corr, r["coords_in"].clone(), tr[0]["prologue"]["kv"], pk["dec"]["chain16"], R, 8)
            assert torch.equal(corr[:, 84:148], r["corr"][:, 84:148]), f"decoder_token_chain, iteration {it}"
        qk, attn = torch.empty(R, 256, device="cuda"), torch.empty(B, N, N, device="cuda")
        ops.gma_attention(tr[0]["prologue"]["inp"], pk["dec"]["qk"], qk, attn, B, N)
        assert torch.equal(attn, tr[0]["prologue"]["attn"]), "gma_attention"
        up = torch.empty(B, 2, 8 * H1, 8 * W1, device="cuda")
        ops.convex_upsample(tr[-1]["coords_out"].clone(), tr[-1]["mask"], up, B, H1, W1)
        assert torch.equal(up, tr[-1]["flow_up"]), "convex_upsample"
