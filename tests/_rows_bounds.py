"""fp64 references and first-order worst-case elementwise error bounds for the C = 128 row kernels of csrc/gemm_rows.hip and
csrc/mlp_split3.h (rowchain128_kernel, rowmlp128_kernel, rowmlp128_split3_kernel, rowlin128_split3_kernel, pe_tail_split3_kernel), the input
generators and the case lists that tests/test_rows_bounds_cpu.py and tests/test_rows_matrix_gpu.py share.  A reference states its operator
from the definition in include/stitch_gfx950.h (affine-free LayerNorm, folded weights, as the kernels see them) in torch fp64, on whatever
device its inputs live, and knows nothing of blocks, rounds or rings.  Every bound E is a sum of the roundings the kernel performs, each at
its worst, to first order in u = 2^-24; every count is read from the kernel text, none is fitted to an output.

A value travels through an operator as a pair (v, E): v the fp64 value, E >= 0 the bound of |computed - v| so far.  The steps:

product  y = x w^T over K             E_y = E_x |w|^T + u n S,   S = |x| |w|^T  (fp64; every partial sum of the chain is below it)
    fp32 kernels   n = K              v_mfma_f32_32x32x2_f32 is an fma chain, one rounding per k (test_gemm_f32_matrix_gpu.py).  No row kernel
                                      folds: rowmlp128_kernel sums fc2's `hidden` k in one chain, so n = hidden there.
    split3 kernels n = 6 K / 16 + 2   x == hi + mid + lo exactly; the dropped mid.lo, lo.mid, lo.lo are <= 2 u |x||w| together; six
                                      v_mfma_f32_32x32x16_bf16 per 16 k add exact products into the fp32 accumulator, one rounding each
                                      (tau of test_split3_matrix_gpu.py).  These kernels never fold either: fc2 runs 6 hidden / 16 MFMAs
                                      into one accumulator.
sum  y = a + b                        E_y = E_a + E_b + u |y|     bias, table, residual and aux adds, one rounding each, in the kernel's order
ReLU                                  E_y = E_x                   1-Lipschitz, exact
GELU  g(v) = v Phi(v)                 E_g = L E_v + |v| (e_y + u) + 2 u |g|,   L = 1.13 >= max |g'| = 1.1290 (at |v| = sqrt 2)
    both forms (st_gelu, ms3_gelu) evaluate y = erfc(s) / 2, s = |v| / sqrt 2, by Abramowitz-Stegun 7.1.26: t = 1 / (1 + p s),
    y = t (a1 + t (a2 + t (a3 + t (a4 + t a5)))) exp(-s^2) / 2, published |error| <= 1.5e-7 on erfc, i.e. 0.75e-7 on y.  Its evaluation:
        t      the product |v| c, the fma, v_rcp_f32 (1 ulp = 2 u) and the rounded constant: relative error <= 5 u, which moves the polynomial
               by <= 5 u D1(t), D1 = sum i |a_i| t^i
        Horner four fmas and the rounded coefficients: <= 5 u A(t), A = sum |a_i| t^i (the signs alternate: the partial sums are bounded by
               A, not by the value)
        exp2   its argument s^2 log2 e through three roundings (3 u s^2 log2 e relative to y), v_exp_f32 1 ulp = 2 u, the two products: 4 u
        e_y = 0.75e-7 + u exp(-s^2) (5 D1 + 5 A) / 2 + u y (4 + 3 s^2 log2 e)
    |v| u: the rounding of 1 - y (st_gelu, v >= 0);  2 u |g|: the product with v, or ms3_gelu's closing fma.
LayerNorm without affine  y = d r,  d = x - mu,  r = (sum d^2 / C + eps)^-1/2      (the formula of _nn_bounds.py with its chain counted here)
    dmu = u (n_m + 2) mean|x|
    E_y = r (dmu + u |d| + |d| (u (n_v + 6) + dmu sum|d| / (sum d^2 + C eps))) + u |y|
          + r Ed + |d| r sum(|d| Ed) / (sum d^2 + C eps),      Ed = E_x + mean E_x
    n_m = n_v = 19 in the four ring kernels: (x + y) + (z + w) is two roundings, a lane adds sixteen of these, one shuffle adds the lane halves
    (the product with 1 / 128 is exact).  pe_tail_split3_kernel sums its mean the same way (19) and its variance as 64 adds in a row + the shuffle: n_v = 65.
    The second line carries an input error through: d moves by E_x and by the mean's share, r by r^3 / C sum d dd = r sum d dd / (sum d^2 + C eps).
    On a constant row d = 0 and r = eps^-1/2: E = eps^-1/2 (dmu + Ed), the amplified rounding of the mean.  With affine (pe_tail):
    E_out = |gamma| E_y + 2 u |out| + u |y gamma|.

Operators (the order of the sums is the kernels'):
    chain     x_{l+1} = act(LN(x_l) w_l^T + b_l) + res_l, res_l none | a tensor | x_m (m <= l, before its LayerNorm)        fp32 products
    mlp       x = a  or  (a wp^T + bp) + res0;   out = ((GELU(LN(x) w1^T + b1) w2^T + b2) + x) + res                     fp32 or split3
    rowlin    out = (LN(a) w^T + b) + aux[row // row_div]                                                                  split3
    pe_tail   out = LN_affine(ReLU(x w1^T + tab[r % P]) w2^T + b2)                                                       split3, K = 64 then 128"""
import math

import torch

U = 2.0 ** -24
LOG2E = 1.44269504088896340736
LN_NS = 19
LN_NV_PE = 65
GELU_L = 1.13
AS_ERFC = 1.5e-7
AS_P = 0.3275911
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)

ROUND_A = 65536          # rows of one round: 512 workgroups x 4 waves x 32 rows (st_linear_chain128, st_mlp128, st_rowlin128_split3)
ROUND_B = 32768          # 256 workgroups (st_mlp128_split3, st_pe_tail_split3)
SMALL_ROWS = (1, 31, 32, 33, 127, 129)


def multi_rows(R):
    return (R, R + 33, 2 * R + 1)


def ratio(out, ref, E):
    """max |out - ref| / E; 0 / 0 = 0; an element that is NaN or wrong where E = 0 gives inf"""
    err = (out.double() - ref).abs()
    r = torch.where(E > 0, err / E.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")))
    r = r.max().item() if r.numel() else 0.0
    return float("inf") if math.isnan(r) else r


# ------------------------------------------------------------------------------------------------ the steps
def n_f32(K):
    return K


def n_s3(K):
    return 6 * K // 16 + 2


def lin(x, Ex, w, n):
    w = w.double()
    return x @ w.t(), Ex @ w.abs().t() + U * n * (x.abs() @ w.abs().t())


def add(y, Ey, t, Et=0.0):
    y = y + t
    return y, Ey + Et + U * y.abs()


def gelu(v, Ev):
    s = v.abs() / math.sqrt(2.0)
    y = 0.5 * torch.special.erfc(s)
    g = torch.where(v >= 0, v * (1.0 - y), v * y)
    t = 1.0 / (1.0 + AS_P * s)
    A = sum(abs(a) * t ** (i + 1) for i, a in enumerate(AS_A))
    D1 = sum((i + 1) * abs(a) * t ** (i + 1) for i, a in enumerate(AS_A))
    ey = 0.5 * AS_ERFC + U * torch.exp(-s * s) * (5 * D1 + 5 * A) / 2 + U * y * (4 + 3 * s * s * LOG2E)
    return g, GELU_L * Ev + v.abs() * (ey + U) + 2 * U * g.abs()


def ln(x, Ex, eps, n_m=LN_NS, n_v=LN_NS, gamma=None, beta=None):
    C = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    ad = d.abs()
    q = (d * d).sum(-1, keepdim=True) + C * eps
    r = torch.sqrt(C / q)
    y = d * r
    dmu = U * (n_m + 2) * x.abs().mean(-1, keepdim=True)
    Ed = Ex + Ex.mean(-1, keepdim=True)
    E = r * (dmu + U * ad + ad * (U * (n_v + 6) + dmu * ad.sum(-1, keepdim=True) / q)) + U * y.abs() + r * Ed + ad * r * (ad * Ed).sum(-1, keepdim=True) / q
    if gamma is not None:
        gamma, beta = gamma.double(), beta.double()
        out = y * gamma + beta
        return out, gamma.abs() * E + 2 * U * out.abs() + U * (y * gamma).abs()
    return y, E


def zeros_like_E(x):
    return torch.zeros_like(x, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ the operators: -> (ref, E), fp64
def chain_bound(a, layers):
    """layers: dicts w [128, 128], bias or None, act in none / relu / gelu, ln_eps or None, res: None | tensor [M, 128] | int m (x_m)"""
    x, Ex = a.double(), zeros_like_E(a)
    inputs = []
    for y in layers:
        inputs.append((x, Ex))
        v, Ev = ln(x, Ex, y["ln_eps"]) if y.get("ln_eps") is not None else (x, Ex)
        v, Ev = lin(v, Ev, y["w"], n_f32(128))
        v, Ev = add(v, Ev, y["bias"].double()) if y.get("bias") is not None else (v, Ev)            # (acc + 0 is exact)
        act = y.get("act", "none")
        if act == "gelu":
            v, Ev = gelu(v, Ev)
        elif act == "relu":
            v = v.clamp_min(0)
        r = y.get("res")
        if isinstance(r, int):
            v, Ev = add(v, Ev, *inputs[r])
        elif r is not None:
            v, Ev = add(v, Ev, r.double())
        x, Ex = v, Ev
    return x, Ex


def mlp_bound(a, w1, b1, w2, b2, ln_eps=None, res=None, proj=None, split3=False):
    """proj = (wp, bp or None, res0 or None)"""
    n = n_s3 if split3 else n_f32
    x, Ex = a.double(), zeros_like_E(a)
    if proj is not None:
        wp, bp, res0 = proj
        x, Ex = lin(x, Ex, wp, n(128))
        x, Ex = add(x, Ex, bp.double()) if bp is not None else (x, Ex)
        x, Ex = add(x, Ex, res0.double()) if res0 is not None else (x, Ex)
    v, Ev = ln(x, Ex, ln_eps) if ln_eps is not None else (x, Ex)
    v, Ev = lin(v, Ev, w1, n(128))
    v, Ev = gelu(*add(v, Ev, b1.double()))
    v, Ev = lin(v, Ev, w2, n(w1.shape[0]))
    v, Ev = add(v, Ev, b2.double())
    v, Ev = add(v, Ev, x, Ex)
    if res is not None:
        v, Ev = add(v, Ev, res.double())
    return v, Ev


def rowlin_bound(a, w, b=None, ln_eps=None, aux=None, row_div=1):
    x, Ex = a.double(), zeros_like_E(a)
    v, Ev = ln(x, Ex, ln_eps) if ln_eps is not None else (x, Ex)
    v, Ev = lin(v, Ev, w, n_s3(128))
    if b is not None:
        v, Ev = add(v, Ev, b.double())
    if aux is not None:
        idx = torch.arange(a.shape[0], device=a.device) // row_div
        v, Ev = add(v, Ev, aux.double()[idx])
    return v, Ev


def pe_tail_bound(x, w1, tab, w2, b2, gamma, beta, eps=1e-5):
    """x [R, 64], w1 [128, 64], tab [P, 128]"""
    x = x.double()
    rows = torch.arange(x.shape[0], device=x.device) % tab.shape[0]
    v, Ev = lin(x, zeros_like_E(x), w1, n_s3(64))
    v, Ev = add(v, Ev, tab.double()[rows])
    v = v.clamp_min(0)
    v, Ev = lin(v, Ev, w2, n_s3(128))
    v, Ev = add(v, Ev, b2.double())
    return ln(v, Ev, eps, LN_NS, LN_NV_PE, gamma, beta)


def chain_ref(a, layers):
    return chain_bound(a, layers)[0]


def mlp_ref(*a, **k):
    return mlp_bound(*a, **k)[0]


def rowlin_ref(*a, **k):
    return rowlin_bound(*a, **k)[0]


def pe_tail_ref(*a, **k):
    return pe_tail_bound(*a, **k)[0]


# ------------------------------------------------------------------------------------------------ inputs (fp32, CPU; the GPU tests move them)
def gen(seed):
    return torch.Generator().manual_seed(seed)


def rows(M, seed, C=128, scale=1.0, mean=0.0):
    return torch.randn(M, C, generator=gen(seed)) * scale + mean


def weight(N, K, seed):
    """scaled by fan-in"""
    return torch.randn(N, K, generator=gen(seed)) / K ** 0.5


def vec(N, seed, scale=0.1):
    return torch.randn(N, generator=gen(seed)) * scale


def table(P, seed, N=128):
    return torch.randn(P, N, generator=gen(seed)) * 0.5


def gamma_beta(seed, C=128):
    return torch.rand(C, generator=gen(seed)) + 0.5, torch.randn(C, generator=gen(seed + 1)) * 0.1


EDGE_KINDS = ("const", "mean1", "mean100", "zero", "onehot")


def edge_row(kind, C, seed):
    n = torch.randn(C, generator=gen(seed))
    if kind == "const":
        return torch.full((C,), 3.0)
    if kind == "mean1":
        return 1.0 + 1e-3 * n
    if kind == "mean100":
        return 100.0 + 1e-3 * n
    if kind == "zero":
        return torch.zeros(C)
    x = torch.zeros(C)
    x[int(seed) % C] = 1e3
    return x


def edge_positions(M):
    """rows 0, 31, 32 and M - 1 (first and last lane of a block, the clamp source of the padding lanes), then their neighbours: every kind once"""
    return [p for p in (0, 31, 32, M - 1, 1, 30, 33, M - 2) if 0 <= p < M]


def edge_rows(M, seed, C=128):
    """Gaussian rows with the LayerNorm edge rows at edge_positions(M), the kinds in turn; finite everywhere"""
    x = rows(M, seed, C)
    for i, p in enumerate(edge_positions(M)):
        x[p] = edge_row(EDGE_KINDS[i % len(EDGE_KINDS)], C, seed + 7 * i + 1)
    return x


# ------------------------------------------------------------------------------------------------ the cases both files walk
def fold(gamma, beta, w, b):
    """Linear(LayerNorm_affine(x)) -> the weights behind an affine-free LayerNorm (fp64 on the host, as ops.fold_layernorm)"""
    w64 = w.double()
    return (w64 * gamma.double()[None, :]).float(), (w64 @ beta.double() + (0 if b is None else b.double())).float()


def chain_layers(form, M, seed):
    """One chain form -> (layers, in_place): CPU fp32 tensors; the GPU file moves them and gives the tensor residual its own row stride"""
    W = lambda i: weight(128, 128, seed + 10 * i)                                   # noqa: E731
    B = lambda i: vec(128, seed + 10 * i + 1)                                       # noqa: E731
    L = lambda i, **k: dict(w=W(i), bias=B(i), **k)                                 # noqa: E731
    R = rows(M, seed + 5)
    forms = {
        "n1": [L(0)],
        "n2": [L(0), L(1)],
        "n3": [L(0), L(1), L(2)],
        "relu": [L(0, act="relu"), L(1)],
        "gelu": [L(0, act="gelu"), L(1, act="gelu")],
        "ln0": [L(0, ln_eps=1e-5), L(1)],
        "ln1": [L(0), L(1, ln_eps=1e-5), L(2)],
        "ln2": [L(0), L(1), L(2, ln_eps=1e-5)],
        "ln012": [L(0, ln_eps=1e-5, act="relu"), L(1, ln_eps=1e-6, act="gelu"), L(2, ln_eps=1e-5)],
        "nobias": [L(0), dict(w=W(1), bias=None, act="gelu"), L(2)],
        "res_tensor": [L(0, act="relu", res=R), L(1)],
        "res_l0_from_l2": [L(0, ln_eps=1e-5), L(1, act="gelu"), L(2, res=0)],
        "res_self": [L(0), L(1, ln_eps=1e-5, act="gelu", res=1)],
        "model_cross": [L(0, ln_eps=1e-5, act="gelu"), L(1, res=0)],                          # flowformer.py _latent_cross
        "model_self": [L(0, res=R), L(1, ln_eps=1e-5, act="gelu"), L(2, res=1)],              # flowformer.py _latent_self
    }
    return forms[form]


CHAIN_FORMS = ("n1", "n2", "n3", "relu", "gelu", "ln0", "ln1", "ln2", "ln012", "nobias", "res_tensor", "res_l0_from_l2", "res_self", "model_cross",
               "model_self")
CHAIN_MODEL_FORMS = ("model_cross", "model_self")
CHAIN_NLAYERS = dict(n1=1, n2=2, n3=3, relu=2, gelu=2, ln0=2, ln1=3, ln2=3, ln012=3, nobias=3, res_tensor=2, res_l0_from_l2=3, res_self=2,
                     model_cross=2, model_self=3)
CHAIN_ROWS = (33, ROUND_A + 33)

MLP_HIDDEN = (32, 64, 96, 128, 192, 512, 2048)
MLP_PROJ = ("none", "full", "bare")               # no projection | projection with bias and res0 | projection alone
# (hidden, with projection) at the multi-round row counts: steps per round 1, 2, 3, 4 and 2 + 4 = 6 -- every residue of the 3-stage ring of the split3
# kernel, odd and even for the 2-stage ring of the fp32 kernel, and the one-chunk pipeline (hidden 32)
MLP_MULTI = ((32, False), (64, False), (96, False), (128, False), (64, True))
ROWLIN_N = (32, 64, 96, 128, 384, 4096)
ROWLIN_MULTI_N = (32, 64, 96, 128)                 # steps per round 1, 2, 3, 4
ROWLIN_AUX = ("none", "div1", "div8", "div7_ld")   # div7_ld: row_div 7, ld_aux = N + 4
# (R, P): what each reaches is asserted by the grid replay of test_rows_bounds_cpu.py
PE_CASES = ((129, 64), (600, 3), (600, 7), (17, 257), (33, 1), (127, 5), (ROUND_B, 64), (ROUND_B + 33, 257), (ROUND_B + 33, 64), (2 * ROUND_B + 1, 5),
            (2 * ROUND_B + 1, 64))


def mlp_inputs(M, hidden, seed, edge=False):
    d = dict(a=edge_rows(M, seed) if edge else rows(M, seed, scale=1.5), w1=weight(hidden, 128, seed + 1), b1=vec(hidden, seed + 2),
             w2=weight(128, hidden, seed + 3), b2=vec(128, seed + 4), res=rows(M, seed + 5), wp=weight(128, 128, seed + 6), bp=vec(128, seed + 7),
             res0=rows(M, seed + 8))
    return d


def rowlin_inputs(M, N, seed, edge=False):
    return dict(a=edge_rows(M, seed) if edge else rows(M, seed, scale=1.5, mean=0.3), w=weight(N, 128, seed + 1), b=vec(N, seed + 2))


def pe_inputs(R, P, seed, edge=False):
    g, b = gamma_beta(seed + 6)
    return dict(x=edge_rows(R, seed, 64) if edge else rows(R, seed, 64), w1=weight(128, 128, seed + 1), tab=table(P, seed + 2), w2=weight(128, 128, seed + 3),
                b2=vec(128, seed + 4), gamma=g, beta=b)
