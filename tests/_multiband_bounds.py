"""A priori bound on |float32 restatement - float64 evaluation| of the multiband pyramid (tests/_multiband_ref.py), in grey levels,
from the number of fp32 roundings per output and the magnitude M = 255.  Nothing here is fitted to a run.

u = 2^-24 is the unit roundoff.  The inputs of the pyramid are integers 0..255 (weights 0 / 1), exact in both precisions.

REDUCE, one axis: 5 products and 4 sums, every partial result of magnitude <= X (the weights are positive and add up to 1), so at most
9 u X of new error; both axes: 18 u X.  The weights are a convex combination, so the error already in the input is not amplified.
    eG(l) <= 18 l u M  for the image pyramids,  eW(l) <= 18 l u  for the weight pyramid (magnitude 1).
EXPAND, one axis: at most 3 products and 2 sums (even sample), partials <= X: 5 u X; both axes 10 u X; convex again.
Laplacian  Lx_l = Gx_l - EXPAND(Gx_{l+1}):   |Lx| <= M,     eL(l) <= eG(l) + eG(l+1) + 10 u M + u M.
d = La - Lb:                                 |d| <= 2 M,    e(d) <= 2 eL + 2 u M.
p = Gw d:                                    |p| <= 2 M,    e(p) <= e(d) + eW(l) 2 M + 2 u M.
s = Lb + p:                                  |s| <= 3 M,    e(s) <= eL + e(p) + 3 u M.
top  R = Gb + Gw (Ga - Gb):  |Ga - Gb| <= M, |R| <= M:      eR(top) <= eG + (2 eG + u M) + eW M + u M + u M.
down R_l = EXPAND(R_{l+1}) + s:  |R_l| <= |R_{l+1}| + 3 M =: X(l);   eR(l) <= eR(l+1) + 10 u X(l+1) + e(s) + u X(l).
The final clamp to 0..255 does not increase a difference."""

U = 2.0 ** -24
M = 255.0


def pyramid_bound(levels):
    """bound for `levels` effective REDUCE steps (tests/_multiband_ref.effective_levels)"""
    def eG(l):
        return 18 * l * U * M

    def eW(l):
        return 18 * l * U
    L = levels
    eR = 3 * eG(L) + eW(L) * M + 3 * U * M
    X = M
    for l in range(L - 1, -1, -1):
        eL = eG(l) + eG(l + 1) + 11 * U * M
        ed = 2 * eL + 2 * U * M
        ep = ed + eW(l) * 2 * M + 2 * U * M
        es = eL + ep + 3 * U * M
        Xl = X + 3 * M
        eR = eR + 10 * U * X + es + U * Xl
        X = Xl
    return eR
