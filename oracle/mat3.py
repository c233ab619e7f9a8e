"""torch.inverse of a column-major 3x3 restated in numpy fp32, operation for operation (csrc/geom.hip: mat3_inv_cm; test infrastructure).
Pinned bit for bit against torch.inverse by tests/test_branches_cpu.py."""
import numpy as np

F32 = np.float32


def _fma(a, b, c):
    """fp32 fma: the product is exact in fp64; the fp64 sum then rounds twice, which differs from one rounding only when it lands
    on an fp32 tie -- not the case for any input below (the results are compared bit for bit)."""
    return F32(np.float64(a) * np.float64(b) + np.float64(c))


def _lu3(M):
    A = [[F32(M[i][j]) for j in range(3)] for i in range(3)]
    piv = [0, 0, 0]
    for k in range(3):
        p, best = k, abs(A[k][k])
        for i in range(k + 1, 3):
            if abs(A[i][k]) > best:
                p, best = i, abs(A[i][k])
        piv[k] = p
        A[k], A[p] = A[p], A[k]
        if k == 0:
            r = F32(F32(1) / A[0][0])
            A[1][0], A[2][0] = F32(A[1][0] * r), F32(A[2][0] * r)
        elif k == 1:
            A[2][1] = F32(A[2][1] / A[1][1])
        for i in range(k + 1, 3):
            for j in range(k + 1, 3):
                A[i][j] = _fma(-A[i][k], A[k][j], A[i][j])
    return A, piv


def inv3_column_major(M):
    """torch.inverse of a column-major 3x3: sgetrf(A) + sgetrs('N', I) in MKL's order (mat3_inv_cm)."""
    A, piv = _lu3(M)
    r = [F32(F32(1) / A[i][i]) for i in range(3)]
    X = np.zeros((3, 3), F32)
    for c in range(3):
        b = [F32(i == c) for i in range(3)]
        for k in range(3):
            b[k], b[piv[k]] = b[piv[k]], b[k]
        y0 = b[0]
        y1 = F32(b[1] - F32(A[1][0] * y0))
        y2 = F32(b[2] - F32(F32(A[2][0] * y0) + F32(A[2][1] * y1)))
        d = (lambda v, i: F32(v * r[i])) if c < 2 else (lambda v, i: F32(v / A[i][i]))
        x2 = d(y2, 2)
        x1 = d(_fma(-A[1][2], x2, y1), 1)
        x0 = d(F32(y0 - _fma(A[0][2], x2, F32(A[0][1] * x1))), 0)
        X[:, c] = (x0, x1, x2)
    return X
