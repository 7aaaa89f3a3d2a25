"""Shared inputs and bounds of the correlation tests (test_corr_cpu.py, test_gpu_corr.py); no tests here."""
import functools
import math

import numpy as np

U = 2.0 ** -53   # unit roundoff of float64
F32 = np.float32


def exact_inputs(seed, N, F):
    """``(X float32 [N, F], mu float64 [F])``: integers in [-8, 8] with about 10% NaN and an integer centre, so every
    product and partial sum of the four tables is an exact double. Planted where the shape has room: +-inf (missing,
    like NaN), an all-missing column (the last, from F = 3 on) and a pair never jointly present (columns 0 and 1,
    from F = 2 and N = 2 on)."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-8, 9, size=(N, F)).astype(F32)
    X[rng.random((N, F)) < 0.10] = np.nan
    r = rng.random((N, F))
    X[r < 0.02] = np.inf
    X[(r >= 0.02) & (r < 0.04)] = -np.inf
    if F >= 2 and N >= 2:
        X[0::2, 0] = np.nan
        X[1::2, 1] = np.nan
    if F >= 3:
        X[:, F - 1] = np.nan
    mu = rng.integers(-3, 4, size=F).astype(np.float64)
    return X, mu


def general_inputs(seed, N, F):
    """``(X float32 [N, F], mu float64 [F])``: continuous columns at scales 1e-3 .. 1e3, column 0 near 1e4 with unit
    spread (loan amounts), column 1 correlated with it, about 10% NaN; mu is the float32-rounded mean of the present
    values."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.integers(-3, 4, size=F)
    X = rng.normal(size=(N, F)) * scale + rng.normal(size=F) * scale
    X[:, 0] = 1.0e4 + rng.normal(size=N)
    if F >= 2:
        X[:, 1] = 0.5 * (X[:, 0] - 1.0e4) + rng.normal(size=N)
    X = X.astype(F32)
    X[rng.random((N, F)) < 0.10] = np.nan
    fin = np.isfinite(X)
    cnt = fin.sum(axis=0)
    mu = np.where(fin, X, 0).astype(np.float64).sum(axis=0) / np.maximum(cnt, 1)
    return X, mu.astype(F32).astype(np.float64)


def moment_terms(X, mu):
    """The centred values and the masks as float64 ``[N, F]``: ``c`` (0 where missing) and ``m``."""
    fin = np.isfinite(X)
    c = np.where(fin, np.where(fin, X, 0).astype(np.float64) - np.asarray(mu, np.float64)[None, :], 0.0)
    return c, fin.astype(np.float64)


def moments_fsum(X, mu):
    """``(n, A, Q, P, A_abs, Q_abs, P_abs)``: every entry of the float tables as ``math.fsum`` of its terms (the
    correctly rounded sum), and the sums of the terms' absolute values, the scale of the bound."""
    c, m = moment_terms(X, mu)
    F = X.shape[1]
    n = np.rint(m.T @ m).astype(np.int64)
    A, Q, P = (np.zeros((F, F)) for _ in range(3))
    c2 = c * c
    for i in range(F):
        for j in range(F):
            A[i, j] = math.fsum((c[:, i] * m[:, j]).tolist())
            Q[i, j] = math.fsum((c2[:, i] * m[:, j]).tolist())
            if i <= j:
                P[i, j] = P[j, i] = math.fsum((c[:, i] * c[:, j]).tolist())
    ca = np.abs(c)
    return n, A, Q, P, ca.T @ m, c2.T @ m, ca.T @ ca   # the scales need no more than float64's own accuracy


def moment_bound(N, abs_sum):
    """``(N + 64) 2^-53 sum |t_i|``: N u is the bound of a sum of N terms added in any order, 64 the allowance for
    the roundings of a term (the square, the product) and of its reference."""
    return (N + 64) * U * abs_sum


@functools.lru_cache(maxsize=None)
def lending_like_nan(n=5000, seed=0):
    """``(X float32 [n, 8], names)``: ``scorecard_cases.lending_like`` columns (one with NaN, a 0/1 dummy, a
    constant) plus a loan amount near 1e4 and an instalment that follows it (r about 0.95), with more NaN planted."""
    from scorecard_cases import lending_like

    X6, _ = lending_like(n, seed)
    rng = np.random.default_rng(seed + 1)
    amnt = (1.0e4 + 3.0e3 * rng.normal(size=n)).astype(F32)
    inst = (amnt / 36.0 * (1.0 + 0.1 * rng.normal(size=n))).astype(F32)
    X = np.concatenate([X6, amnt[:, None], inst[:, None]], axis=1).astype(F32)
    X[rng.random(n) < 0.15, 0] = np.nan
    X[rng.random(n) < 0.05, 7] = np.nan
    X.setflags(write=False)
    return X, ["a", "b", "c_nan", "d", "dummy", "const", "loan_amnt", "installment"]
