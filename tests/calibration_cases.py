"""Inputs shared by test_calibration_cpu.py (the host definitions against brute force and sklearn) and
test_gpu_calibration.py (the kernels against the host definitions). NumPy only; nothing here calls the code
under test except ``iso_groups`` for the row-level cases, which the CPU file checks on its own.

A hull case is a pair ``(cw, cs)`` of int64 cumulative arrays (``cw[0] = cs[0] = 0``, ``cw`` strictly increasing):
the input of ``iso_hull_host`` / ``iso_hull_tiled_host`` / ``ops.calib_ops.iso_hull``.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

PATTERNS = ("random", "all0", "all1", "sorted", "antisorted", "ties", "long_block")
MAX_TOTAL = (1 << 31) - 1


def smooth_rows(n: int, seed: int = 0):
    """Scores from a normal and labels from the logistic model on them: the smooth case."""
    rng = np.random.default_rng(seed + 7919 * n)
    s = rng.normal(size=n).astype(np.float32)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-1.5 * s.astype(np.float64)))).astype(np.int64)
    return s, y


def labels(pattern: str, n: int, seed: int = 0) -> np.ndarray:
    """0/1 labels in ascending score order (one row per group)."""
    rng = np.random.default_rng(seed + 31 * n)
    if pattern == "random":
        return (rng.random(n) < np.linspace(0.05, 0.95, n)).astype(np.int64)
    if pattern == "all0":
        return np.zeros(n, dtype=np.int64)
    if pattern == "all1":
        return np.ones(n, dtype=np.int64)
    if pattern == "sorted":
        return (np.arange(n) >= n // 2).astype(np.int64)
    if pattern == "antisorted":          # one block
        return (np.arange(n) < (n + 1) // 2).astype(np.int64)
    if pattern == "long_block":          # random ends around an anti-sorted middle: a block spanning several tiles
        y = (rng.random(n) < np.linspace(0.05, 0.95, n)).astype(np.int64)
        a, b = n // 8, n - n // 8
        y[a:b] = (np.arange(b - a) < (b - a) // 2).astype(np.int64)
        return y
    raise ValueError(pattern)


def cum_from_labels(y, w=None):
    y = np.asarray(y, dtype=np.int64)
    w = np.ones(y.shape[0], dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(w)]).astype(np.int64), np.concatenate([[0], np.cumsum(w * y)]).astype(np.int64)


def hull_case(pattern: str, n: int, seed: int = 0):
    """``(cw, cs)`` of ``n`` rows. "ties": scores rounded to runs of about six equal values (fewer groups than
    rows, runs crossing every tile edge of the rows); all others: one row per group."""
    if pattern == "ties":
        from cobalt_smart_lender_ai_amd.metrics import calibration as C

        rng = np.random.default_rng(seed + 17 * n)
        s = np.floor(np.sort(rng.random(n)) * max(1, n // 6)).astype(np.float32)
        y = (rng.random(n) < 0.1 + 0.8 * s / max(1.0, float(s.max()))).astype(np.int64)
        _, cw, cs = C.iso_groups(s, y, rng.integers(1, 9, size=n))
        return cw, cs
    return cum_from_labels(labels(pattern, n, seed))


def convex_case(groups: int):
    """Block means strictly increase (group k: weight ``groups``, positives ``k``), so every point is a hull
    vertex and no tile sheds anything."""
    if groups * groups > MAX_TOTAL:
        raise ValueError("too many groups for the weight bound")
    k = np.arange(groups, dtype=np.int64)
    return (np.concatenate([[0], np.cumsum(np.full(groups, groups, dtype=np.int64))]),
            np.concatenate([[0], np.cumsum(k)]))


def weighted_case(n: int, total: int, seed: int = 0):
    """Random labels with random weights whose sum is exactly ``total`` (the last weight takes the rest)."""
    rng = np.random.default_rng(seed)
    y = labels("random", n, seed)
    w = rng.integers(1, max(2, total // n), size=n).astype(np.int64)
    rest = total - int(w[:-1].sum())
    if rest < 1:
        raise ValueError("total too small for n")
    w[-1] = rest
    return cum_from_labels(y, w)


def brute_isotonic(cw, cs) -> list[Fraction]:
    """The fitted value of every group by the min-max formula ``max_{j <= i} min_{k >= i} mean(j .. k)`` in exact
    fractions: O(G^3), for small G."""
    G = len(cw) - 1
    mean = [[Fraction(int(cs[k + 1] - cs[j]), int(cw[k + 1] - cw[j])) if k >= j else None for k in range(G)]
            for j in range(G)]
    return [max(min(mean[j][k] for k in range(i, G)) for j in range(i + 1)) for i in range(G)]


def values_from_hull(hull, cw, cs) -> list[Fraction]:
    """Per-group exact values of a vertex list."""
    out = []
    for a, b in zip(hull[:-1], hull[1:]):
        a, b = int(a), int(b)
        out += [Fraction(int(cs[b] - cs[a]), int(cw[b] - cw[a]))] * (b - a)
    return out


def apply_case(K: int, n: int, seed: int = 0):
    """``K`` knots (float32 positions, fp64 values ascending in [0, 1]) and ``n`` float32 queries: uniform over a
    range wider than the knots, then (where they fit) the first / last / a middle knot exactly, a value below,
    a value above and a NaN."""
    rng = np.random.default_rng(seed + K)
    xk = np.unique(rng.normal(size=2 * K + 8).astype(np.float32))[:K]
    assert xk.shape[0] == K
    vk = np.sort(rng.random(K))
    x = rng.uniform(float(xk[0]) - 1.0, float(xk[-1]) + 1.0, size=n).astype(np.float32)
    special = np.array([xk[0], xk[-1], xk[K // 2], xk[0] - np.float32(3), xk[-1] + np.float32(3), np.nan], dtype=np.float32)
    m = min(n, special.shape[0])
    x[n - m:] = special[special.shape[0] - m:]
    return xk, vk, x


def reliability_case(n: int, B: int, seed: int = 0, weighted: bool = False):
    """float32 probabilities with exact 0, exact 1 and values exactly on edges, labels, optional weights up to
    2^20 and ``B - 1`` float32 interior edges (uniform; ascending)."""
    rng = np.random.default_rng(seed + B)
    edges = (np.arange(1, B, dtype=np.float64) / B).astype(np.float32)
    p = rng.random(n).astype(np.float32)
    p[0], p[1 % n] = 0.0, 1.0
    if B > 1 and n > 4:
        p[2], p[3], p[4] = edges[0], edges[-1], edges[(B - 1) // 2]
    y = (rng.random(n) < p).astype(np.float32)
    wq = None
    if weighted:
        wq = rng.integers(0, 64, size=n).astype(np.int32)
        wq[n // 2] = 1 << 20
    return p, y, wq, edges
