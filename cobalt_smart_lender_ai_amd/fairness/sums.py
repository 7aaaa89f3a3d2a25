"""The fair-lending sums: per bootstrap replicate, protected group and cutoff the exact integers every number of
the audit is a ratio of. This module is the definition and the CPU path; ``csrc/fairness.hip`` (through
``ops.fairness_ops``) computes the same integers on the GPU.

**Per-row facts**, all integers: ``declined_k = score > float32(cutoff_k)`` (the comparison of
``metrics.bootstrap.rank_structure``'s ``pred``; recourse's "approved" is its negation, ``score <= cutoff``); the
score on a 16-bit grid, ``q = min(floor(score * 65536), 65535)`` in float32 (exact: a multiplication by a power of
two), so ``q / 65536 <= score < (q + 1) / 65536`` except at ``score = 1``; the label bit.

**Counts.** Replicate ``b`` gives original row ``i`` the count ``c[b, i]`` of
``metrics.bootstrap.bootstrap_counts_host``: the same resample as ``metrics.bootstrap_ci`` with the same seed, so
the fairness report and the accuracy report of one model are paired. The unit replicate (every count 1) gives
the point estimates.

**Sums** (:func:`field_names`), int64 ``[4 + 2 K, G, B]``: ``n_g = sum c``, ``B_g = sum c y``, ``S1_g = sum c q``,
``S2_g = sum c q^2``, then ``D_gk = sum c declined_k`` for the ``K`` cutoffs and ``DB_gk = sum c declined_k y``.
``n <= 2^27`` rows of at most 12 copies keep ``S2 <= 12 * 2^27 * 2^32 < 2^63``. Without labels ``B`` and ``DB``
are zeros.
"""
from __future__ import annotations

import numpy as np

from ..metrics.bootstrap import MAX_COUNT, bootstrap_counts_host
from ..portfolio.loss import tile_layout

MAX_ROWS = 1 << 27
MAX_GROUPS = 64
MAX_CUTOFFS = 16
MAX_REPS = 1 << 20
Q_SCALE = 65536
Q_MAX = 65535
FIXED_FIELDS = ("n", "B", "S1", "S2")
IDX_BITS = 28
LABEL_BIT, PAD_BIT = 1 << 28, 1 << 29
_HOST_CHUNK = 1 << 22  # count-matrix entries per chunk of replicates


def field_names(K: int) -> tuple[str, ...]:
    """The names of the ``4 + 2 K`` rows of the sums."""
    return FIXED_FIELDS + tuple(f"D{k}" for k in range(K)) + tuple(f"DB{k}" for k in range(K))


def check_cutoffs(cutoffs) -> np.ndarray:
    """The cutoffs as float32 ``[K]``, ``1 <= K <= 16``, none NaN. Order and duplicates are the caller's."""
    c = np.asarray(cutoffs, dtype=np.float64).reshape(-1)
    if not 1 <= c.shape[0] <= MAX_CUTOFFS:
        raise ValueError(f"1 .. {MAX_CUTOFFS} cutoffs, got {c.shape[0]}")
    if np.isnan(c).any():
        raise ValueError("NaN cutoff")
    return c.astype(np.float32)


def score_grid(score) -> np.ndarray:
    """``q``, int64: ``min(floor(float32(score) * 65536), 65535)``. ``ValueError`` for NaN or scores outside
    ``[0, 1]``."""
    s = np.asarray(score).reshape(-1).astype(np.float32)
    if np.isnan(s).any():
        raise ValueError("NaN scores")
    if s.size and (s.min() < 0 or s.max() > 1):
        raise ValueError("scores must lie in [0, 1]")
    return np.minimum(np.floor(s * np.float32(Q_SCALE)), np.float32(Q_MAX)).astype(np.int64)


def decline_mask(score, cutoffs) -> np.ndarray:
    """int64 per row: bit ``k`` is ``float32(score) > float32(cutoffs[k])``."""
    s = np.asarray(score).reshape(-1).astype(np.float32)
    cut = check_cutoffs(cutoffs)
    return ((s[:, None] > cut[None, :]).astype(np.int64) << np.arange(cut.shape[0], dtype=np.int64)[None, :]).sum(axis=1)


def _check(score, group, y, cutoffs, seed, reps, rep0, n_groups, rows):
    s = np.asarray(score).reshape(-1)
    n = s.shape[0]
    if n < 1:
        raise ValueError("empty input")
    if n > MAX_ROWS:
        raise ValueError(f"at most 2^27 rows ({n} given): beyond it S2 can pass 2^63")
    q = score_grid(s)
    cut = check_cutoffs(cutoffs)
    g = np.asarray(group).reshape(-1)
    if g.shape[0] != n:
        raise ValueError(f"{n} scores, {g.shape[0]} group codes")
    if not np.issubdtype(g.dtype, np.integer):
        raise ValueError("group codes must be integers")
    g = g.astype(np.int64)
    G = int(g.max()) + 1 if n_groups is None else int(n_groups)
    if not 1 <= G <= MAX_GROUPS:
        raise ValueError(f"1 .. {MAX_GROUPS} groups, got {G}")
    if g.min() < 0 or g.max() >= G:
        raise ValueError(f"group codes must lie in 0 .. {G - 1}")
    if y is None:
        lab = np.zeros(n, dtype=np.int64)
    else:
        yy = np.asarray(y).reshape(-1)
        if yy.shape[0] != n:
            raise ValueError(f"{n} scores, {yy.shape[0]} labels")
        if not np.all((yy == 0) | (yy == 1)):
            raise ValueError("labels must be 0 or 1")
        lab = yy.astype(np.int64)
    if rows is None:
        idx = np.arange(n, dtype=np.int64)
    else:
        idx = np.asarray(rows).reshape(-1).astype(np.int64)
        if idx.shape[0] != n:
            raise ValueError(f"{n} scores, {idx.shape[0]} row indices")
        if idx.min() < 0 or idx.max() >= 1 << IDX_BITS:
            raise ValueError("original row indices must lie in 0 .. 2^28 - 1")
    reps, rep0, seed = int(reps), int(rep0), int(seed)
    if not 1 <= reps <= MAX_REPS:
        raise ValueError(f"1 .. 2^20 replicates per call, got {reps}")
    if rep0 < 0 or rep0 % 4 or rep0 + reps > 1 << 32:
        raise ValueError("rep0 must be a non-negative multiple of 4")
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit 64 bits")
    mask = decline_mask(s, cut)
    K = cut.shape[0]
    dec = (mask[:, None] >> np.arange(K, dtype=np.int64)[None, :]) & 1
    # one column per field: what a row with count 1 adds to it
    V = np.concatenate([np.ones((n, 1), dtype=np.int64), lab[:, None], q[:, None], (q * q)[:, None], dec,
                        dec * lab[:, None]], axis=1)
    return V, g, G, idx, seed, reps, rep0


def _range_sums(V, idx, seed, reps, rep0, bounds, unit) -> np.ndarray:
    """int64 ``[F, len(bounds) - 1, reps]``: the sums of the row ranges ``bounds[r] .. bounds[r + 1]`` (positions
    in the arrays given). A row of ``V`` that is all zeros counts for nothing."""
    n, F = V.shape
    R = len(bounds) - 1
    out = np.zeros((F, R, reps), dtype=np.int64)
    step = max(4, (_HOST_CHUNK // max(n, 1)) // 4 * 4)
    for b0 in range(0, reps, step):
        b1 = min(b0 + step, reps)
        c = (np.ones((b1 - b0, n), dtype=np.int64) if unit
             else bootstrap_counts_host(seed, idx, b1 - b0, rep0 + b0).astype(np.int64))
        for r in range(R):
            lo, hi = int(bounds[r]), int(bounds[r + 1])
            if hi > lo:
                out[:, r, b0:b1] = (c[:, lo:hi] @ V[lo:hi]).T
    return out


def fairness_sums_host(score, group, y, cutoffs, seed: int = 0, reps: int = 1, rep0: int = 0, *,
                       n_groups: int | None = None, rows=None, unit: bool = False) -> np.ndarray:
    """The direct form: int64 ``[4 + 2 K, G, reps]``, replicates ``rep0 .. rep0 + reps - 1`` (``rep0`` a multiple
    of 4). ``score``: float32 PDs in ``[0, 1]``; ``group``: integer codes ``0 .. G - 1`` (``G = n_groups``, or the
    largest code plus one); ``y``: 0/1 or None; ``cutoffs``: ``K`` values, in any order; ``rows``: the original
    row index of every row (``0 .. n - 1`` when None), which is what a row's counts depend on; ``unit``: every
    count is 1. ``ValueError`` for NaN or out-of-range scores, more than 64 groups or 16 cutoffs, length
    mismatches, labels other than 0/1."""
    V, g, G, idx, seed, reps, rep0 = _check(score, group, y, cutoffs, seed, reps, rep0, n_groups, rows)
    order = np.argsort(g, kind="stable")
    bounds = np.searchsorted(g[order], np.arange(G + 1))
    return _range_sums(V[order], idx[order], seed, reps, rep0, bounds, unit)


def fairness_sums_tiled_host(score, group, y, cutoffs, seed: int = 0, reps: int = 1, rep0: int = 0, *,
                             tile_rows: int, n_groups: int | None = None, rows=None,
                             unit: bool = False) -> np.ndarray:
    """The kernel's decomposition on the host, for any tile length: the rows in
    ``portfolio.loss.tile_layout`` order (sorted by group, every group padded to whole tiles with rows that count
    for nothing), per tile one record of the ``4 + 2 K`` sums, then per group the sum of its tiles in order. Same
    return as :func:`fairness_sums_host`, and the same integers."""
    V, g, G, idx, seed, reps, rep0 = _check(score, group, y, cutoffs, seed, reps, rep0, n_groups, rows)
    src, tile_group = tile_layout(g, G, tile_rows)
    pad = src < 0
    take = np.where(pad, 0, src)
    V_t = np.where(pad[:, None], 0, V[take])
    idx_t = np.where(pad, 0, idx[take])
    tiles = int(tile_group[-1])
    recs = _range_sums(V_t, idx_t, seed, reps, rep0, np.arange(tiles + 1) * int(tile_rows), unit)
    assert recs[0].max(initial=0) <= MAX_COUNT * int(tile_rows)
    out = np.zeros((V.shape[1], G, reps), dtype=np.int64)
    for gg in range(G):
        for t in range(int(tile_group[gg]), int(tile_group[gg + 1])):
            out[:, gg] += recs[:, t]
    return out
