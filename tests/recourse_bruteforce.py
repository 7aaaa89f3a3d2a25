"""The recourse scan from its definition, in plain Python (test_recourse_cpu.py, test_gpu_recourse.py): every
candidate is substituted explicitly into a copy of the row, the copy is scored by
``scoring_forests.predict_rowwise`` (one row at a time; nothing shared with ``predict_margin_host``,
``recourse_scan_host`` or the kernel), and the three slots are picked from the resulting sets by their
definitions (a max, a min, a sort), not by a running fold."""
from __future__ import annotations

import numpy as np

import scoring_forests as sf

EMPTY_BITS = 0x7FC00000


def scan_row(b, x, feats, cands, win, dirs, target, n_trees=None):
    """(idx [A, 3] int, margin bits [A, 3] int) of one row."""
    A = len(feats)
    idx = np.full((A, 3), -1, np.int64)
    bits = np.full((A, 3), EMPTY_BITS, np.int64)
    target = np.float32(target)
    for a, f in enumerate(feats):
        cv = np.asarray(cands[a], np.float32)
        xv = np.float32(x[f])
        if np.isnan(xv):
            continue
        c = sum(1 for v in cv if v <= xv) - 1
        js = [j for j in range(int(win[a][0]), int(win[a][1]) + 1) if j != c]
        if not js:
            continue
        rows = np.repeat(np.asarray(x, np.float32)[None, :], len(js), axis=0)
        rows[:, f] = cv[js]
        m = dict(zip(js, sf.predict_rowwise(b, rows, n_trees)))
        down = [j for j in js if j < c and dirs[a] != 1]
        up = [j for j in js if j > c and dirs[a] != -1]
        picks = (max((j for j in down if m[j] <= target), default=None),
                 min((j for j in up if m[j] <= target), default=None),
                 min(down + up, key=lambda j: (m[j], abs(j - c), j), default=None))
        for s, j in enumerate(picks):
            if j is not None:
                idx[a, s] = j
                bits[a, s] = int(np.float32(m[j]).view(np.uint32))
    return idx, bits


def scan(b, X, feats, cands, win=None, dirs=None, target=0.0, n_trees=None):
    """(idx [N, A, 3] int32, margin bits [N, A, 3] uint32). Equal rows are scored once."""
    X = np.asarray(X, np.float32)
    A = len(feats)
    win = [(0, len(c) - 1) for c in cands] if win is None else np.asarray(win).reshape(A, 2)
    dirs = [0] * A if dirs is None else list(dirs)
    idx = np.empty((X.shape[0], A, 3), np.int32)
    bits = np.empty((X.shape[0], A, 3), np.uint32)
    seen: dict[bytes, tuple] = {}
    for r in range(X.shape[0]):
        key = X[r].tobytes()
        if key not in seen:
            seen[key] = scan_row(b, X[r], feats, cands, win, dirs, target, n_trees)
        idx[r], bits[r] = seen[key]
    return idx, bits


def bits_of(margin) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(margin, np.float32)).view(np.uint32)
