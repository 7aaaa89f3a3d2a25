"""Pairwise-complete correlation moments: ``csrc/corr.hip`` for CUDA tensors, the NumPy definition
``pair_moments_host`` otherwise. A value is present iff it is finite. With ``c = x - mu`` for a present value and
``c = m = 0`` for a missing one, for every ordered pair of columns

    n[i, j] = sum m_i m_j      A[i, j] = sum c_i m_j      Q[i, j] = sum c_i^2 m_j      P[i, j] = sum c_i c_j

``corr_from_moments`` turns the four tables into Pearson's r with pairwise deletion; it is the one piece of code both
paths share. The sums are shift-invariant: ``mu`` only removes the cancellation in ``n P - A A^T``. ``n`` is exact on
both paths, the float sums agree to the summation error, and on the device the same input gives the same bits on
every call. Arguments are checked before any launch (``ValueError``).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _native

_V, _I, _I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
# (X, n, F, ldx, mu, workspace, workspace_bytes, n_out, a_out, q_out, p_out, stream)
_native.register("cobalt_corr_moments", _I, [_V, _I64, _I, _I64, _V, _V, _I64, _V, _V, _V, _V, _V])
# (X, n, F, ldx, sums, counts, stream)
_native.register("cobalt_corr_col_sums", _I, [_V, _I64, _I, _I64, _V, _V, _V])
_native.register("cobalt_corr_workspace_bytes", _I64, [_I64, _I])
_native.register("cobalt_corr_blocks", _I, [_I64])
for _name in ("cobalt_corr_max_features", "cobalt_corr_chunk_rows", "cobalt_corr_block_rows",
              "cobalt_corr_max_blocks"):
    _native.register(_name, _I, [])

GPU_MAX_FEATURES = 128       # kCorrMaxFeatures; test_limits checks it against the library
MAX_RANK_ROWS = 1 << 23      # float32 holds half-integer ranks exactly up to here
_SUM_COLS = 128              # pitch of the column-sum partials


def max_features() -> int:
    """Columns one call of the kernel takes."""
    return int(_native.lib().cobalt_corr_max_features())


def block_rows() -> int:
    """Rows of one block of the moments kernel (until the grid is full)."""
    return int(_native.lib().cobalt_corr_block_rows())


def chunk_rows() -> int:
    """Rows a block stages in LDS at a time."""
    return int(_native.lib().cobalt_corr_chunk_rows())


def _rows(X: torch.Tensor):
    if X.dim() != 2 or X.dtype != torch.float32:
        raise ValueError(f"X must be float32 [rows, features], got {X.dtype} {tuple(X.shape)}")
    N, F = X.shape
    if F < 1 or F > GPU_MAX_FEATURES:
        raise ValueError(f"the GPU correlation kernel takes 1 .. {GPU_MAX_FEATURES} features, got {F}")
    if N > 0 and F > 1 and X.stride(1) != 1:
        raise ValueError(f"X must have unit column stride, got stride {X.stride(1)}")
    ldx = X.stride(0) if N > 1 else F
    if ldx < F:
        raise ValueError(f"rows of X overlap (row stride {ldx} < {F} columns)")
    return N, F, ldx


def _check_mu(mu, F: int) -> np.ndarray:
    m = np.ascontiguousarray(mu.detach().cpu().numpy() if isinstance(mu, torch.Tensor) else mu,
                             dtype=np.float64).reshape(-1)
    if m.shape[0] != F or not bool(np.isfinite(m).all()):
        raise ValueError(f"mu must hold {F} finite values")
    return m


def _host_matrix(X) -> np.ndarray:
    a = X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X)
    if a.ndim != 2 or a.shape[1] < 1:
        raise ValueError(f"X must be [rows, features] with at least one feature, got {a.shape}")
    return a


def column_centre_host(X) -> np.ndarray:
    """float64 ``[F]``: the float32-rounded mean of each column's present values (0 for a column without any)."""
    a = _host_matrix(X)
    fin = np.isfinite(a)
    cnt = fin.sum(axis=0)
    s = np.where(fin, a, 0).astype(np.float64).sum(axis=0)
    with np.errstate(over="ignore"):
        mu = (s / np.maximum(cnt, 1)).astype(np.float32).astype(np.float64)
    return np.where((cnt > 0) & np.isfinite(mu), mu, 0.0)


def column_centre(X: torch.Tensor) -> np.ndarray:
    """``column_centre_host`` of a CUDA tensor from the kernel's column sums (the sums are added in another order, so
    a centre may differ from the host's by one float32 step; any centre gives the same correlation)."""
    N, F, ldx = _rows(X)
    if N == 0:
        return np.zeros(F)
    lib = _native.lib()
    blocks = int(lib.cobalt_corr_blocks(N))
    _native.check(min(blocks, 0), "cobalt_corr_blocks")
    sums = torch.empty((blocks, _SUM_COLS), dtype=torch.float64, device=X.device)
    counts = torch.empty((blocks, _SUM_COLS), dtype=torch.int64, device=X.device)
    with torch.cuda.device(X.device):
        rc = lib.cobalt_corr_col_sums(X.data_ptr(), N, F, ldx, sums.data_ptr(), counts.data_ptr(),
                                      _native.stream_handle())
    _native.check(rc, "cobalt_corr_col_sums")
    s = sums.sum(dim=0)[:F].cpu().numpy()
    cnt = counts.sum(dim=0)[:F].cpu().numpy()
    with np.errstate(over="ignore"):
        mu = (s / np.maximum(cnt, 1)).astype(np.float32).astype(np.float64)
    return np.where((cnt > 0) & np.isfinite(mu), mu, 0.0)


def pair_moments_host(X, mu=None):
    """``(n int64, A, Q, P float64)``, each ``[F, F]``, in NumPy float64: the definition of the module docstring."""
    a = _host_matrix(X)
    F = a.shape[1]
    m = column_centre_host(a) if mu is None else _check_mu(mu, F)
    fin = np.isfinite(a)
    C = np.where(fin, np.where(fin, a, 0).astype(np.float64) - m[None, :], 0.0)
    M = fin.astype(np.float64)
    n = np.rint(M.T @ M).astype(np.int64)
    A = C.T @ M
    Q = (C * C).T @ M
    P = C.T @ C
    P = np.triu(P) + np.triu(P, 1).T
    return n, A, Q, P


def pair_moments(X, mu=None):
    """``(n int64, A, Q, P float64)``, each ``[F, F]``. A CUDA tensor (float32, unit column stride, rows may be
    strided, at most 128 columns) goes to the kernel and CUDA tensors come back; anything else goes to
    ``pair_moments_host`` and NumPy arrays come back. ``mu`` defaults to the float32-rounded column means of the
    present values."""
    if not (isinstance(X, torch.Tensor) and X.device.type == "cuda"):
        return pair_moments_host(X, mu)
    N, F, ldx = _rows(X)
    m = column_centre(X) if mu is None else _check_mu(mu, F)
    dev = X.device
    lib = _native.lib()
    need = int(lib.cobalt_corr_workspace_bytes(N, F))
    _native.check(min(need, 0), "cobalt_corr_workspace_bytes")
    work = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=dev)
    mu_d = torch.from_numpy(m).to(dev)
    n = torch.empty((F, F), dtype=torch.int64, device=dev)
    A, Q, P = (torch.empty((F, F), dtype=torch.float64, device=dev) for _ in range(3))
    with torch.cuda.device(dev):
        rc = lib.cobalt_corr_moments(X.data_ptr(), N, F, ldx, mu_d.data_ptr(), work.data_ptr(), need, n.data_ptr(),
                                     A.data_ptr(), Q.data_ptr(), P.data_ptr(), _native.stream_handle())
    _native.check(rc, "cobalt_corr_moments")
    return n, A, Q, P


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def corr_from_moments(n, A, Q, P, min_periods: int = 1) -> np.ndarray:
    """Pearson's r with pairwise deletion, float64 ``[F, F]`` (NumPy), from the tables of ``pair_moments``. For
    ``i < j``: ``r = (n P_ij - A_ij A_ji) / sqrt((n Q_ij - A_ij^2) (n Q_ji - A_ji^2))``, clamped to [-1, 1] and
    mirrored, so r is bitwise symmetric. NaN where ``n_ij < max(min_periods, 2)`` or a variance term is <= 0
    (pandas' answer for a constant or absent column). The diagonal is exactly 1.0 where the column has positive
    variance over enough rows, NaN otherwise."""
    n = _np(n).astype(np.float64)
    A, Q, P = (_np(t).astype(np.float64) for t in (A, Q, P))
    F = n.shape[0]
    need = max(int(min_periods), 2)
    vi = n * Q - A * A            # [i, j]: n times the sum of squares of i about its mean over the rows of (i, j)
    vj = vi.T
    num = n * P - A * A.T
    ok = (n >= need) & (vi > 0.0) & (vj > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = num / (np.sqrt(np.where(ok, vi, 1.0)) * np.sqrt(np.where(ok, vj, 1.0)))
    r = np.where(ok, np.clip(r, -1.0, 1.0), np.nan)
    r = np.triu(r, 1)
    r = r + r.T
    idx = np.arange(F)
    r[idx, idx] = np.where(ok[idx, idx], 1.0, np.nan)
    return r


def column_ranks(X) -> torch.Tensor:
    """Average ranks (1-based, ties averaged) of each column's present values as float32 ``[N, F]``, missing values
    (NaN, +-inf) left as NaN; on the device of ``X``, with the same bits on the CPU and on the GPU. One sort per
    column (``torch.sort(dim=0)``), run starts by comparison, run ends by a reversed scan."""
    if not isinstance(X, torch.Tensor):
        a = np.asarray(X)
        X = torch.from_numpy(a if a.flags.writeable else a.copy())
    t = X
    if t.dim() != 2:
        raise ValueError(f"X must be [rows, features], got {tuple(t.shape)}")
    N, F = t.shape
    if N > MAX_RANK_ROWS:
        raise ValueError(f"float32 ranks are exact up to {MAX_RANK_ROWS} rows, got {N}")
    if N == 0 or F == 0:
        return torch.full((N, F), float("nan"), dtype=torch.float32, device=t.device)
    x = t if t.dtype in (torch.float32, torch.float64) else t.to(torch.float32)
    x = torch.where(torch.isfinite(x), x, torch.full_like(x, float("nan")))  # the sort puts NaN last
    xs, order = torch.sort(x, dim=0)
    pos = torch.arange(N, device=x.device, dtype=torch.int64).unsqueeze(1).expand(N, F)
    new = torch.ones((N, F), dtype=torch.bool, device=x.device)
    new[1:] = xs[1:] != xs[:-1]                                   # NaN != NaN: every missing value is its own run
    first = torch.cummax(torch.where(new, pos, torch.zeros_like(pos)), dim=0).values
    last_run = torch.ones((N, F), dtype=torch.bool, device=x.device)
    last_run[:-1] = new[1:]
    rev = torch.where(last_run, pos, torch.full_like(pos, N)).flip(0)
    last = torch.cummin(rev, dim=0).values.flip(0)
    rank = ((first + last).to(torch.float32) * 0.5) + 1.0        # (first + last) / 2 is a half-integer below 2^23
    rank = torch.where(torch.isnan(xs), torch.full_like(rank, float("nan")), rank)  # float32 whatever x is
    out = torch.empty_like(rank)
    out.scatter_(0, order, rank)
    return out
