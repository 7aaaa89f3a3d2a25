"""The bootstrap sums on the GPU: ``csrc/bootstrap.hip`` (per replicate the exact integers ``P N U2 KSn TP FP``
and two optional fp64 sums of one sorted score vector under Poisson(1) resampling counts). The definition and
the CPU path are ``metrics.bootstrap.bootstrap_sums_host``; the integers are the same.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _native
from ..metrics import bootstrap as B

_V, _I, _I64, _U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
# (words, terms, n, rep0, reps, seed, flags, workspace, workspace_bytes, out_int, out_f, ld, stream)
_native.register("cobalt_bootstrap", _I, [_V, _V, _I64, _I64, _I, _U64, _I, _V, _I64, _V, _V, _I64, _V])
_native.register("cobalt_bootstrap_workspace_bytes", _I64, [_I64, _I, _I, _I])
_native.register("cobalt_bootstrap_tile_rows", _I, [])
_native.register("cobalt_bootstrap_block_reps", _I, [])
_native.register("cobalt_bootstrap_out_fields", _I, [])
_native.register("cobalt_bootstrap_max_rows", _I64, [])

FLAG_KS, FLAG_UNIT = 1, 2
WORKSPACE_TARGET = 1 << 30   # bytes: replicates are split into calls whose tile records stay under it


def bootstrap_tile_rows() -> int:
    return int(_native.lib().cobalt_bootstrap_tile_rows())


def bootstrap_block_reps() -> int:
    return int(_native.lib().cobalt_bootstrap_block_reps())


def bootstrap_workspace_bytes(n: int, reps: int, with_terms: bool, with_ks: bool) -> int:
    """Bytes of scratch one call needs, or the kernel's negative refusal for these shapes."""
    return int(_native.lib().cobalt_bootstrap_workspace_bytes(int(n), int(reps), int(with_terms), int(with_ks)))


def rank_words_gpu(y_true: torch.Tensor, y_score: torch.Tensor, threshold: float = 0.5):
    """The rank structure on the device: ``torch.sort(stable=True)`` of the float32 scores, then the packed
    int32 words (``metrics.bootstrap.pack_words``) and the sort's index vector. Inputs are checked as the host
    path checks them (one synchronisation)."""
    s = y_score.reshape(-1).to(torch.float32)
    y = y_true.reshape(-1).to(s.device)
    n = s.shape[0]
    if y.shape[0] != n:
        raise ValueError(f"{y.shape[0]} labels, {n} scores")
    if n < 1:
        raise ValueError("empty input")
    if n > B.MAX_ROWS:
        raise ValueError(f"at most 2^28 rows ({n} given): beyond it 2 P N can pass 2^63")
    bad = torch.stack([((y != 0) & (y != 1)).any(), torch.isnan(s).any()]).cpu()
    if bool(bad[0]):
        raise ValueError("labels must be 0 or 1")
    if bool(bad[1]):
        raise ValueError("NaN scores")
    ss, order = torch.sort(s, stable=True)
    start = torch.ones(n, dtype=torch.bool, device=s.device)
    start[1:] = ss[1:] != ss[:-1]
    lab = y[order] != 0
    pred = ss > float(np.float32(threshold))
    words = (order | (lab.to(torch.int64) << 28) | (start.to(torch.int64) << 29) | (pred.to(torch.int64) << 30))
    return words.to(torch.int32).contiguous(), order


def bootstrap_sums_gpu(words: torch.Tensor, reps: int, seed: int = 0, *, terms: torch.Tensor | None = None,
                       ks: bool = True, unit: bool = False, rep0: int = 0):
    """int64 ``[6, reps]`` (``metrics.bootstrap.FIELDS``) and float64 ``[2, reps]`` on the device of ``words``,
    on the current stream: replicates ``rep0 .. rep0 + reps - 1`` (``rep0`` a multiple of 4) of the sorted rows
    ``words`` (int32 ``[n]``, :func:`rank_words_gpu`). ``terms``: float64 ``[2, n]`` in SORTED order or None (the
    float sums are then zeros). ``ks=False`` skips the second row pass (``KSn`` is 0); ``unit`` makes every count
    1 (the point estimate). Replicates are split into calls that keep the scratch near 1 GiB. ``ValueError`` /
    ``RuntimeError`` before any launch."""
    if not isinstance(words, torch.Tensor) or words.device.type != "cuda":
        raise ValueError("bootstrap_sums_gpu takes a CUDA tensor")
    if words.dim() != 1 or words.dtype != torch.int32 or not words.is_contiguous():
        raise ValueError(f"words must be a contiguous int32 vector, got {words.dtype} {tuple(words.shape)}")
    n, reps, rep0, seed = int(words.shape[0]), int(reps), int(rep0), int(seed)
    if n < 1 or n > B.MAX_ROWS:
        raise ValueError(f"1 .. 2^28 rows, got {n}")
    if reps < 1:
        raise ValueError("at least one replicate")
    if rep0 < 0 or rep0 % 4:
        raise ValueError("rep0 must be a non-negative multiple of 4")
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit 64 bits")
    dev = words.device
    if terms is not None:
        if terms.shape != (2, n) or terms.dtype != torch.float64 or terms.device != dev:
            raise ValueError(f"terms must be float64 [2, {n}] on {dev}")
        terms = terms.contiguous()
    flags = (FLAG_KS if ks else 0) | (FLAG_UNIT if unit else 0)
    out_int = torch.zeros((len(B.FIELDS), reps), dtype=torch.int64, device=dev)
    out_f = torch.zeros((2, reps), dtype=torch.float64, device=dev)
    per4 = bootstrap_workspace_bytes(n, 4, terms is not None, ks)
    _native.check(min(per4, 0), "cobalt_bootstrap_workspace_bytes")
    step = min(reps, max(4, WORKSPACE_TARGET // per4 * 4))
    need = bootstrap_workspace_bytes(n, step, terms is not None, ks)
    _native.check(min(need, 0), "cobalt_bootstrap_workspace_bytes")
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    for b0 in range(0, reps, step):
        rc = _native.lib().cobalt_bootstrap(words.data_ptr(), _native.ptr(terms), n, rep0 + b0, min(step, reps - b0),
                                            seed, flags, work.data_ptr(), need, out_int[:, b0:].data_ptr(),
                                            out_f[:, b0:].data_ptr(), reps, _native.stream_handle())
        _native.check(rc, "cobalt_bootstrap")
    return out_int, out_f


def bootstrap_sums_for_ci(y_true, y_score, n_boot: int, seed: int, threshold: float, want_terms: bool, want_ks: bool,
                          device=None):
    """What ``metrics.bootstrap.bootstrap_ci`` needs from the GPU for one score vector: the point sums (every
    count 1) and the replicate sums, each as host arrays ``(int64 [6, .], float64 [2, .])``."""
    dev = torch.device(device) if device is not None else next(
        x.device for x in (y_true, y_score) if isinstance(x, torch.Tensor) and x.is_cuda)
    y = torch.as_tensor(np.asarray(y_true) if not isinstance(y_true, torch.Tensor) else y_true).to(dev)
    s = torch.as_tensor(np.asarray(y_score) if not isinstance(y_score, torch.Tensor) else y_score).to(dev)
    with torch.cuda.device(dev):
        words, order = rank_words_gpu(y, s, threshold)
        terms = None
        if want_terms:
            yo = y.reshape(-1)[order].to(torch.float64)
            p = s.reshape(-1).to(torch.float32)[order].to(torch.float64)
            q = p.clamp(1e-15, 1 - 1e-15)
            terms = torch.stack([-(yo * torch.log(q) + (1 - yo) * torch.log1p(-q)), (p - yo) ** 2]).contiguous()
        point = bootstrap_sums_gpu(words, 1, seed, terms=terms, ks=want_ks, unit=True)
        reps = bootstrap_sums_gpu(words, n_boot, seed, terms=terms, ks=want_ks)
    return tuple(t.cpu().numpy() for t in point), tuple(t.cpu().numpy() for t in reps)
