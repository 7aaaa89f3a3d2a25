"""Score calibration on the GPU: ``csrc/calib.hip`` (the isotonic fit's convex hull, the piecewise-linear apply
and the reliability table). The definitions and the CPU path are in ``metrics.calibration``; the hull, the table
and the applied values are the same bits. Everything around the kernels is plain torch on the current stream
(``torch.sort(stable=True)``, group starts, int64 ``cumsum``).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _native
from ..metrics import calibration as C
from ..models.sketch import WEIGHT_SCALE

_V, _I, _I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
# (cw, cs, m, total_weight, workspace, workspace_bytes, out_idx, out_cnt, rounds_cnt, stream)
_native.register("cobalt_iso_hull", _I, [_V, _V, _I64, _I64, _V, _I64, _V, _V, _V, _V])
_native.register("cobalt_iso_hull_workspace_bytes", _I64, [_I64])
_native.register("cobalt_iso_tile_rows", _I, [])
_native.register("cobalt_iso_rounds", _I, [])
# (x, n, xk, vk, K, out, stream)
_native.register("cobalt_calib_apply", _I, [_V, _I64, _V, _V, _I, _V, _V])
_native.register("cobalt_calib_lds_knots", _I, [])
# (p, y, wq, n, edges, B, out, stream)
_native.register("cobalt_reliability_sums", _I, [_V, _V, _V, _I64, _V, _I, _V, _V])
_native.register("cobalt_reliability_lds_bins", _I, [])
_native.register("cobalt_reliability_max_bins", _I, [])


def iso_tile_rows() -> int:
    return int(_native.lib().cobalt_iso_tile_rows())


def iso_rounds() -> int:
    return int(_native.lib().cobalt_iso_rounds())


def calib_lds_knots() -> int:
    """Knots the apply kernel stages in LDS; above it the search reads global memory."""
    return int(_native.lib().cobalt_calib_lds_knots())


def reliability_lds_bins() -> int:
    """Bins whose counters the reliability kernel keeps in LDS; above it rows add to the table directly."""
    return int(_native.lib().cobalt_reliability_lds_bins())


def _vector(t, name: str, dtype) -> None:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError(f"{name} must be a CUDA tensor")
    if t.dim() != 1 or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} vector, got {t.dtype} {tuple(t.shape)}")


def iso_hull(cw: torch.Tensor, cs: torch.Tensor, total_weight: int | None = None, *, return_rounds: bool = False):
    """int32 ascending indices of the strict lower convex hull of ``(cw[k], cs[k])`` (int64 ``[G + 1]`` CUDA
    vectors as ``metrics.calibration.iso_groups`` builds them), on the device of ``cw``: exactly
    ``iso_hull_host``'s list. ``total_weight`` is ``cw[-1]`` when the caller knows it (else it is read: one
    synchronisation); the read of the vertex count at the end is the only other one. ``return_rounds`` adds the
    survivor count after every tile round (None when the points fit one tile). ``ValueError`` before any launch."""
    _vector(cw, "cw", torch.int64)
    _vector(cs, "cs", torch.int64)
    if cs.device != cw.device or cs.shape != cw.shape:
        raise ValueError("cw and cs must be two vectors of one length on one device")
    m = int(cw.shape[0])
    if m < 2 or m - 1 > C.MAX_ROWS:
        raise ValueError(f"1 .. 2^28 groups, got {m - 1}")
    total = int(cw[-1]) if total_weight is None else int(total_weight)
    if total < 1 or total > C.MAX_TOTAL_WEIGHT:
        raise ValueError(f"total integer weight must lie in 1 .. 2^31 - 1, got {total}")
    dev = cw.device
    lib = _native.lib()
    with torch.cuda.device(dev):
        need = int(lib.cobalt_iso_hull_workspace_bytes(m))
        _native.check(min(need, 0), "cobalt_iso_hull_workspace_bytes")
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty(m, dtype=torch.int32, device=dev)
        cnt = torch.zeros(1 + iso_rounds(), dtype=torch.int32, device=dev)
        rc = lib.cobalt_iso_hull(cw.data_ptr(), cs.data_ptr(), m, total, work.data_ptr(), need, out.data_ptr(),
                                 cnt.data_ptr(), cnt[1:].data_ptr(), _native.stream_handle())
        _native.check(rc, "cobalt_iso_hull")
        counts = cnt.cpu().tolist()
    hull = out[:counts[0]]
    if return_rounds:
        return hull, (counts[1:] if m > iso_tile_rows() else None)
    return hull


def calib_apply(x: torch.Tensor, xk: torch.Tensor, vk: torch.Tensor) -> torch.Tensor:
    """float32 ``[N]``: the piecewise-linear function through the knots (``xk`` float32 ``[K]`` strictly
    increasing, ``vk`` float64 ``[K]``) at the float32 CUDA vector ``x``, bit-equal to
    ``metrics.calibration.calib_apply_host``. ``ValueError`` before any launch."""
    _vector(x, "x", torch.float32)
    _vector(xk, "xk", torch.float32)
    _vector(vk, "vk", torch.float64)
    if xk.device != x.device or vk.device != x.device:
        raise ValueError("x, xk and vk must be on one device")
    K = int(xk.shape[0])
    if K < 1 or vk.shape[0] != K:
        raise ValueError("xk and vk must be two vectors of K >= 1 knots")
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        rc = _native.lib().cobalt_calib_apply(x.data_ptr(), int(x.shape[0]), xk.data_ptr(), vk.data_ptr(), K,
                                              out.data_ptr(), _native.stream_handle())
    _native.check(rc, "cobalt_calib_apply")
    return out


def reliability_sums(p: torch.Tensor, y: torch.Tensor, wq: torch.Tensor | None, edges: torch.Tensor,
                     out: torch.Tensor | None = None, *, check: bool = True) -> torch.Tensor:
    """int64 ``[3, B]`` (``W``, ``S``, ``Pq``; ``metrics.calibration.reliability_sums_host`` is the definition) of
    the float32 CUDA probabilities ``p``, the float32 labels ``y`` (0 / 1), the int32 weights ``wq`` (in
    [0, 2^20]; None: 1 per row) and the ``B - 1`` float32 interior ``edges``, ADDED into ``out`` when one is
    passed (so a long vector can be fed in chunks; the caller keeps the total weight of all chunks at most
    2^31 - 1). ``check`` (one synchronisation) refuses NaN or out-of-range probabilities, labels other than 0 / 1,
    weights outside [0, 2^20], edges that are NaN or descend. ``ValueError`` before any launch."""
    _vector(p, "p", torch.float32)
    _vector(y, "y", torch.float32)
    _vector(edges, "edges", torch.float32)
    dev = p.device
    n, B = int(p.shape[0]), int(edges.shape[0]) + 1
    if y.shape[0] != n or y.device != dev or edges.device != dev:
        raise ValueError("p, y and edges must be on one device, p and y of one length")
    if wq is not None:
        _vector(wq, "wq", torch.int32)
        if wq.shape[0] != n or wq.device != dev:
            raise ValueError(f"wq must be int32 [{n}] on {dev}")
    if B > C.MAX_BINS:
        raise ValueError(f"at most {C.MAX_BINS} bins")
    if n > C.MAX_ROWS:
        raise ValueError(f"at most 2^28 rows ({n} given)")
    if out is not None:
        if (not isinstance(out, torch.Tensor) or out.shape != (3, B) or out.dtype != torch.int64 or out.device != dev
                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous int64 [3, {B}] on {dev}")
    if check and n:
        bad = [torch.isnan(p).any(), ((p < 0) | (p > 1)).any(), ((y != 0) & (y != 1)).any(),
               torch.isnan(edges).any() | (edges[1:] < edges[:-1]).any()]
        if wq is not None:
            bad.append(((wq < 0) | (wq > WEIGHT_SCALE)).any())
            bad.append(wq.sum(dtype=torch.int64) > C.MAX_TOTAL_WEIGHT)
        bad = torch.stack(bad).cpu().tolist()
        for flag, msg in zip(bad, ("NaN probabilities", "probabilities must lie in [0, 1]", "labels must be 0 or 1",
                                   "edges must be ascending and not NaN", "integer weights must lie in [0, 2^20]",
                                   "total integer weight above 2^31 - 1")):
            if flag:
                raise ValueError(msg)
    if out is None:
        out = torch.zeros((3, B), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = _native.lib().cobalt_reliability_sums(p.data_ptr(), y.data_ptr(), _native.ptr(wq), n, edges.data_ptr(),
                                                   B, out.data_ptr(), _native.stream_handle())
    _native.check(rc, "cobalt_reliability_sums")
    return out


# ------------------------------------------------------------------------------------- plumbing around the kernels
def _on(dev, x, dtype=None) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.reshape(-1).to(device=dev, dtype=dtype) if dtype is not None else t.reshape(-1).to(dev)


def iso_groups_gpu(score, y, wq=None):
    """``metrics.calibration.iso_groups`` on the device of the CUDA input: ``(ux float32 [G], cw int64 [G + 1],
    cs int64 [G + 1], total weight)``. The inputs are checked as the host path checks them."""
    dev = next(t.device for t in (score, y) if isinstance(t, torch.Tensor) and t.is_cuda)
    s = _on(dev, score, torch.float32)
    yv = _on(dev, y)
    n = int(s.shape[0])
    if yv.shape[0] != n:
        raise ValueError(f"{yv.shape[0]} labels, {n} scores")
    if n < 1:
        raise ValueError("empty input")
    if n > C.MAX_ROWS:
        raise ValueError(f"at most 2^28 rows ({n} given)")
    w = None
    if wq is not None:
        w = _on(dev, wq)
        if w.shape[0] != n:
            raise ValueError(f"{w.shape[0]} weights, {n} rows")
        if w.dtype.is_floating_point:
            raise ValueError("integer weights expected (quantize_weights)")
        w = w.to(torch.int64)
    flags = [((yv != 0) & (yv != 1)).any(), torch.isnan(s).any()]
    if w is not None:
        flags += [(w < 0).any(), w.max() > C.MAX_TOTAL_WEIGHT]
    sums = torch.stack([f.to(torch.int64) for f in flags] + ([w.clamp(0, C.MAX_TOTAL_WEIGHT + 1).sum()] if w is not None else []))
    sums = sums.cpu().tolist()
    if sums[0]:
        raise ValueError("labels must be 0 or 1")
    if sums[1]:
        raise ValueError("NaN scores")
    total = n
    if w is not None:
        if sums[2]:
            raise ValueError("negative weight")
        if sums[3] or sums[4] > C.MAX_TOTAL_WEIGHT:
            raise ValueError("total integer weight above 2^31 - 1")
        total = int(sums[4])
        keep = w > 0
        if not bool(keep.all()):
            s, yv, w = s[keep], yv[keep], w[keep]
            if s.shape[0] < 1:
                raise ValueError("every row has weight 0")
    ss, order = torch.sort(s, stable=True)
    pos = (yv[order] != 0).to(torch.int64)
    ws = w[order] if w is not None else None
    last = torch.ones(ss.shape[0], dtype=torch.bool, device=dev)   # the last row of every run of equal scores
    last[:-1] = ss[1:] != ss[:-1]
    ends = torch.nonzero(last).reshape(-1)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    if ws is None:
        cw = torch.cat([zero, ends + 1])
        cs = torch.cat([zero, torch.cumsum(pos, 0)[ends]])
    else:
        cw = torch.cat([zero, torch.cumsum(ws, 0)[ends]])
        cs = torch.cat([zero, torch.cumsum(ws * pos, 0)[ends]])
    return ss[ends].contiguous(), cw.contiguous(), cs.contiguous(), total


def iso_fit_gpu(score, y, wq=None):
    """The isotonic fit on the device: ``(xk float32 [K], vk float64 [K])`` as NumPy arrays, bit-equal to
    ``metrics.calibration.iso_fit_host``: the same integers, one fp64 division per block."""
    ux, cw, cs, total = iso_groups_gpu(score, y, wq)
    hull = iso_hull(cw, cs, total).to(torch.int64)
    first, last = hull[:-1], hull[1:] - 1
    vals = (cs[hull[1:]] - cs[hull[:-1]]).to(torch.float64) / (cw[hull[1:]] - cw[hull[:-1]]).to(torch.float64)
    return C.knots_from_blocks(ux[first].cpu().numpy(), ux[last].cpu().numpy(), first.cpu().numpy(),
                               last.cpu().numpy(), vals.cpu().numpy())


def reliability_report_gpu(y, p, wq, n_bins: int, strategy: str, edges=None):
    """``metrics.calibration.reliability_report`` for CUDA inputs: the edges from a device sort, the table from
    ``cobalt_reliability_sums``, the finishing arithmetic shared with the host path."""
    dev = next(t.device for t in (p, y) if isinstance(t, torch.Tensor) and t.is_cuda)
    pv = _on(dev, p, torch.float32).contiguous()
    yv = _on(dev, y, torch.float32).contiguous()
    n = int(pv.shape[0])
    if edges is not None:
        e = C.check_edges(C.edges_to_f32(edges.detach().cpu().numpy() if isinstance(edges, torch.Tensor) else edges))
        strategy = "custom"
    elif strategy == "quantile":
        if bool(torch.isnan(pv).any()):
            raise ValueError("NaN probabilities")
        srt = torch.sort(pv).values
        e = C.edges_for(strategy, n_bins, lambda i: srt[torch.as_tensor(i, device=dev)].cpu().numpy(), n)
    else:
        e = C.edges_for(strategy, n_bins)
    wt = None if wq is None else torch.as_tensor(np.asarray(wq), device=dev).to(torch.int32).contiguous()
    table = reliability_sums(pv, yv, wt, torch.as_tensor(e, device=dev).contiguous())
    return C.report_from_table(table.cpu().numpy(), e, n, strategy)
