"""The scorecard kernels (csrc/scorecard.hip) against their host definitions (models/scorecard.py) at the smallest
shapes where each can still go wrong.

Which test catches which mistake:
  ``<=`` for ``<`` in the edge search, NaN / +-inf / -0 / denormals in the wrong cell ... test_encode
  the row stride taken for the width ................................................ test_encode_strided_view
  the f32 C/D lane map on the f64 MFMA, a swapped A / B operand, a wrong tile index ... test_newton_exact (torch.equal)
  rows past N, the tail of a 4-row step, the last chunk's bytes, empty waves ........ test_newton_exact (N = 1 .. 3 blocks + 3)
  a sigmoid that overflows or cancels ............................................... test_newton_general (+-40, +-800)
  an order of additions that depends on the run ..................................... test_newton_general (two calls)
  a margin added in another order, a tie in the reason codes ........................ test_score
"""
import functools

import numpy as np
import pytest
import torch

from cobalt_smart_lender_ai_amd.models import Scorecard
from cobalt_smart_lender_ai_amd.models import scorecard as S
from cobalt_smart_lender_ai_amd.monitor.drift import cell_pointer, drift_cell
from cobalt_smart_lender_ai_amd.ops import scorecard_ops as ops

from scorecard_cases import beta_distance_bound, lending_like, newton_bounds, newton_inputs

pytestmark = pytest.mark.gpu

F32 = np.float32
ENC_TILE = 512       # kScEncTileRows; test_limits checks both against the library
BLOCK_ROWS = 1024    # kScBlockChunks * 64


def _edges(rng, K):
    z = np.cumsum(rng.uniform(0.01, 1.0, size=K)).astype(F32)
    return z - F32(z[K // 2]) if K else z


def _planted(rng, n, edges):
    """[n, F] float32: edges, their two neighbouring floats, +-0 and denormals (every edge vector has the edge
    0.0), NaN and +-inf planted among uniform values."""
    zeros = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40], F32)
    cols = []
    for z in edges:
        lo, hi = (float(z[0]) - 1.0, float(z[-1]) + 1.0) if len(z) else (-1.0, 1.0)
        x = rng.uniform(lo, hi, size=n).astype(F32)
        kind = rng.integers(8, size=n)
        x = np.where(kind == 3, zeros[rng.integers(len(zeros), size=n)], x)
        if len(z):
            pick = z[rng.integers(len(z), size=n)]
            x = np.where(kind == 0, pick, x)
            x = np.where(kind == 1, np.nextafter(pick, F32(np.inf)), x)
            x = np.where(kind == 2, np.nextafter(pick, F32(-np.inf)), x)
        r = rng.random(n)
        x[r < 0.05] = np.nan
        x[(r >= 0.05) & (r < 0.06)] = np.inf
        x[(r >= 0.06) & (r < 0.07)] = -np.inf
        cols.append(x.astype(F32))
    return np.stack(cols, axis=1)


def _want_codes(X, edges):
    return np.stack([drift_cell(z, X[:, f]) for f, z in enumerate(edges)], axis=1).astype(np.uint8)


def test_limits():
    assert ops.encode_tile_rows() == ENC_TILE and ops.newton_block_rows() == BLOCK_ROWS
    assert ops.GPU_MAX_FEATURES == 63 and ops.GPU_MAX_CELLS == 8192


@pytest.mark.parametrize("F", [1, 15, 16, 17, 33, 63])
def test_encode(F):
    rng = np.random.default_rng(F)
    edges = [_edges(rng, int(k)) for k in rng.integers(0, 9, size=F)]
    edges[F // 2] = _edges(rng, 254)                           # 256 cells: the codes 254 and 255 are in use
    for n in (1, ENC_TILE - 1, ENC_TILE + 1, 2 * ENC_TILE + 1):
        X = _planted(rng, n, edges)
        got = ops.scorecard_encode(torch.from_numpy(X).cuda(), edges)
        assert got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(_want_codes(X, edges))), (F, n)


def test_encode_strided_view():
    rng = np.random.default_rng(7)
    edges = [_edges(rng, 5) for _ in range(4)]
    wide = torch.from_numpy(_planted(rng, 700, [_edges(rng, 5) for _ in range(3)] + edges + [_edges(rng, 5)])).cuda()
    view = wide[:, 3:7]
    assert not view.is_contiguous()
    got = ops.scorecard_encode(view, edges)
    assert torch.equal(got.cpu(), torch.from_numpy(_want_codes(view.cpu().numpy(), edges)))


def _gpu_pass(codes, ptr, tab, y, w, beta):
    return ops.scorecard_newton(torch.from_numpy(codes).cuda(), ptr, tab, torch.from_numpy(y).cuda(),
                                None if w is None else torch.from_numpy(w).cuda(), beta)


NEWTON_N = [1, 3, 4, 5, 63, 64, 65, BLOCK_ROWS + 1, 3 * BLOCK_ROWS + 3]


@pytest.mark.parametrize("P", [2, 16, 17, 32, 33, 64])
def test_newton_exact(P):
    """beta = 0 (p = q = 1/2), integer table and weights: every product and partial sum of grad and hess is an exact
    double, so any order of the additions gives the host's bits; a wrong lane map does not."""
    for N in NEWTON_N:
        args = newton_inputs(1000 * P + N, N, P - 1, exact=True)
        _, g0, H0 = S.scorecard_newton_host(*args)
        loss, g, H = _gpu_pass(*args)
        assert np.array_equal(g, g0), (P, N)
        assert np.array_equal(H, H0), (P, N)
        assert abs(loss - S.scorecard_newton_host(*args)[0]) <= newton_bounds(*args)[0], (P, N)


@pytest.mark.parametrize("P,N", [(2, 65), (21, 5), (21, 3 * BLOCK_ROWS + 3), (33, BLOCK_ROWS + 1), (64, 700)])
def test_newton_general(P, N):
    """|S_gpu - S_host| <= (N + 32) 2^-53 sum |t_i| per entry (scorecard_cases.newton_bounds), rows with margins
    about +-40 and +-800 among them; exactly symmetric; the same bits on a second call."""
    args = newton_inputs(7 * P + N, N, P - 1, extremes=True)
    l0, g0, H0 = S.scorecard_newton_host(*args)
    bl, bg, bh = newton_bounds(*args)
    loss, g, H = _gpu_pass(*args)
    print(f"P={P} N={N}: loss err {abs(loss - l0):.3e} (bound {bl:.3e}), grad err/bound "
          f"{np.max(np.abs(g - g0) / np.maximum(bg, 1e-300)):.3e}, hess err/bound "
          f"{np.max(np.abs(H - H0) / np.maximum(bh, 1e-300)):.3e}")
    assert np.isfinite(loss) and bool(np.isfinite(g).all()) and bool(np.isfinite(H).all())
    assert abs(loss - l0) <= bl
    assert bool((np.abs(g - g0) <= bg).all())
    assert bool((np.abs(H - H0) <= bh).all())
    assert np.array_equal(H, H.T) and bool((np.diag(H) >= 0.0).all())
    again = _gpu_pass(*args)
    assert again[0] == loss and np.array_equal(again[1], g) and np.array_equal(again[2], H)


def test_newton_unweighted_and_many_cells():
    """w = None is 1 per row; a table of 8192 cells (the limit: LDS above 64 KiB) still runs."""
    rng = np.random.default_rng(5)
    F, N = 32, 300
    ptr = cell_pointer([np.zeros(254, F32)] * F)
    codes = rng.integers(0, 256, size=(N, F)).astype(np.uint8)
    tab = rng.integers(-3, 4, size=int(ptr[-1])).astype(np.float64)
    y = (rng.random(N) < 0.5).astype(F32)
    _, g0, H0 = S.scorecard_newton_host(codes, ptr, tab, y, None, np.zeros(F + 1))
    _, g, H = _gpu_pass(codes, ptr, tab, y, None, np.zeros(F + 1))
    assert np.array_equal(g, g0) and np.array_equal(H, H0)


def test_limits_raise_before_any_launch(monkeypatch):
    from cobalt_smart_lender_ai_amd import _native

    calls = []
    real = _native.lib

    class Spy:
        def __getattr__(self, name):
            if name in ("cobalt_sc_encode", "cobalt_sc_newton", "cobalt_sc_score"):
                calls.append(name)
            return getattr(real(), name)

    monkeypatch.setattr(_native, "lib", lambda: Spy())
    X = torch.zeros((4, 64), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="63 features"):
        ops.scorecard_encode(X, [np.zeros(0, F32)] * 64)
    with pytest.raises(ValueError, match="63 features"):
        ops.scorecard_newton(torch.zeros((4, 64), dtype=torch.uint8, device="cuda"), np.arange(65) * 2,
                             np.zeros(128), torch.zeros(4).cuda(), None, np.zeros(65))
    with pytest.raises(ValueError, match="63 features"):
        Scorecard().fit(X, torch.tensor([0.0, 1.0, 0.0, 1.0]).cuda())
    wide = [np.arange(254, dtype=F32)] * 33                    # 33 * 256 = 8448 cells
    with pytest.raises(ValueError, match="8192 cells"):
        ops.scorecard_encode(X[:, :33], wide)
    with pytest.raises(ValueError, match="8192 cells"):
        ops.scorecard_newton(torch.zeros((4, 33), dtype=torch.uint8, device="cuda"), np.arange(34) * 256,
                             np.zeros(8448), torch.zeros(4).cuda(), None, np.zeros(34))
    with pytest.raises(ValueError, match="8192 cells"):
        ops.scorecard_score(X[:, :33], wide, 0.0, np.zeros(8448), np.zeros(8448, np.int32), np.zeros(8448), 2)
    assert calls == []


@functools.lru_cache(maxsize=None)
def _fits():
    X, y = lending_like(5000)
    host = Scorecard().fit(X, y)
    dev = Scorecard().fit(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda())
    return X, y, host, dev


def test_score():
    """Margins, integer scores and reason indices equal the host's bits: on the fitted model, and on a hand-made
    table with tied shortfalls, rows at every maximum and NaN inputs."""
    X, y, host, dev = _fits()
    Xd = torch.from_numpy(X).cuda()
    for top in (0, 1, 4, 8):
        args = (host.edges, float(host.beta[0]), host.contrib, np.concatenate(host.int_points), host.shortfall, top)
        m0, s0, r0 = S.scorecard_score_host(X, *args)
        m, s, r = ops.scorecard_score(Xd, *args)
        assert m.dtype == torch.float64 and torch.equal(m.cpu(), torch.from_numpy(m0))
        assert torch.equal(s.cpu(), torch.from_numpy(s0)) and torch.equal(r.cpu(), torch.from_numpy(r0))
    rng = np.random.default_rng(11)
    F = 9
    edges = [np.array([0.0], F32)] * F                          # cells: x <= 0, x > 0, NaN
    Xh = rng.normal(size=(ENC_TILE + 3, F)).astype(F32)
    Xh[rng.random(Xh.shape) < 0.2] = np.nan
    Xh[0] = -1.0                                                # every feature at its maximum: all -1
    Xh[1] = 1.0                                                 # every shortfall tied at 2.0
    short = np.tile(np.array([0.0, 2.0, 1.0]), F)
    short[3 * 4:3 * 4 + 3] = 0.0                                # a feature that never falls short
    contrib = rng.normal(size=3 * F)
    ipts = rng.integers(-50, 50, size=3 * F).astype(np.int32)
    for top in (3, 8):
        want = S.scorecard_score_host(Xh, edges, 0.25, contrib, ipts, short, top)
        got = ops.scorecard_score(torch.from_numpy(Xh).cuda(), edges, 0.25, contrib, ipts, short, top)
        for a, b in zip(got, want):
            assert torch.equal(a.cpu(), torch.from_numpy(b))
        assert want[2][0].tolist() == [-1] * top and want[2][1, :3].tolist() == [0, 1, 2]


def test_fit_on_the_device_matches_the_host():
    X, y, host, dev = _fits()
    assert all(np.array_equal(a, b) for a, b in zip(host.edges, dev.edges))
    assert all(np.array_equal(a, b) for a, b in zip(host.woe, dev.woe))
    assert all(np.array_equal(a, b) for a, b in zip(host.counts, dev.counts))
    assert host.dropped == dev.dropped == [False] * 5 + [True] and host.iv == dev.iv
    codes = S.scorecard_encode_host(X, host.edges)
    ptr, tab = host.cell_ptr, np.concatenate(host.woe)
    newton = lambda b: S.scorecard_newton_host(codes, ptr, tab, y, None, b)  # noqa: E731
    keep = np.arange(6)
    assert float(np.max(np.abs(newton(dev.beta)[1][keep]))) <= 2.0 * dev.gtol * len(y)
    bound = beta_distance_bound(newton, host.beta, dev.beta, keep)
    dist = float(np.max(np.abs(host.beta - dev.beta)))
    print(f"|beta_host - beta_gpu|_inf = {dist:.3e}, bound {bound:.3e}, passes {dev.fit_info['passes']}")
    assert dist <= bound
    # unrounded points differ by factor * (d beta_f woe + d beta_0 / F'): within factor * bound * (max |woe| + 1)
    wmax = max(float(np.max(np.abs(w))) for w in host.woe)
    for a, b in zip(host.points, dev.points):
        assert float(np.max(np.abs(a - b))) <= host.factor * bound * (wmax + 1.0)
    Xd = torch.from_numpy(X).cuda()
    assert np.array_equal(dev.decision_function(Xd), dev.decision_function(X))
    assert np.array_equal(dev.reasons(Xd), dev.reasons(X)) and np.array_equal(dev.score(Xd), dev.score(X))
