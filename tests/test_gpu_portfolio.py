"""The portfolio kernels (csrc/portfolio.hip) against their definition (``portfolio.loss.portfolio_sums_host``):
the int64 loss and default counts of every segment and scenario compared with ``torch.equal``, never a tolerance.
Every step of a draw is integer arithmetic, so there is one right answer.

Which test catches which mistake in the kernel:
  a Philox round, key bump, output word or the domain word off ............ test_sums (every draw enters the sums)
  the counter taken from the tile position instead of the original index .. test_sums (the loans are shuffled)
  the table index, the fraction or the interpolation shift off ............. test_sums (PDs over four decades)
  tail rows of the last tile; a tile of one row; n below one tile .......... test_sums (n = 1, 3, TILE - 1 .. 3 TILE + 5)
  scenarios past S written or read; the last thread's partial four ......... test_sums (S = 1, 3, 4, 5; block edge +-1)
  blockIdx.y taken for the wrong scenario offset ............................ test_sums (S = BLOCK + 1), test_window
  the offsets of another sector or scenario; the LDS staging of A .......... test_sums (K = 3, 16; the last sector first)
  a tile shared by two segments; padding that defaults or carries a loss ... test_segments (1 loan, exactly a tile)
  a stitch that reads a neighbour's tiles or leaves an empty segment unset . test_segments (empty segments, G = 64)
  X not clamped at 0 or at 16 * 2^20; T[j + 1] read past the table ......... test_table_ends
  a 32-bit compare (thr = 2^32 wraps to 0: PD = 1 never defaults) .......... test_table_ends
  a 32-bit loss accumulator ................................................. test_table_ends (L = 2^32 - 1, a full tile)
  state left in the workspace, uninitialised records ........................ test_repeat_with_a_reused_workspace
  the default stream used instead of the current one ........................ test_non_default_stream
  a launch before the arguments are checked ................................. test_refusals
"""
import functools

import numpy as np
import pytest
import torch

from cobalt_smart_lender_ai_amd import _native, portfolio
from cobalt_smart_lender_ai_amd.ops import portfolio_ops
from cobalt_smart_lender_ai_amd.portfolio import loss as P
from portfolio_cases import SEED, book, heterogeneous_book, offsets

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _tile() -> int:
    return portfolio_ops.portfolio_tile_rows()


@functools.lru_cache(maxsize=None)
def _block() -> int:
    return portfolio_ops.portfolio_block_scenarios()


def _size(expr: str) -> int:
    return int(eval(expr, {"TILE": _tile(), "BLOCK": _block()}))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _device_sums(idx, Q, L, sector, A, seed=SEED, segment=None, n_segments=1, rep0=0):
    return portfolio_ops.portfolio_sums_gpu(
        _dev(idx, torch.int64), _dev(Q), _dev(L.astype(np.int64)), None if sector is None else _dev(sector, torch.int64),
        _dev(A), seed, segment=None if segment is None else _dev(segment, torch.int64), n_segments=n_segments,
        rep0=rep0)


N_CASES = ("1", "3", "TILE-1", "TILE", "TILE+1", "3*TILE+5")
S_CASES = ("1", "3", "4", "5", "BLOCK-1", "BLOCK", "BLOCK+1")


@functools.lru_cache(maxsize=None)
def _case(n_expr: str, K: int):
    """A shuffled book, the offsets and the host sums of BLOCK + 1 scenarios, computed once per (n, K): scenario s
    does not depend on how many scenarios are asked for."""
    idx, Q, L, sector, _, rho = book(_size(n_expr), K)
    A = offsets(rho, _block() + 1)
    want = P.portfolio_sums_host(idx, Q, L, sector, A, SEED)
    return (idx, Q, L, sector), A, torch.from_numpy(want)


@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("s_expr", S_CASES)
@pytest.mark.parametrize("n_expr", N_CASES)
def test_sums(n_expr, s_expr, K):
    loans, A, want = _case(n_expr, K)
    S = _size(s_expr)
    got = _device_sums(*loans, A[:S])
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (2, 1, S)
    assert torch.equal(got.cpu(), want[:, :, :S].contiguous())
    assert int(want[1].sum()) > 0 or _size(n_expr) < 4


@pytest.mark.parametrize("G", [1, 2, 64])
def test_segments(G):
    """G = 2: a segment of exactly one tile and a segment of one loan. G = 64: those two, empty segments (2 and 63
    among them) and the rest spread over the others."""
    T, S = _tile(), 9
    n = T + 1 if G == 2 else 3 * T + 77
    idx, Q, L, sector, _, rho = book(n, 3, seed=G)
    segment = np.zeros(n, dtype=np.int64)
    if G >= 2:
        segment[T] = 1
    if G == 64:
        segment[T + 1:] = np.random.default_rng(5).choice([3, 4, 7, 40, 62], size=n - T - 1)
    segment = segment[np.argsort(idx)]                                    # the tile's loans are not adjacent
    idx, Q, L, sector = (v[np.argsort(idx)] for v in (idx, Q, L, sector))
    A = offsets(rho, S)
    want = P.portfolio_sums_host(idx, Q, L, sector, A, SEED, segment=segment, n_segments=G)
    got = _device_sums(idx, Q, L, sector, A, segment=segment, n_segments=G)
    assert tuple(got.shape) == (2, G, S) and torch.equal(got.cpu(), torch.from_numpy(want))
    whole = _device_sums(idx, Q, L, sector, A)
    assert torch.equal(got.sum(dim=1), whole[:, 0])
    counts = np.bincount(segment, minlength=G)
    assert counts[0] == (n if G == 1 else T) and (G == 1 or counts[1] == 1)
    if G == 64:
        assert counts[2] == 0 and counts[63] == 0 and int(got[:, 2].abs().sum()) == 0 == int(got[:, 63].abs().sum())


def test_table_ends():
    T, S = _tile(), 6
    ones = np.ones(T, dtype=np.int64)
    top = np.full(T, (1 << 32) - 1, dtype=np.uint32)
    A = np.array([[0], [1 << 29], [-(1 << 29)], [12345], [-(1 << 29)], [1 << 29]], dtype=np.int32)
    always = _device_sums(np.arange(T), (ones << 30).astype(np.int32), top, None, A).cpu()
    assert (always[0, 0] == T * ((1 << 32) - 1)).all() and (always[1, 0] == T).all()     # X at 16 * 2^20: thr = 2^32
    never = _device_sums(np.arange(T), (-(ones << 30)).astype(np.int32), top, None, A).cpu()
    assert int(never.abs().sum()) == 0                                                      # X at 0: thr = 0
    # moderate probit points under offsets at their clamp: X clamps at both ends through A, not through Q
    Q = np.linspace(-3.0, 3.0, T) * (1 << 20)
    mid = _device_sums(np.arange(T), Q.astype(np.int32), top, None, A).cpu()
    assert torch.equal(mid, torch.from_numpy(P.portfolio_sums_host(np.arange(T), Q.astype(np.int32), top, None, A, SEED)))
    assert mid[1, 0, 1] == 0 and mid[1, 0, 2] == T and 0 < mid[1, 0, 0] < T
    # probit points one step inside the table's ends, where j + 1 is the last entry
    edge = np.concatenate([np.full(T // 2, (8 << 20) - 1), np.full(T - T // 2, -(8 << 20) + 1)]).astype(np.int32)
    got = _device_sums(np.arange(T), edge, top, None, A[:1]).cpu()
    assert torch.equal(got, torch.from_numpy(P.portfolio_sums_host(np.arange(T), edge, top, None, A[:1], SEED)))


@pytest.mark.parametrize("rep0", [4, 8])
def test_window_of_scenarios(rep0):
    loans, A, want = _case("TILE+1", 3)
    got = _device_sums(*loans, A[rep0:rep0 + 7], rep0=rep0)
    assert torch.equal(got.cpu(), want[:, :, rep0:rep0 + 7].contiguous())


def _raw(loans, A, G=1, segment=None):
    """The arguments of a direct call of cobalt_portfolio, as the wrapper builds them."""
    idx, Q, L, sector = loans
    n = len(idx)
    seg = torch.zeros(n, dtype=torch.int64, device="cuda") if segment is None else _dev(segment, torch.int64)
    recs, tile_seg = portfolio_ops.pack_loans(_dev(idx, torch.int64), _dev(Q), _dev(L.astype(np.int64)),
                                              _dev(sector, torch.int64), seg, G, _tile())
    table = _dev(np.array(P.threshold_table()))
    return recs, tile_seg, _dev(A), table


def test_repeat_with_a_reused_workspace():
    loans, A, want = _case("3*TILE+5", 3)
    S = 37
    recs, tile_seg, Ad, table = _raw(loans, A[:S])
    need = portfolio_ops.portfolio_workspace_bytes(recs.shape[0], S)
    work = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")   # never zeroed
    lib, st = _native.lib(), _native.stream_handle()

    def run(seed):
        out = torch.full((2, 1, S), -7, dtype=torch.int64, device="cuda")
        rc = lib.cobalt_portfolio(recs.data_ptr(), recs.shape[0], Ad.data_ptr(), 3, 2, table.data_ptr(),
                                  tile_seg.data_ptr(), 1, 0, S, seed, work.data_ptr(), need, out.data_ptr(), S, st)
        assert rc == 0
        return out

    a, other, b = run(SEED), run(SEED + 1), run(SEED)
    assert torch.equal(a, b) and not torch.equal(a, other)
    assert torch.equal(a.cpu(), want[:, :, :S].contiguous())


def test_non_default_stream():
    loans, A, want = _case("TILE+1", 3)
    args = [_dev(loans[0], torch.int64), _dev(loans[1]), _dev(loans[2].astype(np.int64)), _dev(loans[3], torch.int64),
            _dev(A[:6])]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = portfolio_ops.portfolio_sums_gpu(*args, SEED)
    stream.synchronize()
    assert torch.equal(got.cpu(), want[:, :, :6].contiguous())


def test_refusals():
    lib = _native.lib()
    assert lib.cobalt_portfolio_tile_rows() == _tile() and _tile() >= 64 and _block() % 4 == 0
    assert lib.cobalt_portfolio_max_rows() == P.MAX_LOANS == 1 << 28
    S, K, G = 8, 2, 3
    idx, Q, L, sector, _, rho = book(100, K)
    segment = np.arange(100) % 2                                          # segment 2 stays empty
    recs, tile_seg, A, table = _raw((idx, Q, L, sector), offsets(rho, S), G, segment)
    n = recs.shape[0]
    need = portfolio_ops.portfolio_workspace_bytes(n, S)
    assert need > 0
    assert portfolio_ops.portfolio_workspace_bytes(0, S) == -1
    assert portfolio_ops.portfolio_workspace_bytes((1 << 28) + 1, S) == -2
    assert portfolio_ops.portfolio_workspace_bytes(n, 0) == -3
    assert portfolio_ops.portfolio_workspace_bytes(n, (1 << 20) + 1) == -3
    work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    out = torch.full((2, G, S), -7, dtype=torch.int64, device="cuda")
    st = _native.stream_handle()
    bad_table = torch.tensor([0, 1, 1, 1], dtype=torch.int32)             # does not end at the number of tiles
    falling = torch.tensor([0, 2, 1, 2], dtype=torch.int32)

    def call(loans_p=recs.data_ptr(), n_=n, A_p=A.data_ptr(), K_=K, smax=K - 1, table_p=table.data_ptr(),
             seg_p=tile_seg.data_ptr(), G_=G, rep0=0, S_=S, work_p=work.data_ptr(), bytes_=need, out_p=out.data_ptr(),
             ld=S):
        return lib.cobalt_portfolio(loans_p, n_, A_p, K_, smax, table_p, seg_p, G_, rep0, S_, SEED, work_p, bytes_,
                                    out_p, ld, st)

    assert call(n_=0) == -1
    assert call(n_=(1 << 28) + 1) == -2
    assert call(S_=0) == -3 and call(S_=(1 << 20) + 1) == -3
    assert call(rep0=2) == -4 and call(rep0=-4) == -4
    assert call(loans_p=None) == -5 and call(A_p=None) == -5 and call(table_p=None) == -5
    assert call(seg_p=None) == -5 and call(work_p=None) == -5 and call(out_p=None) == -5
    assert call(bytes_=need - 1) == -6
    assert call(ld=S - 1) == -7
    assert call(K_=0) == -8 and call(K_=17) == -8
    assert call(G_=0) == -9 and call(G_=65) == -9
    assert call(smax=K) == -10 and call(smax=-1) == -10
    assert call(seg_p=bad_table.data_ptr()) == -11 and call(seg_p=falling.data_ptr()) == -11
    torch.cuda.synchronize()
    assert int((out != -7).sum()) == 0 and int(work.sum()) == 0
    assert call() == 0                                                    # and the same arguments do run
    torch.cuda.synchronize()
    assert int((out == -7).sum()) == 0
    want = P.portfolio_sums_host(idx, Q, L, sector, offsets(rho, S), SEED, segment=segment, n_segments=G)
    assert torch.equal(out.cpu(), torch.from_numpy(want))
    good = [_dev(idx, torch.int64), _dev(Q), _dev(L.astype(np.int64)), _dev(sector, torch.int64), A]
    with pytest.raises(ValueError):
        portfolio_ops.portfolio_sums_gpu(*(t.cpu() for t in good))
    for k, bad in ((0, good[0].to(torch.int32)), (1, good[1].to(torch.int64)), (2, good[2].to(torch.int32)),
                   (3, good[3] + K), (4, A.to(torch.int64)), (2, good[2] + (1 << 32)), (0, good[0][:50])):
        with pytest.raises(ValueError):
            portfolio_ops.portfolio_sums_gpu(*(bad if i == k else t for i, t in enumerate(good)))
    with pytest.raises(ValueError):
        portfolio_ops.portfolio_sums_gpu(*good, rep0=2)
    with pytest.raises(ValueError):
        portfolio_ops.portfolio_sums_gpu(*good, segment=good[3] + 1, n_segments=2)
    with pytest.raises(ValueError, match="PD"):
        portfolio.simulate_losses(torch.tensor([0.1, float("nan")]).cuda(), torch.ones(2).cuda())


def test_simulate_losses_matches_the_host_path():
    pd, ead, lgd, sector, grade = heterogeneous_book(3000)
    kw = dict(rho=[0.08, 0.15, 0.22], n_scenarios=1500, seed=5)
    host = portfolio.simulate_losses(pd, ead, lgd, sector=sector, segment=grade, **kw)
    code = np.unique(grade, return_inverse=True)[1]
    dev = portfolio.simulate_losses(_dev(pd), _dev(ead), _dev(lgd), sector=_dev(sector), segment=grade, **kw)
    assert dev.to_dict() == host.to_dict()
    by_code = portfolio.simulate_losses(_dev(pd), _dev(ead), _dev(lgd), sector=_dev(sector), segment=_dev(code), **kw)
    assert np.array_equal(by_code.sums, host.sums)
    by_name = portfolio.simulate_losses(pd, ead, lgd, sector=sector, segment=grade, device="cuda", **kw)
    assert by_name.to_dict() == host.to_dict()
    one = portfolio.simulate_losses(_dev(pd), _dev(ead), 0.6, rho=0.12, n_scenarios=64, seed=5)
    assert one.to_dict() == portfolio.simulate_losses(pd, ead, 0.6, rho=0.12, n_scenarios=64, seed=5).to_dict()
    assert one.asrf_var is not None and host.expected_loss > 0
