"""The bootstrap kernels (csrc/bootstrap.hip) against their definition (``metrics.bootstrap.bootstrap_sums_host``):
the int64 sums ``P N U2 KSn TP FP`` of every replicate compared with ``torch.equal``, never a tolerance. Every
rank metric is a ratio of exact integers, so there is one right answer.

Which test catches which mistake in the kernel:
  a Philox round, key bump or output word off; thresholds off by one .... test_sums (every count enters P, N)
  counts taken from the sorted position instead of the original row ....... test_sums (scores are shuffled rows)
  tail rows of the last tile; a tile of one row; n below one tile .......... test_sums (n = 1, 3, TILE - 1 .. 3 TILE + 5)
  replicates past B written or read; the last thread's partial four ........ test_sums (B = 1, 3, 4, 5; block edge +-1)
  blockIdx.y taken for the wrong replicate offset ........................... test_sums (B = block + 1), test_window
  a group that spans tiles closed early, late or twice (AUC stitch) ........ test_tie_layouts (one group, 3 TILE group)
  head / middle / tail split wrong when a start is a tile's first or last row test_tie_layouts (first_last, only_last)
  Lm without the negatives below, or 2 Pm Ncl forgotten ..................... test_tie_layouts (distinct), test_sums
  KS offset or sign wrong; a group end skipped at a tile boundary .......... test_tie_layouts (distinct, first_last)
  a division or a wrap on a replicate with P = 0 or N = 0 ................... test_tie_layouts (all_positive)
  fp64 sums out of row order, or accumulated in fp32 ........................ test_float_sums
  state left in the workspace, uninitialised records ........................ test_repeat_is_bit_identical
  the default stream used instead of the current one ........................ test_non_default_stream
  a launch before the arguments are checked ................................. test_refusals
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from cobalt_smart_lender_ai_amd import _native, metrics
from cobalt_smart_lender_ai_amd.metrics import bootstrap as B
from cobalt_smart_lender_ai_amd.ops import metrics_ops

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x9e3779b97f4a7c15


@functools.lru_cache(maxsize=None)
def _tile() -> int:
    return metrics_ops.bootstrap_tile_rows()


@functools.lru_cache(maxsize=None)
def _block() -> int:
    return metrics_ops.bootstrap_block_reps()


def _device_sums(y, s, reps, threshold=0.5, seed=SEED, **kw):
    words, order = metrics_ops.rank_words_gpu(torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda(), threshold)
    return metrics_ops.bootstrap_sums_gpu(words, reps, seed, **kw), order


def _host_sums(y, s, reps, threshold=0.5, seed=SEED, terms=None):
    rs = B.rank_structure(y, s, threshold)
    return B.bootstrap_sums_host(rs, B.bootstrap_counts_host(seed, rs.n, reps), terms)


N_CASES = ("1", "3", "TILE-1", "TILE", "TILE+1", "3*TILE+5")
B_CASES = ("1", "3", "4", "5", "BLOCK-1", "BLOCK", "BLOCK+1")


def _size(expr: str) -> int:
    return int(eval(expr, {"TILE": _tile(), "BLOCK": _block()}))


@functools.lru_cache(maxsize=None)
def _case(n_expr: str):
    """Labels, scores with many ties (two decimals) and the host sums of BLOCK + 1 replicates, computed once per
    n: replicate b does not depend on how many replicates are asked for."""
    n = _size(n_expr)
    rng = np.random.default_rng(n)
    y = rng.integers(0, 2, size=n)
    s = np.round(0.25 * y + 0.75 * rng.random(n), 2).astype(F32)
    want, _ = _host_sums(y, s, _block() + 1)
    return y, s, torch.from_numpy(want)


@pytest.mark.parametrize("b_expr", B_CASES)
@pytest.mark.parametrize("n_expr", N_CASES)
def test_sums(n_expr, b_expr):
    y, s, want = _case(n_expr)
    reps = _size(b_expr)
    (got, _), _ = _device_sums(y, s, reps)
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (len(B.FIELDS), reps)
    assert torch.equal(got.cpu(), want[:, :reps].contiguous())


def test_window_of_replicates():
    """rep0: replicates 8 .. 8 + 6 of a longer run, as the wrapper's chunks ask for them."""
    y, s, want = _case("TILE+1")
    (got, _), _ = _device_sums(y, s, 7, rep0=8)
    assert torch.equal(got.cpu(), want[:, 8:15].contiguous())
    (no_ks, _), _ = _device_sums(y, s, 7, rep0=8, ks=False)
    keep = [0, 1, 2, 4, 5]
    assert torch.equal(no_ks[keep], got[keep]) and int(no_ks[3].abs().sum()) == 0


def _layout(name: str):
    T = _tile()
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "all_equal":                       # one group across every tile
        s = np.full(4 * T + 3, 0.7, F32)
    elif name == "group_of_3_tiles":              # exactly 3 TILE equal rows starting on a tile boundary
        s = np.concatenate([np.arange(T) / (4.0 * T), np.full(3 * T, 0.5), 0.6 + np.arange(T // 2) / (4.0 * T)])
    elif name == "first_last":                    # a start on a tile's first row and one on its last row
        s = np.concatenate([np.full(T, 0.1), [0.2], np.full(T - 2, 0.3), [0.4], np.full(7, 0.4)])
    elif name == "only_last":                     # tile 1's only start is its last row
        s = np.concatenate([np.full(2 * T - 1, 0.1), np.full(T, 0.9)])
    elif name == "distinct":
        s = np.arange(2 * T + 11) / (2.0 * T + 11)
    elif name == "all_positive":
        s = np.round(rng.random(T + 9), 1)
    else:
        raise KeyError(name)
    s = s.astype(F32)
    n = s.shape[0]
    y = np.ones(n, dtype=np.int64) if name == "all_positive" else rng.integers(0, 2, size=n)
    perm = rng.permutation(n)                     # the rows arrive unsorted: original index != sorted position
    return y[perm], s[perm]


@pytest.mark.parametrize("name", ["all_equal", "group_of_3_tiles", "first_last", "only_last", "distinct",
                                  "all_positive"])
def test_tie_layouts(name):
    y, s = _layout(name)
    T = _tile()
    starts = np.flatnonzero(B.rank_structure(y, s).start)
    if name == "all_equal":
        assert starts.tolist() == [0]
    elif name == "group_of_3_tiles":
        assert T in starts and 4 * T in starts and not ((starts > T) & (starts < 4 * T)).any()
    elif name == "first_last":
        assert starts.tolist() == [0, T, T + 1, 2 * T - 1]
    elif name == "only_last":
        assert starts.tolist() == [0, 2 * T - 1]
    reps = 9
    want, _ = _host_sums(y, s, reps, threshold=0.35)
    (got, _), _ = _device_sums(y, s, reps, threshold=0.35)
    assert torch.equal(got.cpu(), torch.from_numpy(want)), name
    unit, _ = _device_sums(y, s, 1, threshold=0.35, unit=True)          # the point estimate: every count 1
    one, _ = B.bootstrap_sums_host(B.rank_structure(y, s, 0.35), np.ones((1, len(y)), np.uint8))
    assert torch.equal(unit[0].cpu(), torch.from_numpy(one)), name
    if name == "all_positive":
        assert int(got[1].abs().sum()) == 0 and int(got[2].abs().sum()) == 0 and int(got[3].abs().sum()) == 0
        m = B.metrics_from_sums(got.cpu().numpy(), np.zeros((2, reps)), ("auc", "ks", "recall"))
        assert np.isnan(m["auc"]).all() and np.isnan(m["ks"]).all() and not np.isnan(m["recall"]).any()


def test_float_sums():
    """Device and host, each within the sequential-sum bound (P + N) 2^-52 sum c |t| of math.fsum."""
    n, reps = _tile() + 37, 5
    rng = np.random.default_rng(21)
    y = rng.integers(0, 2, size=n)
    s = np.clip(0.3 * y + 0.7 * rng.random(n), 0, 1).astype(F32)
    s[:4] = [0.0, 1.0, 0.5, 0.5]                                        # clamped logloss terms
    terms = B.loss_terms(y, s)
    host_i, host_f = _host_sums(y, s, reps, terms=terms)
    words, order = metrics_ops.rank_words_gpu(torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda())
    td = torch.from_numpy(terms).cuda()[:, order].contiguous()
    dev_i, dev_f = metrics_ops.bootstrap_sums_gpu(words, reps, SEED, terms=td)
    assert torch.equal(dev_i.cpu(), torch.from_numpy(host_i))
    dev_f = dev_f.cpu().numpy()
    counts = B.bootstrap_counts_host(SEED, n, reps).astype(np.float64)
    for k in range(2):
        for b in range(reps):
            exact = math.fsum(counts[b] * terms[k])
            bound = float(host_i[0, b] + host_i[1, b]) * 2.0 ** -52 * math.fsum(counts[b] * np.abs(terms[k]))
            print(f"term {k} replicate {b}: device off by {abs(dev_f[k, b] - exact):.3e}, host by "
                  f"{abs(host_f[k, b] - exact):.3e}, bound {bound:.3e}")
            assert abs(dev_f[k, b] - exact) <= bound
            assert abs(host_f[k, b] - exact) <= bound
    none_i, none_f = metrics_ops.bootstrap_sums_gpu(words, reps, SEED)
    assert torch.equal(none_i, dev_i) and float(none_f.abs().sum()) == 0.0


def test_repeat_is_bit_identical():
    y, s, _ = _case("3*TILE+5")
    words, order = metrics_ops.rank_words_gpu(torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda())
    td = torch.from_numpy(B.loss_terms(y, s)).cuda()[:, order].contiguous()
    a_i, a_f = metrics_ops.bootstrap_sums_gpu(words, 37, SEED, terms=td)
    b_i, b_f = metrics_ops.bootstrap_sums_gpu(words, 37, SEED, terms=td)
    assert torch.equal(a_i, b_i) and torch.equal(a_f.view(torch.int64), b_f.view(torch.int64))
    c_i, _ = metrics_ops.bootstrap_sums_gpu(words, 37, SEED + 1, terms=td)
    assert not torch.equal(a_i, c_i)


def test_non_default_stream():
    y, s, want = _case("TILE+1")
    words, _ = metrics_ops.rank_words_gpu(torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda())
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got, _ = metrics_ops.bootstrap_sums_gpu(words, 6, SEED)
    stream.synchronize()
    assert torch.equal(got.cpu(), want[:, :6].contiguous())


def test_refusals():
    lib = _native.lib()
    assert lib.cobalt_bootstrap_tile_rows() == _tile() and _tile() >= 64
    assert _block() % 4 == 0 and lib.cobalt_bootstrap_out_fields() == len(B.FIELDS)
    assert lib.cobalt_bootstrap_max_rows() == B.MAX_ROWS == 1 << 28
    n, reps = 100, 8
    need = metrics_ops.bootstrap_workspace_bytes(n, reps, True, True)
    assert need > 0
    assert metrics_ops.bootstrap_workspace_bytes(0, reps, True, True) == -1
    assert metrics_ops.bootstrap_workspace_bytes((1 << 28) + 1, reps, True, True) == -2
    assert metrics_ops.bootstrap_workspace_bytes(n, 0, True, True) == -3
    words = torch.arange(n, dtype=torch.int32, device="cuda") | (1 << 29)
    terms = torch.ones((2, n), dtype=torch.float64, device="cuda")
    work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    out_i = torch.full((6, reps), -7, dtype=torch.int64, device="cuda")
    out_f = torch.full((2, reps), -7.0, dtype=torch.float64, device="cuda")
    st = _native.stream_handle()

    def call(words_p=words.data_ptr(), terms_p=terms.data_ptr(), n_=n, rep0=0, reps_=reps, flags=1,
             work_p=work.data_ptr(), bytes_=need, oi=out_i.data_ptr(), of=out_f.data_ptr(), ld=reps):
        return lib.cobalt_bootstrap(words_p, terms_p, n_, rep0, reps_, SEED, flags, work_p, bytes_, oi, of, ld, st)

    assert call(n_=0) == -1
    assert call(n_=(1 << 28) + 1) == -2
    assert call(reps_=0) == -3
    assert call(rep0=2) == -4 and call(rep0=-4) == -4
    assert call(words_p=None) == -5 and call(work_p=None) == -5 and call(oi=None) == -5
    assert call(bytes_=need - 1) == -6
    assert call(ld=reps - 1) == -7
    assert call(of=None) == -8
    assert call(flags=4) == -9
    torch.cuda.synchronize()
    assert int((out_i != -7).sum()) == 0 and int((out_f != -7.0).sum()) == 0 and int(work.sum()) == 0
    assert call() == 0                                                   # and the same arguments do run
    torch.cuda.synchronize()
    assert int((out_i == -7).sum()) == 0
    with pytest.raises(ValueError):
        metrics_ops.bootstrap_sums_gpu(words.cpu(), reps)
    with pytest.raises(ValueError):
        metrics_ops.bootstrap_sums_gpu(words, reps, rep0=2)
    with pytest.raises(ValueError, match="NaN"):
        metrics.bootstrap_ci(torch.ones(4).cuda(), torch.tensor([0.1, float("nan"), 0.2, 0.3]).cuda())
    with pytest.raises(ValueError, match="0 or 1"):
        metrics.bootstrap_ci(torch.tensor([0, 1, 2, 0]).cuda(), torch.rand(4).cuda())


@functools.lru_cache(maxsize=None)
def _synthetic():
    rng = np.random.default_rng(77)
    n = 5000
    y = (rng.random(n) < 0.2).astype(np.int64)
    a = np.round(1.0 / (1.0 + np.exp(-(1.5 * y - 1.2 + rng.normal(0, 1.0, n)))), 3).astype(F32)
    b = np.round(1.0 / (1.0 + np.exp(-(1.5 * y - 1.2 + rng.normal(0, 1.6, n)))), 3).astype(F32)
    return y, a, b


CI_METRICS = ("auc", "gini", "ks", "error", "precision", "recall")


@pytest.mark.parametrize("paired", [False, True])
def test_bootstrap_ci_matches_the_host_path(paired):
    y, a, b = _synthetic()
    kw = dict(metrics=CI_METRICS, n_boot=300, seed=5, alpha=0.1)
    host = metrics.bootstrap_ci(y, a, b if paired else None, **kw)
    yd, ad, bd = (torch.from_numpy(v).cuda() for v in (y, a, b))
    dev = metrics.bootstrap_ci(yd, ad, bd if paired else None, **kw)
    assert dev.to_dict() == host.to_dict()
    assert host["auc"].n_degenerate == 0 and host["auc"].low < host["auc"].point < host["auc"].high
    if paired:
        assert host.delta["auc"].share_le_zero < 0.05                    # a is the sharper model, by construction
        by_name = metrics.bootstrap_ci(y, a, b, device="cuda", **kw)     # host arrays sent to the GPU by name
        assert by_name.to_dict() == host.to_dict()
