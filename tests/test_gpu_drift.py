"""The count kernel under the drift reports (csrc/bincount.hip) against its definition
(``monitor.drift.bin_counts_host``): int64 tables compared with ``torch.equal``, never a tolerance. Integer
accumulation has one right answer in any order.

Which test catches which mistake in the kernel:
  ``<=`` for ``<`` in the edge search, NaN or +-inf in the wrong cell .. test_counts (values on edges, one ulp off)
  a feature group that starts at the wrong edge or cell ................ test_counts (F = 107, K = 255: several groups)
  tail lanes of the last tile, a block without a full tile ............. test_counts (N = tile + 1, 2 tiles + 1)
  counters lost, or counted twice, between the tiles of one block ...... test_blocks_with_several_tiles
  a weighted block that does not flush after every tile (2^32 wraps) ... test_weighted_block_flushes_every_tile
  the 64-bit table behind the counters (sums beyond 2^32) .............. test_counter_wrap
  a device that flushes denormals, or tells -0.0 from 0.0 .............. test_counts (planted in every column)
  the row stride taken for the width ................................... test_strided_view
"""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from cobalt_smart_lender_ai_amd import _native, monitor
from cobalt_smart_lender_ai_amd.models import gbdt
from cobalt_smart_lender_ai_amd.monitor import drift as D
from cobalt_smart_lender_ai_amd.ops import monitor_ops

pytestmark = pytest.mark.gpu

F32 = np.float32
TILE = 2048          # kBinTileRows; test_limits checks it against the library
MAX_BLOCKS = 1024    # kBinMaxBlocksX


def _edges(rng, K):
    """K strictly increasing float32 edges around 0 (steps of at least 0.01, far above the spacing at 4096)."""
    z = np.cumsum(rng.uniform(0.01, 1.0, size=K)).astype(F32)
    return z - F32(z[K // 2]) if K else z


def _rows(rng, n, edges):
    """[n, F] float32: per cell an edge, its two neighbouring floats, a value in between, +-0 or a denormal
    (every edge vector of _edges has the edge 0.0), NaN or +-inf."""
    zeros = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40], F32)   # +-0, the smallest and a larger denormal
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
    X = np.stack(cols, axis=1)
    if X.shape[1] >= 3:
        X[:, 1] = np.nan                                     # an all-NaN column
    return X


def _check(X, edges, y=None, wq=None, label=""):
    want, _ = D.bin_counts_host(X, edges, y, wq)
    Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    yd = None if y is None else torch.from_numpy(y).cuda()
    wd = None if wq is None else torch.from_numpy(wq).cuda()
    got = monitor_ops.bin_counts_gpu(Xd, edges, y=yd, wq=wd)
    assert got.dtype == torch.int64 and got.is_cuda
    assert torch.equal(got.cpu(), torch.from_numpy(want)), label
    return got


# N, F, K per feature (cycled), labels, weights
CASES = [
    (1, 1, (0,), False, False),
    (63, 3, (1,), True, False),
    (65, 20, (9,), False, True),
    (257, 107, (255,), True, True),
    (65, 107, (255,), False, False),
    (257, 1, (4096,), False, False),
    (TILE + 1, 3, (4096,), True, True),
    (TILE + 1, 107, (9,), False, True),
    (2 * TILE + 1, 20, (0, 1, 9, 255), True, False),
    (2 * TILE + 1, 3, (9, 0, 4096), False, True),
]


@pytest.mark.parametrize("N,F,Ks,has_y,has_w", CASES)
def test_counts(N, F, Ks, has_y, has_w):
    rng = np.random.default_rng(N * 131 + F)
    edges = [_edges(rng, Ks[f % len(Ks)]) for f in range(F)]
    X = _rows(rng, N, edges)
    y = (rng.random(N) < 0.3).astype(F32) if has_y else None
    wq = rng.integers(0, (1 << 20) + 1, size=N) if has_w else None
    if has_w:
        wq[0] = 1 << 20
    if (F, Ks) == (107, (255,)):
        plan = monitor_ops.bin_counts_plan(edges, 2 if has_y else 1)
        assert plan[0] == 0 and plan[-1] == F and len(plan) - 1 >= 3, plan   # several feature groups
    _check(X, edges, y, wq, f"N={N} F={F} K={Ks}")


def test_limits():
    lib = _native.lib()
    assert int(lib.cobalt_bin_counts_tile_rows()) == TILE
    assert int(lib.cobalt_bin_counts_max_blocks()) == MAX_BLOCKS
    assert int(lib.cobalt_bin_counts_max_edges()) == monitor_ops.BIN_MAX_EDGES >= 4096
    assert TILE * monitor_ops.BIN_MAX_WEIGHT < 1 << 32          # a tile of maximum weights fits a 32-bit counter
    assert monitor_ops.bin_counts_plan([np.zeros(0, F32)] * 5, 1) == [0, 5]


@pytest.mark.parametrize("has_w", [False, True])
def test_blocks_with_several_tiles(has_w):
    """More tiles than blocks: every block walks two tiles, and no row is lost or counted twice at the seam.
    (The counters stay far from 2^32 here; the flush that keeps weighted ones there is
    test_weighted_block_flushes_every_tile's.)"""
    rng = np.random.default_rng(11)
    N = TILE * MAX_BLOCKS + 1
    edges = [_edges(rng, 9)]
    X = rng.uniform(-3, 3, size=(N, 1)).astype(F32)
    X[rng.random(N) < 0.01] = np.nan
    y = (rng.random(N) < 0.5).astype(F32)
    wq = rng.integers(0, (1 << 20) + 1, size=N) if has_w else None
    _check(X, edges, y, wq)


def test_weighted_block_flushes_every_tile():
    """Every row in one cell at the maximum weight 2^20, and blocks of five tiles: between two flushes a 32-bit
    counter may take one tile (2048 * 2^20 = 2^31). A block that kept its counters over its tiles would reach
    5 * 2^31 and wrap; the table is compared exactly, so that shows."""
    lib = _native.lib()
    tile, blocks = int(lib.cobalt_bin_counts_tile_rows()), int(lib.cobalt_bin_counts_max_blocks())
    N = 4 * tile * blocks + 1
    tiles = -(-N // tile)
    tiles_per_block = -(-tiles // blocks)
    assert tiles_per_block == 5 and tiles_per_block * tile * monitor_ops.BIN_MAX_WEIGHT >= 1 << 32
    X = np.full((N, 1), 0.25, F32)
    edges = [np.array([0.0, 1.0], F32)]
    wq = np.full(N, 1 << 20, np.int64)
    got = _check(X, edges, None, wq).cpu().numpy()
    np.testing.assert_array_equal(got, [[0, N << 20, 0, 0]])
    y = np.ones(N, F32)
    np.testing.assert_array_equal(_check(X, edges, y, wq).cpu().numpy(), [[0, 0, 0, 0], [0, N << 20, 0, 0]])


def test_signed_zeros_and_denormals():
    """-0.0 and 0.0 are one value, and denormal values and edges are compared as they are (nothing flushed)."""
    z = np.array([-1e-40, 0.0, 1e-45, 1.0], F32)
    x = np.array([-1e-38, -1e-40, -1e-45, -0.0, 0.0, 1e-45, 3e-45, 1e-40, 1.0], F32)
    want = np.array([0, 0, 1, 1, 1, 2, 3, 3, 3])
    np.testing.assert_array_equal(D.drift_cell(z, x), want)
    got = _check(x[:, None], [z]).cpu().numpy()
    np.testing.assert_array_equal(got[0], np.bincount(want, minlength=6))


def test_strided_view():
    rng = np.random.default_rng(12)
    edges = [_edges(rng, 9) for _ in range(20)]
    wide = torch.from_numpy(np.concatenate([rng.normal(size=(300, 3)).astype(F32), _rows(rng, 300, edges),
                                            rng.normal(size=(300, 7)).astype(F32)], axis=1)).cuda()
    view = wide[:, 3:23]
    assert not view.is_contiguous() and view.data_ptr() == wide.data_ptr() + 3 * 4 and view.stride(0) == 30
    got = monitor_ops.bin_counts_gpu(view, edges)
    want, _ = D.bin_counts_host(view.cpu().numpy(), edges)
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_counter_wrap():
    """70,000 rows of one value, every weight 2^20: the cell's sum, 7.3e10, is far beyond 2^32. Every block has
    one tile here, so this is the 64-bit table and a full tile of maximum weights in one counter (2^31)."""
    N = 70_000
    X = np.full((N, 2), 0.25, F32)
    edges = [np.array([-1.0, 0.0, 1.0], F32), np.array([0.25], F32)]
    wq = np.full(N, 1 << 20, np.int64)
    got = _check(X, edges, None, wq).cpu().numpy()
    assert got[0, 2] == N << 20 > 1 << 32 and got[0, 5] == N << 20 and got.sum() == 2 * (N << 20)
    y = np.ones(N, F32)
    assert _check(X, edges, y, wq).cpu().numpy()[1, 2] == N << 20


def test_one_hot_columns_conserve_every_sum():
    rng = np.random.default_rng(13)
    N, F = (1 << 16) + 1, 20
    X = (rng.random((N, F)) < 0.1).astype(F32)
    y = (rng.random(N) < 0.2).astype(F32)
    edges = [D.drift_edges(X[:, f]) for f in range(F)]
    assert all(len(z) == 1 for z in edges)
    got = _check(X, edges, y, None).cpu().numpy()
    per = got.reshape(2, F, 3)
    assert (per.sum(2) == np.array([[(y <= 0.5).sum()], [(y > 0.5).sum()]])).all()
    np.testing.assert_array_equal(per[:, :, 1].sum(0), X.sum(0).astype(np.int64))


def test_two_runs_agree_and_out_is_added_to():
    rng = np.random.default_rng(14)
    edges = [_edges(rng, k) for k in (9, 255, 0, 1)]
    X = _rows(rng, 3 * TILE + 5, edges)
    y = (rng.random(X.shape[0]) < 0.4).astype(F32)
    wq = rng.integers(0, 1 << 20, size=X.shape[0])
    a = _check(X, edges, y, wq)
    b = _check(X, edges, y, wq)
    assert torch.equal(a, b)
    out = torch.full_like(a, 7)
    back = monitor_ops.bin_counts_gpu(torch.from_numpy(X).cuda(), edges, y=torch.from_numpy(y).cuda(),
                                      wq=torch.from_numpy(wq).cuda(), out=out)
    assert back is out and torch.equal(out, a + 7)
    half = X.shape[0] // 2                                         # a streaming caller: two calls, one table
    acc = torch.zeros_like(a)
    for s in (slice(0, half), slice(half, None)):
        monitor_ops.bin_counts_gpu(torch.from_numpy(X[s]).cuda(), edges, y=torch.from_numpy(y[s]).cuda(),
                                   wq=torch.from_numpy(wq[s]).cuda(), out=acc)
    assert torch.equal(acc, a)


def test_refusals_leave_counts_untouched():
    """Every refusal is a return code before any launch; nothing is provoked on the device."""
    lib = _native.lib()
    X = torch.zeros((8, 4), dtype=torch.float32, device="cuda")
    ptr = np.array([0, 3, 6, 9, 12], np.int32)                     # four features of one edge each
    pd = torch.from_numpy(ptr).cuda()
    ed = torch.zeros(4, dtype=torch.float32, device="cuda")
    counts = torch.full((1, 12), 5, dtype=torch.int64, device="cuda")
    wide = np.array([0, 4099], np.int32)                           # one feature of 4097 edges
    bad0 = np.array([1, 4, 7, 10, 13], np.int32)
    thin = np.array([0, 3, 4, 7, 10], np.int32)                    # a feature of one cell

    def call(n=8, F=4, ldx=4, host=ptr, out=counts.data_ptr(), Xp=X.data_ptr()):
        return int(lib.cobalt_bin_counts(Xp, n, F, ldx, ed.data_ptr(), host.ctypes.data, pd.data_ptr(), None, None,
                                         out, _native.stream_handle()))

    assert call(F=0) == -1
    assert call(ldx=3) == -2
    assert call(n=-1) == -3
    assert call(out=None) == -4
    assert call(F=1, ldx=4, host=wide) == -5
    assert call(host=bad0) == -5 and call(host=thin) == -5
    codes = {call(F=0), call(ldx=3), call(n=-1), call(out=None), call(F=1, host=wide)}
    assert len(codes) == 5 and all(c < 0 for c in codes)
    assert call(n=0) == 0                                          # a successful no-op
    torch.cuda.synchronize()
    assert bool((counts == 5).all())
    assert call() == 0                                             # the same arguments, unrefused, do count
    torch.cuda.synchronize()
    assert int(counts.sum()) == 12 * 5 + 8 * 4
    Xd = torch.zeros((4, 1), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        monitor_ops.bin_counts_gpu(Xd, [np.arange(4097, dtype=F32)])
    with pytest.raises(ValueError):
        monitor_ops.bin_counts_gpu(Xd, [np.array([1.0, 1.0], F32)])
    with pytest.raises(ValueError):
        monitor_ops.bin_counts_gpu(Xd, [np.zeros(0, F32)], wq=torch.full((4,), (1 << 20) + 1, device="cuda"))
    with pytest.raises(ValueError):
        monitor_ops.bin_counts_gpu(Xd.cpu(), [np.zeros(0, F32)])


# ------------------------------------------------------------------------------------ public path
@functools.lru_cache(maxsize=None)
def _fitted():
    rng = np.random.default_rng(21)
    X = rng.normal(size=(600, 6)).astype(F32)
    X[rng.random(X.shape) < 0.05] = np.nan
    y = (np.nan_to_num(X[:, 0]) - 0.7 * np.nan_to_num(X[:, 2]) + 0.4 * rng.normal(size=600) > 0).astype(F32)
    b = gbdt.train(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda(),
                   gbdt.GBDTParams(n_estimators=5, max_depth=3, learning_rate=0.3), device="cuda")
    return b, X, y


def _same(a, b):
    assert json.dumps(a.to_dict(), sort_keys=True) == json.dumps(b.to_dict(), sort_keys=True)


def test_device_report_equals_host_report():
    b, X, y = _fitted()
    rng = np.random.default_rng(22)
    Xc = X.copy()                      # the same rows and weights: an untouched column has PSI exactly 0
    Xc[:, 0] += F32(0.8)
    Xc[:, 3] *= F32(1.5)
    w = rng.uniform(0.5, 2.0, size=600)
    host = monitor.DriftBaseline.fit(X, model=b, n_bins=10, y=y, sample_weight=w)
    dev = monitor.DriftBaseline.fit(torch.from_numpy(X).cuda(), model=b, n_bins=10, y=torch.from_numpy(y).cuda(),
                                    sample_weight=w)
    np.testing.assert_array_equal(host.ref_counts, dev.ref_counts)
    assert all(z0.tobytes() == z1.tobytes() for z0, z1 in zip(host.edges, dev.edges))
    rh = host.compare(Xc, y=y, sample_weight=w)
    rd = dev.compare(torch.from_numpy(Xc).cuda(), y=y, sample_weight=w)
    _same(rh, rd)
    assert rd.rows[0]["feature"] == "score" and rd.rows[0]["psi"] > 0
    assert rd["f0"]["status"] == "shifted" and rd["f1"]["psi"] == 0.0
    acc = dev.accumulator()
    for s in range(0, 600, 250):
        acc.update(torch.from_numpy(Xc[s:s + 250]).cuda(), y=y[s:s + 250])
    _same(acc.report(), host.compare(Xc, y=y))
    with pytest.raises(ValueError):
        acc.update(Xc[:10], y=y[:10])                # a host chunk after device chunks: one place only


def test_device_information_value_equals_host():
    _, X, y = _fitted()
    th = monitor.information_value(X, y, n_bins=8)
    td = monitor.information_value(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda(), n_bins=8)
    assert [r["feature"] for r in th] == [r["feature"] for r in td]
    for a, c in zip(th, td):
        assert a["iv"] == c["iv"] and np.array_equal(a["woe"], c["woe"]) and np.array_equal(a["counts"], c["counts"])
    assert th[0]["feature"] in ("f0", "f2")
