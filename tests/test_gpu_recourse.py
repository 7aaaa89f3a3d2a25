"""The recourse scan kernel (csrc/recourse.hip) on the hand-built forests of scoring_forests.py, bit for bit (idx
and margin bits) against the plain-Python brute force of recourse_bruteforce.py (explicit substitution,
``predict_rowwise`` one row at a time, the slots picked from their definitions), and ``counterfactuals`` on the
GPU against the CPU report. Exact comparisons: no tolerance.

Which test catches which mistake in the kernel:
  ``<`` instead of ``<=`` in the position search ... test_value_edges (row values exactly on the candidates)
  a launch chunk without its row offset ............. test_launch_chunks (chunk rows + 1; X, idx and margin offsets)
  a dropped or folded chunk tail .................... test_candidate_counts (K + 1 = 1, 2, 15, 16, 17, 33 in one call),
                                                      test_windows_and_directions (windows that end mid-chunk)
  CSR offsets of the candidate table ................ test_candidate_counts (segments of different lengths)
  override at ``r * F + f`` (even F) ................ test_widths (F = 2, 8, 80 have F | 1 != F)
  rows past n walking or writing .................... test_rows (N = 1, 63, 65, 257; outputs sized exactly [N, A, 3])
  the own position reported, or the window ignored .. test_windows_and_directions (windows without c, empty windows)
  ``dir`` mixed up .................................. test_windows_and_directions (all three values, per feature)
  the slot-2 tie rule ............................... test_ties (equal minimal margins at different distances)
  tile staging per chunk ............................ test_multi_tile_and_prefix (64-node tiles, n_trees prefix)
  "tree ignores f" with the wrong feature ........... the kernel has no such shortcut; test_candidate_counts has a
                                                      feature every tree uses next to one none uses
"""
import functools

import numpy as np
import pytest
import torch

import recourse_bruteforce as bf
import scoring_forests as sf
from cobalt_smart_lender_ai_amd import _native, explain
from cobalt_smart_lender_ai_amd.models import gbdt
from cobalt_smart_lender_ai_amd.ops import predict_ops

pytestmark = pytest.mark.gpu

NEG_INF = np.float32(-np.inf)


def _chunk() -> int:
    return int(_native.lib().cobalt_recourse_chunk())


def _intervals(b, f, n_trees=None):
    return np.concatenate([[NEG_INF], b.split_values(f, n_trees)]).astype(np.float32)


def _gpu(b, Xd, feats, cands, win=None, dirs=None, target=0.0, n_trees=None):
    idx, m = predict_ops.recourse_scan_gpu(b, Xd, feats, cands, win=win, dirs=dirs, target_margin=target,
                                           n_trees=n_trees)
    assert idx.dtype == torch.int32 and m.dtype == torch.float32
    assert tuple(idx.shape) == tuple(m.shape) == (Xd.shape[0], len(feats), 3)
    return idx.cpu().numpy(), bf.bits_of(m.cpu().numpy())


def _check(b, X, feats, cands, label, win=None, dirs=None, target=0.0, n_trees=None):
    X = np.ascontiguousarray(X, np.float32)
    Xd = torch.from_numpy(X).cuda()
    idx, bits = _gpu(b, Xd, feats, cands, win, dirs, target, n_trees)
    want_idx, want_bits = bf.scan(b, X, feats, cands, win, dirs, target, n_trees)
    np.testing.assert_array_equal(idx, want_idx, err_msg=label)
    np.testing.assert_array_equal(bits, want_bits, err_msg=label)
    assert np.array_equal(Xd.cpu().numpy(), X, equal_nan=True), label  # X is never written
    return idx


def _normal_rows(rng, n, F, nan=0.05):
    X = rng.normal(size=(n, F)).astype(np.float32)
    X[rng.random(X.shape) < nan] = np.nan
    return X


def _split_stump(f, thr, left, right, default_left=0):
    nodes = sf._Nodes()
    nodes.split(0, f, thr, default_left)
    t = nodes.finish(np.random.default_rng(0))
    t.split_conditions[1], t.split_conditions[2] = np.float32(left), np.float32(right)
    return t


def _median_margin(b, X):
    return float(np.nanmedian(sf.predict_rowwise(b, X[:64])))


# ------------------------------------------------------------------------------------- rows
@functools.lru_cache(maxsize=None)
def _rows_case():
    rng = np.random.default_rng(11)
    F = 7
    b = sf.random_forest(rng, F, 6, 3)
    X = _normal_rows(rng, 257, F)
    feats = [3, 0, 6]
    cands = [_intervals(b, f) for f in feats]
    target = _median_margin(b, X)
    want = bf.scan(b, X, feats, cands, None, [0, 1, -1], target)
    for w in want:
        w.setflags(write=False)
    return b, X, feats, cands, target, want


@pytest.mark.parametrize("N", [1, 63, 65, 257])
def test_rows(N):
    b, X, feats, cands, target, (want_idx, want_bits) = _rows_case()
    idx, bits = _gpu(b, torch.from_numpy(X[:N].copy()).cuda(), feats, cands, None, [0, 1, -1], target)
    np.testing.assert_array_equal(idx, want_idx[:N])
    np.testing.assert_array_equal(bits, want_bits[:N])
    assert (idx[..., :2] >= 0).any() or N == 1


def test_launch_chunks():
    """chunk rows + 1 rows on a two-stump forest: the last row is a launch of its own. The rows repeat 251
    distinct ones (251 is prime: the chunk boundary falls inside a period), so the brute force scores 251."""
    n = int(_native.lib().cobalt_recourse_chunk_rows()) + 1
    rng = np.random.default_rng(12)
    b = sf.make_booster([_split_stump(0, 0.25, -0.5, 0.75, 1), _split_stump(1, -1.0, 0.5, -0.25, 0)], 2)
    base = sf.edge_rows(rng, 251, 2)
    base[-1] = (2.5, -1.5)                       # the row of the second launch: both moves exist
    X = base[np.arange(n) % 251]
    X[-1] = base[-1]
    feats, cands = [1, 0], [_intervals(b, 1), _intervals(b, 0)]
    idx = _check(b, X, feats, cands, "chunk rows + 1", target=float(np.float32(b.base_margin)) + 0.1)
    assert (idx[-1, :, 2] >= 0).all() and (idx[-1, :, :2] >= 0).any()


# ------------------------------------------------------------------------------- candidates
def test_candidate_counts():
    """K + 1 = 1, 2, 15, 16, 17, 33 candidates, one feature each, in one call (chunk 16): feature 0 is used by
    every tree, feature 1 by none."""
    assert _chunk() == 16
    rng = np.random.default_rng(13)
    F = 6
    trees = [sf.random_tree(rng, F, 4, cols=[0, 2, 3, 4, 5]) for _ in range(6)]
    for t in trees:
        t.split_indices[0] = 0                   # every root splits on feature 0
    b = sf.make_booster(trees, F)
    assert all(0 in sf.tree_features(t) and 1 not in sf.tree_features(t) for t in b.trees)
    sizes = {1: 1, 0: 2, 2: 15, 3: 16, 4: 17, 5: 33}
    feats = [1, 0, 2, 3, 4, 5]
    cands = []
    for f in feats:
        own = b.split_values(f)
        extra = rng.normal(size=64).astype(np.float32)
        vals = np.unique(np.concatenate([own, extra]))[: sizes[f] - 1] if sizes[f] > 1 else np.zeros(0, np.float32)
        cands.append(np.concatenate([[NEG_INF], np.sort(vals)]).astype(np.float32))
        assert len(cands[-1]) == sizes[f]
    X = _normal_rows(rng, 130, F)
    idx = _check(b, X, feats, cands, "mixed candidate counts", target=_median_margin(b, X))
    assert (idx[:, 0] == -1).all()               # one candidate: the row's own position
    assert (idx[:, 1:, 2] >= 0).any(axis=0).all()


@pytest.mark.parametrize("F", [2, 8, 80])
def test_widths(F):
    """F | 1 != F; F = 80 needs more than 64 KiB of LDS. The last and the first feature are scanned."""
    rng = np.random.default_rng(20 + F)
    b = sf.random_forest(rng, F, 10, 4)
    X = _normal_rows(rng, 65, F)
    feats = [F - 1, 0]
    _check(b, X, feats, [_intervals(b, f) for f in feats], f"F={F}", target=_median_margin(b, X))


def test_value_edges():
    """Rows drawn from edge_values(): every threshold (c follows ``<=``), its neighbours, below the first, above
    the last, +-inf, NaN, +-0, denormals; thresholds one ulp apart; default-left and default-right nodes."""
    rng = np.random.default_rng(30)
    F = 5
    b = sf.random_forest(rng, F, 10, 4, grid=sf.THRESHOLD_GRID)
    assert {int(d) for t in b.trees for d in t.default_left[~t.is_leaf]} == {0, 1}
    X = sf.edge_rows(rng, 70, F)
    feats = [2, 0, 4]
    cands = [_intervals(b, 2), np.sort(sf.THRESHOLD_GRID), _intervals(b, 4)]   # feature 0: no -inf, c = -1 exists
    assert (X[:, 0] < cands[1][0]).any() and np.isin(X[:, 2], cands[0]).any() and np.isnan(X[:, feats]).any()
    idx = _check(b, X, feats, cands, "edge values", target=_median_margin(b, X))
    assert (idx[np.isnan(X[:, 2]), 0] == -1).all()
    on = np.flatnonzero(np.isin(X[:, 2], cands[0][1:]))
    own = np.searchsorted(cands[0], X[on, 2], side="right") - 1
    assert (cands[0][own] == X[on, 2]).all() and (idx[on, 0] != own[:, None]).all()


def test_windows_and_directions():
    rng = np.random.default_rng(40)
    F = 4
    b = sf.random_forest(rng, F, 8, 4)
    X = _normal_rows(rng, 130, F)
    grid = np.sort(rng.normal(size=40).astype(np.float32))
    feats = [0, 1, 2, 3, 0, 1]
    cands = [grid] * 6
    # full; ends mid-chunk (19 candidates from 3); a window above most rows' own position; empty; one candidate; empty
    win = [(0, 39), (3, 21), (30, 39), (5, 4), (17, 17), (39, 0)]
    target = _median_margin(b, X)
    for dirs in ([0, 1, -1, 0, 0, 1], [-1, 0, 1, 1, -1, 0], [1, -1, 0, -1, 1, -1]):
        idx = _check(b, X, feats, cands, f"dirs={dirs}", win=win, dirs=dirs, target=target)
        assert (idx[:, 3] == -1).all() and (idx[:, 5] == -1).all()
        for a, d in enumerate(dirs):
            if d == 1:
                assert (idx[:, a, 0] == -1).all()
            if d == -1:
                assert (idx[:, a, 1] == -1).all()
    own = np.searchsorted(grid, X[:, 2], side="right") - 1
    assert (own < 30).any()                      # windows that exclude c


def test_ties():
    """x0 in {< 0, [0, 1), [1, 2), >= 2} -> leaf {1, 0, 1, 0}: from either "1" interval the two "0" intervals tie
    for the lowest margin; the nearer one wins, and at equal distance the lower one."""
    nodes = sf._Nodes()
    l, r = nodes.split(0, 0, 1.0, 0)
    ll, lr = nodes.split(l, 0, 0.0, 0)
    rl, rr = nodes.split(r, 0, 2.0, 0)
    t = nodes.finish(np.random.default_rng(0))
    for j, v in ((ll, 1.0), (lr, 0.0), (rl, 1.0), (rr, 0.0)):
        t.split_conditions[j] = np.float32(v)
    b = sf.make_booster([t, sf.stump(0.125)], 2, base_score=0.5)
    X = np.array([[-5.0, 0.0], [1.5, 0.0], [0.5, 0.0], [np.nan, 0.0]], np.float32)
    cands = [_intervals(b, 0)]                   # [-inf, 0, 1, 2]
    idx = _check(b, X, [0], cands, "ties", target=0.5)
    assert idx[0, 0, 2] == 1 and idx[1, 0, 2] == 1 and idx[2, 0, 2] == 3
    # five intervals 1 0 1 1 0 with the row in the middle one: the nearer of the two minima, not the later one
    wide = np.array([NEG_INF, 0.0, 1.0, 1.5, 2.0], np.float32)
    idx = _check(b, np.array([[1.2, 0.0]], np.float32), [0], [wide], "ties at equal distance", target=-9.0)
    assert idx[0, 0, 2] == 1 and (idx[0, 0, :2] == -1).all()


def test_multi_tile_and_prefix(monkeypatch):
    monkeypatch.setattr(predict_ops, "TILE_NODES", 64)
    rng = np.random.default_rng(50)
    F = 9
    b = sf.make_booster([sf.grown_tree(rng, F, 9, 7) for _ in range(11)], F)   # 17 nodes a tree: 3 per tile
    tiles = np.diff(predict_ops.pack_forest(b)[2])
    assert predict_ops.tile_capacity(b) == 64 and len(tiles) >= 3, tiles
    X = _normal_rows(rng, 130, F)
    feats = [4, 8, 0]
    seen = []
    for n_trees in (None, 11, 4, 1):
        cands = [_intervals(b, f) for f in feats]    # the whole model's candidates for every prefix
        seen.append(_check(b, X, feats, cands, f"n_trees={n_trees}", dirs=[0, -1, 1],
                           target=_median_margin(b, X), n_trees=n_trees))
    np.testing.assert_array_equal(seen[0], seen[1])
    assert not np.array_equal(seen[1], seen[2])


# ------------------------------------------------------------------------------ fitted model
def test_gpu_report_equals_cpu_report():
    rng = np.random.default_rng(5)
    n, F = 400, 5
    X = rng.normal(size=(n, F)).astype(np.float32)
    X[rng.random(X.shape) < 0.05] = np.nan
    Z = np.nan_to_num(X)
    y = (Z[:, 0] - 0.8 * Z[:, 1] + 0.6 * Z[:, 2] * Z[:, 3] + 0.5 * rng.normal(size=n) > 0).astype(np.float32)
    b = gbdt.GBDTClassifier(n_estimators=10, max_depth=3, learning_rate=0.3, device="cpu").fit(X, y).get_booster()
    Xd = torch.from_numpy(X).cuda()
    for max_changes in (1, 2):
        for kw in ({}, {"increase_only": (0,), "decrease_only": (1,), "bounds": {2: (-1.0, 1.0)}, "reference": X}):
            g = explain.counterfactuals(b, Xd, cutoff=0.3, max_changes=max_changes, **kw)
            c = explain.counterfactuals(b, X, cutoff=0.3, max_changes=max_changes, device="cpu", **kw)
            assert list(g.status) == list(c.status)
            np.testing.assert_array_equal(g.change_feature, c.change_feature)
            for name in ("change_from", "change_to", "margin_before", "margin_after"):
                np.testing.assert_array_equal(bf.bits_of(getattr(g, name)), bf.bits_of(getattr(c, name)), err_msg=name)
            np.testing.assert_array_equal(g.change_cost, c.change_cost)
            np.testing.assert_array_equal(g.total_cost, c.total_cost)
            assert g.to_records() == c.to_records()
            assert (c.status == "resolved").sum() >= 20
        if max_changes == 2:
            assert ((c.change_feature >= 0).sum(1) == 2).any()       # the greedy second round ran
    assert np.array_equal(Xd.cpu().numpy(), X, equal_nan=True)


# ------------------------------------------------------------------------------- entry point
def test_entry_point_refusals_and_empty_input():
    rng = np.random.default_rng(60)
    b = sf.random_forest(rng, 6, 3, 3)
    Xd = torch.zeros((8, 6), dtype=torch.float32, device="cuda")
    cands = [np.array([-1.0, 0.0, 1.0], np.float32)]
    with pytest.raises(ValueError, match="features"):
        predict_ops.recourse_scan_gpu(b, Xd[:, :5], [0], cands, target_margin=0.0)
    with pytest.raises(ValueError, match="float32"):
        predict_ops.recourse_scan_gpu(b, Xd.double(), [0], cands, target_margin=0.0)
    for bad in (dict(feats=[6]), dict(feats=[]), dict(cands=[cands[0][::-1].copy()]), dict(win=[(0, 3)]),
                dict(dirs=[2])):
        kw = dict(feats=[0], cands=cands, win=None, dirs=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            predict_ops.recourse_scan_gpu(b, Xd, kw["feats"], kw["cands"], win=kw["win"], dirs=kw["dirs"],
                                          target_margin=0.0)
    wide = sf.random_forest(rng, 144, 2, 3)      # 2048 * 8 + 256 * (144 | 1) * 4 bytes > 160 KiB
    with pytest.raises(RuntimeError, match="code -3"):
        predict_ops.recourse_scan_gpu(wide, torch.zeros((4, 144), dtype=torch.float32, device="cuda"), [0], cands,
                                      target_margin=0.0)
    # n = 0: accepted, nothing to launch
    idx, m = predict_ops.recourse_scan_gpu(b, Xd[:0], [0], cands, target_margin=0.0)
    assert tuple(idx.shape) == (0, 1, 3) and tuple(m.shape) == (0, 1, 3)
    # the entry point itself refuses what the wrapper checks first
    lib = _native.lib()
    gf = predict_ops.gpu_forest(b, Xd.device)
    table = np.array([0, 0, 3, 0, 2, 0], np.int32)           # feats | cand_ptr | win | dir for A = 1
    vals = torch.from_numpy(cands[0]).cuda()
    idx = torch.full((8, 1, 3), 7, dtype=torch.int32, device="cuda")
    m = torch.full((8, 1, 3), 7.0, dtype=torch.float32, device="cuda")

    def call(tab, A=1, n=8, n_cand=3, tile_cap=gf.tile_cap, F=6, val_ptr=vals.data_ptr()):
        tab = np.ascontiguousarray(tab, np.int32)
        dev = torch.from_numpy(tab).cuda()
        off = [0, 4 * A, 4 * (2 * A + 1), 4 * (4 * A + 1)]
        hp, dp = tab.ctypes.data, dev.data_ptr()
        rc = lib.cobalt_recourse_scan(Xd.data_ptr(), n, F, F, gf.nodes.data_ptr(), gf.tree_ptr.data_ptr(),
                                      gf.tile_ptr.data_ptr(), gf.n_tiles, tile_cap, 0.0, *(hp + o for o in off),
                                      dp + off[0], dp + off[1], val_ptr, n_cand, dp + off[2], dp + off[3], A, 0.0,
                                      idx.data_ptr(), m.data_ptr(), _native.stream_handle())
        torch.cuda.synchronize()
        return rc

    assert call(table, A=0) == -8
    assert call(table, A=65536) == -8
    assert call([6, 0, 3, 0, 2, 0]) == -8        # feature outside [0, F)
    assert call([-1, 0, 3, 0, 2, 0]) == -8
    assert call(table, val_ptr=None) == -8       # a null table
    assert call([0, 0, 3, 0, 3, 0]) == -8        # window past the segment
    assert call([0, 0, 3, -1, 1, 0]) == -8
    assert call([0, 0, 4, 0, 2, 0]) == -8        # segment past the table
    assert call([0, 0, 3, 0, 2, 2]) == -8        # direction
    assert call([0, 0, 3, 0, 2, -2]) == -8
    assert call(table, tile_cap=8193) == -2
    assert call(table, tile_cap=0) == -2
    assert call(table, F=144) == -3
    assert call(table, n=0) == 0
    assert bool((idx == 7).all()) and bool((m == 7.0).all())     # nothing was launched
    assert call([0, 0, 3, 2, 1, 0]) == 0         # an empty window is not an error: every result is empty
    assert bool((idx == -1).all()) and bool((m.view(torch.int32) == bf.EMPTY_BITS).all())
    assert call(table) == 0
    assert bool((idx[..., 2] >= 0).all())
