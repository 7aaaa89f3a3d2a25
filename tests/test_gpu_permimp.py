"""The permutation-importance kernel (csrc/permimp.hip) on the hand-built forests of scoring_forests.py and on
small fitted models.

Margins: bit for bit against ``scoring_forests.predict_rowwise`` (one row at a time, independent of the kernel
and of ``predict_margin_host``) on explicitly substituted copies of X; the one large N (a row-chunk boundary)
against ``predict_gpu`` on a ``torch.gather``-substituted matrix.

Sums: ``|sum_gpu - sum_exact| <= (N + 8) * 2^-52 * sum w|t|`` for each numerator (``t`` = the logloss or the
error term) and for ``sum w``, where ``sum_exact`` is the ``math.fsum`` of the terms computed in NumPy float64
from the GPU's own margins: the standard bound ``(N - 1) u sum|x_i|`` (u = 2^-53) of a floating-point sum of N
terms in any order, doubled, plus a few ulp for ``exp`` / ``log1p``. Derived, not measured; the tests print the
largest ratio to the bound they saw as ``[permimp] ...``. With unit weights the error sums are integers: exact.

Which test catches which mistake in the kernel:
  ``cols`` offset by the row chunk ........... test_row_chunk_boundary (perm maps rows across the boundary)
  a dropped or rescored repeat-chunk tail .... test_rows_and_repeats (R = chunk +- 1, 2 chunk + 1)
  jobs laid out as r * nf + i ................ test_rows_and_repeats, test_feature_subset (two / three features)
  substitution at ``r * F + f`` (even F) ..... test_widths (F = 2, 8, 80 have F | 1 != F)
  gather from X instead of cols .............. test_row_strided_and_wider_input (ldx > F)
  tail lanes contributing weight ............. test_sums (N = 65, 257 unweighted), test_tail_lanes_have_no_weight
  "tree ignores f" with the wrong feature .... the kernel has no such shortcut; test_unused_feature_is_exactly_zero
                                               and test_feature_subset would catch one
"""
import functools
import math

import numpy as np
import pytest
import torch

import scoring_forests as sf
from cobalt_smart_lender_ai_amd import _native, explain
from cobalt_smart_lender_ai_amd.models import booster as B
from cobalt_smart_lender_ai_amd.models import gbdt
from cobalt_smart_lender_ai_amd.ops import predict_ops

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------ helpers
def _chunk() -> int:
    return int(_native.lib().cobalt_perm_rep_chunk())


def _chunk_rows() -> int:
    return int(_native.lib().cobalt_perm_chunk_rows())


def _want(b, X, feats, perm, n_trees=None):
    """[1 + nf R, N]: predict_rowwise on X and on the copies of X for the jobs (i, r), job 1 + i R + r."""
    X = np.asarray(X, np.float32)
    mats = [X]
    for f in feats:
        for p in perm:
            Xs = X.copy()
            Xs[:, f] = X[p, f]
            mats.append(Xs)
    return sf.predict_rowwise(b, np.concatenate(mats), n_trees).reshape(len(mats), X.shape[0])


def _gpu(b, Xd, feats, perm, y=None, w=None, n_trees=None, margins=True, sums=False):
    dev = Xd.device
    m, s = predict_ops.permutation_scores_gpu(
        b, Xd, None if y is None else torch.as_tensor(y, device=dev), feats,
        torch.as_tensor(np.ascontiguousarray(perm, np.int32), device=dev), n_trees=n_trees,
        weights=None if w is None else torch.as_tensor(w, device=dev), want_margins=margins, want_sums=sums)
    return (None if m is None else m.cpu().numpy()), (None if s is None else s.cpu().numpy())


def _check_margins(b, X, feats, perm, label, n_trees=None):
    X = np.ascontiguousarray(X, np.float32)
    Xd = torch.from_numpy(X).cuda()
    got, _ = _gpu(b, Xd, feats, perm, n_trees=n_trees)
    want = _want(b, X, feats, perm, n_trees)
    assert got.dtype == np.float32 and got.shape == want.shape, (label, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=label)
    assert np.array_equal(Xd.cpu().numpy(), X, equal_nan=True), label  # X is never written
    return got


def _normal_rows(rng, n, F, nan=0.05):
    X = rng.normal(size=(n, F)).astype(np.float32)
    X[rng.random(X.shape) < nan] = np.nan
    return X


def _perms(rng, R, N):
    return np.stack([rng.permutation(N) for _ in range(R)]).astype(np.int32)


def _labels(rng, n):
    y = (rng.random(n) < 0.4).astype(np.float32)
    y[: min(n, 2)] = (0.0, 1.0)[: min(n, 2)]
    return y


def _sums_ratio(margins, sums, y, w):
    """Asserts the summation bound for every job's two numerators and for sum w; returns the largest
    |error| / bound."""
    J, N = margins.shape
    assert sums.shape == (2 * J + 1,)
    wd = np.ones(N) if w is None else np.asarray(w, np.float32).astype(np.float64)
    yd = np.asarray(y, np.float32).astype(np.float64)
    u = (N + 8) * 2.0 ** -52
    sw = math.fsum(wd)
    assert abs(sums[-1] - sw) <= u * sw
    worst = abs(sums[-1] - sw) / (u * sw)
    for k in range(J):
        m = margins[k].astype(np.float64)
        loss = np.log1p(np.exp(-np.abs(m))) + np.maximum(m, 0.0) - yd * m
        err = ((margins[k] > 0) != (np.asarray(y, np.float32) > np.float32(0.5))).astype(np.float64)
        for t, got in ((loss, sums[2 * k]), (err, sums[2 * k + 1])):
            exact = math.fsum(wd * t)
            bound = u * math.fsum(wd * np.abs(t))
            assert abs(got - exact) <= bound, (k, got, exact, bound)
            worst = max(worst, abs(got - exact) / bound if bound > 0 else 0.0)
        if w is None:
            assert sums[2 * k + 1] == float(err.sum())  # integers: exact
    return worst


# --------------------------------------------------------------------------- margins, bit for bit
@functools.lru_cache(maxsize=None)
def _rows_forest():
    rng = np.random.default_rng(11)
    return sf.random_forest(rng, 7, 4, 3), _normal_rows(rng, 257, 7)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257])
def test_rows_and_repeats(N):
    """Two features (the job index is 1 + i R + r) and R around the repeat chunk; job (i, r) depends on
    perm[r] only, so one reference at the largest R serves every shorter prefix."""
    b, X = _rows_forest()
    c = _chunk()
    rng = np.random.default_rng(100 + N)
    feats = (3, 0)
    Rmax = 2 * c + 1
    perm = _perms(rng, Rmax, N)
    want = _want(b, X[:N], feats, perm)
    Xd = torch.from_numpy(X[:N].copy()).cuda()
    for R in (1, c - 1, c, c + 1, Rmax):
        got, _ = _gpu(b, Xd, feats, perm[:R])
        assert got.shape == (1 + 2 * R, N)
        pick = [0] + [1 + i * Rmax + r for i in range(2) for r in range(R)]
        np.testing.assert_array_equal(got, want[pick], err_msg=f"N={N} R={R}")


def test_both_repeat_chunks(monkeypatch):
    """The kernel is built for 8 and for 16 repeats per block (``predict_ops.PERM_REP_CHUNK``; 0 = the
    default): the same margins and, bit for bit, the same sums, at R = 17 (blocks of 8 + 8 + 1 or 16 + 1)."""
    rng = np.random.default_rng(13)
    F, N, R = 5, 130, 17
    b = sf.random_forest(rng, F, 5, 3)
    X = _normal_rows(rng, N, F)
    Xd = torch.from_numpy(X).cuda()
    y = _labels(rng, N)
    w = rng.uniform(0.0, 2.0, size=N).astype(np.float32)
    perm = _perms(rng, R, N)
    want = _want(b, X, (4, 1), perm)
    seen = []
    for chunk in (8, 16, 0):
        monkeypatch.setattr(predict_ops, "PERM_REP_CHUNK", chunk)
        margins, sums = _gpu(b, Xd, (4, 1), perm, y=y, w=w, sums=True)
        np.testing.assert_array_equal(margins, want, err_msg=f"chunk={chunk}")
        _sums_ratio(margins, sums, y, w)
        seen.append(sums)
    np.testing.assert_array_equal(seen[0], seen[1])
    np.testing.assert_array_equal(seen[0], seen[2])


def test_row_chunk_boundary():
    """N = chunk_rows + 3: two launches. perm maps rows of the second chunk to rows of the first and back, so
    a cols pointer offset by the chunk's first row reads the wrong (or no) row."""
    N = _chunk_rows() + 3
    rng = np.random.default_rng(12)
    F = 4
    b = sf.random_forest(rng, F, 3, 3)
    Xd = torch.from_numpy(_normal_rows(rng, N, F)).cuda()
    keep = Xd.clone()
    perm = _perms(rng, 2, N)
    perm[0] = (np.arange(N) + N - 5) % N   # row n <- row n - 5: the second chunk reads the end of the first
    assert (perm[1][-3:] < N - 3).any() or (perm[1][: N - 3] >= N - 3).any()
    pd = torch.from_numpy(perm).cuda()
    feats = [2, 1]
    got, _ = predict_ops.permutation_scores_gpu(b, Xd, None, feats, pd, want_margins=True, want_sums=False)
    want = torch.empty_like(got)
    predict_ops.predict_gpu(b, Xd, out_margin=want[0])
    for i, f in enumerate(feats):
        for r in range(2):
            Xs = Xd.clone()
            Xs[:, f] = torch.gather(Xd[:, f], 0, pd[r].long())
            predict_ops.predict_gpu(b, Xs, out_margin=want[1 + i * 2 + r])
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(got[1], got[0])
    assert torch.equal(Xd.view(torch.int32), keep.view(torch.int32))


@pytest.mark.parametrize("F", [1, 2, 8, 80])
def test_widths(F):
    """Even and odd F | 1 (the staged row stride); F = 80 needs more than 64 KiB of LDS. The shuffled features
    are the last and the first (for F = 1 the only one)."""
    rng = np.random.default_rng(20 + F)
    b = sf.random_forest(rng, F, 6, 4)
    X = _normal_rows(rng, 65, F)
    _check_margins(b, X, (F - 1, 0) if F > 1 else (0,), _perms(rng, 3, 65), f"F={F}")


def test_feature_subset():
    """A strict subset, out of order, with the last column; one feature that every tree uses next to one that
    none uses (its jobs are the baseline, bit for bit)."""
    rng = np.random.default_rng(30)
    F = 6
    trees = [sf.random_tree(rng, F, 4, cols=[5]) for _ in range(3)]
    trees += [sf.caterpillar(rng, 4, [0, 2, 3, 5]) for _ in range(4)]
    trees += [sf.stump(0.125)]
    for t in trees[:-1]:
        assert 5 in sf.tree_features(t) and 1 not in sf.tree_features(t)
    b = sf.make_booster(trees, F)
    X = _normal_rows(rng, 130, F)
    got = _check_margins(b, X, (5, 1, 0), _perms(rng, 3, 130), "subset")
    for r in range(3):
        np.testing.assert_array_equal(got[1 + 3 + r], got[0])
    assert not np.array_equal(got[1], got[0])
    assert _gpu(b, torch.from_numpy(X).cuda(), (), _perms(rng, 2, 130))[0].shape == (1, 130)  # baseline only


# leaves per tree -> trees per 64-node tile (2 * leaves - 1 nodes each), as test_gpu_pdp.py
_TILE_CASES = {1: 32, 3: 11, 9: 4}


@pytest.mark.parametrize("per_tile", sorted(_TILE_CASES))
def test_tile_populations(per_tile, monkeypatch):
    """Tiles of 1, 3 and 9 trees (64-node tiles), at least three tiles, a smaller last one."""
    monkeypatch.setattr(predict_ops, "TILE_NODES", 64)
    rng = np.random.default_rng(40 + per_tile)
    F = 9
    n_trees = 2 * per_tile + max(1, per_tile - 2)
    b = sf.make_booster([sf.grown_tree(rng, F, _TILE_CASES[per_tile], 7) for _ in range(n_trees)], F)
    tiles = np.diff(predict_ops.pack_forest(b)[2])
    assert predict_ops.tile_capacity(b) == 64 and list(tiles[:2]) == [per_tile, per_tile] and len(tiles) >= 3, tiles
    assert tiles[-1] < per_tile or per_tile == 1
    X = _normal_rows(rng, 70, F)
    _check_margins(b, X, (4, 8), _perms(rng, 2, 70), f"{per_tile} trees per tile")


def test_tree_prefixes():
    rng = np.random.default_rng(60)
    b = sf.random_forest(rng, 6, 7, 4)
    X = _normal_rows(rng, 90, 6)
    perm = _perms(rng, 2, 90)
    seen = [_check_margins(b, X, (2,), perm, f"n_trees={n}", n) for n in (1, 2, 5, 7, None)]
    np.testing.assert_array_equal(seen[-1], seen[-2])
    assert not np.array_equal(seen[0], seen[1])


def test_row_strided_and_wider_input():
    rng = np.random.default_rng(70)
    F = 7
    b = sf.random_forest(rng, F, 6, 4)
    wide = _normal_rows(rng, 200, F + 5)
    Xd = torch.from_numpy(wide).cuda()
    view = Xd[:, :F]
    assert view.stride(0) == F + 5 and not view.is_contiguous()
    perm = _perms(rng, 3, 200)
    y = _labels(rng, 200)
    got, sums = _gpu(b, view, (6, 2), perm, y=y, sums=True)
    np.testing.assert_array_equal(got, _want(b, wide[:, :F], (6, 2), perm))
    _sums_ratio(got, sums, y, None)
    got2, _ = _gpu(b, Xd, (6, 2), perm)  # a matrix wider than the model: the extra columns are ignored
    np.testing.assert_array_equal(got2, got)
    assert np.array_equal(Xd.cpu().numpy(), wide, equal_nan=True)


def test_value_edges_and_repeated_rows():
    """Rows drawn from edge_values() (every threshold, its neighbours, +-inf, NaN, +-0, denormals): a swapped-in
    value equal to a threshold goes right, a swapped-in NaN takes the default direction. The second perm is
    not a bijection (rows drawn with replacement, row 0 for a whole stretch)."""
    rng = np.random.default_rng(80)
    F, N = 5, 70
    b = sf.random_forest(rng, F, 10, 4, grid=sf.THRESHOLD_GRID)
    X = sf.edge_rows(rng, N, F)
    assert np.isnan(X[:, 2]).any() and np.isinf(X[:, 2]).any()
    perm = _perms(rng, 3, N)
    perm[1] = rng.integers(0, N, size=N)
    perm[1][10:30] = 0
    perm[2] = N - 1
    assert len(np.unique(perm[1])) < N
    got = _check_margins(b, X, (2, 4), perm, "edge values")
    assert len(np.unique(got, axis=0)) > 3


# -------------------------------------------------------------------------------------- sums
def test_sums():
    rng = np.random.default_rng(90)
    F = 4
    b = sf.make_booster([sf.random_tree(rng, F, 3) for _ in range(3)], F, base_score=0.5)
    worst = 0.0
    for N in (65, 257, 2 * _chunk_rows() + 3):
        X = _normal_rows(rng, N, F)
        Xd = torch.from_numpy(X).cuda()
        y = _labels(rng, N)
        y[5 % N] = 0.25  # a soft label
        w = rng.uniform(0.0, 2.0, size=N).astype(np.float32)
        w[rng.random(N) < 0.1] = 0.0
        perm = _perms(rng, 2, N)
        for wt in (None, w):
            margins, sums = _gpu(b, Xd, (1,), perm, y=y, w=wt, sums=True)
            worst = max(worst, _sums_ratio(margins, sums, y, wt))
            only, none = _gpu(b, Xd, (1,), perm)
            assert none is None
            np.testing.assert_array_equal(only, margins)  # the margins-only launch gives the same margins
            none, alone = _gpu(b, Xd, (1,), perm, y=y, w=wt, margins=False, sums=True)
            assert none is None
            np.testing.assert_array_equal(alone, sums)    # and the sums-only launch the same sums
        if N == 65:  # the margins behind the sums are the right ones
            np.testing.assert_array_equal(margins, _want(b, X, (1,), perm))
    print(f"[permimp] sums: largest |sum_gpu - sum_exact| / bound = {worst:.3g}")


def test_tail_lanes_have_no_weight():
    """65 rows against the same 65 rows padded to 128 with zero weights (the padding's perm entries point inside
    [0, 65)): same sums, bit for bit."""
    rng = np.random.default_rng(91)
    F = 4
    b = sf.random_forest(rng, F, 5, 3)
    X = _normal_rows(rng, 128, F)
    y = _labels(rng, 128)
    w = rng.uniform(0.5, 2.0, size=128).astype(np.float32)
    w[65:] = 0.0
    perm = np.concatenate([_perms(rng, 3, 65), rng.integers(0, 65, size=(3, 63)).astype(np.int32)], axis=1)
    Xd = torch.from_numpy(X).cuda()
    _, short = _gpu(b, Xd[:65], (3, 0), perm[:, :65], y=y[:65], w=w[:65], margins=False, sums=True)
    _, padded = _gpu(b, Xd, (3, 0), perm, y=y, w=w, margins=False, sums=True)
    np.testing.assert_array_equal(short, padded)
    _, ones = _gpu(b, Xd[:65], (3, 0), perm[:, :65], y=y[:65], w=np.ones(65, np.float32), margins=False, sums=True)
    _, unweighted = _gpu(b, Xd[:65], (3, 0), perm[:, :65], y=y[:65], margins=False, sums=True)
    np.testing.assert_array_equal(ones, unweighted)
    assert unweighted[-1] == 65.0


def test_determinism_and_baseline():
    rng = np.random.default_rng(92)
    F, N = 6, 1000
    b = sf.random_forest(rng, F, 9, 4)
    X = _normal_rows(rng, N, F)
    Xd = torch.from_numpy(X).cuda()
    y = _labels(rng, N)
    w = rng.uniform(0, 1, size=N).astype(np.float32)
    perm = _perms(rng, 5, N)
    a = _gpu(b, Xd, (5, 2, 0), perm, y=y, w=w, sums=True)
    c = _gpu(b, Xd, (5, 2, 0), perm, y=y, w=w, sums=True)
    assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes()
    plain = torch.empty(N, dtype=torch.float32, device="cuda")
    predict_ops.predict_gpu(b, Xd, out_margin=plain)
    np.testing.assert_array_equal(a[0][0], plain.cpu().numpy())  # the baseline job is the predictor
    assert np.array_equal(Xd.cpu().numpy(), X, equal_nan=True)


def test_workspace_is_bounded():
    lib = _native.lib()
    rows = _chunk_rows()
    assert _chunk() in (8, 16)
    assert lib.cobalt_perm_workspace(1, 5) == (5 * 4 * 2 + 4) * 8
    assert lib.cobalt_perm_workspace(1 << 24, 101) == lib.cobalt_perm_workspace(rows, 101)
    assert lib.cobalt_perm_workspace(rows, 101) == (101 * 2 + 1) * (rows // 64) * 8


# ------------------------------------------------------------------------ the public interface
def test_unused_feature_is_exactly_zero():
    rng = np.random.default_rng(93)
    F, N = 5, 300
    b = sf.make_booster([sf.random_tree(rng, F, 4, cols=[0, 1, 3, 4]) for _ in range(8)], F, base_score=0.5)
    X = torch.from_numpy(_normal_rows(rng, N, F)).cuda()
    y = _labels(rng, N)
    for metric in ("logloss", "error", "auc"):
        r = b.permutation_importance(X, y, n_repeats=_chunk() + 1, metric=metric)
        assert r["importances"].shape == (F, _chunk() + 1)
        assert (r["importances"][2] == 0.0).all(), metric
        assert (r["importances"][[0, 1, 3, 4]] != 0.0).any(), metric


def _data(seed=0, n=2000, F=6):
    """Label driven by features 0 and 1 only (test_permimp_cpu.informative_data)."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, F)).astype(np.float32)
    y = (X[:, 0] - 0.8 * X[:, 1] + 0.3 * rng.normal(size=n) > 0).astype(np.float32)
    return X, y


def test_gpu_dict_equals_cpu_dict(monkeypatch):
    X, y = _data(1, n=600, F=4)
    X[np.random.default_rng(3).random(X.shape) < 0.05] = np.nan
    b = gbdt.train(torch.as_tensor(X).cuda(), torch.as_tensor(y).cuda(),
                   dict(n_estimators=8, max_depth=3, learning_rate=0.3), device="cuda")
    N = X.shape[0]
    perm = B.draw_permutations(N, 3, 7)
    w = np.random.default_rng(2).uniform(0.5, 1.5, size=N).astype(np.float32)
    worst = 0.0
    for metric, wt in (("logloss", None), ("logloss", w), ("error", None), ("auc", None)):
        if metric == "auc":  # job groups of the AUC staging: one feature at a time, then two repeats at a time
            monkeypatch.setattr(predict_ops, "AUC_STAGE_BYTES", 4 * N * 4)
        g = b.permutation_importance(torch.from_numpy(X).cuda(), y, metric=metric, sample_weight=wt, perm=perm,
                                     n_trees=6)
        c = b.permutation_importance(X, y, metric=metric, sample_weight=wt, perm=perm, n_trees=6, device="cpu")
        assert set(g) == set(c) and g["features"] == c["features"] and g["feature_names"] == c["feature_names"]
        assert g["importances"].shape == (4, 3) and g["importances"].dtype == np.float64
        if metric != "logloss":
            np.testing.assert_array_equal(g["importances"], c["importances"])
            assert g["baseline_score"] == c["baseline_score"]
            continue
        # each score is a ratio of two sums within (N + 8) 2^-52 sum w|t| of the CPU path's exact (fsum) sums:
        # 2 (N + 8) 2^-52 sum w|t| / sum w per score (and one part in 100 for the second-order term), once for
        # the job and once for the baseline
        wd = np.ones(N) if wt is None else wt.astype(np.float64)
        u = 2.01 * (N + 8) * 2.0 ** -52 / wd.sum()
        yd = y.astype(np.float64)

        def abs_terms(Xs):
            m = B.predict_margin_host(b, Xs, 6).astype(np.float64)
            return float((wd * np.abs(np.log1p(np.exp(-np.abs(m))) + np.maximum(m, 0.0) - yd * m)).sum())

        base_bound = u * abs_terms(X)
        assert abs(g["baseline_score"] - c["baseline_score"]) <= base_bound
        for i, f in enumerate(g["features"]):
            for r in range(3):
                Xs = X.copy()
                Xs[:, f] = X[perm[r], f]
                bound = u * abs_terms(Xs) + base_bound
                err = abs(g["importances"][i, r] - c["importances"][i, r])
                assert err <= bound, (metric, f, r, err, bound)
                worst = max(worst, err / bound)
    print(f"[permimp] GPU dict against CPU dict: largest |logloss importance difference| / bound = {worst:.3g}")
    # two-repeat groups of one feature
    monkeypatch.setattr(predict_ops, "AUC_STAGE_BYTES", 3 * N * 4)
    g2 = b.permutation_importance(torch.from_numpy(X).cuda(), y, metric="auc", perm=perm, n_trees=6)
    np.testing.assert_array_equal(g2["importances"], g["importances"])


def test_explain_front_end_on_the_gpu():
    X, y = _data()
    clf = gbdt.GBDTClassifier(n_estimators=6, max_depth=3, learning_rate=0.3, device="cuda").fit(X, y)
    r = explain.permutation_importance(clf, X, y, n_repeats=3)
    assert r["importances"].shape == (6, 3) and r["metric"] == "logloss" and r["n_repeats"] == 3
    assert sorted(np.argsort(-r["importances_mean"])[:2]) == [0, 1]
    again = explain.permutation_importance(clf, X, y, n_repeats=3)
    np.testing.assert_array_equal(again["importances"], r["importances"])  # the device draw is seeded
    perm = B.draw_permutations(len(y), 2, 5)
    part = explain.permutation_importance(clf, X, y, [4, 1], metric="error", perm=perm, iteration_range=(0, 3))
    want = clf.get_booster().permutation_importance(X, y, [4, 1], metric="error", perm=perm, n_trees=3, device="cpu")
    np.testing.assert_array_equal(part["importances"], want["importances"])
    d = B.draw_permutations(1000, 2, 0, torch.device("cuda", 0))
    assert d.dtype == torch.int32 and d.is_cuda and tuple(d.shape) == (2, 1000)
    assert all(torch.equal(torch.sort(p).values, torch.arange(1000, dtype=torch.int32, device="cuda")) for p in d)


# ---------------------------------------------------------------------------------- refusals
def test_refusals_before_any_launch():
    rng = np.random.default_rng(100)
    b = sf.random_forest(rng, 6, 3, 3)
    Xd = torch.zeros((8, 6), dtype=torch.float32, device="cuda")
    perm = torch.from_numpy(_perms(rng, 2, 8)).cuda()
    y = torch.zeros(8, device="cuda")
    kw = dict(want_margins=True, want_sums=True)
    for bad in (8, -1):
        p = perm.clone()
        p[1, 3] = bad
        with pytest.raises(ValueError, match="perm"):
            predict_ops.permutation_scores_gpu(b, Xd, y, (0,), p, **kw)
        with pytest.raises(ValueError, match="perm"):
            b.permutation_importance(Xd, y, perm=p)
        with pytest.raises(ValueError, match="perm"):
            b.permutation_importance(Xd, y, perm=p.long())
    with pytest.raises(ValueError, match="perm"):
        predict_ops.permutation_scores_gpu(b, Xd, y, (0,), perm[:, :7].contiguous(), **kw)
    with pytest.raises(ValueError, match="perm"):
        predict_ops.permutation_scores_gpu(b, Xd, y, (0,), perm.long(), **kw)
    with pytest.raises(ValueError, match="features"):
        predict_ops.permutation_scores_gpu(b, Xd[:, :5], y, (0,), perm, **kw)   # narrow X
    with pytest.raises(ValueError, match="float32"):
        predict_ops.permutation_scores_gpu(b, Xd.double(), y, (0,), perm, **kw)
    with pytest.raises(ValueError):
        predict_ops.permutation_scores_gpu(b, Xd, y, (6,), perm, **kw)
    with pytest.raises(ValueError, match="weights"):
        predict_ops.permutation_scores_gpu(b, Xd, y, (0,), perm, weights=torch.ones(7, device="cuda"), **kw)
    with pytest.raises(ValueError, match="y"):
        predict_ops.permutation_scores_gpu(b, Xd, None, (0,), perm, **kw)
    # a footprint beyond the LDS limit: 2048 * 8 + 256 * (144 | 1) * 4 bytes > 160 KiB
    wide = sf.random_forest(rng, 144, 2, 3)
    with pytest.raises(RuntimeError, match="code -3"):
        predict_ops.permutation_scores_gpu(wide, torch.zeros((8, 144), dtype=torch.float32, device="cuda"), y, (0,),
                                           perm, **kw)
    # the entry point itself refuses what the wrapper checks first
    lib = _native.lib()
    gf = predict_ops.gpu_forest(b, Xd.device)
    ft = torch.zeros(1, dtype=torch.int32, device="cuda")
    cols = torch.zeros((1, 8), dtype=torch.float32, device="cuda")
    out = torch.full((3, 8), 7.0, dtype=torch.float32, device="cuda")
    sums = torch.full((7,), 7.0, dtype=torch.float64, device="cuda")
    work = torch.empty(int(lib.cobalt_perm_workspace(8, 3)), dtype=torch.uint8, device="cuda")

    def call(nf=1, R=2, feats=ft.data_ptr(), cols=cols.data_ptr(), perm=perm.data_ptr(), y=y.data_ptr(),
             work=work.data_ptr(), sums=sums.data_ptr(), chunk=0, tile_cap=gf.tile_cap, F=6, ldx=6):
        return lib.cobalt_perm_importance(Xd.data_ptr(), 8, F, ldx, gf.nodes.data_ptr(), gf.tree_ptr.data_ptr(),
                                          gf.tile_ptr.data_ptr(), gf.n_tiles, tile_cap, 0.0, feats, nf, cols, perm, R,
                                          y, None, out.data_ptr(), work, sums, chunk, _native.stream_handle())

    assert call(R=0) == -8
    assert call(nf=-1) == -8
    assert call(feats=None) == -8
    assert call(cols=None) == -8
    assert call(perm=None) == -8
    assert call(y=None) == -8            # sums without labels
    assert call(chunk=5) == -8
    assert call(F=0) == -8
    assert call(ldx=5) == -8
    assert call(nf=70000) == -8          # more blocks than gridDim.y holds
    assert call(tile_cap=8193) == -2
    assert call(F=144, ldx=144) == -3
    assert call(work=None) == -7
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((sums == 7.0).all())  # nothing was launched
