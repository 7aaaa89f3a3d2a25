"""GPU (gfx950) learning curves (``csrc/evalcurve.hip``) against the predictor and the host oracle
``eval_curve_host`` (itself checked against an independent formula in test_eval_curve_cpu.py), and early
stopping through the GPU trainer.

Tolerances: the stage margins are the predictor's fp32 sums in the same order -> bit-equal. The "error"
sums are sums of weights from {0.5, 1, 2} (or of ones) -> exact in any order -> equal. "logloss": every
term is non-negative, host and device differ by a few ulps per term (exp / log1p) plus at most
(N - 1) 2^-53 relative from the order of the additions, below 1e-12 for N <= 1000; rtol 1e-10 leaves a
factor of 100 for the device's exp / log1p."""
import numpy as np
import pytest
import torch

from cobalt_smart_lender_ai_amd.dataio import synth
from cobalt_smart_lender_ai_amd.models import booster as B
from cobalt_smart_lender_ai_amd.models import gbdt
from cobalt_smart_lender_ai_amd.ops import predict_ops

from test_eval_curve_cpu import FIT, ROUNDS, apply_rule, assert_same_trees, make_data

pytestmark = pytest.mark.gpu

N_MAX = 1000
LOGLOSS_RTOL = 1e-10


def check_against_predictor_and_oracle(b, X, y, w):
    """``X`` [N, F] float32 host rows: stage margins / final margins against the GPU predictor of every
    prefix, the curve against the host oracle; returns the GPU curve and margins."""
    Xg = torch.as_tensor(X).cuda()
    curve, m_out = b.eval_curve(Xg, y, w, ("logloss", "error"))
    stages = b.staged_margins(Xg)
    assert stages.dtype == torch.float32 and tuple(stages.shape) == (b.num_trees, len(y))
    for t in range(b.num_trees):
        assert torch.equal(stages[t], b.predict_margin(Xg, n_trees=t + 1)), f"stage {t}"
    assert torch.equal(m_out, stages[-1])
    want, m_host = B.eval_curve_host(b, X, y, w, ("logloss", "error"))
    assert np.array_equal(m_out.cpu().numpy(), m_host)
    rel = np.abs(curve["logloss"] - want["logloss"]) / want["logloss"]
    print(f"N={len(y)} weights={'yes' if w is not None else 'no'}: max rel logloss diff {rel.max():.3e}")
    assert np.array_equal(curve["error"], want["error"])
    np.testing.assert_allclose(curve["logloss"], want["logloss"], rtol=LOGLOSS_RTOL, atol=0)
    assert curve["logloss"].dtype == np.float64 and curve["logloss"].shape == (b.num_trees,)
    return curve, m_out


@pytest.fixture(scope="module")
def rows():
    X, y = synth.make_lendingclub(N_MAX, seed=33)
    X, y = X.numpy().copy(), y.numpy().astype(np.float32)
    X[np.random.default_rng(8).random(X.shape) < 0.05] = np.nan
    w = np.random.default_rng(9).choice([0.5, 1.0, 2.0], size=N_MAX).astype(np.float32)
    return X, y, w


@pytest.mark.parametrize("n", [1, 63, 257, 1000])
def test_shipped_model(reference_booster, rows, n):
    """20 features, 300 depth-7 trees in ~30 LDS tiles whose tree counts are no multiples of the 4-tree
    walk; 1 row, less than a wave, one block + 1 row, four blocks with a partial last one."""
    b = reference_booster
    _, _, tiles = predict_ops.pack_forest(b)
    assert len(tiles) - 1 > 20 and (np.diff(tiles) % 4 != 0).any()
    X, y, w = rows
    if n == 1:
        y = np.array([1.0], np.float32)
    check_against_predictor_and_oracle(b, X[:n], y[:n], None)
    check_against_predictor_and_oracle(b, X[:n], y[:n], w[:n])


def _leaf(v):
    z = np.zeros(1, np.float32)
    return B.Tree(np.array([-1], np.int32), np.array([-1], np.int32), np.array([B.ROOT_PARENT], np.int32),
                  np.zeros(1, np.int32), np.array([v], np.float32), np.zeros(1, np.uint8), z, z, np.ones(1, np.float32))


def _stump(f, thr, lo, hi, default_left):
    z = np.zeros(3, np.float32)
    return B.Tree(np.array([1, -1, -1], np.int32), np.array([2, -1, -1], np.int32),
                  np.array([B.ROOT_PARENT, 0, 0], np.int32), np.array([f, 0, 0], np.int32),
                  np.array([thr, lo, hi], np.float32), np.array([default_left, 0, 0], np.uint8), z, z,
                  np.array([4, 2, 2], np.float32))


def test_root_only_tree_among_three():
    b = B.Booster([_stump(1, 0.25, -0.75, 0.5, 1), _leaf(0.125), _stump(0, -0.5, 1.5, -2.0, 0)], num_feature=3,
                  base_score=0.3)
    rng = np.random.default_rng(4)
    X = rng.normal(size=(130, 3)).astype(np.float32)
    X[rng.random(X.shape) < 0.2] = np.nan
    y = (rng.random(130) < 0.5).astype(np.float32)
    y[:5] = [0.0, 1.0, 0.25, 0.5, 0.75]  # labels inside (0, 1) are legal for the logistic loss
    w = rng.choice([0.5, 1.0, 2.0], size=130).astype(np.float32)
    check_against_predictor_and_oracle(b, X, y, None)
    check_against_predictor_and_oracle(b, X, y, w)


def test_rows_beyond_one_chunk():
    """2^19 + 300 rows: two row chunks (the second a partial one) whose sums are added in chunk order. The
    order of the additions costs at most (N - 1) 2^-53 = 5.8e-11 relative here, still inside rtol 1e-10."""
    b = B.Booster([_stump(1, 0.25, -0.75, 0.5, 1), _leaf(0.125), _stump(0, -0.5, 1.5, -2.0, 0)], num_feature=3,
                  base_score=0.3)
    n = (1 << 19) + 300
    rng = np.random.default_rng(14)
    X = rng.normal(size=(n, 3)).astype(np.float32)
    X[rng.random(X.shape) < 0.05] = np.nan
    y = (rng.random(n) < 0.4).astype(np.float32)
    w = rng.choice([0.5, 1.0, 2.0], size=n).astype(np.float32)
    Xg = torch.as_tensor(X).cuda()
    want, m_host = B.eval_curve_host(b, X, y, w, ("logloss", "error"))
    got, m = b.eval_curve(Xg, y, w, ("logloss", "error"))
    assert np.array_equal(m.cpu().numpy(), m_host)
    assert torch.equal(b.staged_margins(Xg)[-1], b.predict_margin(Xg))
    assert np.array_equal(got["error"], want["error"])
    print("max rel logloss diff", (np.abs(got["logloss"] - want["logloss"]) / want["logloss"]).max())
    np.testing.assert_allclose(got["logloss"], want["logloss"], rtol=LOGLOSS_RTOL, atol=0)
    again, _ = b.eval_curve(Xg, y, w, ("logloss", "error"))
    assert again["logloss"].tobytes() == got["logloss"].tobytes()


def test_many_shallow_trees_in_one_tile():
    X, y = synth.make_lendingclub(1500, seed=12)
    X[::7, 3] = float("nan")
    p = gbdt.GBDTParams(n_estimators=41, max_depth=3, learning_rate=0.3)
    b = gbdt.train(X.cuda(), y.cuda(), p, device="cuda")
    _, _, tiles = predict_ops.pack_forest(b)
    assert len(tiles) == 2 and b.num_trees == 41  # one tile, a tree count that is no multiple of the walk
    w = np.random.default_rng(2).choice([0.5, 1.0, 2.0], size=321).astype(np.float32)
    check_against_predictor_and_oracle(b, X[:321].numpy(), y[:321].numpy().astype(np.float32), w)


def test_margin_continuation_equals_one_pass(reference_booster, rows):
    b = reference_booster
    X, y, w = rows
    Xg = torch.as_tensor(X[:257]).cuda()
    y, w = y[:257], w[:257]
    whole, m_all = b.eval_curve(Xg, y, w, ("logloss", "error"))
    head, m_head = b.slice(100).eval_curve(Xg, y, w, ("logloss", "error"))
    rest = B.Booster(b.trees[100:], base_score=b.base_score, num_feature=b.num_feature)
    tail, m_tail = rest.eval_curve(Xg, y, w, ("logloss", "error"), margin=m_head)
    assert torch.equal(m_tail, m_all)
    for k in ("logloss", "error"):
        assert np.array_equal(np.concatenate([head[k], tail[k]]), whole[k]), k


def test_two_runs_give_identical_bits(reference_booster, rows):
    b = reference_booster
    X, y, w = rows
    Xg = torch.as_tensor(X).cuda()
    first, m1 = b.eval_curve(Xg, y, w, ("logloss", "error"))
    again, m2 = b.eval_curve(Xg, y, w, ("logloss", "error"))
    assert torch.equal(m1, m2)
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), k
    # host rows in, host arrays out -- the same numbers
    host, mh = b.eval_curve(X, y, w, ("logloss", "error"), device="cuda")
    assert isinstance(mh, np.ndarray) and np.array_equal(mh, m1.cpu().numpy())
    assert host["logloss"].tobytes() == first["logloss"].tobytes()


def test_auc_curve_in_tree_chunks(reference_booster, rows, monkeypatch):
    from cobalt_smart_lender_ai_amd.metrics.auc import roc_auc

    b = reference_booster.slice(37)
    X, y, _ = rows
    X, y = X[:300], y[:300]
    want, _ = B.eval_curve_host(b, X, y, None, ("auc", "error"))
    monkeypatch.setattr(predict_ops, "AUC_STAGE_BYTES", 300 * 4 * 10)  # chunks of 10 trees: 10 + 10 + 10 + 7
    got, m = b.eval_curve(torch.as_tensor(X).cuda(), y, None, ("auc", "error"))
    assert list(got) == ["auc", "error"]
    assert np.array_equal(got["auc"], want["auc"]) and np.array_equal(got["error"], want["error"])
    assert got["auc"][-1] == roc_auc(y, B.predict_margin_host(b, X))
    assert np.array_equal(m.cpu().numpy(), B.predict_margin_host(b, X))


def test_limits_are_refused_before_any_launch(reference_booster, rows):
    b = reference_booster
    X, y, _ = rows
    Xg = torch.as_tensor(X[:8]).cuda()
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        b.eval_curve(Xg, y[:8] * 2 - 1)
    with pytest.raises(ValueError, match="rows"):
        b.eval_curve(Xg, y[:9])
    lib = predict_ops._native.lib()
    args = (None, 8, 20, 20, None, None, None, None, None, 1)
    assert lib.cobalt_eval_curve(*args, 8193, 3, 0.0, None, None, None, None, None, None) == -2   # tile too large
    wide = (None, 8, 40000, 40000, None, None, None, None, None, 1)
    assert lib.cobalt_eval_curve(*wide, 2048, 3, 0.0, None, None, None, None, None, None) == -3   # LDS > 160 KiB
    assert lib.cobalt_eval_curve_workspace(1, 300) == (300 * 4 * 2 + 4) * 8
    assert lib.cobalt_eval_curve_workspace(1 << 22, 300) == lib.cobalt_eval_curve_workspace(1 << 19, 300)


# ------------------------------------------------------------------------------- early stopping, GPU trainer
@pytest.fixture(scope="module")
def es_data():
    (X, y), (Xv, yv) = make_data(4096, 1024)
    return torch.as_tensor(X).cuda(), torch.as_tensor(y).cuda(), Xv, yv


def test_early_stopping_on_the_gpu_trainer(es_data):
    X, y, Xv, yv = es_data
    p = gbdt.GBDTParams(**FIT)
    hist = {}
    plain = gbdt.train(X, y, p, device="cuda", evals=[(Xv, yv)], evals_result=hist)
    curve = hist["validation_0"]["logloss"]
    assert plain.num_trees == 30 and len(curve) == 30
    want, _ = B.eval_curve_host(plain, Xv, yv)
    np.testing.assert_allclose(curve, want["logloss"], rtol=LOGLOSS_RTOL, atol=0)
    stop, best, best_score = apply_rule(curve, ROUNDS)
    print(f"rule: stop at round {stop}, best round {best}, best logloss {best_score:.6f}")
    assert stop is not None and stop + 1 < 30, "the rule must fire before n_estimators"
    fits = []
    for seg in (None, 3):
        h = {}
        b = gbdt.train(X, y, p, device="cuda", evals=[(Xv, yv)], early_stopping_rounds=ROUNDS, evals_result=h,
                       es_segment=seg)
        assert b.num_trees == stop + 1
        assert_same_trees(b.trees, plain.trees[: stop + 1])
        assert (b.best_iteration, b.best_score) == (best, best_score)
        assert h == {"validation_0": {"logloss": curve[: stop + 1]}}
        fits.append(b)
    assert fits[0].save_raw() == fits[1].save_raw()
    # the trainer context parked by the early exit serves the next fit of these shapes
    after = gbdt.train(X, y, p, device="cuda")
    assert_same_trees(after.trees, plain.trees)
    host = gbdt.train(X.cpu().numpy(), y.cpu().numpy(), p, device="cpu")
    for tg, tc in zip(after.trees, host.trees):  # (the fields test_gpu_gbdt.py holds the GPU trainer to)
        for f in ("split_indices", "left_children", "default_left", "split_conditions", "loss_changes", "sum_hessian"):
            assert np.array_equal(getattr(tg, f), getattr(tc, f)), f


def test_estimator_early_stopping_on_the_gpu(es_data):
    X, y, Xv, yv = es_data
    clf = gbdt.GBDTClassifier(**FIT, early_stopping_rounds=ROUNDS, eval_metric=["error", "logloss"], device="cuda")
    clf.fit(X.cpu().numpy(), y.cpu().numpy(), eval_set=[(Xv, yv)])
    b = clf.get_booster()
    res = clf.evals_result()["validation_0"]
    assert list(res) == ["error", "logloss"] and len(res["logloss"]) == b.num_trees < 30
    assert clf.best_iteration == int(np.argmin(res["logloss"])) == b.num_trees - 1 - ROUNDS
    Xg = torch.as_tensor(Xv).cuda()
    p = clf.predict_proba(Xv)[:, 1]
    assert np.array_equal(p, b.predict_proba(Xg, n_trees=clf.best_iteration + 1).cpu().numpy())
    assert np.array_equal(b.predict_margin(Xg, n_trees=clf.best_iteration + 1).cpu().numpy(),
                          B.predict_margin_host(b, Xv, clf.best_iteration + 1))
    p_all = clf.predict_proba(Xv, iteration_range=(0, b.num_trees))[:, 1]
    assert np.array_equal(p_all, b.predict_proba(Xg).cpu().numpy()) and not np.array_equal(p, p_all)
