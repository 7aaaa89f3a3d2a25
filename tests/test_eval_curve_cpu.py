"""Validation curves and early stopping on the CPU: the NumPy oracle ``eval_curve_host`` against an
independent formula, the early-stopping rule through the host trainer and the estimator, persistence of
``best_iteration`` / ``best_score``, and the refused inputs."""
import numpy as np
import pytest

from cobalt_smart_lender_ai_amd.dataio import synth
from cobalt_smart_lender_ai_amd.metrics.auc import roc_auc
from cobalt_smart_lender_ai_amd.models import booster as B
from cobalt_smart_lender_ai_amd.models import gbdt
from cobalt_smart_lender_ai_amd.ops import predict_ops

TREE_FIELDS = ("left_children", "right_children", "parents", "split_indices", "split_conditions", "default_left",
               "base_weights", "loss_changes", "sum_hessian")
FIT = dict(n_estimators=30, max_depth=4, learning_rate=0.3)
ROUNDS = 5


def make_rows(rng, n):
    """X ~ N(0, 1) [n, 8] float32 with 5% NaN cells; y = (x0 + 0.5 x1 x2 + N(0, 1.5) > 0), NaN read as 0."""
    X = rng.normal(size=(n, 8)).astype(np.float32)
    X[rng.random(X.shape) < 0.05] = np.nan
    Z = np.nan_to_num(X, nan=0.0).astype(np.float64)
    s = Z[:, 0] + 0.5 * Z[:, 1] * Z[:, 2]
    y = (s + rng.normal(0.0, 1.5, size=n) > 0).astype(np.float32)
    return X, y


def make_data(n_train, n_val):
    rng = np.random.default_rng(7)
    return make_rows(rng, n_train), make_rows(rng, n_val)


def apply_rule(curve, rounds, maximize=False, first=0):
    """XGBoost's early-stopping rule over a full curve: (stop round or None, best round, best score)."""
    best = best_score = None
    for j, s in enumerate(curve):
        r = first + j
        if best is None or (s > best_score if maximize else s < best_score):
            best, best_score = r, s
        elif r - best >= rounds:
            return r, best, best_score
    return None, best, best_score


def assert_same_trees(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        for f in TREE_FIELDS:
            assert np.array_equal(getattr(a, f), getattr(b, f)), f


# ------------------------------------------------------------------ the oracle against another formula
@pytest.fixture(scope="module")
def shipped_rows():
    X, y = synth.make_lendingclub(200, seed=21)
    X, y = X.numpy().copy(), y.numpy().astype(np.float32)
    X[np.random.default_rng(5).random(X.shape) < 0.05] = np.nan
    return X, y


def test_host_curve_matches_independent_formula(reference_booster, shipped_rows):
    b = reference_booster
    X, y = shipped_rows
    w = np.random.default_rng(6).choice([0.5, 1.0, 2.0], size=len(y)).astype(np.float32)
    assert 0 < y.sum() < len(y)
    stages = b.staged_margins(X, device="cpu")
    assert stages.dtype == np.float32 and stages.shape == (b.num_trees, len(y))
    assert np.abs(stages).max() < 10  # below that p and 1 - p lose nothing that matters to rtol 1e-9
    prefix = [B.predict_margin_host(b, X, t + 1) for t in range(b.num_trees)]  # the T-call loop, once
    for weights in (None, w):
        curve, final = b.eval_curve(X, y, weights, ("logloss", "error", "auc"), device="cpu")
        wd = np.ones(len(y)) if weights is None else weights.astype(np.float64)
        assert list(curve) == ["logloss", "error", "auc"]
        for t, m in enumerate(prefix):
            assert np.array_equal(stages[t], m)
            p = 1.0 / (1.0 + np.exp(-m.astype(np.float64)))
            ll = np.sum(wd * (-y * np.log(p) - (1 - y) * np.log(1 - p))) / wd.sum()
            np.testing.assert_allclose(curve["logloss"][t], ll, rtol=1e-9, atol=0)
            assert curve["error"][t] == np.sum(wd * ((m > 0) != (y > 0.5))) / wd.sum()
            assert curve["auc"][t] == roc_auc(y, m)
        assert np.array_equal(final, stages[-1])
        assert all(v.dtype == np.float64 and v.shape == (b.num_trees,) for v in curve.values())


def test_margin_continuation_on_the_host(reference_booster, shipped_rows):
    b = reference_booster
    X, y = shipped_rows
    whole, m_all = b.eval_curve(X, y, device="cpu", metrics=("logloss", "error"))
    head, m_head = b.slice(100).eval_curve(X, y, device="cpu", metrics=("logloss", "error"))
    rest = B.Booster(b.trees[100:], base_score=b.base_score, num_feature=b.num_feature)
    tail, m_tail = rest.eval_curve(X, y, device="cpu", metrics=("logloss", "error"), margin=m_head)
    assert np.array_equal(m_tail, m_all)
    for k in whole:
        assert np.array_equal(np.concatenate([head[k], tail[k]]), whole[k])


def test_eval_curve_refuses_bad_inputs(reference_booster, shipped_rows):
    b = reference_booster
    X, y = shipped_rows
    for fn in (lambda **kw: b.eval_curve(device="cpu", **kw), lambda **kw: B.eval_curve_host(b, **kw)):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            fn(X=X, y=np.where(y > 0, 2.0, 0.0))
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            fn(X=X, y=np.where(y > 0, np.nan, 0.0))
        with pytest.raises(ValueError, match="sum to zero"):
            fn(X=X, y=y, sample_weight=np.zeros(len(y)))
        with pytest.raises(ValueError, match="rows"):
            fn(X=X, y=y[:-1])
        with pytest.raises(ValueError, match="rows"):
            fn(X=X, y=y, sample_weight=np.ones(len(y) + 1))
        with pytest.raises(ValueError, match="rows"):
            fn(X=X, y=y, margin=np.zeros(3, np.float32))
        with pytest.raises(ValueError, match="unknown eval metric"):
            fn(X=X, y=y, metrics=("rmse",))
        with pytest.raises(ValueError, match="one class"):
            fn(X=X, y=np.zeros(len(y)), metrics=("auc",))
    # the checks come before the device is touched (this machine may have none)
    with pytest.raises(ValueError, match="unknown eval metric"):
        predict_ops.eval_curve(b, X, y, metrics=("mae",), device="cpu")


# ------------------------------------------------------------------------- early stopping, CPU trainer
@pytest.fixture(scope="module")
def data():
    return make_data(2000, 1000)


@pytest.fixture(scope="module")
def plain_fit(data):
    """The 30-tree fit without early stopping, with its validation curve."""
    (X, y), (Xv, yv) = data
    hist = {}
    b = gbdt.train(X, y, gbdt.GBDTParams(**FIT), device="cpu", evals=[(Xv, yv)], eval_metric="logloss",
                   evals_result=hist)
    return b, hist


@pytest.fixture(scope="module")
def stopped_clf(data):
    (X, y), (Xv, yv) = data
    clf = gbdt.GBDTClassifier(**FIT, early_stopping_rounds=ROUNDS, eval_metric="logloss", device="cpu")
    return clf.fit(X, y, eval_set=[(Xv, yv)])


def test_plain_fit_records_the_curve_and_stays_the_plain_fit(plain_fit, data):
    b, hist = plain_fit
    (X, y), (Xv, yv) = data
    assert b.num_trees == 30 and b.best_iteration is None and b.best_score is None
    assert list(hist) == ["validation_0"] and list(hist["validation_0"]) == ["logloss"]
    want, _ = B.eval_curve_host(b, Xv, yv)
    assert hist["validation_0"]["logloss"] == want["logloss"].tolist()


def test_early_stopped_fit_is_a_prefix_of_the_plain_fit(plain_fit, stopped_clf, data):
    """(With these rows the validation logloss has its minimum at round 7 and the rule fires at round 12:
    the model keeps 13 trees and predicts with 8.)"""
    plain, hist = plain_fit
    (X, y), (Xv, yv) = data
    curve = hist["validation_0"]["logloss"]
    stop, best, best_score = apply_rule(curve, ROUNDS)
    print(f"rule: stop at round {stop}, best round {best}, best logloss {best_score:.6f}")
    assert stop is not None and stop + 1 < FIT["n_estimators"], "the rule must fire before n_estimators"
    clf = stopped_clf
    b = clf.get_booster()
    assert b.num_trees == stop + 1
    assert_same_trees(b.trees, plain.trees[: stop + 1])
    assert b.base_score == plain.base_score
    assert clf.best_iteration == best and clf.best_score == best_score
    assert b.attributes == {"best_iteration": str(best), "best_score": repr(best_score)}
    assert clf.evals_result() == {"validation_0": {"logloss": curve[: stop + 1]}}
    # predictions use the best round's prefix by default; an explicit range overrides that
    p_best = B.sigmoid32(B.predict_margin_host(plain, Xv, best + 1))
    assert np.array_equal(clf.predict_proba(Xv)[:, 1], p_best)
    assert np.array_equal(clf.predict(Xv), (p_best > 0.5).astype(np.int64))
    p_all = B.sigmoid32(B.predict_margin_host(plain, Xv, stop + 1))
    assert np.array_equal(clf.predict_proba(Xv, iteration_range=(0, stop + 1))[:, 1], p_all)
    assert np.array_equal(clf.predict_proba(Xv, iteration_range=(0, 0))[:, 1], p_all)
    assert not np.array_equal(p_best, p_all)
    with pytest.raises(ValueError, match="iteration_range"):
        clf.predict_proba(Xv, iteration_range=(1, 3))


def test_segment_length_does_not_change_the_result(stopped_clf, data):
    (X, y), (Xv, yv) = data
    hist = {}
    b = gbdt.train(X, y, gbdt.GBDTParams(**FIT), device="cpu", evals=[(Xv, yv)], early_stopping_rounds=ROUNDS,
                   evals_result=hist, es_segment=3)
    ref = stopped_clf.get_booster()
    assert_same_trees(b.trees, ref.trees)
    assert b.attributes == ref.attributes
    assert hist == stopped_clf.evals_result()


def test_best_round_survives_model_and_pickle_round_trips(stopped_clf, tmp_path):
    clf = stopped_clf
    b = clf.get_booster()
    again = B.Booster.load_raw(b.save_raw("ubj"))
    assert (again.best_iteration, again.best_score) == (clf.best_iteration, clf.best_score)
    assert B.Booster.load_raw(b.save_raw("json")).best_iteration == clf.best_iteration
    clf.save_pickle(tmp_path / "m.pkl")
    back = gbdt.GBDTClassifier.load_pickle(tmp_path / "m.pkl")
    assert back.early_stopping_rounds == ROUNDS and back.eval_metric == "logloss"
    assert (back.best_iteration, back.best_score) == (clf.best_iteration, clf.best_score)
    assert back._n_trees(None) == clf.best_iteration + 1


def test_pickle_bytes_are_unchanged_without_early_stopping(reference_booster):
    a = gbdt.GBDTClassifier(n_estimators=300, max_depth=7)
    a._Booster = reference_booster
    state = {k: v for k, v in a.sklearn_state_params().items() if k != "early_stopping_rounds"}
    assert "early_stopping_rounds" in a.sklearn_state_params()
    assert B.dump_pickle_bytes(reference_booster, a.sklearn_state_params()) == B.dump_pickle_bytes(
        reference_booster, state)
    with pytest.raises(AttributeError):
        a.best_iteration
    with pytest.raises(ValueError, match="eval_set"):
        a.evals_result()
    assert a._n_trees(None) is None


def test_metric_and_set_order_follow_xgboost(data):
    """Two sets, two metrics: the LAST set's LAST metric drives the stop; "auc" is maximised; weights of
    an eval set enter its metrics; ``init_booster`` makes the rounds global."""
    (X, y), (Xv, yv) = data
    X, y = X[:400], y[:400]
    wv = np.random.default_rng(3).choice([0.5, 1.0, 2.0], size=len(yv)).astype(np.float32)
    p = gbdt.GBDTParams(n_estimators=6, max_depth=2, learning_rate=0.5)
    first = gbdt.train(X, y, gbdt.GBDTParams(n_estimators=2, max_depth=2, learning_rate=0.5), device="cpu")
    full = gbdt.train(X, y, p, device="cpu", init_booster=first)
    assert full.num_trees == 8
    hist = {}
    b = gbdt.train(X, y, p, device="cpu", init_booster=first, evals=[(X, y), (Xv, yv, wv)],
                   eval_metric=["logloss", "auc"], early_stopping_rounds=1, evals_result=hist, es_segment=2)
    assert list(hist) == ["validation_0", "validation_1"]
    assert all(list(h) == ["logloss", "auc"] for h in hist.values())
    new = B.Booster(full.trees[2:], base_score=full.base_score, num_feature=full.num_feature)
    want, _ = B.eval_curve_host(new, Xv, yv, wv, ("logloss", "auc"), margin=B.predict_margin_host(first, Xv))
    stop, best, best_score = apply_rule(want["auc"].tolist(), 1, maximize=True, first=2)
    kept = (stop + 1 if stop is not None else 8)
    assert b.num_trees == kept and (b.best_iteration, b.best_score) == (best, best_score)
    assert_same_trees(b.trees, full.trees[:kept])
    assert hist["validation_1"]["auc"] == want["auc"][: kept - 2].tolist()
    assert hist["validation_1"]["logloss"] == want["logloss"][: kept - 2].tolist()
    train_curve, _ = B.eval_curve_host(new, X, y, None, ("logloss",), margin=B.predict_margin_host(first, X))
    assert hist["validation_0"]["logloss"] == train_curve["logloss"][: kept - 2].tolist()


def test_training_refuses_what_it_does_not_support(data, tmp_path):
    (X, y), (Xv, yv) = data
    X, y = X[:64], y[:64]
    p = gbdt.GBDTParams(n_estimators=2, max_depth=2)
    with pytest.raises(ValueError, match="validation set"):
        gbdt.train(X, y, p, device="cpu", early_stopping_rounds=3)
    with pytest.raises(ValueError, match="validation set"):
        gbdt.GBDTClassifier(n_estimators=2, early_stopping_rounds=3, device="cpu").fit(X, y)
    with pytest.raises(ValueError, match="checkpoint_path"):
        gbdt.train(X, y, p, device="cpu", evals=[(Xv, yv)], early_stopping_rounds=3,
                   checkpoint_path=str(tmp_path / "c.ubj"), checkpoint_every=1)
    assert not (tmp_path / "c.ubj").exists()

    class TwoRanks:
        world, rank = 2, 0

        def __getattr__(self, name):  # any collective would be a failure of the test
            raise AssertionError(f"dist.{name} used before the refusal")

    with pytest.raises(ValueError, match="data-parallel"):
        gbdt.train(X, y, p, device="cpu", evals=[(Xv, yv)], dist=TwoRanks())
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        gbdt.train(X, y, p, device="cpu", evals=[(Xv, yv * 3)])
    with pytest.raises(ValueError, match="features"):
        gbdt.train(X, y, p, device="cpu", evals=[(Xv[:, :5], yv)])
    with pytest.raises(ValueError, match="unknown eval metric"):
        gbdt.train(X, y, p, device="cpu", evals=[(Xv, yv)], eval_metric="rmse")
    with pytest.raises(ValueError, match="early_stopping_rounds must be"):
        gbdt.train(X, y, p, device="cpu", evals=[(Xv, yv)], early_stopping_rounds=0)
    from cobalt_smart_lender_ai_amd.models.external import train_external

    def source():
        raise AssertionError("the stream was read before the refusal")

    with pytest.raises(ValueError, match="train_external does not support"):
        train_external(source, p, device="cpu", evals=[(Xv, yv)])
    with pytest.raises(ValueError, match="train_external does not support"):
        train_external(source, p, device="cpu", early_stopping_rounds=2)


def test_estimator_protocol_keeps_working(data):
    from sklearn.base import clone

    clf = gbdt.GBDTClassifier(n_estimators=3, max_depth=2, early_stopping_rounds=4, eval_metric="error")
    twin = clone(clf)
    assert twin.get_params() == clf.get_params() and twin.early_stopping_rounds == 4
    plain = gbdt.GBDTClassifier(n_estimators=3, max_depth=2)
    assert set(clf.get_params()) - {"early_stopping_rounds"} == set(plain.get_params()) - {"early_stopping_rounds"}
    assert len(plain.get_params()) == 21 and plain.get_params()["early_stopping_rounds"] is None
    # eval labels are encoded like the training labels; the metric is the constructor's
    (X, y), (Xv, yv) = data
    names = np.array(["bad", "good"])
    est = gbdt.GBDTClassifier(n_estimators=3, max_depth=2, eval_metric="error", device="cpu")
    est.fit(X[:300], names[y[:300].astype(int)], eval_set=[(Xv[:200], names[yv[:200].astype(int)])])
    want, _ = B.eval_curve_host(est.get_booster(), Xv[:200], yv[:200], None, ("error",))
    assert est.evals_result() == {"validation_0": {"error": want["error"].tolist()}}
    assert est.get_booster().best_iteration is None
    with pytest.raises(ValueError, match="training classes"):
        est.fit(X[:300], names[y[:300].astype(int)], eval_set=[(Xv[:200], np.full(200, "ugly"))])
    # a second fit without eval_set forgets the first one's curve
    est.fit(X[:300], y[:300])
    with pytest.raises(ValueError, match="eval_set"):
        est.evals_result()
