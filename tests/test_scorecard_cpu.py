"""The WoE points scorecard on the host (models/scorecard.py): the classing rules on hand-written count tables,
the Newton pass against a plain-Python loop, the fit against scikit-learn, the points arithmetic, the JSON round
trip, the command-line verb and the service route."""
import json
import math

import numpy as np
import pytest

from cobalt_smart_lender_ai_amd.models import Scorecard
from cobalt_smart_lender_ai_amd.models import scorecard as S
from cobalt_smart_lender_ai_amd.monitor.drift import cell_pointer, woe_iv
from cobalt_smart_lender_ai_amd.ops import scorecard_ops as ops

from scorecard_cases import U, beta_distance_bound, lending_like, newton_bounds, newton_inputs, newton_loop

F32 = np.float32


def _edges(k):
    return np.arange(1, k + 1, dtype=F32)


def _rates(cl):
    c = cl["counts"][:, :-1].astype(float)
    return c[1] / c.sum(0)


# ------------------------------------------------------------------------------------------------- classing
def test_classing_monotone_share_classes_and_subset():
    # 8 value cells of 100 rows with a noisy, mostly rising bad rate; an empty missing cell
    bad = np.array([5, 12, 9, 20, 18, 30, 45, 40])
    counts = np.stack([100 - bad, bad]).astype(np.int64)
    counts = np.concatenate([counts, [[0], [0]]], axis=1)
    z = _edges(7)
    cl = S.coarse_classing(counts, z, max_bins=4, min_bin_share=0.05, monotone="auto")
    r = _rates(cl)
    assert cl["direction"] == 1 and bool((np.diff(r) > 0).all())
    assert 2 <= len(r) <= 4
    tot = cl["counts"][:, :-1].sum(0)
    assert bool((tot >= 0.05 * counts.sum()).all()) and bool((cl["counts"][:, :-1] > 0).all())
    assert set(cl["edges"].tolist()) <= set(z.tolist()) and cl["edges"].dtype == np.float32
    assert int(cl["counts"].sum()) == int(counts.sum())
    assert np.array_equal(cl["woe"][:-1], woe_iv(np.concatenate([cl["counts"][:, :-1], [[0], [0]]], axis=1))[0][:-1])
    assert cl["woe"][-1] == 0.0 and not cl["missing_own_bin"] and not cl["dropped"]


def test_classing_pure_cell_and_thin_cell_are_merged():
    #           pure (no bad)      thin (2 rows of 400)
    good = np.array([100, 90, 80, 1, 60, 0])
    bad = np.array([0, 10, 20, 1, 30, 0])
    cl = S.coarse_classing(np.stack([good, bad]), _edges(4), max_bins=6, min_bin_share=0.05, monotone=0)
    # the pure first cell joins its only neighbour; the thin cell joins the lighter neighbour, the right one (90 < 100)
    assert cl["edges"].tolist() == [2.0, 3.0]
    assert cl["counts"].tolist() == [[190, 80, 61, 0], [10, 20, 31, 0]]


def test_classing_tie_breaks():
    # step 1: the thin cell's neighbours weigh the same: the LEFT one takes it
    good = np.array([90, 2, 90, 0])
    bad = np.array([10, 0, 10, 0])
    cl = S.coarse_classing(np.stack([good, bad]), _edges(2), min_bin_share=0.05, monotone=0)
    assert cl["edges"].tolist() == [2.0] and cl["counts"][:, 0].tolist() == [92, 10]
    # "auto": a symmetric rate has the same IV pooled either way: decreasing wins
    bad = np.array([10, 30, 10, 0])
    cl = S.coarse_classing(np.stack([100 - bad, bad])[:, :4] * np.array([1, 1, 1, 0]), _edges(2), monotone="auto")
    assert cl["direction"] == -1
    # step 3: equal WoE gaps (the same three bad rates twice): the LEFTMOST pair is merged
    bad = np.array([10, 20, 10, 20, 0])
    counts = np.stack([100 - bad, bad]) * np.array([1, 1, 1, 1, 0])
    cl = S.coarse_classing(counts, _edges(3), max_bins=3, min_bin_share=0.0, monotone=0)
    assert cl["edges"].tolist() == [2.0, 3.0]
    # an equal bad rate violates strict monotonicity and is pooled
    bad = np.array([10, 10, 30, 0])
    cl = S.coarse_classing(np.stack([100 - bad, bad]) * np.array([1, 1, 1, 0]), _edges(2), monotone=1)
    assert cl["edges"].tolist() == [2.0]


def test_classing_explicit_directions():
    bad = np.array([10, 30, 20, 40, 0])
    counts = np.stack([100 - bad, bad]) * np.array([1, 1, 1, 1, 0])
    up = S.coarse_classing(counts, _edges(3), monotone=1)
    assert up["direction"] == 1 and up["edges"].tolist() == [1.0, 3.0] and bool((np.diff(_rates(up)) > 0).all())
    down = S.coarse_classing(counts, _edges(3), monotone=-1)
    assert down["direction"] == -1 and len(down["edges"]) == 0 and down["dropped"]   # everything pools
    free = S.coarse_classing(counts, _edges(3), monotone=0)
    assert free["direction"] == 0 and free["edges"].tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError):
        S.coarse_classing(counts, _edges(3), monotone=2)


def test_classing_missing_cell_and_constant_column():
    bad = np.array([10, 30])
    thin = np.concatenate([np.stack([100 - bad, bad]), [[3], [1]]], axis=1)       # 4 of 204 rows missing
    cl = S.coarse_classing(thin, _edges(1))
    assert not cl["missing_own_bin"] and cl["woe"][-1] == 0.0 and cl["counts"][:, -1].tolist() == [3, 1]
    own = np.concatenate([np.stack([100 - bad, bad]), [[30], [30]]], axis=1)
    cl = S.coarse_classing(own, _edges(1))
    assert cl["missing_own_bin"] and cl["woe"][-1] < 0.0
    const = S.coarse_classing(np.array([[150, 0], [50, 0]]), np.zeros(0, F32))
    assert const["dropped"] and const["woe"].tolist() == [0.0, 0.0]
    with pytest.raises(ValueError):
        S.coarse_classing(np.array([[150, 0], [0, 0]]), np.zeros(0, F32))           # one class only
    with pytest.raises(ValueError):
        Scorecard(n_fine=255)                                                       # 257 cells do not fit uint8


def test_fit_reports_dropped_and_neutral():
    X, y = lending_like(3000)
    sc = Scorecard().fit(X, y, feature_names=list("abcdef"))
    assert sc.dropped == [False, False, False, False, False, True] and sc.beta[6] == 0.0
    rows = [r for r in sc.table() if r["feature"] == "f"]
    assert all(r["points"] == 0.0 and r["note"] == "dropped" for r in rows)
    assert [r["note"] for r in sc.table() if r["feature"] == "a"][-1] == "neutral: thin missing cell"
    assert sc.missing_own_bin[2] and all(len(z) + 1 <= sc.max_bins for z in sc.edges)
    mono = Scorecard(monotone={"a": -1}).fit(X, y, feature_names=list("abcdef"))
    assert mono.direction[0] == -1 and mono.direction[1] == sc.direction[1]


# ----------------------------------------------------------------------------------------------- Newton pass
def test_newton_pass_against_python_loop():
    args = newton_inputs(1, 200, 5, extremes=True)
    loss, g, H = S.scorecard_newton_host(*args)
    l0, g0, H0 = newton_loop(*args)
    bl, bg, bh = newton_bounds(*args)
    assert abs(loss - l0) <= bl and bool((np.abs(g - g0) <= bg).all()) and bool((np.abs(H - H0) <= bh).all())
    assert np.array_equal(H, H.T)


@pytest.mark.parametrize("eta", [40.0, -40.0, 800.0, -800.0])
def test_newton_pass_extreme_margins(eta):
    codes = np.zeros((4, 1), np.uint8)
    out = S.scorecard_newton_host(codes, [0, 2], [1.0, 0.0], np.array([0, 1, 0, 1], F32), None, [0.0, eta])
    assert all(bool(np.isfinite(np.asarray(v)).all()) for v in out)
    assert bool((np.diag(out[2]) >= 0.0).all()) and out[0] >= 0.0


# -------------------------------------------------------------------------------------------------------- fit
@pytest.fixture(scope="module")
def fitted():
    X, y = lending_like(5000)
    return X, y, Scorecard().fit(X, y)


def test_fit_meets_the_stopping_rule(fitted):
    X, y, sc = fitted
    codes = S.scorecard_encode_host(X, sc.edges)
    _, g, _ = S.scorecard_newton_host(codes, sc.cell_ptr, np.concatenate(sc.woe), y, None, sc.beta)
    assert sc.fit_info["converged"] and float(np.max(np.abs(g[:6]))) <= sc.gtol * len(y)


def test_fit_agrees_with_sklearn(fitted):
    from sklearn.linear_model import LogisticRegression

    X, y, sc = fitted
    codes = S.scorecard_encode_host(X, sc.edges)
    ptr, tab = sc.cell_ptr, np.concatenate(sc.woe)
    kept = [f for f in range(6) if not sc.dropped[f]]
    Z = np.stack([tab[ptr[f] + codes[:, f]] for f in kept], axis=1)
    try:
        lr = LogisticRegression(penalty=None, solver="newton-cholesky", tol=1e-12, max_iter=200).fit(Z, y)
    except (ValueError, TypeError):
        lr = LogisticRegression(penalty=None, solver="lbfgs", tol=1e-12, max_iter=5000).fit(Z, y)
    keep = np.array([0] + [f + 1 for f in kept])
    b_sk = np.zeros(7)
    b_sk[keep] = np.concatenate([lr.intercept_, lr.coef_[0]])
    bound = beta_distance_bound(lambda b: S.scorecard_newton_host(codes, ptr, tab, y, None, b), sc.beta, b_sk, keep)
    dist = float(np.max(np.abs(sc.beta - b_sk)))
    print(f"|beta - beta_sk|_inf = {dist:.3e}, bound {bound:.3e}")
    assert dist <= bound


# ----------------------------------------------------------------------------------------------------- points
def test_points_scale_and_sums(fitted):
    X, y, sc = fitted
    m = sc.decision_function(X)
    score = sc.score(X, rounded=False)
    assert math.isclose(sc.factor * math.log(2.0), sc.pdo) and sc.factor == 20.0 / math.log(2.0)
    lowered = sc.offset - sc.factor * (m - math.log(2.0))
    assert np.allclose(lowered - score, sc.pdo, rtol=0, atol=1e-9)
    assert math.isclose(sc.offset - sc.factor * (-math.log(sc.base_odds)), sc.base_points)   # base odds -> base points
    codes = sc.encode(X)
    attr = np.stack([sc.points[f][codes[:, f]] for f in range(6)], axis=1)
    assert np.allclose(attr.sum(1), score, rtol=0, atol=1e-9)
    ints = np.stack([sc.int_points[f][codes[:, f]] for f in range(6)], axis=1)
    assert np.array_equal(ints.sum(1), sc.score(X)) and sc.score(X).dtype == np.int32
    p = sc.predict_proba(X)
    assert np.allclose(p.sum(1), 1.0) and np.array_equal(p[:, 1] > 0.5, sc.predict(X) == 1)
    assert np.allclose(p[:, 1], 1.0 / (1.0 + np.exp(-m)))


def test_reason_codes_order_and_ties():
    sf = np.array([[3.0, 5.0, 5.0, 0.0, 1.0],      # tie between 1 and 2: the lower index first
                   [0.0, 0.0, 0.0, 0.0, 0.0],      # nothing below its maximum
                   [0.0, 2.0, 0.0, 0.0, 0.0]])
    assert S.reason_codes_host(sf, 3).tolist() == [[1, 2, 0], [-1, -1, -1], [1, -1, -1]]
    assert S.reason_codes_host(sf, 8)[0].tolist() == [1, 2, 0, 4, -1, -1, -1, -1]
    with pytest.raises(ValueError):
        S.reason_codes_host(sf, 9)


def test_reasons_point_below_maximum(fitted):
    X, y, sc = fitted
    rs = sc.reasons(X[:50], top=3)
    codes = sc.encode(X[:50])
    for i in range(50):
        short = np.array([sc.points[f].max() - sc.points[f][codes[i, f]] for f in range(6)])
        want = [f for f in np.argsort(-short, kind="stable")[:3]]
        assert rs[i].tolist() == [int(f) if short[f] > 0 else -1 for f in want]


def test_json_round_trip_is_bit_identical(fitted, tmp_path):
    X, y, sc = fitted
    path = sc.save(tmp_path / "m")
    assert path.endswith("scorecard.json")
    back = Scorecard.load(tmp_path / "m")
    assert np.array_equal(back.decision_function(X), sc.decision_function(X))
    assert np.array_equal(back.score(X), sc.score(X)) and np.array_equal(back.reasons(X), sc.reasons(X))
    assert back.table() == sc.table() or json.dumps(back.to_dict()) == json.dumps(sc.to_dict())
    with pytest.raises(ValueError):
        Scorecard.from_dict({"version": 2})


def test_ops_dispatch_to_the_host_definitions(fitted):
    X, y, sc = fitted
    codes = ops.scorecard_encode(X, sc.edges)
    assert isinstance(codes, np.ndarray) and codes.dtype == np.uint8
    assert np.array_equal(codes, S.scorecard_encode_host(X, sc.edges))
    a = ops.scorecard_newton(codes, sc.cell_ptr, np.concatenate(sc.woe), y, None, sc.beta)
    b = S.scorecard_newton_host(codes, sc.cell_ptr, np.concatenate(sc.woe), y, None, sc.beta)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_scorecard_plot(fitted):
    from cobalt_smart_lender_ai_amd.utils import plots

    fig = plots.scorecard_plot(fitted[2], "f0")
    assert len(fig.axes) == 2
    plots.close(fig)


# -------------------------------------------------------------------------------------------- CLI and service
def test_cli_scorecard(tmp_path):
    import pandas as pd

    from cobalt_smart_lender_ai_amd.cli import main

    X, y = lending_like(2000)
    df = pd.DataFrame(X[:, :5], columns=["a", "b", "c", "d", "e"])
    df["loan_default"] = y
    df.to_csv(tmp_path / "train.csv", index=False)
    df.head(20).drop(columns=["loan_default"]).to_csv(tmp_path / "rows.csv", index=False)
    out = tmp_path / "out"
    assert main(["--device", "cpu", "scorecard", str(tmp_path / "train.csv"), "--label", "loan_default", "--out",
                 str(out), "--score", str(tmp_path / "rows.csv"), "--top", "2"]) == 0
    sc = Scorecard.load(out)
    assert sc.feature_names == ["a", "b", "c", "d", "e"]
    pts = pd.read_csv(out / "scorecard_points.csv")
    assert {"feature", "bin", "label", "count", "bad_rate", "woe", "iv", "coefficient", "points"} <= set(pts.columns)
    scored = pd.read_csv(out / "scorecard_scored.csv")
    assert len(scored) == 20 and {"score", "prob_default", "reason_1", "reason_2"} <= set(scored.columns)
    assert np.array_equal(scored["score"].to_numpy(), sc.score(X[:20, :5]))


def test_service_scorecard_route(reference_booster, tmp_path):
    from fastapi.testclient import TestClient

    from cobalt_smart_lender_ai_amd.config import DEPLOYED_FEATURES, ServeConfig
    from cobalt_smart_lender_ai_amd.dataio import synth
    from cobalt_smart_lender_ai_amd.serve.app import create_app

    X, y = synth.make_lendingclub(4000, seed=3)
    sc = Scorecard().fit(X.numpy(), y.numpy(), feature_names=list(DEPLOYED_FEATURES))
    body = {f: float(v) for f, v in zip(DEPLOYED_FEATURES, X[0].tolist())}
    for f in DEPLOYED_FEATURES[12:]:
        body[f] = int(body[f])
    (tmp_path / "with").mkdir()
    sc.save(tmp_path / "with")
    app = create_app(ServeConfig(device="cpu", model_path=str(tmp_path / "with" / "model.pkl")),
                     booster=reference_booster)
    with TestClient(app) as c:
        r = c.post("/scorecard?top=3", json=body)
        assert r.status_code == 200, r.text
        j = r.json()
        row = np.array([[body[f] for f in DEPLOYED_FEATURES]], dtype=np.float32)
        assert j["score"] == int(sc.score(row)[0]) and j["prob_default"] == float(sc.predict_proba(row)[0, 1])
        assert len(j["reasons"]) <= 3 and all(r_["max_points"] > r_["points"] for r_ in j["reasons"])
        assert [r_["feature"] for r_ in j["reasons"]] == [DEPLOYED_FEATURES[f] for f in sc.reasons(row, 3)[0] if f >= 0]
        assert c.post("/predict", json=body).status_code == 200
    app = create_app(ServeConfig(device="cpu", model_path=str(tmp_path / "without" / "model.pkl")),
                     booster=reference_booster)
    with TestClient(app) as c:
        r = c.post("/scorecard", json=body)
        assert r.status_code == 404 and "scorecard.json" in r.json()["detail"]
