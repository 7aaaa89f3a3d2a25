"""The correlation matrix, VIF and the collinearity screen on the host path (select/collinearity.py, ops/corr_ops.py)
against pandas and the textbook definitions."""
import json

import numpy as np
import pandas as pd
import pytest
import torch

from cobalt_smart_lender_ai_amd.ops import corr_ops
from cobalt_smart_lender_ai_amd.prep import eda
from cobalt_smart_lender_ai_amd.select import (CorrelationReport, correlation_matrix, drop_correlated,
                                               vif)

from corr_cases import exact_inputs, general_inputs, moment_bound, moments_fsum


def _frame(seed=0, n=400):
    """Continuous columns at different scales with planted NaN; a constant column, an all-NaN column, a pair never
    jointly present (p, q), a column with 40 present values (below min_periods = 50) and a non-numeric column."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=n)
    df = pd.DataFrame({
        "a": a,
        "b": 0.6 * a + rng.normal(size=n),
        "loan": 1.0e4 + rng.normal(size=n),
        "small": 1e-3 * rng.normal(size=n) - 0.4 * 1e-3 * a,
        "const": np.full(n, 3.25),
        "empty": np.full(n, np.nan),
        "p": rng.normal(size=n),
        "q": rng.normal(size=n),
        "few": rng.normal(size=n),
        "count": rng.integers(0, 5, size=n),
        "grade": ["A", "B"] * (n // 2),
    })
    for c in ("a", "b", "loan", "small"):
        df.loc[rng.random(n) < 0.15, c] = np.nan
    df.loc[df.index % 2 == 0, "p"] = np.nan
    df.loc[df.index % 2 == 1, "q"] = np.nan
    df.loc[40:, "few"] = np.nan
    return df


@pytest.mark.parametrize("min_periods", [1, 2, 50])
def test_correlation_matches_pandas(min_periods):
    df = _frame()
    want = df.corr(numeric_only=True, min_periods=min_periods)
    got = eda.correlation(df, min_periods=min_periods, device="cpu")
    assert list(got.columns) == list(want.columns) and list(got.index) == list(want.index)
    g, w = got.to_numpy(), want.to_numpy()
    assert np.array_equal(np.isnan(g), np.isnan(w)), (np.isnan(g) ^ np.isnan(w)).nonzero()
    err = float(np.nanmax(np.abs(g - w)))
    print(f"min_periods={min_periods}: max |r - pandas| = {err:.3e}")
    assert err <= 1e-10
    assert np.isnan(g[:, list(got.columns).index("const")]).all()
    assert np.isnan(g[:, list(got.columns).index("empty")]).all()
    assert np.isnan(got.loc["p", "q"])
    assert np.array_equal(g, g.T, equal_nan=True)
    if min_periods == 50:
        assert np.isnan(got.loc["few", "a"]) and np.isnan(got.loc["few", "few"])
    else:
        assert got.loc["few", "few"] == 1.0 and np.isfinite(got.loc["few", "a"])


def test_report_counts_and_pairs():
    df = _frame()
    rep = correlation_matrix(df)
    num = df.select_dtypes("number")
    m = num.notna().to_numpy().astype(np.int64)
    assert rep.names == list(num.columns) and np.array_equal(rep.n, m.T @ m)
    pairs = rep.pairs(0.3)
    assert [abs(p["r"]) for p in pairs] == sorted((abs(p["r"]) for p in pairs), reverse=True)
    assert (pairs[0]["a"], pairs[0]["b"]) == ("a", "b") and pairs[0]["n"] == int(rep.n[0, 1])
    assert all(abs(p["r"]) >= 0.3 for p in pairs) and rep.pairs(1.1) == []


def test_spearman_matches_pandas_without_missing_and_listwise():
    rng = np.random.default_rng(3)
    n = 500
    ties = pd.DataFrame({"u": rng.integers(0, 4, size=n).astype(np.float64),       # heavy ties
                         "v": rng.integers(0, 7, size=n).astype(np.float64),
                         "w": np.round(rng.normal(size=n), 1),
                         "x": rng.normal(size=n)})
    ties["v"] = ties["v"] + ties["u"]
    want = ties.corr("spearman").to_numpy()
    got = correlation_matrix(ties, method="spearman")
    assert got.method == "spearman" and float(np.max(np.abs(got.r - want))) <= 1e-10
    assert float(np.max(np.abs(eda.correlation(ties, "spearman", device="cpu").to_numpy() - want))) <= 1e-10
    holes = ties.copy()
    for c in holes.columns:
        holes.loc[rng.random(n) < 0.1, c] = np.nan
    want = holes.dropna().corr("spearman").to_numpy()
    before = holes.to_numpy().copy()
    got = correlation_matrix(holes, method="spearman", missing="listwise")
    assert np.array_equal(holes.to_numpy(), before, equal_nan=True)                # blanked in a copy
    assert float(np.max(np.abs(got.r - want))) <= 1e-10
    assert int(got.n.max()) == len(holes.dropna()) == int(got.n.min())
    arr = holes.to_numpy(dtype=np.float32)
    keep = arr.copy()
    correlation_matrix(arr, method="pearson", missing="listwise")
    assert np.array_equal(arr, keep, equal_nan=True)


def test_column_ranks():
    X = np.array([[3.0, np.nan], [1.0, 2.0], [3.0, np.inf], [np.nan, 2.0], [-1.0, -0.0], [3.0, 0.0]], np.float32)
    got = corr_ops.column_ranks(X)
    assert got.dtype == torch.float32
    want = pd.DataFrame(np.where(np.isfinite(X), X, np.nan)).rank().to_numpy(dtype=np.float32)
    assert np.array_equal(got.numpy(), want, equal_nan=True)
    one = corr_ops.column_ranks(np.array([[5.0, np.nan]], np.float32))
    assert one[0, 0] == 1.0 and torch.isnan(one[0, 1])
    rng = np.random.default_rng(0)
    Y = rng.integers(0, 50, size=(1000, 3)).astype(np.float32)
    Y[rng.random(Y.shape) < 0.1] = np.nan
    assert np.array_equal(corr_ops.column_ranks(Y).numpy(), pd.DataFrame(Y).rank().to_numpy(dtype=np.float32),
                          equal_nan=True)
    with pytest.raises(ValueError, match="rows"):
        corr_ops.column_ranks(torch.empty((corr_ops.MAX_RANK_ROWS + 1, 0)))


def test_host_moments_against_fsum_and_shift_invariance():
    X, mu = exact_inputs(5, 65, 17)
    n, A, Q, P = corr_ops.pair_moments_host(X, mu)
    n0, A0, Q0, P0, _, _, _ = moments_fsum(X, mu)
    assert n.dtype == np.int64 and np.array_equal(n, n0)
    assert np.array_equal(A, A0) and np.array_equal(Q, Q0) and np.array_equal(P, P0)
    assert (n[:, 16] == 0).all() and (n[16] == 0).all() and n[0, 1] == 0 and n[0, 0] > 0
    X, mu = general_inputs(6, 300, 9)
    n, A, Q, P = corr_ops.pair_moments_host(X, mu)
    _, A0, Q0, P0, Aa, Qa, Pa = moments_fsum(X, mu)
    for got, ref, scale in ((A, A0, Aa), (Q, Q0, Qa), (P, P0, Pa)):
        assert bool((np.abs(got - ref) <= moment_bound(300, scale)).all())
    assert np.array_equal(P, P.T)
    r = corr_ops.corr_from_moments(n, A, Q, P)
    r2 = corr_ops.corr_from_moments(*corr_ops.pair_moments_host(X, mu + 0.25))     # another centre, the same r
    assert float(np.nanmax(np.abs(r - r2))) <= 1e-10
    want = pd.DataFrame(X.astype(np.float64)).corr().to_numpy()
    assert float(np.nanmax(np.abs(r - want))) <= 1e-10 and np.array_equal(r, r.T, equal_nan=True)
    assert np.nanmax(np.abs(r)) <= 1.0 and (np.diag(r) == 1.0).all()


def test_argument_checks():
    X = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="3 finite"):
        corr_ops.pair_moments(X, mu=np.zeros(2))
    with pytest.raises(ValueError, match="3 finite"):
        corr_ops.pair_moments(X, mu=np.array([0.0, np.nan, 0.0]))
    with pytest.raises(ValueError, match="method"):
        correlation_matrix(X, method="kendall")
    with pytest.raises(ValueError, match="missing"):
        correlation_matrix(X, missing="drop")
    with pytest.raises(ValueError, match="feature names"):
        correlation_matrix(X, ["a", "b"])
    with pytest.raises(ValueError, match="min_periods"):
        correlation_matrix(X, min_periods=0)


def test_vif_matches_the_regression_definition():
    rng = np.random.default_rng(2)
    n, F = 600, 7
    Z = rng.normal(size=(n, F))
    Z[:, 3] = 0.8 * Z[:, 0] - 0.5 * Z[:, 1] + 0.3 * rng.normal(size=n)
    Z[:, 6] = Z[:, 5] + 0.1 * rng.normal(size=n)
    Z = Z.astype(np.float32)
    rep = correlation_matrix(Z, [f"z{i}" for i in range(F)])
    got = rep.vif()
    assert list(got) == rep.names and got == vif(rep)
    Zd = Z.astype(np.float64)
    for j in range(F):
        others = np.column_stack([np.ones(n), np.delete(Zd, j, axis=1)])
        beta, *_ = np.linalg.lstsq(others, Zd[:, j], rcond=None)
        res = Zd[:, j] - others @ beta
        r2 = 1.0 - float(res @ res) / float(np.sum((Zd[:, j] - Zd[:, j].mean()) ** 2))
        want = 1.0 / (1.0 - r2)
        assert abs(got[f"z{j}"] - want) <= 1e-9 * want, (j, got[f"z{j}"], want)
    assert got["z6"] > 50.0 and got["z2"] < 1.1


def test_vif_refuses_duplicates_nan_and_indefinite_matrices():
    rng = np.random.default_rng(4)
    Z = rng.normal(size=(200, 4)).astype(np.float32)
    dup = np.column_stack([Z, Z[:, 1]])
    with pytest.raises(ValueError, match="smallest eigenvalue.*listwise.*duplicate"):
        vif(correlation_matrix(dup))
    const = Z.copy()
    const[:, 2] = 1.0
    with pytest.raises(ValueError, match="undefined"):
        correlation_matrix(const).vif()
    # pairwise deletion: a ~ b on one third of the rows, b ~ c on another, a ~ -c on the last: no complete data set
    # has these three correlations
    t = rng.normal(size=300)
    e = lambda: 0.05 * rng.normal(size=300)  # noqa: E731
    a, b, c = t + e(), t + e(), t + e()
    third = np.arange(300) // 100
    c = np.where(third == 2, -a + e(), c)
    P = np.column_stack([a, b, c]).astype(np.float32)
    P[third == 0, 2] = np.nan                     # rows 0..99: a, b
    P[third == 1, 0] = np.nan                     # rows 100..199: b, c
    P[third == 2, 1] = np.nan                     # rows 200..299: a, c (opposed)
    rep = correlation_matrix(P)
    assert rep.r[0, 1] > 0.9 and rep.r[1, 2] > 0.9 and rep.r[0, 2] < -0.9
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(rep.r)
    with pytest.raises(ValueError, match="not positive definite.*listwise"):
        rep.vif()


def _hand_report():
    r = np.array([[1.0, 0.9, 0.1, -0.8, np.nan],
                  [0.9, 1.0, 0.2, 0.3, np.nan],
                  [0.1, 0.2, 1.0, 0.75, np.nan],
                  [-0.8, 0.3, 0.75, 1.0, np.nan],
                  [np.nan, np.nan, np.nan, np.nan, np.nan]])
    return CorrelationReport(r=r, n=np.full((5, 5), 10, np.int64), names=["a", "b", "c", "d", "e"])


def test_drop_correlated_known_answers():
    rep = _hand_report()
    s = drop_correlated(rep, 0.7)                                  # column order: a keeps, b and d fall to a
    assert s.kept == [0, 2, 4] and s.kept_names == ["a", "c", "e"]
    assert [(d["feature"], d["by"], d["r"]) for d in s.dropped] == [("b", "a", 0.9), ("d", "a", -0.8)]
    s = drop_correlated(rep, 0.7, priority=[0.1, 0.5, 0.2, 0.9, 0.3])    # d, b, e, c, a
    assert s.kept == [3, 1, 4]
    assert [(d["feature"], d["by"], d["r"]) for d in s.dropped] == [("c", "d", 0.75), ("a", "d", -0.8)]
    s = drop_correlated(rep, 0.75, priority=[1.0, 1.0, 1.0, 1.0, 1.0])   # all tied: column order, >= at the edge
    assert s.kept == [0, 2, 4] and [d["feature"] for d in s.dropped] == ["b", "d"]
    assert drop_correlated(rep, 0.7, priority=[2, 2, 1, 1, 0]).kept == [0, 2, 4]
    assert drop_correlated(rep, 0.95).kept == [0, 1, 2, 3, 4]      # NaN (feature e) never drops, nor is dropped
    assert s.to_dict()["kept"] == ["a", "c", "e"]
    with pytest.raises(ValueError, match="priority"):
        drop_correlated(rep, 0.7, priority=[1.0, 2.0])


def test_report_round_trip():
    rep = correlation_matrix(_frame(), method="spearman", min_periods=2)
    d = json.loads(json.dumps(rep.to_dict()))
    back = CorrelationReport.from_dict(d)
    assert back.names == rep.names and back.method == "spearman"
    assert np.array_equal(back.r, rep.r, equal_nan=True) and np.array_equal(back.n, rep.n)
    assert back.to_dict() == rep.to_dict()
    assert rep.to_frame().shape == (len(rep.names),) * 2 and list(rep.to_frame().columns) == rep.names


def test_heatmap_and_cli(tmp_path, capsys):
    from cobalt_smart_lender_ai_amd import cli
    from cobalt_smart_lender_ai_amd.utils import plots

    df = _frame().drop(columns=["grade", "empty"])
    df["y"] = (np.nan_to_num(df["a"].to_numpy()) + np.random.default_rng(0).normal(size=len(df)) > 0).astype(int)
    fig = plots.correlation_heatmap(correlation_matrix(df), top=4)
    assert len(fig.axes[0].get_xticklabels()) == 4
    plots.close(fig)
    path = tmp_path / "train.csv"
    df.to_csv(path, index=False)
    out = tmp_path / "out"
    assert cli.main(["--device", "cpu", "corr", str(path), "--threshold", "0.4", "--label", "y", "--out",
                     str(out)]) == 0
    text = capsys.readouterr().out
    d = json.loads((out / "correlation.json").read_text())
    assert "y" not in d["names"] and d["method"] == "pearson" and set(d["priority"]) == set(d["names"])
    assert {"a", "b"} == {d["pairs"][0]["a"], d["pairs"][0]["b"]} and "a\tb" in text
    dropped = [x["feature"] for x in d["screen"]["dropped"]]
    assert len(dropped) == 1 and dropped[0] in ("a", "b") and "[DROP]" in text
    assert sorted(d["screen"]["kept"] + dropped) == sorted(d["names"])
