"""The definition of the bootstrap intervals (``metrics/bootstrap.py``) on the host: the generator, the counts,
the integer sums against independent references, the kernel's tile decomposition emulated for any tile length,
degenerate replicates, the paired comparison, the refusals and the JSON form. No GPU is needed."""
import json
import math

import numpy as np
import pytest

from cobalt_smart_lender_ai_amd import metrics
from cobalt_smart_lender_ai_amd.metrics import bootstrap as B
from cobalt_smart_lender_ai_amd.metrics.auc import roc_auc
from cobalt_smart_lender_ai_amd.metrics.classification import confusion_matrix

F32 = np.float32


def _words(hexes):
    return [int(h, 16) for h in hexes.split()]


# counter, key -> output (the Random123 known answers for Philox4x32-10)
KAT = [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = B.philox4x32_10(np.array(_words(ctr)), np.array(_words(key)))
    assert got.dtype == np.uint32 and got.tolist() == _words(want)


def test_philox_is_vectorised():
    ctr = np.array([_words(c) for c, _, _ in KAT])
    key = np.array([_words(k) for _, k, _ in KAT])
    assert B.philox4x32_10(ctr, key).tolist() == [_words(w) for _, _, w in KAT]


def test_threshold_table_is_the_scaled_poisson_cdf():
    from fractions import Fraction

    # e^-1 as an exact rational to far more digits than 2^-32 needs: the alternating series, 40 terms
    inv_e = sum(Fraction((-1) ** k, math.factorial(k)) for k in range(40))
    cdf, want = Fraction(0), []
    for k in range(B.MAX_COUNT):
        cdf += inv_e / math.factorial(k)
        want.append(int(cdf * 2 ** 32))          # floor
    assert [int(t) for t in B.POISSON1_THRESHOLDS] == want
    assert B.MAX_COUNT == 12
    assert B.poisson1_count(np.array([0, 0x5e2d58d7, 0x5e2d58d8, 0xfffffffb, 0xfffffffc, 0xffffffff])).tolist() == \
        [0, 0, 1, 11, 12, 12]


def test_count_moments():
    """Seed fixed: a regression value, not a statistical test (mean 0.9937, variance 0.9942 in a prototype)."""
    c = B.bootstrap_counts_host(0, 1 << 16, 1)[0].astype(np.float64)
    print("mean", c.mean(), "variance", c.var())
    assert abs(c.mean() - 1.0) < 0.02
    assert abs(c.var() - 1.0) < 0.02


def test_four_replicates_share_one_philox_call():
    seed, n = 0x123456789abcdef, 50
    c = B.bootstrap_counts_host(seed, n, 12)
    key = np.array([seed & 0xffffffff, seed >> 32])
    for k in range(3):
        ctr = np.stack([np.arange(n), np.full(n, k), np.zeros(n, int), np.zeros(n, int)], axis=1)
        u = B.philox4x32_10(ctr, key)
        for j in range(4):
            want = (u[:, j].astype(np.uint64)[:, None] >= B.POISSON1_THRESHOLDS[None, :]).sum(axis=1)
            assert c[4 * k + j].tolist() == want.tolist()
    assert not np.array_equal(c[0:4], c[4:8]) and not np.array_equal(c[4:8], c[8:12])
    # a window of replicates, and rows named by index, are the same counts
    assert np.array_equal(B.bootstrap_counts_host(seed, n, 5, rep0=4), c[4:9])
    assert np.array_equal(B.bootstrap_counts_host(seed, np.array([7, 3, 49]), 12), c[:, [7, 3, 49]])


def _data(rng, n, kind):
    y = rng.integers(0, 2, size=n)
    if kind == "ties":
        s = np.round(rng.random(n), 1).astype(F32)
    elif kind == "equal":
        s = np.full(n, 0.25, F32)
    else:
        s = rng.permutation(n).astype(F32) / F32(n)
    return y, s


@pytest.mark.parametrize("kind", ["ties", "equal", "distinct"])
def test_sums_against_expanded_data(kind):
    from scipy.stats import ks_2samp

    rng = np.random.default_rng(5)
    n = 200
    y, s = _data(rng, n, kind)
    y[:2] = [0, 1]
    counts = rng.poisson(1.0, size=(6, n)).astype(np.uint8)
    counts[:, :2] = 1                                   # both classes present in every replicate
    rs = B.rank_structure(y, s, 0.5)
    ints, _ = B.bootstrap_sums_host(rs, counts)
    m = B.metrics_from_sums(ints, np.zeros((2, 6)), ("auc", "gini", "ks"))
    for b in range(6):
        ye, se = np.repeat(y, counts[b]), np.repeat(s, counts[b])
        assert abs(m["auc"][b] - roc_auc(ye, se)) < 1e-12
        assert abs(m["gini"][b] - (2 * roc_auc(ye, se) - 1)) < 1e-12
        assert abs(m["ks"][b] - ks_2samp(se[ye == 1], se[ye == 0]).statistic) < 1e-12
        cm = confusion_matrix(ye, (se > F32(0.5)).astype(np.int64))
        assert (ints[4, b], ints[5, b]) == (cm[1, 1], cm[0, 1])
        assert (ints[0, b], ints[1, b]) == (cm[1].sum(), cm[0].sum())


@pytest.mark.parametrize("kind", ["ties", "equal", "distinct"])
def test_tiled_equals_direct(kind):
    rng = np.random.default_rng(11)
    n = 157
    y, s = _data(rng, n, kind)
    rs = B.rank_structure(y, s, 0.45)
    counts = B.bootstrap_counts_host(3, n, 9)
    terms = B.loss_terms(y, s)
    want, want_f = B.bootstrap_sums_host(rs, counts, terms)
    for tile in (1, 2, 7, 64, n, n + 5):
        got, got_f = B.bootstrap_sums_tiled_host(rs, counts, tile, terms)
        assert np.array_equal(got, want), (kind, tile)
        assert np.allclose(got_f, want_f, rtol=1e-13, atol=0), (kind, tile)


def test_operating_point_follows_classification_report():
    from cobalt_smart_lender_ai_amd.metrics.classification import classification_report

    rng = np.random.default_rng(2)
    y, s = _data(rng, 300, "ties")
    rep = metrics.bootstrap_ci(y, s, metrics=("error", "precision", "recall", "f1"), n_boot=4)
    want = classification_report(y, (s > F32(0.5)).astype(np.int64), output_dict=True)
    assert rep["precision"].point == want["1"]["precision"]
    assert rep["recall"].point == want["1"]["recall"]
    assert abs(rep["f1"].point - want["1"]["f1-score"]) < 1e-15
    assert abs(rep["error"].point - (1.0 - want["accuracy"])) < 1e-15
    # empty denominators give 0: nothing predicted positive, no positives
    ints = np.array([[0, 3], [4, 0], [0, 0], [0, 0], [0, 0], [0, 0]], dtype=np.int64)
    m = B.metrics_from_sums(ints, np.zeros((2, 2)), ("precision", "recall", "f1", "error", "auc"))
    assert m["precision"].tolist() == [0.0, 0.0] and m["recall"].tolist() == [0.0, 0.0]
    assert m["f1"].tolist() == [0.0, 0.0] and m["error"].tolist() == [0.0, 1.0]
    assert np.isnan(m["auc"]).all()


def test_point_estimate_is_the_all_ones_replicate():
    rng = np.random.default_rng(3)
    y, s = _data(rng, 500, "ties")
    rep = metrics.bootstrap_ci(y, s, metrics=("auc", "gini", "ks", "logloss", "brier"), n_boot=8, seed=1)
    rs = B.rank_structure(y, s)
    ints, fl = B.bootstrap_sums_host(rs, np.ones((1, 500), dtype=np.uint8), B.loss_terms(y, s))
    m = B.metrics_from_sums(ints, fl, ("auc", "gini", "ks", "logloss", "brier"))
    for k, v in m.items():
        assert rep[k].point == v[0]
    assert abs(rep["auc"].point - roc_auc(y, s)) < 1e-12
    from cobalt_smart_lender_ai_amd.metrics.classification import log_loss
    assert abs(rep["logloss"].point - log_loss(y, s)) < 1e-12
    assert abs(rep["brier"].point - np.mean((s.astype(np.float64) - y) ** 2)) < 1e-12
    assert rep["auc"].low <= rep["auc"].high and rep["auc"].values.shape == (8,)


def _degenerate_share(seed, n_boot):
    c = B.bootstrap_counts_host(seed, 3, n_boot).astype(np.int64)
    return ((c[:, 0] == 0) | (c[:, 1] + c[:, 2] == 0)), c


def test_degenerate_replicates_are_nan_and_left_out():
    y, s = np.array([0, 1, 1]), np.array([0.2, 0.9, 0.4], F32)
    seed, n_boot = 0, 200
    deg, _ = _degenerate_share(seed, n_boot)
    assert 0 < deg.sum() < n_boot / 2, deg.sum()        # the seed gives some, and fewer than half
    rep = metrics.bootstrap_ci(y, s, metrics=("auc", "ks", "recall"), n_boot=n_boot, seed=seed, alpha=0.1)
    for k in ("auc", "ks"):
        v = rep[k].values
        assert np.array_equal(np.isnan(v), deg)
        assert rep[k].n_degenerate == int(deg.sum())
        lo, hi = np.quantile(v[~deg], [0.05, 0.95])
        assert (rep[k].low, rep[k].high) == (lo, hi)
        assert rep[k].std == np.std(v[~deg], ddof=1)
    assert rep["recall"].n_degenerate == 0 and not np.isnan(rep["recall"].values).any()
    json.dumps(rep.to_dict(), allow_nan=False)


def test_paired_comparison():
    rng = np.random.default_rng(8)
    n = 400
    y = rng.integers(0, 2, size=n)
    a = (0.3 * y + 0.7 * rng.random(n)).astype(F32)
    b = (0.1 * y + 0.9 * rng.random(n)).astype(F32)
    rep = metrics.bootstrap_ci(y, a, b, metrics=("auc", "ks", "error"), n_boot=64, seed=9)
    ia, ib = rep.sums["a"][0], rep.sums["b"][0]
    assert np.array_equal(ia[:2], ib[:2])               # the same resample: equal P and N per replicate
    assert not np.array_equal(ia[2], ib[2])
    d = rep.delta["auc"]
    assert np.array_equal(d.values, rep["auc"].values - rep.metrics_b["auc"].values)
    assert d.point == rep["auc"].point - rep.metrics_b["auc"].point
    assert d.low <= d.high and 0.0 <= d.share_le_zero <= 1.0
    assert d.share_le_zero == float((d.values <= 0).mean())
    same = metrics.bootstrap_ci(y, a, a, metrics=("auc", "ks", "error"), n_boot=64, seed=9)
    for k in ("auc", "ks", "error"):
        assert np.all(same.delta[k].values == 0.0) and same.delta[k].point == 0.0
        assert same.delta[k].share_le_zero == 1.0 and (same.delta[k].low, same.delta[k].high) == (0.0, 0.0)


def test_tensors_are_taken():
    import torch

    rng = np.random.default_rng(4)
    y, s = _data(rng, 100, "ties")
    a = metrics.bootstrap_ci(y, s, n_boot=8).to_dict()
    b = metrics.bootstrap_ci(torch.from_numpy(y), torch.from_numpy(s), n_boot=8, device="cpu").to_dict()
    assert a == b


def test_refusals():
    y, s = np.array([0, 1, 1, 0]), np.array([0.1, 0.8, 0.6, 0.3], F32)
    with pytest.raises(ValueError, match="sample_weight"):
        metrics.bootstrap_ci(y, s, sample_weight=np.ones(4))
    with pytest.raises(ValueError, match="0 or 1"):
        metrics.bootstrap_ci(np.array([0, 1, 2, 0]), s)
    with pytest.raises(ValueError, match="0 or 1"):
        metrics.bootstrap_ci(np.array([0.0, 1.0, 0.5, 0.0]), s)
    with pytest.raises(ValueError, match="NaN"):
        metrics.bootstrap_ci(y, np.array([0.1, np.nan, 0.6, 0.3], F32))
    with pytest.raises(ValueError, match="n_boot"):
        metrics.bootstrap_ci(y, s, n_boot=0)
    with pytest.raises(ValueError, match="unknown metric"):
        metrics.bootstrap_ci(y, s, metrics=("auc", "lift"))
    with pytest.raises(ValueError, match="labels"):
        metrics.bootstrap_ci(y[:3], s)

    class Huge:                                         # 2^28 + 1 rows without the memory
        shape = ((1 << 28) + 1,)

    with pytest.raises(ValueError, match="2\\^28"):
        metrics.bootstrap_ci(Huge(), Huge())


def test_to_dict_round_trips_through_json():
    rng = np.random.default_rng(6)
    y, s = _data(rng, 120, "ties")
    s2 = np.clip(s + rng.normal(0, 0.3, 120), 0, 1).astype(F32)
    rep = metrics.bootstrap_ci(y, s, s2, metrics=("auc", "gini", "ks", "error", "f1", "logloss"), n_boot=16, seed=2)
    assert isinstance(rep, metrics.BootstrapReport)
    d = rep.to_dict()
    back = json.loads(json.dumps(d, allow_nan=False))
    assert back == d
    assert set(d) == {"n", "n_boot", "alpha", "seed", "threshold", "metrics", "metrics_b", "delta"}
    assert set(d["metrics"]["auc"]) == {"point", "std", "low", "high", "n_degenerate", "values"}
    assert set(d["delta"]["auc"]) == {"point", "low", "high", "share_le_zero", "n_degenerate", "values"}
    assert type(d["metrics"]["auc"]["point"]) is float and len(d["metrics"]["ks"]["values"]) == 16
    assert d["metrics"]["gini"]["point"] == 2 * d["metrics"]["auc"]["point"] - 1


def test_ci_plot():
    from cobalt_smart_lender_ai_amd.utils import plots

    rng = np.random.default_rng(7)
    y, s = _data(rng, 150, "ties")
    fig = plots.ci_plot(metrics.bootstrap_ci(y, s, s[::-1].copy(), n_boot=16))
    assert len(fig.axes) >= 1
    plots.close(fig)
