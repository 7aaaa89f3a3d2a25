"""Monotone constraints on the GPU trainer (``csrc/gbdt.hip``: ``k_eval_mono`` / ``k_eval_finish_mono``)
against the host oracle (``models/gbdt_host.py``, itself checked against a brute-force re-derivation in
test_monotone_cpu.py). Device and host evaluate the same fp64 expressions in the same order on exact
integer histograms, so the models are compared byte for byte."""
import numpy as np
import pytest
import torch

from cobalt_smart_lender_ai_amd.models import gbdt
from cobalt_smart_lender_ai_amd.models.gbdt import GBDTClassifier

from test_eval_curve_cpu import assert_same_trees
from test_monotone_cpu import check_prediction_property, check_structure, make_data

pytestmark = pytest.mark.gpu

CONS6 = (1, -1, 0, 1, 0, -1)


def make_base(n=20_000, seed=7):
    """6 features, NaNs in two of them, one feature with 256 distinct values and no NaN (a 256-bin
    feature: code 255 is a real bin); 20 000 rows are two histogram items at the root."""
    X, y = make_data(n, seed)
    r = np.random.default_rng(seed + 1)
    X[:, 5] = r.integers(0, 256, n).astype(np.float32)
    z = 0.01 * (128 - X[:, 5])
    y = np.where(r.uniform(size=n) < 0.15, (r.uniform(size=n) < 1 / (1 + np.exp(-z))).astype(np.float32), y)
    return X, y.astype(np.float32)


def both(X, y, p, **kw):
    g = gbdt.train(torch.as_tensor(X).cuda(), torch.as_tensor(y).cuda(), dict(p), device="cuda", **kw)
    c = gbdt.train(X, y, dict(p), device="cpu", **kw)
    return g, c


@pytest.fixture(scope="module")
def base():
    return make_base()


BASE = dict(n_estimators=12, max_depth=6, learning_rate=0.3, monotone_constraints=CONS6)


@pytest.mark.parametrize("extra", [
    {},
    dict(reg_alpha=0.5, gamma=1.0, subsample=0.8, colsample_bytree=0.7),
], ids=["base", "alpha_gamma_sampling"])
def test_gpu_equals_host_oracle(base, extra):
    X, y = base
    g, c = both(X, y, dict(BASE, **extra))
    assert g.save_raw("ubj") == c.save_raw("ubj")
    assert g.monotone_constraints == CONS6
    # the trees reach max depth (the max-depth leaf finalisation ran) and split on constrained features
    assert max(t.depth() for t in g.trees) == 6
    assert check_structure(g, CONS6) > 20
    assert g.save_raw("ubj") != gbdt.train(torch.as_tensor(X).cuda(), torch.as_tensor(y).cuda(),
                                          {k: v for k, v in dict(BASE, **extra).items() if k != "monotone_constraints"},
                                          device="cuda").save_raw("ubj")


def test_gpu_wide_gradients_equal_host_oracle(base):
    """grad_bits=25. The GPU's wide histogram cells exist for 32-byte row records only (9-24 features;
    cobalt_gbdt_create refuses narrower records with -6, constrained or not), so the six base features are
    followed by six noise columns: 12 features, the narrowest matrix a wide GPU fit accepts."""
    X, y = base
    X = np.concatenate([X, np.random.default_rng(3).uniform(-2, 2, (len(X), 6)).astype(np.float32)], axis=1)
    cons = CONS6 + (0, 1, 0, 0, -1, 0)
    p = dict(BASE, grad_bits=25, monotone_constraints=cons)
    g, c = both(X, y, p)
    assert g.save_raw("ubj") == c.save_raw("ubj")
    assert max(t.depth() for t in g.trees) == 6 and check_structure(g, cons) > 20
    assert g.save_raw("ubj") != gbdt.train(torch.as_tensor(X).cuda(), torch.as_tensor(y).cuda(), dict(p, grad_bits=17),
                                          device="cuda").save_raw("ubj")


def test_gpu_grouped_evaluation_equals_host_oracle():
    """40 features: the grouped evaluation (5 groups of 8 features + the per-node reduction), constraints on
    features of different groups."""
    r = np.random.default_rng(5)
    N, F = 6000, 40
    X = r.uniform(-2, 2, (N, F)).astype(np.float32)
    z = 1.5 * np.sin(2 * X[:, 0]) + X[:, 9] - 0.8 * X[:, 17] + 0.6 * X[:, 26] * X[:, 3] - np.cos(2 * X[:, 39])
    y = (r.uniform(size=N) < 1 / (1 + np.exp(-z))).astype(np.float32)
    X[r.uniform(size=N) < 0.05, 9] = np.nan
    X[r.uniform(size=N) < 0.05, 39] = np.nan
    cons = [0] * F
    for f, c in ((0, 1), (9, -1), (17, 1), (26, -1), (39, 1)):
        cons[f] = c
    g, c = both(X, y, dict(n_estimators=6, max_depth=5, learning_rate=0.3, monotone_constraints=tuple(cons)))
    assert g.save_raw("ubj") == c.save_raw("ubj")
    assert check_structure(g, cons) > 10


def test_context_reuse_clears_the_constraints(base):
    """Trainer contexts are cached by shape: free, constrained, free again on one context."""
    X, y = base
    Xg, yg = torch.as_tensor(X).cuda(), torch.as_tensor(y).cuda()
    free_p = {k: v for k, v in BASE.items() if k != "monotone_constraints"}
    first = gbdt.train(Xg, yg, dict(free_p), device="cuda").save_raw("ubj")
    mono = gbdt.train(Xg, yg, dict(BASE), device="cuda").save_raw("ubj")
    third = gbdt.train(Xg, yg, dict(free_p), device="cuda").save_raw("ubj")
    zeros = gbdt.train(Xg, yg, dict(free_p, monotone_constraints=(0,) * 6), device="cuda").save_raw("ubj")
    assert first == third == zeros
    assert mono != first
    assert first == gbdt.train(X, y, dict(free_p), device="cpu").save_raw("ubj")


def test_prediction_property_on_the_gpu(base):
    X, y = base
    rep = gbdt.FitReport()
    b = gbdt.train(torch.as_tensor(X).cuda(), torch.as_tensor(y).cuda(), dict(BASE), device="cuda", report=rep)
    Xh = make_base(200, 8)[0]

    def predict(Xs):
        return b.predict_margin(torch.as_tensor(Xs).cuda(), device="cuda").cpu().numpy()
    check_prediction_property(predict, rep.extra["cuts"].cpu().numpy(), rep.extra["nbins"].cpu().numpy(), Xh, CONS6)


def test_classifier_early_stopping_under_constraints():
    import pandas as pd

    X, y = make_base(5000, 9)
    Xv, yv = make_base(1500, 10)
    names = [f"x{i}" for i in range(6)]
    by_name = {n: c for n, c in zip(names, CONS6) if c}
    kw = dict(n_estimators=40, max_depth=4, learning_rate=0.5, device="cuda", monotone_constraints=by_name)
    df, dfv = pd.DataFrame(X, columns=names), pd.DataFrame(Xv, columns=names)
    full = GBDTClassifier(**kw).fit(df, y).get_booster()
    clf = GBDTClassifier(early_stopping_rounds=5, **kw).fit(df, y, eval_set=[(dfv, yv)])
    b = clf.get_booster()
    assert b.num_trees < full.num_trees and b.num_trees == clf.best_iteration + 1 + 5
    assert b.monotone_constraints == CONS6
    # a byte-identical prefix of the full constrained fit (the stopped model also carries best_iteration)
    assert_same_trees(b.trees, full.trees[: b.num_trees])
    plain = b.slice(b.num_trees)
    plain.attributes.clear()
    assert plain.save_raw("ubj") == full.slice(b.num_trees).save_raw("ubj")
    assert check_structure(b, CONS6) > 10
