"""Monotone constraints on the host trainer (``models/gbdt_host.py``, the oracle of the GPU kernels):
parsing, an independent brute-force re-derivation of the constrained grower, the structural and the
prediction property, round trips, RFE, the refused combinations and sklearn's constrained engine.

The host trainer costs seconds per fit, so the fits are small (<= 2000 rows, <= 12 trees, depth <= 4)
and shared by the tests of this module."""
import dataclasses
import math

import numpy as np
import pytest

from cobalt_smart_lender_ai_amd.metrics.auc import roc_auc
from cobalt_smart_lender_ai_amd.models import gbdt, gbdt_host
from cobalt_smart_lender_ai_amd.models.booster import Booster, predict_margin_host
from cobalt_smart_lender_ai_amd.models.gbdt import GBDTClassifier, GBDTParams, resolve_monotone

CONS = (1, -1, 0, 0, 0, 0)
FIT = dict(n_estimators=10, max_depth=4, learning_rate=0.3)


def make_data(n, seed):
    r = np.random.default_rng(seed)
    X = r.uniform(-2, 2, (n, 6)).astype(np.float32)
    z = 2 * np.sin(3 * X[:, 0]) + 0.8 * X[:, 0] - X[:, 1] + 0.5 * X[:, 2] * X[:, 3]
    y = (r.uniform(size=n) < 1 / (1 + np.exp(-z))).astype(np.float32)
    X[r.uniform(size=n) < 0.05, 0] = np.nan
    X[r.uniform(size=n) < 0.05, 1] = np.nan
    return X, y


def check_structure(b: Booster, cons) -> int:
    """At every split on a feature with c = +1: max leaf of the left subtree <= min leaf of the right one
    (reversed for c = -1). Returns the number of constrained splits seen."""
    seen = 0
    for t in b.trees:
        def leaves(i):
            if t.left_children[i] == -1:
                return [t.split_conditions[i]]
            return leaves(t.left_children[i]) + leaves(t.right_children[i])
        for i in range(len(t.left_children)):
            if t.left_children[i] == -1 or cons[t.split_indices[i]] == 0:
                continue
            lo, hi = leaves(t.left_children[i]), leaves(t.right_children[i])
            if cons[t.split_indices[i]] < 0:
                lo, hi = hi, lo
            assert max(lo) <= min(hi), f"split on feature {t.split_indices[i]}"
            seen += 1
    return seen


def sweep_values(cuts_f: np.ndarray) -> np.ndarray:
    c = np.asarray(cuts_f, dtype=np.float32)
    return np.unique(np.concatenate([c[np.isfinite(c)], np.float32([-3.0, 3.0])]))


def check_prediction_property(predict, cuts: np.ndarray, nbins: np.ndarray, Xh: np.ndarray, cons) -> None:
    """Each constrained feature replaced by every cut value and +-3, ascending: the margins of every row
    never move against the constraint. Exact: every tree is monotone in float32 and float32 addition in a
    fixed order is monotone in each operand."""
    for f, c in enumerate(cons):
        if c == 0:
            continue
        prev = None
        for v in sweep_values(cuts[f, : int(nbins[f])]):
            Xs = Xh.copy()
            Xs[:, f] = v
            m = predict(Xs)
            if prev is not None:
                assert np.all(m >= prev) if c > 0 else np.all(m <= prev), f"feature {f} at {v}"
            prev = m


@pytest.fixture(scope="module")
def data():
    return make_data(2000, 0)


@pytest.fixture(scope="module")
def holdout():
    return make_data(200, 1)[0]


@pytest.fixture(scope="module")
def fits(data):
    """The shared fits: unconstrained and constrained, with the constrained fit's cuts."""
    X, y = data
    rep = gbdt.FitReport()
    free = gbdt.train(X, y, dict(FIT), device="cpu")
    mono = gbdt.train(X, y, dict(FIT, monotone_constraints=CONS), device="cpu", report=rep)
    return free, mono, rep.extra["cuts"].numpy(), rep.extra["nbins"].numpy()


# ------------------------------------------------------------------------------- 1. parsing
def test_accepted_forms_resolve_to_one_vector():
    names = [f"x{i}" for i in range(6)]
    want = np.array(CONS, dtype=np.int8)
    for form in (CONS, list(CONS), np.array(CONS), "(1,-1,0,0,0,0)", " ( 1, -1, 0, 0, 0, 0 ) ", {"x0": 1, "x1": -1}):
        got = resolve_monotone(form, 6, names)
        assert got.dtype == np.int8 and np.array_equal(got, want), form
    for form in (None, (), "()", "", {}, (0,) * 6, "(0,0,0,0,0,0)", {"x3": 0}):
        assert resolve_monotone(form, 6, names) is None, form
    assert GBDTParams.from_kwargs(monotone_constraints="(1,-1)").monotone_constraints == "(1,-1)"


@pytest.mark.parametrize("form, names", [
    ((1, -1, 0), None),                      # a length other than the feature count
    ("(1,-1,0,0,0,0,0)", None),
    ((1, -1, 0, 0, 0, 2), None),             # a value outside {-1, 0, 1}
    ((1, -1, 0, 0, 0, 0.5), None),
    ("(1,-1,0,0,0,x)", None),
    ({"x0": 1}, None),                       # a dict without feature names
    ({"nope": 1}, [f"x{i}" for i in range(6)]),   # ... with an unknown name
    ({"x0": 3}, [f"x{i}" for i in range(6)]),
])
def test_invalid_constraints_raise(form, names):
    with pytest.raises(ValueError, match="monotone_constraints"):
        resolve_monotone(form, 6, names)
    X, y = make_data(64, 3)
    with pytest.raises(ValueError, match="monotone_constraints"):
        gbdt.train(X, y, dict(n_estimators=1, max_depth=2, monotone_constraints=form), device="cpu",
                   feature_names=names)


def test_empty_forms_equal_the_unconstrained_fit_and_constraints_change_the_model():
    X, y = make_data(600, 4)
    p = dict(n_estimators=3, max_depth=3)
    free = gbdt.train(X, y, dict(p), device="cpu").save_raw("ubj")
    for form in ((0,) * 6, None, (), "()"):
        assert gbdt.train(X, y, dict(p, monotone_constraints=form), device="cpu").save_raw("ubj") == free, form
    # (the key was dropped before the feature existed: the constrained model equalled the free one)
    mono = gbdt.train(X, y, dict(p, monotone_constraints="(1,-1,0,0,0,0)"), device="cpu")
    assert mono.save_raw("ubj") != free
    assert mono.monotone_constraints == CONS


# --------------------------------------------------------------- 2. independent re-derivation
def brute_force_tree(bins, cuts, nbins, gq, hq, p, cons):
    """The constrained grower of the issue in plain loops over (node, feature, bin, direction), straight
    from ``bins`` / ``gq`` / ``hq``: no histograms, no subtraction, no vector code."""
    D, lam, alpha, mcw = p.max_depth, p.reg_lambda, p.reg_alpha, p.min_child_weight
    ginv, hinv = 1.0 / p.gscale, 1.0 / p.hscale
    N, F = bins.shape

    def thr(g):
        if alpha == 0.0:
            return g
        return g - alpha if g > alpha else (g + alpha if g < -alpha else 0.0)

    def weight(g, h, lo, hi):
        w = 0.0 if (h < mcw or h <= 0.0) else -thr(g) / (h + lam)
        return min(max(w, lo), hi)

    def gw(g, h, w):
        return -(2.0 * thr(g) * w + (h + lam) * w * w)

    out = {}
    work = [(0, list(range(N)), -math.inf, math.inf, 0, 1)]
    while work:
        n, rows, lo, hi, level, build = work.pop(0)
        G, H = sum(int(gq[r]) for r in rows), sum(int(hq[r]) for r in rows)
        Gd, Hd = G * ginv, H * hinv
        wn = weight(Gd, Hd, lo, hi)
        rec = dict(G=G, H=H, start=0, count=len(rows), build=build, status=3, feat=-1, bin=-1, default_left=0,
                   loss_chg=np.float32(0), leaf_value=np.float32(0), sum_hess=np.float32(Hd),
                   base_weight=np.float32(wn * p.eta))
        best = None
        if level < D:
            pg = 0.0 if Hd < mcw else gw(Gd, Hd, wn)
            for f in range(F):
                nb = int(nbins[f])
                miss = [r for r in rows if bins[r, f] == 255 and nb < 256]
                mg, mh = sum(int(gq[r]) for r in miss), sum(int(hq[r]) for r in miss)
                for direction in ((0, 1) if (mg != 0 or mh != 0) else (0,)):
                    for b in range(nb):
                        # direction 0: left = bins <= b; direction 1: left = bins <= b - 1, + the missing rows
                        j = b if direction == 0 else b - 1
                        left = [r for r in rows if r not in miss and bins[r, f] <= j]
                        GL, HL = sum(int(gq[r]) for r in left), sum(int(hq[r]) for r in left)
                        if direction == 1:
                            GL, HL = GL + mg, HL + mh
                        gl, hl, gr, hr = GL * ginv, HL * hinv, (G - GL) * ginv, (H - HL) * hinv
                        if not (hl >= mcw and hr >= mcw):
                            continue
                        wl, wr = weight(gl, hl, lo, hi), weight(gr, hr, lo, hi)
                        if (cons[f] > 0 and wl > wr) or (cons[f] < 0 and wl < wr):
                            continue
                        gain = gw(gl, hl, wl) + gw(gr, hr, wr) - pg
                        key = f * 1024 + (b if direction == 0 else 512 + (nb - 1 - b))
                        if best is None or gain > best[0] or (gain == best[0] and key < best[1]):
                            best = (gain, key, f, j, direction, wl, wr)
        if best is not None and np.float32(best[0]) > np.float32(1e-6) and np.float32(best[0]) >= np.float32(p.gamma):
            gain, _, f, j, dl, wl, wr = best
            rec.update(status=2, feat=f, bin=j, default_left=dl, loss_chg=np.float32(gain),
                       split_cond=cuts[f, j] if j >= 0 else -gbdt_host.FLT_MAX)
            go_left = [(dl == 1) if (bins[r, f] == 255 and int(nbins[f]) < 256) else bins[r, f] <= j for r in rows]
            mid = (wl + wr) / 2
            lb, rb = ((lo, mid), (mid, hi)) if cons[f] > 0 else (((mid, hi), (lo, mid)) if cons[f] < 0 else ((lo, hi),) * 2)
            left, right = [r for r, g in zip(rows, go_left) if g], [r for r, g in zip(rows, go_left) if not g]
            small = sum(int(hq[r]) for r in left) <= sum(int(hq[r]) for r in right)  # the child built from rows
            work.append((2 * n + 1, left, lb[0], lb[1], level + 1, 1 if small else 0))
            work.append((2 * n + 2, right, rb[0], rb[1], level + 1, 0 if small else 1))
        else:
            rec.update(leaf_value=np.float32(wn * p.eta), split_cond=np.float32(wn * p.eta))
        out[n] = rec
    return out


@pytest.mark.parametrize("alpha", [0.0, 0.5])
def test_brute_force_grower_reproduces_the_host_tree(alpha):
    r = np.random.default_rng(11)
    N = 200
    X = r.uniform(-2, 2, (N, 3)).astype(np.float32)
    y = (r.uniform(size=N) < 1 / (1 + np.exp(-(1.5 * X[:, 0] - X[:, 1] + np.sin(2 * X[:, 2]))))).astype(np.float32)
    X[r.uniform(size=N) < 0.1, 1] = np.nan
    cons = np.array([1, -1, 0], dtype=np.int8)
    bd = gbdt.bin_dataset(X, max_bin=16, device="cpu")
    cuts, nbins = bd.cuts.numpy(), bd.nbins.numpy()
    gs, hs = gbdt_host.quant_scales(1.0)
    p = gbdt_host.HostGbdtParams(max_depth=2, eta=0.3, reg_lambda=1.0, reg_alpha=alpha, gamma=0.0, min_child_weight=1.0,
                                 subsample=1.0, seed=0, gscale=gs, hscale=hs, monotone=cons)
    margin = np.zeros(N, dtype=np.float32)
    splits = 0
    for tree in range(2):  # the second tree starts from the first one's (constrained) leaves
        gq, hq = gbdt_host.gradients_host(margin, y, np.ones(N, np.float32), p, tree)
        want = brute_force_tree(bd.bins_host, cuts, nbins, gq, hq, p, cons)
        nodes = gbdt_host.grow_tree_host(bd.bins_host, cuts, nbins, gq, hq, margin, p, np.ones(3, np.uint8))
        assert sorted(want) == [int(i) for i in np.nonzero(nodes["status"])[0]]
        for n, rec in want.items():
            for k, v in rec.items():
                assert nodes[n][k] == v, f"tree {tree} node {n} field {k}: {nodes[n][k]} != {v}"
            splits += rec["status"] == 2
    assert splits >= 4  # (both levels split: the children's bounds were in use)


# --------------------------------------------------------------------- 3. / 4. the properties
def test_structure(fits):
    free, mono, _, _ = fits
    assert check_structure(mono, CONS) > 20
    with pytest.raises(AssertionError):  # (the check can fail: the free model breaks it)
        check_structure(free, CONS)


def test_prediction_property(fits, holdout):
    free, mono, cuts, nbins = fits
    check_prediction_property(lambda Xs: predict_margin_host(mono, Xs), cuts, nbins, holdout, CONS)
    with pytest.raises(AssertionError):
        check_prediction_property(lambda Xs: predict_margin_host(free, Xs), cuts, nbins, holdout, CONS)


def test_exact_fp64_mode_supports_constraints(data, holdout):
    X, y = data
    rep = gbdt.FitReport()
    b = gbdt.train(X[:800], y[:800], dict(n_estimators=4, max_depth=3, monotone_constraints=CONS), device="cpu",
                   exact_fp64=True, report=rep)
    assert check_structure(b, CONS) > 4
    check_prediction_property(lambda Xs: predict_margin_host(b, Xs), rep.extra["cuts"].numpy(),
                              rep.extra["nbins"].numpy(), holdout[:50], CONS)


# -------------------------------------------------------------------------- 5. round trips
def test_model_round_trips(fits, data, tmp_path):
    _, mono, _, _ = fits
    raw = mono.save_raw("ubj")
    cfg = mono.to_doc()["Config"]["learner"]["gradient_booster"]["tree_train_param"]
    assert cfg["monotone_constraints"] == "(1,-1,0,0,0,0)"
    for fmt in ("ubj", "json"):
        back = Booster.load_raw(mono.save_raw(fmt))
        assert back.monotone_constraints == CONS and back.save_raw("ubj") == raw
    assert mono.slice(3).monotone_constraints == CONS
    free = fits[0]
    assert free.to_doc()["Config"]["learner"]["gradient_booster"]["tree_train_param"]["monotone_constraints"] == "()"
    assert Booster.load_raw(free.save_raw("ubj")).monotone_constraints is None


def test_classifier_params_clone_and_pickle(data, tmp_path):
    from sklearn.base import clone

    X, y = data
    with pytest.raises(TypeError):
        GBDTClassifier(no_such_parameter=1)
    clf = GBDTClassifier(n_estimators=3, max_depth=3, device="cpu", monotone_constraints=CONS)
    assert clf.get_params()["monotone_constraints"] == CONS
    # (listed when set: an estimator without constraints keeps the parameter set it had before)
    assert "monotone_constraints" not in GBDTClassifier(n_estimators=3).get_params()
    assert clone(clf).set_params(monotone_constraints=None).get_params() == GBDTClassifier(
        n_estimators=3, max_depth=3, device="cpu").get_params()
    assert clone(clf).monotone_constraints == CONS
    assert clone(clf).set_params(monotone_constraints="(0,0,0,0,0,1)").monotone_constraints == "(0,0,0,0,0,1)"
    clf.fit(X[:600], y[:600])
    want = gbdt.train(X[:600], y[:600], dict(n_estimators=3, max_depth=3, monotone_constraints=CONS), device="cpu")
    assert clf.get_booster().save_raw("ubj") == want.save_raw("ubj")
    path = tmp_path / "m.pkl"
    clf.save_pickle(path)
    back = GBDTClassifier.load_pickle(path)
    assert back.monotone_constraints == "(1,-1,0,0,0,0)"  # (a sequence is stored in XGBoost's string form)
    assert np.array_equal(resolve_monotone(back.monotone_constraints, 6), CONS)
    assert back.get_booster().monotone_constraints == CONS
    assert back.get_booster().save_raw("ubj") == want.save_raw("ubj")


def test_checkpoints(tmp_path):
    X, y = make_data(600, 5)
    p = dict(n_estimators=4, max_depth=3, monotone_constraints=CONS)
    whole = gbdt.train(X, y, dict(p), device="cpu").save_raw("ubj")
    path = str(tmp_path / "ck.ubj")
    # a fit that checkpoints every 2 trees equals the uninterrupted one ...
    assert gbdt.train(X, y, dict(p), device="cpu", checkpoint_path=path, checkpoint_every=2).save_raw("ubj") == whole
    # ... a resume from its first half (the checkpoint of a 2-tree fit) too ...
    path2 = str(tmp_path / "half.ubj")
    gbdt.train(X, y, dict(p, n_estimators=2), device="cpu", checkpoint_path=path2, checkpoint_every=2)
    assert gbdt.train(X, y, dict(p), device="cpu", checkpoint_path=path2, checkpoint_every=2).save_raw("ubj") == whole
    # ... and other constraints (or none) are refused like any other parameter change
    for other in ((1, 1, 0, 0, 0, 0), None):
        with pytest.raises(ValueError, match="different parameters"):
            gbdt.train(X, y, dict(p, monotone_constraints=other), device="cpu", checkpoint_path=path2, checkpoint_every=2)
    # the same constraints in another form are the same parameter
    gbdt.train(X, y, dict(p, monotone_constraints="(1,-1,0,0,0,0)"), device="cpu", checkpoint_path=path2,
               checkpoint_every=2)


# ---------------------------------------------------------------------------------- 6. RFE
def test_rfe_repack_and_dict_form():
    from cobalt_smart_lender_ai_amd.select.rfe import rfe

    r = np.random.default_rng(21)
    N = 800
    X = r.uniform(-2, 2, (N, 8)).astype(np.float32)
    z = 1.5 * X[:, 0] - X[:, 1] + 0.7 * X[:, 4] + 0.5 * X[:, 6] * X[:, 7] + np.sin(3 * X[:, 5])
    y = (r.uniform(size=N) < 1 / (1 + np.exp(-z))).astype(np.float32)
    X[r.uniform(size=N) < 0.05, 1] = np.nan
    names = [f"f{i}" for i in range(8)]
    cons = (1, -1, 1, 0, 1, 0, 0, -1)   # (f2 and f3 are noise: constrained features get eliminated too)
    p = GBDTParams(n_estimators=3, max_depth=3, monotone_constraints=cons)
    packed = rfe(X, y, p, n_features_to_select=5, device="cpu", feature_names=names, repack=True)
    masked = rfe(X, y, p, n_features_to_select=5, device="cpu", feature_names=names, repack=False)
    assert np.array_equal(packed.support_, masked.support_) and packed.n_features_ == 5
    assert packed.estimator_.save_raw("ubj") == masked.estimator_.save_raw("ubj")
    assert packed.estimator_.monotone_constraints == cons
    by_name = dataclasses.replace(p, monotone_constraints={n: c for n, c in zip(names, cons) if c})
    named = rfe(X, y, by_name, n_features_to_select=5, device="cpu", feature_names=names, repack=True)
    assert named.estimator_.save_raw("ubj") == packed.estimator_.save_raw("ubj")
    assert check_structure(packed.estimator_, cons) > 0


# ----------------------------------------------------------------------------- 7. refusals
def test_refused_combinations():
    from cobalt_smart_lender_ai_amd.models import external, stream
    from cobalt_smart_lender_ai_amd.parallel import loopback

    X, y = make_data(256, 6)
    p = dict(n_estimators=1, max_depth=2, monotone_constraints=CONS)
    src = stream.array_chunks(X, y, 128)
    with pytest.raises(ValueError, match="monotone_constraints"):
        stream.train_stream(src, dict(p), device="cpu")
    with pytest.raises(ValueError, match="monotone_constraints"):
        external.train_external(src, dict(p), device="cpu")

    class OneRank:  # any dist object refuses, before it is used
        world, rank = 1, 0
    with pytest.raises(ValueError, match="monotone_constraints"):
        gbdt.train(X, y, dict(p), device="cpu", dist=OneRank())
    with pytest.raises(ValueError, match="monotone_constraints"):
        gbdt.train_binned(gbdt.bin_dataset(X, device="cpu"), y, dict(p), dist=OneRank())
    # all-zero constraints are no constraints: nothing to refuse
    stream.train_stream(src, dict(p, monotone_constraints=(0,) * 6), device="cpu")


# -------------------------------------------------------------------- 8. independent engine
# Held-out AUC (2000 rows of seed + 100) of the constrained fits on 2000 rows, 12 trees, depth 4, eta 0.3,
# ours (device="cpu") vs sklearn's HistGradientBoostingClassifier(monotonic_cst=...), five seeds:
#   seed   ours     sklearn   gap (sklearn - ours)
#   0      0.7637   0.7695    +0.0059
#   1      0.7570   0.7621    +0.0051
#   2      0.7463   0.7545    +0.0082
#   3      0.7257   0.7272    +0.0016
#   4      0.7714   0.7694    -0.0019
# The engines differ in binning (sklearn bins a subsample's quantiles and keeps missing values in a bin of their
# own) and in growth order (sklearn grows leaf-wise under max_depth). Margin = the mean gap (0.0038) + the
# spread of the gap over the seeds (max - min = 0.0101), rounded up: 0.014. The test runs seed 0.
AUC_MARGIN = 0.014


def test_auc_against_sklearn_constrained_engine(data):
    from sklearn.ensemble import HistGradientBoostingClassifier

    X, y = data
    Xh, yh = make_data(2000, 100)
    ours = gbdt.train(X, y, dict(n_estimators=12, max_depth=4, learning_rate=0.3, monotone_constraints=CONS), device="cpu")
    sk = HistGradientBoostingClassifier(monotonic_cst=list(CONS), max_iter=12, max_depth=4, learning_rate=0.3,
                                        early_stopping=False, random_state=0).fit(X, y)
    a_ours = roc_auc(yh, ours.predict_proba(Xh, device="cpu"))
    a_sk = roc_auc(yh, sk.predict_proba(Xh)[:, 1])
    print(f"constrained held-out AUC: ours {a_ours:.4f}, sklearn {a_sk:.4f}, gap {a_sk - a_ours:+.4f}")
    assert a_ours >= a_sk - AUC_MARGIN
