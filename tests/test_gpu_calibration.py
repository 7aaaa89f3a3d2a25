"""The calibration kernels (csrc/calib.hip) against their host definitions (metrics/calibration.py): hull vertex
lists and reliability tables compared as integers, applied values as float32 bit patterns, never a tolerance.

Which test catches which mistake in the kernel:
  a merge that stops too early, or pops with a non-strict / reversed test ...... test_hull (random, sorted, ties)
  links or alive bytes stale after a pop; head or tail of a run popped ........... test_hull (antisorted, long_block)
  the last, partial tile; a tile of one point; m at a tile edge .................. test_hull (T - 1, T, T + 1, 2 T + 1)
  tile offsets, the gather, device counts feeding the second round ............... test_hull (40 T + 5)
  a final stage that assumes the survivors fit a tile ............................ test_hull_no_tile_sheds_a_point
  a 32-bit product or a signed staging of cw / cs ................................ test_hull_weight_bound
  search off by one at a knot, clip, NaN, the K = 1 / K = 2 paths, FMA contraction test_apply
  LDS staging against the global fallback ........................................ test_apply (cap, cap + 1)
  the 16-byte path's tail rows; an unaligned view ................................. test_apply (N = 1 .. 4099), test_apply_unaligned
  bin of p on an edge, p = 0, p = 1; a 32-bit Pq; the flush per weighted tile .... test_reliability_sums
  LDS counters against direct adds ................................................ test_reliability_sums (2048, 2049, 4096)
  `out` overwritten instead of added to ........................................... test_reliability_accumulates
  a launch before the arguments are checked ....................................... test_refusals
"""
import functools

import numpy as np
import pytest
import torch

import calibration_cases as cc
from cobalt_smart_lender_ai_amd.metrics import calibration as C
from cobalt_smart_lender_ai_amd.models import calibration as MC
from cobalt_smart_lender_ai_amd.ops import calib_ops

pytestmark = pytest.mark.gpu

F32 = np.float32


@functools.lru_cache(maxsize=None)
def _tile() -> int:
    return calib_ops.iso_tile_rows()


def _size(expr: str) -> int:
    return int(eval(expr, {"T": _tile(), "CAP": calib_ops.calib_lds_knots() if "CAP" in expr else 0}))


def _device_hull(cw, cs, **kw):
    return calib_ops.iso_hull(torch.from_numpy(cw).cuda(), torch.from_numpy(cs).cuda(), **kw)


N_CASES = ("1", "2", "3", "T-1", "T", "T+1", "2*T+1", "40*T+5")


@pytest.mark.parametrize("pattern", cc.PATTERNS)
@pytest.mark.parametrize("n_expr", N_CASES)
def test_hull(n_expr, pattern):
    n = _size(n_expr)
    cw, cs = cc.hull_case(pattern, n)
    got, rounds = _device_hull(cw, cs, return_rounds=True)
    assert got.dtype == torch.int32
    assert torch.equal(got.cpu(), torch.from_numpy(C.iso_hull_host(cw, cs)))
    if len(cw) > _tile():
        assert len(rounds) == calib_ops.iso_rounds() == C.HULL_ROUNDS
        assert len(cw) >= rounds[0] >= rounds[1] >= got.shape[0]
    else:
        assert rounds is None


def test_hull_smooth_score_sheds_as_expected():
    """Rows from a logistic model through the whole plumbing: after one round a tile keeps a handful of points."""
    s, y = cc.smooth_rows(40 * _tile() + 5)
    ux, cw, cs = C.iso_groups(s, y)
    got, rounds = _device_hull(cw, cs, return_rounds=True)
    assert torch.equal(got.cpu(), torch.from_numpy(C.iso_hull_host(cw, cs)))
    tiles = -(-len(cw) // _tile())
    assert rounds[0] <= 40 * tiles          # measured on the host: 7 to 11 a tile


def test_hull_no_tile_sheds_a_point():
    cw, cs = cc.convex_case(3 * _tile())
    got, rounds = _device_hull(cw, cs, return_rounds=True)
    assert rounds == [3 * _tile() + 1] * 2
    assert torch.equal(got.cpu(), torch.arange(3 * _tile() + 1, dtype=torch.int32))


def test_hull_weight_bound():
    cw, cs = cc.weighted_case(2 * _tile() + 1, cc.MAX_TOTAL)
    assert int(cw[-1]) == (1 << 31) - 1
    assert torch.equal(_device_hull(cw, cs).cpu(), torch.from_numpy(C.iso_hull_host(cw, cs)))
    cw, cs = cc.weighted_case(2 * _tile() + 1, 1 << 31)
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        _device_hull(cw, cs)
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        _device_hull(cw, cs, total_weight=1 << 31)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n_expr", ["7", "T+1", "40*T+5"])
def test_isotonic_fit_equals_host(n_expr, weighted):
    n = _size(n_expr)
    s, y = cc.smooth_rows(n)
    s = np.round(s, 3).astype(F32)                      # some equal scores
    w = (np.random.default_rng(n).random(n) * (np.arange(n) % 5 > 0)) if weighted else None   # zero weights too
    host = MC.IsotonicCalibrator().fit(s, y, w)
    dev = MC.IsotonicCalibrator().fit(torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda(),
                                      None if w is None else torch.from_numpy(w).cuda())
    assert np.array_equal(dev.x_thresholds_.view(np.int32), host.x_thresholds_.view(np.int32))
    assert np.array_equal(dev.y_thresholds_.view(np.int64), host.y_thresholds_.view(np.int64))
    q = torch.linspace(-4, 4, 1001)
    assert torch.equal(dev.transform(q.cuda()).cpu().view(torch.int32), host.transform(q).view(torch.int32))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
@pytest.mark.parametrize("k_expr", ["1", "2", "37", "CAP", "CAP+1"])
def test_apply(k_expr, n):
    xk, vk, x = cc.apply_case(_size(k_expr), n)
    got = calib_ops.calib_apply(torch.from_numpy(x).cuda(), torch.from_numpy(xk).cuda(), torch.from_numpy(vk).cuda())
    want = C.calib_apply_host(x, xk, vk)
    assert got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


def test_apply_on_every_knot_and_unaligned():
    xk, vk, _ = cc.apply_case(300, 8)
    x = np.concatenate([xk, np.nextafter(xk, F32(np.inf)), np.nextafter(xk, F32(-np.inf))]).astype(F32)
    want = C.calib_apply_host(x, xk, vk)
    assert np.array_equal(want[:300], vk.astype(F32))
    buf = torch.zeros(x.shape[0] + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(x).cuda()
    for xt in (buf[1:].clone(), buf[1:]):               # 16-byte aligned, then 4 bytes off
        got = calib_ops.calib_apply(xt, torch.from_numpy(xk).cuda(), torch.from_numpy(vk).cuda())
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B", [1, 2, 10, 2048, 2049, 4096])
def test_reliability_sums(B, weighted):
    n = 3 * 2048 + 5
    p, y, wq, edges = cc.reliability_case(n, B, weighted=weighted)
    got = calib_ops.reliability_sums(torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda(),
                                     None if wq is None else torch.from_numpy(wq).cuda(),
                                     torch.from_numpy(edges).cuda())
    want = C.reliability_sums_host(p, y, wq, edges)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.from_numpy(want))


def test_reliability_accumulates_over_chunks():
    p, y, wq, edges = cc.reliability_case(5000, 10, weighted=True)
    e = torch.from_numpy(edges).cuda()
    pt, yt, wt = (torch.from_numpy(a).cuda() for a in (p, y, wq))
    out = torch.zeros((3, 10), dtype=torch.int64, device="cuda")
    for a, b in ((0, 2047), (2047, 5000)):
        r = calib_ops.reliability_sums(pt[a:b].contiguous(), yt[a:b].contiguous(), wt[a:b].contiguous(), e, out)
        assert r is out
    assert torch.equal(out.cpu(), torch.from_numpy(C.reliability_sums_host(p, y, wq, edges)))


@pytest.mark.parametrize("strategy", ["quantile", "uniform"])
def test_reliability_report_equals_host(strategy):
    rng = np.random.default_rng(4)
    p = rng.beta(0.7, 2.0, size=10007).astype(F32)
    y = (rng.random(10007) < p).astype(np.int64)
    w = rng.random(10007)
    for sw in (None, w):
        host = C.reliability_report(y, p, n_bins=12, strategy=strategy, sample_weight=sw)
        dev = C.reliability_report(torch.from_numpy(y).cuda(), torch.from_numpy(p).cuda(), n_bins=12,
                                   strategy=strategy, sample_weight=sw)
        assert np.array_equal(dev.edges.view(np.int32), host.edges.view(np.int32))
        assert np.array_equal(dev.table, host.table)
        assert dev.to_dict() == host.to_dict()


# ------------------------------------------------------------------------------------------------ the workflow
def _synthetic(n, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 6)).astype(F32)
    z = 1.2 * X[:, 0] - 0.8 * X[:, 1] + 0.5 * X[:, 2] * X[:, 3] - 2.0
    return X, (rng.random(n) < 1 / (1 + np.exp(-z))).astype(np.int64)


def test_classifier_workflow():
    from cobalt_smart_lender_ai_amd.models.gbdt import GBDTClassifier

    X, y = _synthetic(40000)
    Xt, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    clf = GBDTClassifier(n_estimators=5, max_depth=3, scale_pos_weight=6.7)
    clf.fit(Xt[:20000], y[:20000])
    X_cal, y_cal = Xt[20000:], yt[20000:]
    raw = clf.predict_proba(X_cal)
    before = clf.reliability(X_cal, y_cal)
    cm = clf.calibrate(X_cal, y_cal, "isotonic")
    proba = cm.predict_proba(X_cal)
    assert proba.is_cuda and proba.shape == (20000, 2) and proba.dtype == torch.float32
    assert np.array_equal(clf.predict_proba(X_cal), raw)            # the classifier is unchanged
    after = cm.reliability(X_cal, y_cal)
    assert after.ece <= before.ece
    # the same inputs on the host: the drop is large, so the assertion above is not vacuous
    m = clf.get_booster().predict_margin(X_cal).cpu().numpy()
    host_cal = MC.IsotonicCalibrator().fit(m, y[20000:])
    host_before = C.reliability_report(y[20000:], clf.get_booster().predict_proba(X_cal).cpu().numpy())
    host_after = C.reliability_report(y[20000:], host_cal.transform(m))
    assert host_before.ece > 0.1 and host_after.ece < 0.2 * host_before.ece
    assert before.to_dict() == host_before.to_dict() and after.to_dict() == host_after.to_dict()
    # on its own fitting set, with its own constant runs as bins, isotonic regression gives the observed rate
    xk, vk = cm.calibrator.x_thresholds_, cm.calibrator.y_thresholds_
    run_start = np.concatenate([[True], vk[1:] != vk[:-1]])         # first knot of every constant run
    edges = cm.calibrator.transform(torch.from_numpy(xk[run_start][1:]).cuda())
    rep = C.reliability_report(y_cal, proba[:, 1].contiguous(), edges=edges)
    assert rep.n_bins == int(run_start.sum()) and np.all(rep.table[0] > 0)
    assert np.max(np.abs(rep.gap)) <= 2.0 ** -23


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    cw, cs = cc.hull_case("random", 10)
    cwt, cst = torch.from_numpy(cw).cuda(), torch.from_numpy(cs).cuda()
    for bad in ((torch.from_numpy(cw), cst), (cwt.to(torch.int32), cst), (cwt, cst[:-1]),
                (torch.stack([cwt, cwt], 1)[:, 0], cst), (cwt[:1], cst[:1])):
        with pytest.raises(ValueError):
            calib_ops.iso_hull(*bad)
    xk, vk, x = cc.apply_case(5, 16)
    xt, xkt, vkt = (torch.from_numpy(a).cuda() for a in (x, xk, vk))
    for bad in ((x, xkt, vkt), (xt.cpu(), xkt, vkt), (xt.double(), xkt, vkt), (xt, xkt, vkt.float()),
                (xt[::2], xkt, vkt), (xt, xkt, vkt[:-1]), (xt, xkt[:0], vkt[:0])):
        with pytest.raises(ValueError):
            calib_ops.calib_apply(*bad)
    p, y, wq, edges = cc.reliability_case(64, 4, weighted=True)
    pt, yt, wt, et = (torch.from_numpy(a).cuda() for a in (p, y, wq, edges))
    nan = pt.clone()
    nan[5] = float("nan")
    for bad in ((pt.cpu(), yt, wt, et), (pt.double(), yt, wt, et), (pt[::2], yt[::2], wt[::2], et), (nan, yt, wt, et),
                (pt + 0.5, yt, wt, et), (pt, yt * 2, wt, et), (pt, yt, wt.long(), et), (pt, yt, wt * (1 << 20), et),
                (pt, yt, wt, et.flip(0)), (pt, yt[:-1], wt, et),
                (pt, yt, wt, torch.zeros(4096, dtype=torch.float32, device="cuda"))):
        with pytest.raises(ValueError):
            calib_ops.reliability_sums(*bad)
    with pytest.raises(ValueError, match="out must be"):
        calib_ops.reliability_sums(pt, yt, wt, et, torch.zeros((3, 5), dtype=torch.int64, device="cuda"))
    s, yy = cc.smooth_rows(10)
    st = torch.from_numpy(s).cuda()
    with pytest.raises(ValueError, match="labels must be 0 or 1"):
        MC.IsotonicCalibrator().fit(st, torch.from_numpy(yy * 2).cuda())
    with pytest.raises(ValueError, match="NaN scores"):
        MC.IsotonicCalibrator().fit(st * float("nan"), torch.from_numpy(yy).cuda())
    with pytest.raises(ValueError, match="empty"):
        MC.IsotonicCalibrator().fit(st[:0], torch.from_numpy(yy[:0]).cuda())
