"""External-memory GBDT (host pages + per-tree MVS sample on the device): models/external.py.

CPU: the MVS threshold solver, the ghat binning, and the host path's quality against the in-core
fit. GPU: ``k_ooc_page`` + sampled growth give exactly the host path's model, over several pages.
"""
import numpy as np
import pytest

from cobalt_smart_lender_ai_amd.dataio import synth
from cobalt_smart_lender_ai_amd.metrics.auc import roc_auc
from cobalt_smart_lender_ai_amd.models import external, gbdt
from cobalt_smart_lender_ai_amd.models.stream import array_chunks

PARAMS = dict(n_estimators=12, max_depth=5, learning_rate=0.3, gamma=1.0, random_state=11, scale_pos_weight=5.0)


def _lc(n, seed):
    X, y = synth.make_lendingclub(n, seed=seed)
    return X.numpy(), y.numpy()


def test_ghat_bins_are_monotone_and_exact():
    v = np.array([0.0, 1e-16, 1e-9, 0.0999, 0.1, 0.25, 0.5, 0.75, 1.0, 6.7, 1e3])
    b = external.ghat_bin(v)
    assert b[0] == 0 and np.all(np.diff(b[1:]) >= 0)
    assert external.ghat_bin(np.array([0.5]))[0] == 64 * 16 and external.ghat_bin(np.array([1.0]))[0] == 65 * 16


def test_mvs_threshold_hits_the_target():
    rng = np.random.default_rng(0)
    gh = np.exp(rng.normal(-2, 1.5, 200_000))
    counts = np.bincount(external.ghat_bin(gh), minlength=external.OOC_BINS)
    for target in (10_000, 50_000, 150_000):
        mu = external.mvs_threshold(counts, target, mu_max=1e9)
        expect = np.minimum(1.0, gh / mu).sum()
        assert abs(expect - target) / target < 0.03
    assert external.mvs_threshold(counts, 1e9, mu_max=1e9) <= gh.min()   # target >= N: keep every row
    assert external.mvs_threshold(counts, 10, mu_max=0.5) == 0.5          # capped at w_max


def test_external_host_path_quality_matches_in_core():
    X, y = _lc(40_000, 3)
    Xte, yte = _lc(20_000, 4)
    ref = gbdt.train(X, y, PARAMS, device="cpu")
    rep = external.ExternalReport()
    b = external.train_external(array_chunks(X, y, 7_000), PARAMS, device="cpu", sample_rate=0.3, report=rep)
    assert b.num_trees == 12 and rep.n_pages == 6
    assert all(0.2 * 40_000 < s < 0.45 * 40_000 for s in rep.sample_rows), rep.sample_rows
    a_ref = roc_auc(yte, ref.predict_proba(Xte, device="cpu"))
    a_ext = roc_auc(yte, b.predict_proba(Xte, device="cpu"))
    assert abs(a_ref - a_ext) < 0.01, (a_ref, a_ext)
    # sample_rate=1: exact streaming (every row every tree, the in-core fixed point): the in-core trees
    full = external.train_external(array_chunks(X, y, 9_000), PARAMS, device="cpu", sample_rate=1.0)
    _same_trees(full, ref)


def _same_trees(a, b):
    assert a.num_trees == b.num_trees
    for ta, tb in zip(a.trees, b.trees):
        for k in ("left_children", "right_children", "split_indices", "split_conditions", "default_left",
                  "base_weights", "loss_changes", "sum_hessian"):
            assert np.array_equal(getattr(ta, k), getattr(tb, k)), k
    assert a.base_score == b.base_score


@pytest.mark.gpu
@pytest.mark.parametrize("colsample", [0.8, 1.0])
def test_external_exact_streaming_gpu_equals_in_core(colsample):
    """sample_rate=1 on the GPU: level-wise page streaming (csrc/gbdt_ox.h k_ox_page / k_ox_reduce + the
    in-core k_eval), the trees of the in-core GPU fit byte for byte -- pages spilled to host DRAM, and
    partly resident in HBM. Depth 7: the deep levels' pair slots span several LDS groups (the routing
    of a row is shared by the groups' blocks), and every tree level re-streams the staging buffers."""
    import torch

    X, y = _lc(90_000, 6)
    params = {**PARAMS, "colsample_bytree": colsample, "max_depth": 7, "n_estimators": 9}
    ref = gbdt.train(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda(), params, device="cuda")
    src = array_chunks(X, y, 13_000)
    ext = external.train_external(src, params, device="cuda", sample_rate=1.0)
    _same_trees(ext, ref)
    ps = external.page_stride(X.shape[1])
    mixed = external.train_external(src, params, device="cuda", sample_rate=1.0, device_page_bytes=40_000 * ps)
    _same_trees(mixed, ref)
    # every page within the HBM budget: the in-core trainer on the streamed-in records, same trees
    rep = external.ExternalReport()
    hbm = external.train_external(src, params, device="cuda", sample_rate=1.0, device_page_bytes=90_000 * ps,
                                  report=rep)
    assert rep.mode == "in-core" and rep.host_bytes == 0, rep
    _same_trees(hbm, ref)
    # ... and with n_rows given and the raw matrix fitting too: one pass over the stream + the in-core fit
    rep = external.ExternalReport()
    raw = external.train_external(src, params, n_rows=90_000, device="cuda", sample_rate=1.0,
                                  device_page_bytes=90_000 * ps, report=rep)
    assert rep.mode == "in-core" and rep.device_page_bytes == 90_000 * X.shape[1] * 4, rep
    _same_trees(raw, ref)


@pytest.mark.gpu
def test_external_gpu_equals_host_path():
    X, y = _lc(60_000, 5)
    src = array_chunks(X, y, 11_000)
    params = {**PARAMS, "colsample_bytree": 0.8, "max_depth": 6}
    host = external.train_external(src, params, device="cpu", sample_rate=0.25)
    rep = external.ExternalReport()
    dev = external.train_external(src, params, device="cuda", sample_rate=0.25, report=rep)
    ps = external.page_stride(X.shape[1])  # compact spill format: 20 B for 20 features
    assert ps == 20 and rep.n_pages == 6 and rep.host_bytes == 60_000 * ps
    assert dev.save_raw("ubj") == host.save_raw("ubj")
    # half the pages resident in HBM, the rest spilled: the same model
    rep2 = external.ExternalReport()
    mixed = external.train_external(src, params, device="cuda", sample_rate=0.25, device_page_bytes=33_000 * ps,
                                    report=rep2)
    assert rep2.device_page_bytes == 33_000 * ps and rep2.host_bytes == 27_000 * ps
    assert mixed.save_raw("ubj") == host.save_raw("ubj")


def test_exact_out_of_core_refuses_unsupported_shapes_before_streaming():
    """Exact streaming (sample_rate=1) supports max_depth <= 7 and <= 32 features on the GPU
    (cobalt_gbdt_ox_init); it says so with a ValueError before the sketch and page passes, not with a
    native error code after them (advisor finding, round 4). No GPU is touched before the check."""
    import numpy as np
    import torch

    from cobalt_smart_lender_ai_amd.models.external import train_external

    reads = []

    def source(F):
        def gen():
            reads.append(F)
            yield np.zeros((16, F), np.float32), np.zeros(16, np.float32)
        return gen

    with pytest.raises(ValueError, match="max_depth <= 7"):
        train_external(source(4), {"max_depth": 8}, device=torch.device("cuda", 0), sample_rate=1.0)
    assert reads == []  # refused before reading the stream
    with pytest.raises(ValueError, match="<= 32 features"):
        train_external(source(40), {"max_depth": 6}, device=torch.device("cuda", 0), sample_rate=1.0)
    assert reads == [40]  # one chunk peeked for the feature count
