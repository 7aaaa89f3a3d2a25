"""The contract and the cases of knn_cases.py, checked without a GPU, so that test_gpu_knn_edges.py cannot hide a
failure behind a contract that decides nothing or a case that cannot see the bug it is there for:

  * the fp64 reference satisfies its own contract and agrees with scikit-learn's brute force;
  * a NumPy model of the kernel's fp32 formula on mean-centred inputs satisfies the contract on every case with
    no violation, and the contract decides >= 95 % of every case's (query, slot) pairs -- a condition the cases
    are built to meet, not a measurement;
  * the same model WITHOUT the centring violates the contract on the off-origin cases: they detect the bug;
  * the duplicate-order and grid-independence assertions hold for the model and reject a wrong order;
  * the guards of kneighbors and SMOTE raise ValueError on the cpu path, and on the cuda path before any device
    work (this machine has no device to do any on).
"""
import numpy as np
import pytest

import knn_cases as kc
from cobalt_smart_lender_ai_amd.nn.smote import SMOTE, kneighbors


@pytest.mark.parametrize("name", kc.CASE_NAMES)
def test_case_is_decided_and_model_meets_contract(name):
    c = kc.CASES[name]
    Q, R, k = c["Q"], c["R"], c["k"]
    assert Q.dtype == np.float64 and R.dtype == np.float64
    share_ref = kc.decided_share_of_reference(name)
    idx, dist = kc.model_knn(Q, R, k)
    share = kc.assert_knn_contract(idx, dist, Q, R, k)
    print(f"[knn] {name}: decided {share:.4f}, model |dist^2 - ref| / tau <= {kc.worst_dist_ratio(idx, dist, Q, R):.3f}")
    assert share == share_ref            # the share is a property of the case, not of the answer
    assert share >= kc.MIN_DECIDED, (name, share)
    if c.get("duplicates"):
        kc.assert_duplicates_in_index_order(idx, R)
    if Q is R:
        sure = kc.self_is_decided_first(R)
        assert np.array_equal(idx[sure, 0], np.flatnonzero(sure))


def test_case_list_covers_the_shape_edges():
    shapes = {(len(c["Q"]), len(c["R"]), c["R"].shape[1], c["k"]) for c in kc.CASES.values()}
    for k in (1, 6, 16):
        assert {nr for _, nr, _, kk in shapes if kk == k} >= {k, k + 1, 31, 32, 33, 255, 256, 257, 513} - set(range(k))
    assert {nq for nq, _, _, _ in shapes} >= {1, 31, 33, 127, 128, 129, 300}
    assert {F for _, _, F, _ in shapes} >= {1, 2, 3, 19, 20, 31, 32}
    assert {k for _, nr, _, k in shapes if nr == 300} >= set(kc.COMPILED_K)
    assert {nr for _, nr, _, k in shapes if k == 16} >= {16, 17, 20}
    assert max(len(c["Q"]) * len(c["R"]) * c["R"].shape[1] for c in kc.CASES.values()) == 777 * 777 * 20
    assert set(kc.GRID_CASES) <= set(kc.CASE_NAMES) and len(kc.OFF_ORIGIN_CASES) >= 4 and len(kc.DUPLICATE_CASES) == 2


def test_reference_agrees_with_sklearn_brute_force():
    from sklearn.neighbors import NearestNeighbors

    for name in ("nq300", "F32", "mixed_scale"):
        c = kc.CASES[name]
        idx, d2 = kc.reference(c["Q"], c["R"], c["k"])
        mu = c["R"].mean(axis=0)       # scikit-learn's brute force uses the norm trick in fp64: keep it accurate
        sd, si = NearestNeighbors(n_neighbors=c["k"], algorithm="brute").fit(c["R"] - mu).kneighbors(c["Q"] - mu)
        assert np.array_equal(idx, si)
        np.testing.assert_allclose(np.sqrt(d2), sd, rtol=1e-9, atol=1e-9 * float(np.sqrt(d2.max())))


@pytest.mark.parametrize("name", kc.OFF_ORIGIN_CASES)
def test_uncentred_formula_violates_the_contract(name):
    """The formula on float32(X) -- kneighbors before it centred -- must be caught by every off-origin case."""
    c = kc.CASES[name]
    idx, dist = kc.model_knn(c["Q"], c["R"], c["k"], centre=False)
    with pytest.raises(AssertionError):
        kc.assert_knn_contract(idx, dist, c["Q"], c["R"], c["k"])


def test_uncentred_formula_loses_self_and_neighbours_at_1e4():
    """What the violation means on N(0,1) + 1e4: the row itself is not first, most neighbours are wrong."""
    c = kc.CASES["plus1e4"]
    ref, _ = kc.reference(c["Q"], c["R"], c["k"])
    idx, _ = kc.model_knn(c["Q"], c["R"], c["k"], centre=False)
    assert (idx[:, 0] == np.arange(len(idx))).mean() < 0.05
    assert (idx == ref).mean() < 0.05
    good, _ = kc.model_knn(c["Q"], c["R"], c["k"])
    assert np.array_equal(good, ref)


def test_contract_rejects_wrong_answers():
    c = kc.CASES["nq129"]
    Q, R, k = c["Q"], c["R"], c["k"]
    idx, d2 = kc.reference(Q, R, k)
    dist = np.sqrt(d2)
    kc.assert_knn_contract(idx, dist, Q, R, k)
    far = np.argsort(kc.sqdist(Q, R), axis=1)[:, k + 3]
    bad = idx.copy(); bad[5, k - 1] = far[5]                       # a far row instead of the k-th nearest
    with pytest.raises(AssertionError, match="missing|beyond"):
        kc.assert_knn_contract(bad, dist, Q, R, k)
    bad = idx.copy(); bad[0, 1] = 0x7fffffff                       # the kernel's empty-slot index
    with pytest.raises(AssertionError, match="outside"):
        kc.assert_knn_contract(bad, dist, Q, R, k)
    bad = idx.copy(); bad[7, 2] = bad[7, 1]
    with pytest.raises(AssertionError, match="repeats"):
        kc.assert_knn_contract(bad, dist, Q, R, k)
    with pytest.raises(AssertionError, match="more than tau"):
        kc.assert_knn_contract(idx, dist * (1 + 1e-4), Q, R, k)
    with pytest.raises(AssertionError, match="decreases"):
        kc.assert_knn_contract(idx[:, ::-1], dist[:, ::-1], Q, R, k)


@pytest.mark.parametrize("name", kc.DUPLICATE_CASES)
def test_duplicate_order_assertion(name):
    c = kc.CASES[name]
    Q, R = c["Q"], c["R"]
    idx, dist = kc.model_knn(Q, R, kc.DUPLICATE_CUT_K)
    kc.assert_knn_contract(idx, dist, Q, R, kc.DUPLICATE_CUT_K)
    assert kc.assert_duplicates_in_index_order(idx, R) == len(Q)   # every query cuts its second group of copies
    swapped = idx.copy()
    swapped[:, [0, 1]] = swapped[:, [1, 0]]                        # two copies of the query in descending order
    with pytest.raises(AssertionError, match="ascending"):
        kc.assert_duplicates_in_index_order(swapped, R)
    ref, _ = kc.reference(Q, R, 6)
    highest = idx.copy()
    highest[:, 3] = ref[:, 5]                                      # the highest copy of the cut group, not the lowest
    with pytest.raises(AssertionError, match="lowest"):
        kc.assert_duplicates_in_index_order(highest, R)


@pytest.mark.parametrize("name", kc.GRID_CASES)
def test_regrid_moves_every_query_and_keeps_its_answer(name):
    c = kc.CASES[name]
    idx, dist = kc.model_knn(c["Q"], c["R"], c["k"])
    for Q2, rows in kc.regrid(c["Q"]):
        assert np.array_equal(Q2[rows], c["Q"]) and not np.array_equal(rows, np.arange(len(rows)))
        i2, d2 = kc.model_knn(Q2, c["R"], c["k"])
        assert np.array_equal(i2[rows], idx) and np.array_equal(d2[rows].view(np.int32), dist.view(np.int32))


def test_smote_frame_is_fully_decided():
    """The cuda-vs-cpu fit_resample comparison asks for equal rows, which holds only if no minority row has a
    near-tie among its 6 nearest (itself and 5) or at the cut after them: every slot is decided by more than
    2 tau_q between consecutive neighbours. SMOTE_SEED is the first seed for which that is so."""
    X, y = kc.smote_frame()
    assert X.shape == (600, 7) and (y == 1).sum() == 78 and set(np.unique(y)) == {0, 1}
    assert kc.smote_neighbours_decided(X[y == 1], 5)


# ------------------------------------------------------------------------------------------ guards
def _guard_inputs():
    rng = np.random.default_rng(5)
    R = rng.normal(size=(40, 4))
    bad_nan, bad_inf = R.copy(), R.copy()
    bad_nan[17, 2] = np.nan
    bad_inf[3, 0] = np.inf
    return R, bad_nan, bad_inf


# device="cuda" too: the guards stand before any device work, so they raise ValueError here, where there is no
# device (anything that got past them would fail otherwise, and differently)
@pytest.mark.parametrize("device", ["cpu", "cuda"])
def test_kneighbors_guards(device):
    R, bad_nan, bad_inf = _guard_inputs()
    with pytest.raises(ValueError, match="reference rows"):
        kneighbors(R[:9], R[:5], 6, device=device)
    with pytest.raises(ValueError, match="reference rows"):
        kneighbors(R, R, 0, device=device)
    for bad in (bad_nan, bad_inf):
        with pytest.raises(ValueError, match="finite"):
            kneighbors(bad, R, 6, device=device)
        with pytest.raises(ValueError, match="finite"):
            kneighbors(R, bad, 6, device=device)
    with pytest.raises(ValueError, match="columns"):
        kneighbors(R[:, :3], R, 6, device=device)


def test_kneighbors_cuda_refuses_what_fp32_cannot_hold():
    R, _, _ = _guard_inputs()
    with pytest.raises(ValueError, match="overflows"):
        kneighbors(R * 1e19, R * 1e19, 6, device="cuda")
    with pytest.raises(ValueError, match="must be one of"):
        kneighbors(R, R, 9, device="cuda")


def test_kneighbors_cpu_keeps_fp64():
    """The cpu path searches the float64 inputs as given: its distances match the fp64 reference to 1e-10, where
    inputs cast to fp32 first (as they once were) would be off by 1e-7."""
    c = kc.CASES["nq129"]
    i, d = kneighbors(c["Q"], c["R"], c["k"], device="cpu")
    ref_i, ref_d2 = kc.reference(c["Q"], c["R"], c["k"])
    assert np.array_equal(i, ref_i)
    np.testing.assert_allclose(d, np.sqrt(ref_d2), rtol=1e-10)
    _, d32 = kc.reference(c["Q"].astype(np.float32), c["R"].astype(np.float32), c["k"])
    assert np.abs(np.sqrt(d32) / np.sqrt(ref_d2) - 1).max() > 1e-8


@pytest.mark.parametrize("device", ["cpu", "cuda"])
@pytest.mark.parametrize("n_min", [1, 5])
def test_smote_refuses_a_class_of_at_most_k_rows(device, n_min):
    rng = np.random.default_rng(8)
    X = rng.normal(size=(60, 3))
    y = np.zeros(60, dtype=np.int64)
    y[:n_min] = 1
    with pytest.raises(ValueError, match="k_neighbors=5 needs at least 6"):
        SMOTE(random_state=1, k_neighbors=5, device=device).fit_resample(X, y)


def test_smote_accepts_a_class_of_k_plus_one_rows():
    rng = np.random.default_rng(8)
    X = rng.normal(size=(60, 3))
    y = np.zeros(60, dtype=np.int64)
    y[:6] = 1
    Xr, yr = SMOTE(random_state=1, k_neighbors=5, device="cpu").fit_resample(X, y)
    assert len(Xr) == 108 and (yr == 1).sum() == 54
