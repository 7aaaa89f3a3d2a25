"""The SMOTE k-nearest-neighbour kernel (csrc/knn.hip k_knn<K>, k_smote_interp) off the origin and at its shape
edges (run with -m gpu). Inputs, the fp64 brute-force reference and the accuracy contract: knn_cases.py, checked
themselves in test_knn_cases_cpu.py against a NumPy model of the kernel's formula.

Which test catches which mistake:
  the fp32 norm trick on un-centred data (self not first, wrong neighbours) ....... test_contract[plus1e4, mixed_scale, ...]
  a sub-tile / LDS-pass / workgroup edge, the zero pad of odd F, a wrong K ......... test_contract[nr*, nq*, F*, K*]
  INF sentinels mishandled in the half merge ...................................... test_contract[sentinel_*, nr16_k16, ...]
  ties between bit-identical distances broken by position, not index ............... test_duplicates_*
  an answer that depends on the query's lane, wave or workgroup .................... test_grid_independence
  the out_dist == nullptr branch, the k > nr return code ........................... test_native_*
  interpolation towards the wrong rows on a loan-like frame ........................ test_smote_cuda_equals_cpu_*
  the kernel's empty-slot index 2^31-1 reaching k_smote_interp ..................... test_*_guard* (reject before any launch)
"""
import functools

import numpy as np
import pytest
import torch

import knn_cases as kc
from cobalt_smart_lender_ai_amd import _native
from cobalt_smart_lender_ai_amd.nn.smote import SMOTE, kneighbors

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _gpu(name):
    c = kc.CASES[name]
    return kneighbors(c["Q"], c["R"], c["k"], device=DEV)


@pytest.mark.parametrize("name", kc.CASE_NAMES)
def test_contract(name):
    c = kc.CASES[name]
    idx, dist = _gpu(name)
    assert idx.dtype == np.int64 and dist.dtype == np.float32
    print(f"[knn] {name}: |dist^2 - ref| / tau <= {kc.worst_dist_ratio(idx, dist, c['Q'], c['R']):.3f}, "
          f"indices equal to the reference {(idx == kc.reference(c['Q'], c['R'], c['k'])[0]).mean():.4f}")
    share = kc.assert_knn_contract(idx, dist, c["Q"], c["R"], c["k"])
    assert share >= kc.MIN_DECIDED, (name, share)
    if c["Q"] is c["R"]:   # SMOTE drops column 0 as "the row itself": it must be, wherever the bound decides it
        sure = kc.self_is_decided_first(c["R"])
        assert np.array_equal(idx[sure, 0], np.flatnonzero(sure))


@pytest.mark.parametrize("name", kc.DUPLICATE_CASES)
def test_duplicates_come_out_in_index_order(name):
    c = kc.CASES[name]
    idx, dist = _gpu(name)
    assert kc.assert_duplicates_in_index_order(idx, c["R"]) == 0    # k = 6: two whole groups of three copies
    assert np.array_equal(dist[:, 0], dist[:, 2]) and np.array_equal(dist[:, 3], dist[:, 5])


@pytest.mark.parametrize("name", kc.DUPLICATE_CASES)
def test_duplicates_cut_by_k_keep_the_lowest_indices(name):
    c = kc.CASES[name]
    idx, dist = kneighbors(c["Q"], c["R"], kc.DUPLICATE_CUT_K, device=DEV)
    kc.assert_knn_contract(idx, dist, c["Q"], c["R"], kc.DUPLICATE_CUT_K)
    assert kc.assert_duplicates_in_index_order(idx, c["R"]) == len(idx)


@pytest.mark.parametrize("name", kc.GRID_CASES)
def test_grid_independence(name):
    c = kc.CASES[name]
    idx, dist = _gpu(name)
    for Q2, rows in kc.regrid(c["Q"]):
        i2, d2 = kneighbors(Q2, c["R"], c["k"], device=DEV)
        assert np.array_equal(i2[rows], idx)
        assert np.array_equal(d2[rows].view(np.int32), dist.view(np.int32))


def _native_knn(Qc, Rc, k, with_dist):
    """cobalt_knn on fp32 inputs as given; idx pre-filled with -1, dist with NaN."""
    Qd, Rd = torch.as_tensor(Qc, device=DEV), torch.as_tensor(Rc, device=DEV)
    idx = torch.full((len(Qc), k), -1, dtype=torch.int32, device=DEV)
    dist = torch.full((len(Qc), k), float("nan"), dtype=torch.float32, device=DEV) if with_dist else None
    rc = _native.lib().cobalt_knn(Qd.data_ptr(), len(Qc), Rd.data_ptr(), len(Rc), Qc.shape[1], k, idx.data_ptr(),
                                  _native.ptr(dist), _native.stream_handle())
    torch.cuda.synchronize()
    return rc, idx.cpu().numpy(), None if dist is None else dist.cpu().numpy()


def test_native_call_without_distances_writes_every_index():
    c = kc.CASES["nq129"]
    mu = c["R"].mean(axis=0)
    Qc, Rc = (c["Q"] - mu).astype(np.float32), (c["R"] - mu).astype(np.float32)
    rc, idx, _ = _native_knn(Qc, Rc, c["k"], with_dist=False)
    assert rc == 0
    assert idx.min() >= 0 and idx.max() < len(Rc)                  # no slot left at -1, no empty-slot index
    rc, idx2, dist2 = _native_knn(Qc, Rc, c["k"], with_dist=True)
    assert rc == 0 and np.array_equal(idx, idx2) and not np.isnan(dist2).any()
    assert np.array_equal(idx, _gpu("nq129")[0])


def test_native_call_refuses_k_above_nr_without_writing():
    rng = np.random.default_rng(3)
    Rc = rng.normal(size=(5, 4)).astype(np.float32)
    rc, idx, dist = _native_knn(Rc, Rc, 6, with_dist=True)
    assert rc == -4
    assert (idx == -1).all() and np.isnan(dist).all()              # nothing was launched


def test_smote_cuda_equals_cpu_on_a_mixed_scale_frame():
    X, y = kc.smote_frame()
    assert kc.smote_neighbours_decided(X[y == 1], 5)               # else near-ties may legitimately differ
    Xg, yg = SMOTE(random_state=123, device=DEV).fit_resample(X, y)
    Xc, yc = SMOTE(random_state=123, device="cpu").fit_resample(X, y)
    assert len(Xg) == 2 * (y == 0).sum() and np.array_equal(yg, yc)
    np.testing.assert_allclose(Xg, Xc, rtol=0, atol=1e-9 * np.abs(X).max())


# The guards reject before any launch: nothing below reaches a kernel (test_knn_cases_cpu.py runs the same calls
# where there is no device at all).
def test_kneighbors_guards_reject_before_any_launch():
    rng = np.random.default_rng(5)
    R = rng.normal(size=(40, 4))
    bad = R.copy()
    bad[17, 2] = np.nan
    with pytest.raises(ValueError, match="reference rows"):
        kneighbors(R[:9], R[:5], 6, device=DEV)
    with pytest.raises(ValueError, match="finite"):
        kneighbors(bad, R, 6, device=DEV)
    with pytest.raises(ValueError, match="finite"):
        kneighbors(R, bad, 6, device=DEV)


def test_smote_guard_rejects_a_minority_of_k_rows():
    rng = np.random.default_rng(8)
    X = rng.normal(size=(60, 3))
    y = np.zeros(60, dtype=np.int64)
    y[:5] = 1
    with pytest.raises(ValueError, match="k_neighbors=5 needs at least 6"):
        SMOTE(random_state=1, k_neighbors=5, device=DEV).fit_resample(X, y)
