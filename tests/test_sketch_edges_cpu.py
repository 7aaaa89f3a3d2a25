"""The oracle and the cases of sketch_edge_cases.py, checked without a GPU, so that a wrong oracle cannot pass a
wrong kernel (test_gpu_sketch_edges.py): ``compute_cuts`` on the CPU -- the sort-based form the device sketch must
reproduce -- equals the NumPy oracle on every case over the whole cut table, every case still has the properties
it was designed for (recomputed from its inputs by the NumPy mirror of the bucket arithmetic), every branch the
suite is meant to reach is reached by a named case, and the cases tell a subtly wrong sketch from a right one."""
import dataclasses

import numpy as np
import pytest
import torch

import sketch_edge_cases as ce
from cobalt_smart_lender_ai_amd import _native
from cobalt_smart_lender_ai_amd.models import sketch


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("name", ce.CASE_NAMES)
def test_compute_cuts_equals_the_numpy_oracle(name, weighted):
    b = ce.build(name)
    w = b.weights(weighted)
    want_c, want_n = ce.oracle(name, weighted)
    got_c, got_n = sketch.compute_cuts(b.X, 256, None if w is None else torch.from_numpy(w))
    assert got_c.shape == (b.X.shape[1], 256) and got_c.dtype == torch.float32 and got_n.dtype == torch.int32
    assert np.array_equal(got_n.numpy(), want_n)
    assert np.array_equal(_bits(got_c.numpy()), _bits(want_c))
    # the table's own shape: the sentinel in slot nbins - 1 and every later slot, strictly rising cuts below
    for f in range(len(want_n)):
        nb = int(want_n[f])
        assert 1 <= nb <= 256 and (want_c[f, nb - 1:] == ce.FLT_MAX).all()
        assert (np.diff(want_c[f, :nb - 1].astype(np.float64)) > 0).all()


def _check(props: dict, got: dict, where: str):
    for key, want in props.items():
        if key in ("unit", "weighted"):
            continue
        if isinstance(want, dict):
            for f, v in want.items():
                assert got[key][f] == v, (where, key, f, got[key][f], v)
        else:
            assert got[key] == want, (where, key, got[key], want)


@pytest.mark.parametrize("name", ce.CASE_NAMES)
def test_case_has_its_designed_properties(name):
    b = ce.build(name)
    assert b.props, name
    for weighted in (False, True):
        got = ce.measure(b, weighted)
        _check(b.props, got, name)
        _check(b.props.get("weighted" if weighted else "unit", {}), got, name)


def _m(name, weighted=False):
    return ce.measure(ce.build(name), weighted)


def test_every_listed_branch_has_a_case():
    # pass 1 block count; row-range and row-count alignment (k_sk_gather<.., true>, k_sk_transpose)
    assert _m("A_1x1")["nblk"] == 1 and _m("A_65536x4")["nblk"] == 1 and _m("A_65537x3")["nblk"] == 2
    assert _m("A_131076x4")["nblk"] == 3
    g = _m("A_65540x4")   # ldx % 4 == 0 with block starts off the 4-grid: the vector path's head and tail
    assert g["n_mod4"] == 0 and g["per_mod4"] == 2
    g = _m("A_65537x3")   # ldx % 4 != 0: the scalar branch
    assert g["n_mod4"] == 1 and g["per_mod4"] == 1
    assert _m("A_131073x5")["per_mod4"] == 3
    assert {_m(f"A_{n}x{F}")["n_mod4"] for n, F in ce.A_SHAPES} == {0, 1, 2, 3}
    for name in ("A_65540x4", "A_65537x3", "A_131073x5", "A_131076x4"):  # the gather runs: open targets exist
        assert max(_m(name)["seg_target"]) > 0
    # transpose: scalar stores, a ragged last tile, F = 32, the two fallbacks, the scalar loads
    assert _m("A_257x32")["n_mod4"] == 1 and _m("A_256x32")["F"] == 32 and _m("A_1025x33")["F"] == 33
    assert not _m("A_noncontiguous_4099x5")["contiguous"]
    g = _m("A_misaligned_base_4099x5")
    assert g["contiguous"] and not g["aligned16"] and ce.build("A_misaligned_base_4099x5").X.storage_offset() == 1
    assert {_m("A_float64_1025x3")["dtype"], _m("A_float16_1025x3")["dtype"]} == {"float64", "float16"}
    # boundary sort sizes on both sides of 4095 boundaries, the cap and the switch to torch.sort
    assert [_m(f"D_S{S}_distinct")["S"] for S in ce.D_SIZES] == [1, 2, 4094, 4095, 4096, 5000, 32768, 32769]
    assert [_m(f"D_S{S}_distinct")["m"][0] for S in ce.D_SIZES] == [1, 2, 4094, 4095, 4095, 4095, 4095, 4095]
    assert _m("D_S32768_distinct")["S"] == ce.SAMPLE_CAP and _m("D_S32769_dups_nan_inf")["S"] == ce.SAMPLE_CAP + 1
    x = ce.build("D_S5000_dups_nan_inf").x32()
    assert np.isnan(x).any() and np.isinf(x).any() and np.signbit(x[x == 0]).any()
    # select edges: one segment of exactly L rows with targets; beyond the cap the host fallbacks
    for L in ce.B_LENGTHS:
        for weighted in (False, True):
            g, h = _m(f"B_L{L}_distinct", weighted), _m(f"B_L{L}_dup200", weighted)
            assert g["seg_target"] == [L] and h["seg_any"] == [L, L] and h["cls"][0] == "uncertain"
            assert h["nd"][0] == min(L, 200) + 1 <= h["maxb"][0]   # decided by the select kernels' distinct values
    assert ce.SORT_CAP in ce.B_LENGTHS and ce.SORT_CAP + 1 in ce.B_LENGTHS and ce.SORT_CAP - 1 in ce.B_LENGTHS
    # the distinct-count class at maxb and maxb + 1, with and without a missing value
    for mode in ("unsampled", "sampled", "interleaved"):
        for nan, maxb in ((0, 256), (1, 255)):
            for d in (maxb, maxb + 1):
                g = _m(f"C_{mode}_{d}" + ("_nan" if nan else ""))
                assert g["nd"] == [d, d] and g["maxb"] == [maxb, maxb]
                if mode != "unsampled":
                    assert g["cls"][0] == ("many" if d > maxb else "exact" if mode == "sampled" else "uncertain")
    assert _m("C_every_value_sampled_no_segment")["nseg"] == 0
    # values: the specials are present; in the sparse-sample case none of them is a boundary
    for name in ("E_values_every_row_sampled", "E_values_sparse_sample"):
        x = ce.build(name).x32()
        assert np.isposinf(x[:, 0]).any() and np.isneginf(x[:, 0]).any()
        assert (x[:, 1] == ce.FLT_MAX).any() and (x[:, 1] == -ce.FLT_MAX).any()
        d = x[:, 2][x[:, 2] != 0]
        assert len(d) and (np.abs(d) < np.finfo(np.float32).tiny).all() and np.signbit(x[:, 2][x[:, 2] == 0]).any()
        assert len(np.unique(x[:, 3])) == 1 and np.isnan(x[:, 4]).all() and (~np.isnan(x[:, 5])).sum() == 1
        assert np.isnan(x[-1, 6]) and not np.isnan(x[:-1, 6]).any()
    s = ce.build("E_values_sparse_sample").x32()[::126]
    assert not np.isinf(s[:, 0]).any() and not (np.abs(s[:, 1]) == ce.FLT_MAX).any()
    # weights
    assert _m("F_zero_weight_on_one_feature", True)["W"][0] == 0 < _m("F_zero_weight_on_one_feature", True)["W"][1]
    assert float(ce.build("F_all_weights_zero").w.max()) == 0.0
    q = ce.quantize_np(ce.build("F_one_heavy_row").w, 9001)
    assert q.sum() == ce.WEIGHT_SCALE and (q > 0).sum() == 1
    assert (ce.quantize_np(ce.build("F_equal_weights_70001").w, 70_001) == ce.WEIGHT_SCALE).all()
    # data parallel and streamed: the host-fallback segment spans the ranks; a 1-row, an empty and a 2-block chunk
    col = ce.build("DP_70001x5").x32()[:, 3]
    for shards in (ce.DP_WORLD2, ce.DP_WORLD3):
        assert shards[0][0] == 0 and shards[-1][1] == ce.DP_ROWS
        assert all(a[1] == b[0] for a, b in zip(shards, shards[1:]))
        assert all(s % 3 for s, e in shards[1:]) and sum((col[s:e] > 0).sum() > 0 for s, e in shards) >= 2
    assert ce.DP_WORLD3[1][0] == ce.DP_WORLD3[1][1] and ce.DP_WORLD3[2][0] <= ce.DP_ROWS - 7
    for name in ce.STREAM_CASES:
        sizes = np.diff(ce.stream_bounds(ce.build(name).X.shape[0]))
        assert sizes[0] == 1 and sizes[1] == 0 and sizes[2] == 257 and sizes.sum() == ce.build(name).X.shape[0]
    assert ce.nblk_of(int(np.diff(ce.stream_bounds(131073))[3])) == 2
    stream_s = [-(-ce.build(k).X.shape[0] // ce.sample_stride(ce.build(k).X.shape[0], v)) for k, v in ce.STREAM_CASES.items()]
    assert min(stream_s) < ce.SAMPLE_CAP < max(stream_s)
    for k, v in ce.STREAM_CASES.items():  # both streamed runs have open targets, so both walk the chunks twice
        assert ce.measure(dataclasses.replace(ce.build(k), sample_rows=v), False)["nseg"] > 0


def test_constants_are_the_librarys():
    """The mirror's table sizes are the library's own, and S = 32769 is past its LDS sample sort."""
    if not _native.available():
        pytest.skip("native library not built")
    lib = sketch._sk_lib()
    assert (lib.cobalt_sk_bounds(), lib.cobalt_sk_buckets(), lib.cobalt_sk_sort_cap(), lib.cobalt_sk_sample_cap()) == (
        ce.NBND, ce.NB, ce.SORT_CAP, ce.SAMPLE_CAP)
    assert ce.measure(ce.build("D_S32769_distinct"), False)["S"] > lib.cobalt_sk_sample_cap()
    assert ce.measure(ce.build("D_S32768_distinct"), False)["S"] <= lib.cobalt_sk_sample_cap()


def test_no_case_is_left_out_of_the_gpu_file():
    import test_gpu_sketch_edges as gpu

    assert list(gpu.E2E_CASES) == ce.CASE_NAMES and len(set(ce.CASE_NAMES)) == len(ce.CASE_NAMES)
    assert set(gpu.STREAM_CASES) == set(ce.STREAM_CASES)


# ------------------------------------------------------------------------------------------ sensitivity
def _differs(fn, name, weighted):
    b = ce.build(name)
    c, nb = fn(b.x32(), b.weights(weighted))
    want_c, want_n = ce.oracle(name, weighted)
    return not (np.array_equal(nb, want_n) and np.array_equal(_bits(c), _bits(want_c)))


def test_cases_catch_an_order_statistic_off_by_one(monkeypatch):
    """With the sort-based sketch in the kernel's place (it equals the oracle, above), a sketch that takes ``>=``
    for ``>`` in the threshold rule is told apart by the L-series (every length that takes the quantile path) and
    by the threshold cases past ``maxb``. ``compute_cuts`` itself with that mistake (its searchsorted made
    left-sided) gives the wrong oracle's table, so the two stand for each other."""
    class _LeftSided:
        def __getattr__(self, k):
            return getattr(torch, k)

        @staticmethod
        def searchsorted(a, v, right=False):
            return torch.searchsorted(a, v, right=False)

    with monkeypatch.context() as mp:
        mp.setattr(sketch, "torch", _LeftSided())
        for name in ("B_L8193_distinct", "C_sampled_257", "A_1025x33"):
            b = ce.build(name)
            c, nb = sketch.compute_cuts(b.X, 256)
            wc, wn = ce.cuts_off_by_one_np(b.x32(), None)
            assert np.array_equal(nb.numpy(), wn) and np.array_equal(_bits(c.numpy()), _bits(wc)), name
    # ``>=`` and ``>`` are one function on an input where no j * W is a multiple of maxb: with unit weights that is
    # every odd row count, so the L-series tells them apart at its even row counts (L + 1 rows), unit-weighted ...
    for L in ce.B_LENGTHS:
        if L + 1 > 256:
            assert _differs(ce.cuts_off_by_one_np, f"B_L{L}_distinct", False) == ((L + 1) % 2 == 0), L
            # ... and tells an answer one order statistic late apart at every length, both weight settings
            assert _differs(ce.cuts_one_late_np, f"B_L{L}_distinct", False), L
            assert _differs(ce.cuts_one_late_np, f"B_L{L}_distinct", True), L
    assert {L for L in ce.B_LENGTHS if L > 255 and L % 2} == {4097, 8191, 8193}
    # the threshold cases: past maxb every unit-weight target rank ends a run of equal values (by construction), so
    # the wrong rule moves the cuts; at or below maxb there is one bin per value and no threshold to get wrong
    for mode in ("unsampled", "sampled", "interleaved"):
        for nan, maxb in ((0, 256), (1, 255)):
            for d in (255, 256, 257):
                assert _differs(ce.cuts_off_by_one_np, f"C_{mode}_{d}" + ("_nan" if nan else ""), False) == (d > maxb)
    assert sum(_differs(ce.cuts_off_by_one_np, n, wt) for n in ce.CASE_NAMES for wt in (False, True)) >= 30


def test_cases_catch_signed_zeros_counted_twice():
    assert _differs(ce.cuts_signed_zero_np, "C_signed_zero_in_open_bucket", False)
    assert _differs(ce.cuts_signed_zero_np, "C_signed_zero_in_open_bucket", True)
    assert not _differs(ce.cuts_signed_zero_np, "C_unsampled_256", False)
