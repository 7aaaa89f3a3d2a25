"""Data modes of the fused root pass (csrc/gbdt.hip grad_hist_body: kRootRec, kRootRecOrig, kRootGeneric).

Every case fits on the GPU and compares the model (every node of every tree, through the serialised
model) and the training margins, bit for bit, with the host oracle (models/gbdt_host.py, device="cpu").
The shapes are the smallest at which the pass's row loop changes behaviour: one row, a block's thread count
+- 1, one root item and one row more, and a ragged last unrolled iteration (U = 2 rows per thread)."""
import numpy as np
import pytest
import torch

from cobalt_smart_lender_ai_amd.dataio import synth
from cobalt_smart_lender_ai_amd.models import gbdt

pytestmark = pytest.mark.gpu

BLOCK, U = 512, 2  # k_grad_hist's threads per block and rows in flight per thread


def root_chunk(n: int, per_cu: int, cus: int) -> int:
    """Rows per root item as grow_impl sizes them: whole rounds of per_cu resident blocks per CU of ~8k
    rows, a multiple of 64 in [1024, 16384]."""
    res = per_cu * cus
    rounds = max(1, (n + res * 4096) // (res * 8192))
    return min(16384, max(1024, (-(-n // (rounds * res)) + 63) // 64 * 64))


def _shapes():
    # (at these sizes the item is the rule's floor, whatever the CU count and the resident blocks per CU)
    chunk = root_chunk(2 * U * BLOCK + 7, 3, 256)
    assert chunk == root_chunk(2 * U * BLOCK + 7, 2, 256) == root_chunk(2 * U * BLOCK + 7, 2, 8) == 1024
    return [1, BLOCK - 1, BLOCK, BLOCK + 1, chunk, chunk + 1, 2 * U * BLOCK + 7]


SHAPES = _shapes()
P = dict(n_estimators=4, max_depth=3, learning_rate=0.3, gamma=0.0, scale_pos_weight=4.0, random_state=7)

# variant -> (parameter overrides, COBALT_MARGIN_IN_RECORD, row_reorder, soft labels + weights,
#             the root mode of the fit's last grow call as the launch plan reports it)
VARIANTS = {
    "rec": ({}, "2", "off", False, "rec"),                 # kRootRec in every tree
    "rec_orig": ({}, "2", [0], False, "rec_orig"),         # kRootRec in tree 0, kRootRecOrig in trees 1-3
    # colsample masks features out of a tree: the record modes add them into their own, unread cells
    "rec_colsample": ({"colsample_bytree": 0.5}, "2", "off", False, "rec"),
    "rec_orig_colsample": ({"colsample_bytree": 0.5}, "2", [0], False, "rec_orig"),
    "generic_margin_array": ({}, "0", "off", False, "generic"),
    "generic_subsample": ({"subsample": 0.5}, "2", "off", False, "generic"),
    "generic_wide": ({"grad_bits": 25}, "2", "off", False, "generic"),
    "generic_label_weight_arrays": ({}, "2", "off", True, "generic"),
}
REC_BLOCKS_PER_CU = 3  # 78-79 VGPRs x 512 threads and 3 x ~50 KB of LDS on the MI355X's CU

_data, _oracle = {}, {}


def _xyw(n, soft, F=20):
    if (n, soft, F) not in _data:
        X, y = synth.make_lendingclub(n, seed=11)
        X = X[:, :F].contiguous()
        w = None
        if soft:  # labels that are no 0 / 1 and non-unit weights: the pass reads the label and weight arrays
            g = torch.Generator().manual_seed(n)
            y = (y * 0.75 + 0.125).to(torch.float32)
            w = torch.rand(n, generator=g) + 0.5
        _data[(n, soft, F)] = (X, y, w)
    return _data[(n, soft, F)]


def _fit(n, over, soft, device, reorder="off", F=20):
    X, y, w = _xyw(n, soft, F)
    rep = gbdt.FitReport()
    p = gbdt.GBDTParams(**{**P, **over, "row_reorder": reorder})
    b = gbdt.train(X, y, p, device=device, report=rep, sample_weight=w)
    m = rep.extra["margin"]
    m = m.cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
    return b.save_raw("ubj"), m.astype(np.float32, copy=False), rep


def _oracle_of(n, over, soft, F=20):
    """The host oracle's model and margins, computed once per (shape, parameters) and shared."""
    key = (n, tuple(sorted(over.items())), soft, F)
    if key not in _oracle:
        raw, m, _ = _fit(n, over, soft, "cpu", F=F)
        m.setflags(write=False)
        _oracle[key] = (raw, m)
    return _oracle[key]


def _check(n, over, soft, reorder="off", F=20, mode=None, blocks=None):
    """GPU fit == oracle; `mode` / `blocks`: the root pass's data mode and resident blocks per CU that the
    launch plan of the fit's last grow call must report."""
    ref_raw, ref_m = _oracle_of(n, over, soft, F)
    raw, m, rep = _fit(n, over, soft, "cuda", reorder, F)
    assert raw == ref_raw
    assert m.shape == ref_m.shape == (n,)
    assert np.array_equal(m.view(np.uint32), ref_m.view(np.uint32))
    if reorder != "off":  # the rows were regrouped after tree 0, so the later trees ran with orig
        assert rep.extra["row_reorder"] == {"trees": [0], "off": None}
    plan = rep.extra["plan"]
    if mode is not None:
        assert plan["root_mode"] == mode, plan
        assert plan["root_blocks_per_cu"] == (blocks if blocks is not None else 2 if mode == "generic" else REC_BLOCKS_PER_CU), plan
    return rep


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_mode_equals_oracle(variant, n, monkeypatch):
    over, mrec, reorder, soft, mode = VARIANTS[variant]
    monkeypatch.setenv("COBALT_MARGIN_IN_RECORD", mrec)
    _check(n, over, soft, reorder, mode=mode)


@pytest.mark.parametrize("reorder", ["off", [0]], ids=["rec", "rec_orig"])
@pytest.mark.parametrize("n", [BLOCK + 1, 2 * U * BLOCK + 7])
@pytest.mark.parametrize("F", [9, 10, 14, 18, 19])
def test_record_modes_at_other_feature_counts(F, n, reorder, monkeypatch):
    """Every tile width of the record kernels (FT4 = 12, 16, 20: 32-byte records hold 9 .. 24 features); F % 4 != 0
    leaves padding features in the tile (9 features: three, the most), which add into the trash cells."""
    monkeypatch.setenv("COBALT_MARGIN_IN_RECORD", "2")
    _check(n, {}, False, reorder, F=F, mode="rec" if reorder == "off" else "rec_orig")


@pytest.mark.parametrize("reorder", ["off", [0]], ids=["rec", "rec_orig"])
@pytest.mark.parametrize("depth", [9, 10])
def test_record_modes_with_a_deep_staged_tree(depth, reorder, monkeypatch):
    """From depth 9 the tile + the staged previous tree pass 64 KB of dynamic LDS (20 features: 74 KB, 107 KB):
    the record kernels need the large-LDS opt-in, and fewer blocks fit a CU."""
    monkeypatch.setenv("COBALT_MARGIN_IN_RECORD", "2")
    lds = (20 * 256 + 64) * 8 + (2 ** (depth + 1) - 1) * 32 + 1040
    assert lds > 64 * 1024
    _check(2 * U * BLOCK + 7, {"max_depth": depth}, False, reorder, mode="rec" if reorder == "off" else "rec_orig",
           blocks=min(REC_BLOCKS_PER_CU, 160 * 1024 // lds))


def test_mode_follows_the_knob_between_fits(monkeypatch):
    """Margin in record on, then off, on one (parked and reused) context: the kernel is chosen per launch
    (the launch plan reports the mode that ran)."""
    n = SHAPES[-1]
    for mrec, mode in (("2", "rec"), ("0", "generic"), ("2", "rec")):
        monkeypatch.setenv("COBALT_MARGIN_IN_RECORD", mrec)
        _check(n, {}, False, mode=mode)
