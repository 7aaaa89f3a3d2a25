"""The fair-lending sums (``fairness.sums``), the report built on them (``fairness.fair_lending_audit``), the CLI
verb and the plots, on the host. The sums are integers: every comparison of sums is exact.

Interval tests assert ``n_degenerate == 0``: their inputs have at least 50 rows in the smallest group and
per-group approval and bad rates between 0.2 and 0.8 (``test_interval_inputs_are_not_degenerate`` checks that on
the definition). ``test_degenerate_replicates`` is the one test that allows degenerate replicates."""
import json
import math

import numpy as np
import pytest

from cobalt_smart_lender_ai_amd import cli, fairness
from cobalt_smart_lender_ai_amd.fairness import sums as S
from cobalt_smart_lender_ai_amd.metrics import bootstrap as B
from fairness_cases import CUTOFFS, SEED, audit_population, population, two_groups


def _same(a, b) -> bool:
    """Equality of two to_dict() trees, NaN (None after _plain) equal to itself."""
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)


def test_hand_case():
    score, group = two_groups(100, 50, 100, 60)
    rep = fairness.fair_lending_audit(score, group, n_boot=200, seed=SEED)
    a, b = rep["group"]["A"], rep["group"]["B"]
    assert rep["group"].reference == "A" and a.is_reference and not b.is_reference
    assert (a.n, b.n) == (100, 100)
    assert a["approval_rate"].point == 0.5 and b["approval_rate"].point == 0.4
    assert b["air"].point == 0.4 / 0.5 and a["air"].point == 1.0
    assert b["parity_diff"].point == 0.4 - 0.5 and b["parity_diff"].point == pytest.approx(-0.1, abs=1e-15)
    assert b["share"].point == 0.5
    assert all(m.n_degenerate == 0 for g in (a, b) for m in g.metrics.values() if m is not g["smd"])
    assert b["air"].low < 0.8 < b["air"].high and a.verdict == "pass"
    # by the other reference the ratio turns over
    other = fairness.fair_lending_audit(score, group, n_boot=8, seed=SEED, reference="B")
    assert other["group"]["A"]["air"].point == 0.5 / 0.4 and other["group"].reference == "B"


def test_an_interval_across_the_floor_is_inconclusive():
    score, group = two_groups(1000, 500, 1000, 605)      # 0.395 / 0.5 = 0.79
    rep = fairness.fair_lending_audit(score, group, n_boot=400, seed=SEED)
    b = rep["group"]["B"]
    assert b["air"].point == 0.395 / 0.5 and b["air"].point == pytest.approx(0.79, abs=1e-15)
    assert b["air"].n_degenerate == 0 and b["air"].low < 0.8 < b["air"].high
    assert b.verdict == "inconclusive"
    assert fairness.verdict(0.5, 0.79) == "adverse" and fairness.verdict(0.8, 0.9) == "pass"
    assert fairness.verdict(0.7, 0.8) == "inconclusive" and fairness.verdict(math.nan, math.nan) == "inconclusive"
    clear = fairness.fair_lending_audit(*two_groups(1000, 500, 1000, 800), n_boot=400, seed=SEED)
    assert clear["group"]["B"].verdict == "adverse" and clear["group"]["B"]["air"].n_degenerate == 0


def test_smd_against_numpy_on_the_grid():
    score, groups, _ = audit_population()
    rep = fairness.fair_lending_audit(score, groups["region"], n_boot=50, seed=SEED, reference="north")
    q = np.minimum(np.floor(score.astype(np.float64) * 65536.0), 65535.0) / 65536.0
    ref = q[groups["region"] == "north"]
    for name in ("south", "west"):
        g = q[groups["region"] == name]
        want = (g.mean() - ref.mean()) / math.sqrt((g.var() + ref.var()) / 2.0)
        # the report forms E[q^2] - E[q]^2 in fp64 from exact sums: terms below 1, so an absolute error of a few
        # 2^-53 in a variance of about 0.04, far inside 1e-9 of the ratio
        assert rep["group"][name]["smd"].point == pytest.approx(want, rel=1e-9, abs=1e-12)
        assert rep["group"][name]["smd"].n_degenerate == 0
    assert rep["group"]["north"]["smd"].point == 0.0
    assert rep["group"]["south"]["smd"].point > 0.1      # the builder shifts the south's scores up


@pytest.mark.parametrize("threshold", [0.5, 0.35])
def test_sums_agree_with_the_bootstrap_sums(threshold):
    _, score, group, y = population(700, 5, seed=3)
    reps = 24
    got = S.fairness_sums_host(score, group, y, [threshold], SEED, reps)
    rs = B.rank_structure(y, score, threshold)
    want, _ = B.bootstrap_sums_host(rs, B.bootstrap_counts_host(SEED, 700, reps))
    P, N, TP, FP = want[0], want[1], want[4], want[5]
    n, Bd, D, DB = got[0], got[1], got[4], got[5]
    assert np.array_equal(DB.sum(axis=0), TP) and np.array_equal((D - DB).sum(axis=0), FP)
    assert np.array_equal(Bd.sum(axis=0), P) and np.array_equal(n.sum(axis=0), P + N)
    assert TP.min() > 0 and FP.min() > 0


@pytest.mark.parametrize("tile_rows", [1, 7, 1024])
def test_tiled_form_equals_direct_form(tile_rows):
    rows, score, group, y = population(2300 if tile_rows == 1024 else 150, 5, seed=tile_rows)
    for K in (1, 16):
        kw = dict(n_groups=6, rows=rows)                      # group 5 stays empty
        want = S.fairness_sums_host(score, group, y, CUTOFFS[K], SEED, 9, **kw)
        got = S.fairness_sums_tiled_host(score, group, y, CUTOFFS[K], SEED, 9, tile_rows=tile_rows, **kw)
        assert want.shape == (4 + 2 * K, 6, 9) and want.dtype == np.int64 and np.array_equal(got, want)
        assert int(np.abs(want[:, 5]).sum()) == 0 and want[0, :5].min() > 0
    assert len(S.field_names(16)) == 36 and S.field_names(2) == ("n", "B", "S1", "S2", "D0", "D1", "DB0", "DB1")


def test_unit_replicate_gives_the_plain_counts():
    rows, score, group, y = population(400, 3, seed=8)
    cut = CUTOFFS[2]
    for fn in (S.fairness_sums_host, lambda *a, **k: S.fairness_sums_tiled_host(*a, tile_rows=64, **k)):
        got = fn(score, group, y, cut, SEED, 1, rows=rows, unit=True)
        q = np.minimum(np.floor(score * np.float32(65536)), 65535).astype(np.int64)
        for g in range(3):
            m = group == g
            dec = [score[m] > np.float32(c) for c in cut]
            want = [m.sum(), y[m].sum(), q[m].sum(), (q[m] ** 2).sum(), dec[0].sum(), dec[1].sum(),
                    (dec[0] & (y[m] == 1)).sum(), (dec[1] & (y[m] == 1)).sum()]
            assert got[:, g, 0].tolist() == [int(v) for v in want]
    none = S.fairness_sums_host(score, group, None, cut, SEED, 5)
    with_y = S.fairness_sums_host(score, group, y, cut, SEED, 5)
    assert int(np.abs(none[[1, 6, 7]]).sum()) == 0 and np.array_equal(none[[0, 2, 3, 4, 5]], with_y[[0, 2, 3, 4, 5]])


def test_windows_of_replicates():
    rows, score, group, y = population(300, 4, seed=9)
    whole = S.fairness_sums_host(score, group, y, CUTOFFS[2], SEED, 8, rows=rows)
    parts = [S.fairness_sums_host(score, group, y, CUTOFFS[2], SEED, 4, r0, rows=rows) for r0 in (0, 4)]
    assert np.array_equal(np.concatenate(parts, axis=2), whole)
    assert not np.array_equal(parts[0], parts[1])
    assert not np.array_equal(S.fairness_sums_host(score, group, y, CUTOFFS[2], SEED + 1, 8, rows=rows), whole)


def test_row_order_does_not_matter():
    rows, score, group, y = population(500, 4, seed=10)
    want = S.fairness_sums_host(score, group, y, CUTOFFS[16], SEED, 6, rows=rows)
    perm = np.random.default_rng(0).permutation(500)
    got = S.fairness_sums_host(score[perm], group[perm], y[perm], CUTOFFS[16], SEED, 6, rows=rows[perm])
    assert np.array_equal(got, want)
    other = S.fairness_sums_host(score[perm], group[perm], y[perm], CUTOFFS[16], SEED, 6)   # other indices
    assert not np.array_equal(other, want) and np.array_equal(
        S.fairness_sums_host(score, group, y, CUTOFFS[16], SEED, 1, unit=True),
        S.fairness_sums_host(score[perm], group[perm], y[perm], CUTOFFS[16], SEED, 1, unit=True))


def test_renamed_groups_keep_their_rows():
    score, groups, y = audit_population()
    names = {"north": "zeta", "south": "alpha", "west": "mid"}     # the sorted order, and so every code, changes
    renamed = np.array([names[g] for g in groups["region"]])
    a = fairness.fair_lending_audit(score, groups["region"], y, n_boot=60, seed=SEED)
    b = fairness.fair_lending_audit(score, renamed, y, n_boot=60, seed=SEED)
    assert list(b["group"].groups) == ["alpha", "mid", "zeta"] and b["group"].reference == names[a["group"].reference]
    for old, new in names.items():
        da, db = a["group"][old].to_dict(values=True), b["group"][new].to_dict(values=True)
        assert da.pop("name") == old and db.pop("name") == new and _same(da, db)
    # integer codes with names, in another order of the codes
    code = np.array([{"north": 2, "south": 0, "west": 1}[g] for g in groups["region"]])
    c = fairness.fair_lending_audit(score, code, y, n_boot=60, seed=SEED, group_names=["south", "west", "north"])
    for name in names:
        assert _same(c["group"][name].to_dict(values=True), a["group"][name].to_dict(values=True))
    assert all(m.n_degenerate == 0 for g in a["group"].groups.values() for m in g.metrics.values())


def test_a_dict_of_attributes_is_one_audit_each():
    score, groups, y = audit_population()
    kw = dict(cutoffs=[0.4, 0.6], n_boot=60, seed=SEED)
    both = fairness.fair_lending_audit(score, groups, y, reference={"region": "north", "age": "under40"}, **kw)
    assert list(both.attributes) == ["region", "age"]
    for name, ref in (("region", "north"), ("age", "under40")):
        one = fairness.fair_lending_audit(score, groups[name], y, reference=ref, **kw)
        da, db = both[name].to_dict(values=True), one["group"].to_dict(values=True)
        assert da.pop("name") == name and db.pop("name") == "group" and _same(da, db)
    rows = both.table()
    assert [(r["attribute"], r["group"]) for r in rows] == [("region", "north"), ("region", "south"), ("region", "west"),
                                                             ("age", "over40"), ("age", "under40")]
    assert {"air", "air_low", "air_high", "air_std", "smd", "auc", "equal_opportunity_gap", "false_positive_gap",
            "calibration_gap", "bad_rate", "verdict", "n"} <= set(rows[0])
    curve = both.air_curve()
    assert len(curve) == 5 * 2 and {r["cutoff"] for r in curve} == {float(np.float32(0.4)), float(np.float32(0.6))}
    assert fairness.fair_lending_audit(score, groups["age"], n_boot=8).air_curve() == []
    assert "region (reference: north)" in both.summary() and json.dumps(both.to_dict())
    # the per-group AUC is the bootstrap report's on the group's rows, resample included
    m = groups["age"] == "over40"
    idx = np.flatnonzero(m)
    rs = B.rank_structure(y[m], score[m], 0.5)
    ints, fl = B.bootstrap_sums_host(rs, B.bootstrap_counts_host(SEED, idx, 60))
    assert np.array_equal(both["age"]["over40"]["auc"].values, B.metrics_from_sums(ints, fl, ("auc",))["auc"])


def test_interval_inputs_are_not_degenerate():
    """The condition the interval tests rest on, checked on the definition alone."""
    score, groups, y = audit_population()
    for name, v in groups.items():
        names, code = np.unique(v, return_inverse=True)
        for unit in (True, False):
            s = S.fairness_sums_host(score, code, y, [0.5], SEED, 1 if unit else 60, unit=unit).astype(np.float64)
            n, Bd, D, DB = s[0], s[1], s[4], s[5]
            assert n.min() >= 50 and Bd.min() > 0 and (n - Bd).min() > 0 and (n - D).min() > 0
            if unit:
                assert 0.2 < (1 - D / n).min() and (1 - D / n).max() < 0.8
                assert 0.2 < (Bd / n).min() and (Bd / n).max() < 0.8


def test_degenerate_replicates():
    score, group = two_groups(300, 150, 2, 1)
    y = np.concatenate([np.arange(300) % 2, [1, 0]])
    rep = fairness.fair_lending_audit(score, group, y, n_boot=200, seed=SEED)
    air, eo = rep["group"]["B"]["air"], rep["group"]["B"]["equal_opportunity_gap"]
    empty = int((rep["group"].sums["reps"][0, 1] == 0).sum())
    assert air.n_degenerate == empty > 0 and eo.n_degenerate >= air.n_degenerate
    assert math.isfinite(air.low) and math.isfinite(air.high) and math.isfinite(air.std) and air.point == 1.0
    assert np.isnan(air.values).sum() == air.n_degenerate
    assert rep["group"]["A"]["approval_rate"].n_degenerate == 0
    assert rep["group"]["B"]["auc"].n_degenerate > 0 and rep["group"]["B"]["auc"].point in (0.0, 0.5, 1.0)


def test_refusals():
    score, groups, y = audit_population(200)
    g = groups["age"]
    nan, high = score.copy(), score.copy()
    nan[3], high[5] = np.nan, 1.5
    for bad in (dict(p_default=nan), dict(p_default=high), dict(p_default=-high), dict(group=np.arange(200)),
                dict(cutoffs=np.linspace(0.1, 0.9, 16)), dict(group=g[:150]), dict(y=y[:150]), dict(reference="nobody"),
                dict(y=y + 1), dict(y=y * 0.5), dict(n_boot=0), dict(alpha=1.0), dict(group=np.linspace(0, 1, 200)),
                dict(group={"age": g, "wide": np.arange(200) % 65})):
        with pytest.raises(ValueError):
            fairness.fair_lending_audit(**{**dict(p_default=score, group=g, y=y, n_boot=8), **bad})
    code = np.unique(g, return_inverse=True)[1]
    ok = dict(score=score, group=code, y=y, cutoffs=[0.5], seed=SEED, reps=4)
    for bad in (dict(score=nan), dict(score=high), dict(group=code + 63), dict(group=code, n_groups=65),
                dict(cutoffs=[0.5] * 17), dict(cutoffs=[]), dict(y=y[:-1]), dict(y=y * 2), dict(group=code[:-1]),
                dict(rep0=2), dict(rep0=-4), dict(reps=0), dict(rows=np.arange(199)), dict(rows=np.arange(200) + (1 << 28)),
                dict(group=code.astype(np.float64)), dict(seed=-1)):
        for fn in (S.fairness_sums_host, lambda **k: S.fairness_sums_tiled_host(tile_rows=64, **k)):
            with pytest.raises(ValueError):
                fn(**{**ok, **bad})
    assert S.fairness_sums_host(**ok).shape == (6, 2, 4)
    assert S.fairness_sums_host(**{**ok, "group": code * 63, "cutoffs": [0.5] * 16}).shape == (36, 64, 4)


def test_cli_round_trip(tmp_path, capsys):
    import pandas as pd

    score, groups, y = audit_population(600)
    csv, out = tmp_path / "scores.csv", tmp_path / "report.json"
    pd.DataFrame({"p": score, "addr_state": groups["region"], "age": groups["age"], "y": y}).to_csv(csv, index=False)
    rc = cli.main(["--device", "cpu", "fairness", str(csv), "--score", "p", "--group", "addr_state", "--label", "y",
                   "--cutoff", "0.5", "--reference", "north", "--n-boot", "40", "--cutoffs", "0.4,0.6", "--out",
                   str(out)])
    assert rc == 0 and "addr_state (reference: north)" in capsys.readouterr().out
    back = pd.read_csv(csv)
    want = fairness.fair_lending_audit(back["p"].to_numpy(dtype="float32"), {"addr_state": back["addr_state"].to_numpy()},
                                       back["y"].to_numpy(), reference={"addr_state": "north"}, n_boot=40,
                                       cutoffs=[0.4, 0.6])
    assert _same(json.loads(out.read_text()), want.to_dict())
    two = tmp_path / "two.json"
    assert cli.main(["--device", "cpu", "fairness", str(csv), "--score", "p", "--group", "addr_state", "--group", "age",
                     "--n-boot", "8", "--out", str(two)]) == 0
    assert list(json.loads(two.read_text())["attributes"]) == ["addr_state", "age"]
    with pytest.raises(SystemExit):
        cli.main(["--device", "cpu", "fairness", str(csv), "--score", "p", "--group", "nowhere"])


def test_plots():
    from cobalt_smart_lender_ai_amd.utils import plots

    score, groups, y = audit_population()
    rep = fairness.fair_lending_audit(score, groups, y, cutoffs=[0.3, 0.4, 0.6, 0.7], n_boot=40, seed=SEED)
    for fig in (plots.adverse_impact_plot(rep), plots.adverse_impact_plot(rep, "age"), plots.air_curve_plot(rep),
                plots.air_curve_plot(rep, "age")):
        assert fig.axes and fig.axes[0].lines
        plots.close(fig)
    with pytest.raises(ValueError):
        plots.air_curve_plot(fairness.fair_lending_audit(score, groups["age"], n_boot=8))
