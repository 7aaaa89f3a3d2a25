"""Command-line entry point: ``python -m cobalt_smart_lender_ai_amd <command>``.

Commands mirror the reference's scripts:

  synth     write a synthetic LendingClub-shaped raw CSV into the store (offline stand-in for the
            Kaggle download, reference README "Data" section)
  clean     stage 1 (clean_data.py; ``--full`` = ``python clean_data.py full``)
  features  stage 2 (feature_engineering.py)
  train     tree model training (model_tree_train_test.py)
  train-nn  NN challenger (notebook 04 cells 31-44)
  explain-nn  per-row integrated-gradients attributions of the NN challenger against a background CSV
            (explain/nn.py)
  serve     FastAPI scoring service (cobalt_fast_api.py, uvicorn)
  dictionary  descriptions of columns from the LendingClub data dictionary workbook (LCDataDictionary.xlsx)
  drift     population-stability (PSI / CSI) report of one CSV against another (monitor/drift.py)
  bootstrap bootstrap confidence intervals of AUC, KS, ... from a CSV of labels and scores (metrics/bootstrap.py)
  calibration reliability report (ECE, Brier decomposition, Hosmer-Lemeshow) of a CSV of labels and probabilities,
            and optionally an isotonic / sigmoid calibrator fitted on it (metrics/calibration.py)
  recourse  counterfactual recourse for a CSV of applicants: the nearest allowed change that brings each declined
            row to the cutoff (explain/recourse.py)
  scorecard fit a WoE points scorecard, the transparent challenger, on a CSV and score rows with it
            (models/scorecard.py)
  corr      correlation matrix of a CSV's numeric columns with missing values, the pairs above a threshold and the
            greedy collinearity screen (select/collinearity.py)
  portfolio-loss  Monte-Carlo loss distribution of a CSV of PDs and exposures under the Gaussian-copula factor
            model: expected loss, VaR, expected shortfall and the segments' share of the tail (portfolio/)
  fairness  fair-lending audit of a CSV of scores and protected attributes: adverse impact ratio, score and
            error-rate gaps per group against a reference group, with bootstrap intervals (fairness/)

The artifact store is ``--store`` or ``$COBALT_ARTIFACT_URI`` (a local directory or ``s3://bucket``).
"""
from __future__ import annotations

import argparse
import json
import logging
import sys
from .config import knob


def _store(args):
    from .dataio.artifacts import get_store

    return get_store(args.store)


def cmd_synth(args) -> int:
    from .config import RAW_DATA_KEY_FULL, RAW_DATA_KEY_SAMPLE
    from .dataio.synth_raw import make_raw_lendingclub

    st = _store(args)
    df = make_raw_lendingclub(args.rows, seed=args.seed)
    st.write_csv(df, RAW_DATA_KEY_FULL if args.full else RAW_DATA_KEY_SAMPLE)
    if args.both:
        st.write_csv(df, RAW_DATA_KEY_SAMPLE if args.full else RAW_DATA_KEY_FULL)
    print(f"[INFO] wrote {len(df)} synthetic raw rows")
    return 0


def cmd_clean(args) -> int:
    from .pipeline.prep_flow import run_clean

    run_clean(_store(args), use_sample=not args.full, device=args.device, preset=args.preset, engine=args.engine)
    return 0


def cmd_features(args) -> int:
    from .pipeline.prep_flow import run_features

    run_features(_store(args), device=args.device, reference_date=args.reference_date, engine=args.engine)
    return 0


def cmd_train(args) -> int:
    from .config import TrainConfig
    from .pipeline.train_tree import run_training

    st = _store(args)
    cfg = TrainConfig(device=args.device)
    if args.n_iter is not None:
        cfg.search_n_iter = args.n_iter
    if args.gpus is not None:
        cfg.fits_in_parallel = args.gpus
    from .parallel.taskpool import GpuTaskPool, resolve_workers

    # the search's worker processes are spawned first, before this process touches the GPU
    nw = resolve_workers(cfg.fits_in_parallel)
    pool = GpuTaskPool(nw) if nw > 1 else None
    try:
        from .pipeline.prep_flow import read_table

        df = read_table(st, cfg.input_key, args.device)
        m = run_training(df, cfg, store=st, local_dir=args.local_dir, device=args.device, pool=pool)
    finally:
        if pool is not None:
            pool.close()
    print(json.dumps({k: m[k] for k in ("auc", "best_params", "timing_s", "selected_features")}, indent=2))
    return 0


def cmd_train_nn(args) -> int:
    from .config import CLEAN_DATA_KEY_NN
    from .nn.mlp import MLPConfig
    from .pipeline.train_nn import NNTrainConfig, run_nn_training

    st = _store(args)
    cfg = NNTrainConfig(reproduce_reference=not args.use_smote, mlp=MLPConfig(epochs=args.epochs))
    from .pipeline.prep_flow import read_table

    m = run_nn_training(read_table(st, CLEAN_DATA_KEY_NN, args.device), cfg, store=st, local_dir=args.local_dir,
                        device=args.device, explain_rows=args.explain)
    print(json.dumps({k: m[k] for k in ("auc", "auc_thresholded", "selected_features", "train_seconds")}, indent=2))
    return 0


def cmd_explain_nn(args) -> int:
    """Integrated gradients (explain/nn.py) of the rows of ROWS.csv under the MLP challenger MODEL, against the
    rows of --background: per row the base value, the model output and the contributions, as JSON records."""
    import pandas as pd

    from .explain import MLPExplainer, force_data
    from .nn.mlp import MLPModel
    from .nn.smote import MinMaxScaler

    model = MLPModel.load(args.model)
    rows, bg = pd.read_csv(args.rows), pd.read_csv(args.background)
    names = list(model.feature_names or rows.columns[: model.n_features])
    for path, df in ((args.rows, rows), (args.background, bg)):
        missing = [c for c in names if c not in df.columns]
        if missing:
            raise SystemExit(f"{path} lacks the model's columns {missing}")
    X, Z = rows[names].to_numpy(dtype="float64"), bg[names].to_numpy(dtype="float64")
    if args.scaler:
        with open(args.scaler) as fh:
            scaler = MinMaxScaler.from_json(fh.read())
        X, Z = scaler.transform(X), scaler.transform(Z)
    ex = MLPExplainer(model, Z.astype("float32"), model_output=args.output, n_steps=args.steps, device=args.device)
    exp = ex(X.astype("float32"))
    exp.feature_names = names
    print(json.dumps([force_data(exp, i) for i in range(len(X))]))
    return 0


def cmd_serve(args) -> int:
    import os
    import subprocess
    import sys
    import tempfile

    import uvicorn

    # One Python event loop tops out near ~1.7k requests/s on HTTP parsing and validation. With
    # --workers N > 1 the N uvicorn workers stay CPU-only and forward rows to ONE scorer process that
    # owns the GPU (serve/scorer.py): one engine, one set of hipGraphs, and micro-batches that pool the
    # requests of every worker.
    scorer = None
    if args.workers > 1 and not knob("COBALT_SCORER_SOCKET"):
        sock = os.path.join(tempfile.mkdtemp(prefix="cobalt_scorer_"), "scorer.sock")
        cmd = [sys.executable, "-m", "cobalt_smart_lender_ai_amd.serve.scorer", "--socket", sock]
        if args.device:
            cmd += ["--device", args.device]
        scorer = subprocess.Popen(cmd)
        os.environ["COBALT_SCORER_SOCKET"] = sock  # inherited by the spawned workers
    try:
        if args.workers > 1:
            from .serve.workers import run_workers  # SO_REUSEPORT workers (see there: TCP_NODELAY)

            return run_workers(args.host, args.port, args.workers, args.log_level)
        uvicorn.run("cobalt_smart_lender_ai_amd.serve.app:create_app", factory=True, host=args.host,
                    port=args.port, log_level=args.log_level)
    finally:
        if scorer is not None:
            scorer.terminate()
            scorer.wait(timeout=30)
    return 0


def cmd_dvc(args) -> int:
    """DVC-compatible versioning of raw data files (dataio/dvc.py): add / status / push / pull."""
    from .dataio import dvc

    st = _store(args)
    for target in args.targets:
        if args.action == "add":
            print(dvc.add(target))
        elif args.action == "status":
            for p, s in dvc.status(target).items():
                print(f"{s}\t{p}")
        elif args.action == "push":
            print("\n".join(dvc.push(target, st, prefix=args.prefix)))
        else:
            print("\n".join(str(p) for p in dvc.pull(target, st, prefix=args.prefix)))
    return 0


def cmd_dictionary(args) -> int:
    from .dataio import dictionary, synth

    dd = dictionary.load_data_dictionary(args.xlsx)
    cols = args.columns or synth.FEATURES
    for c, desc in dictionary.describe_columns(cols, dd).items():
        print(f"{c}\t{desc}")
    return 0


def cmd_drift(args) -> int:
    """PSI / CSI of CUR.csv against REF.csv (monitor/drift.py): the report as JSON, the top rows on stdout."""
    import pandas as pd
    import torch

    from .monitor import DriftBaseline

    ref, cur = pd.read_csv(args.ref), pd.read_csv(args.cur)
    model = None
    if args.model:
        from .models.booster import Booster

        model = Booster.load_model(args.model)
    if model is not None and model.feature_names:
        cols = list(model.feature_names)
    else:
        num = [c for c in ref.columns if c in cur.columns and pd.api.types.is_numeric_dtype(ref[c])
               and pd.api.types.is_numeric_dtype(cur[c])]
        cols = [c for c in num if c != args.label]
    if not cols:
        raise SystemExit("no numeric column is common to both files")
    y_ref = ref[args.label].to_numpy() if args.label and args.label in ref.columns else None
    y_cur = cur[args.label].to_numpy() if args.label and args.label in cur.columns else None

    def mat(df):
        X = df[cols].to_numpy(dtype="float32", na_value=float("nan"))
        dev = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
        return torch.as_tensor(X, device=dev) if str(dev).startswith("cuda") else X

    base = DriftBaseline.fit(mat(ref), feature_names=cols, model=model, n_bins=args.bins, y=y_ref)
    rep = base.compare(mat(cur), y=y_cur)
    with open(args.out, "w") as fh:
        json.dump(rep.to_dict(), fh)
    for r in list(rep)[:args.top]:
        print(f"{r['feature']}\t{r['psi']:.6f}\t{r['status']}")
    print(f"[INFO] wrote {args.out} ({len(rep)} rows)")
    return 0


def cmd_bootstrap(args) -> int:
    """Bootstrap intervals (metrics/bootstrap.py) of the scores in SCORES.csv against its label column, and the
    paired comparison when a second score column is named: the report as JSON on stdout."""
    import pandas as pd
    import torch

    from .metrics import bootstrap_ci

    df = pd.read_csv(args.csv)
    for c in [args.label, args.score] + ([args.score_b] if args.score_b else []):
        if c not in df.columns:
            raise SystemExit(f"{args.csv} has no column {c!r}")
    dev = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    rep = bootstrap_ci(df[args.label].to_numpy(), df[args.score].to_numpy(dtype="float32"),
                       df[args.score_b].to_numpy(dtype="float32") if args.score_b else None,
                       metrics=tuple(args.metrics.split(",")), n_boot=args.n_boot, alpha=args.alpha, seed=args.seed,
                       threshold=args.threshold, device=dev)
    d = rep.to_dict()
    if not args.values:
        for part in ("metrics", "metrics_b", "delta"):
            for m in d.get(part, {}).values():
                m.pop("values")
    print(json.dumps(d))
    return 0


def cmd_calibration(args) -> int:
    """The reliability report (metrics/calibration.py) of the probabilities in SCORES.csv against its label
    column, as JSON on stdout. With --fit, a calibrator is fitted on the log-odds of that column, written to
    --out, and the report of the calibrated probabilities is printed beside the first ("calibrated")."""
    import numpy as np
    import pandas as pd
    import torch

    from .metrics.calibration import reliability_report
    from .models.calibration import make_calibrator

    df = pd.read_csv(args.csv)
    for c in (args.label, args.score):
        if c not in df.columns:
            raise SystemExit(f"{args.csv} has no column {c!r}")
    dev = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    y = torch.as_tensor(df[args.label].to_numpy()).to(dev)
    p = torch.as_tensor(df[args.score].to_numpy(dtype="float32")).to(dev)
    d = reliability_report(y, p, n_bins=args.bins, strategy=args.strategy).to_dict()
    if args.fit:
        p64 = p.to(torch.float64).clamp(1e-12, 1 - 1e-12)
        margin = (torch.log(p64) - torch.log1p(-p64)).to(torch.float32)
        cal = make_calibrator(args.fit).fit(margin, y)
        cal.save(args.out)
        d["calibrated"] = reliability_report(y, cal.transform(margin), n_bins=args.bins,
                                             strategy=args.strategy).to_dict()
        d["calibrator"] = args.out
    print(json.dumps(d))
    return 0


def cmd_recourse(args) -> int:
    """Counterfactual recourse (explain/recourse.py) for the rows of ROWS.csv: per row the nearest allowed change
    that brings the probability of default to the cutoff, as JSON records (or CSV, by --out's suffix). The
    policy is config.RECOURSE_POLICY with the three direction lists replaced by the flags that are given."""
    import pandas as pd
    import torch

    from .config import ServeConfig, from_env
    from .explain.recourse import counterfactuals, default_policy
    from .serve.app import load_model

    cfg = from_env(ServeConfig)
    if args.model:
        cfg.model_path, cfg.source = args.model, "local"
    b = load_model(cfg)
    df = pd.read_csv(args.rows)
    names = list(b.feature_names or df.columns[: b.num_feature])
    missing = [c for c in names if c not in df.columns]
    if missing:
        raise SystemExit(f"{args.rows} lacks the model's columns {missing}")
    policy = default_policy(b)
    for key in ("immutable", "increase_only", "decrease_only"):
        v = getattr(args, key)
        if v is not None:
            policy[key] = tuple(s for s in v.split(",") if s)
    dev = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    X = df[names].to_numpy(dtype="float32", na_value=float("nan"))
    rep = counterfactuals(b, X, cutoff=args.cutoff, max_changes=args.max_changes, device=dev, **policy)
    recs = rep.to_records()
    if args.out and args.out.lower().endswith(".csv"):
        flat = [{**{k: v for k, v in r.items() if k != "changes"}, "n_changes": len(r["changes"]),
                 "changes": "; ".join(f"{c['feature']}: {c['from']:g} -> {c['to']:g}" for c in r["changes"])}
                for r in recs]
        pd.DataFrame(flat).to_csv(args.out, index=False)
    elif args.out:
        with open(args.out, "w") as fh:
            json.dump(recs, fh)
    else:
        print(json.dumps(recs))
    if args.out:
        print(f"[INFO] wrote {args.out} ({len(recs)} rows): {json.dumps(rep.summary())}")
    return 0


def cmd_scorecard(args) -> int:
    """A WoE points scorecard (models/scorecard.py) fitted on TRAIN.csv: ``scorecard.json`` and
    ``scorecard_points.csv`` in --out; with --score, the rows of that CSV with ``score``, ``prob_default`` and
    ``reason_1..k`` as ``scorecard_scored.csv``."""
    import os

    import pandas as pd
    import torch

    from .models.scorecard import Scorecard

    df = pd.read_csv(args.train)
    if args.label not in df.columns:
        raise SystemExit(f"{args.train} has no column {args.label!r}")
    cols = args.features.split(",") if args.features else [
        c for c in df.columns if c != args.label and pd.api.types.is_numeric_dtype(df[c])]
    missing = [c for c in cols if c not in df.columns]
    if missing or not cols:
        raise SystemExit(f"{args.train} lacks the columns {missing}" if missing else "no numeric feature column")
    dev = args.device or ("cuda" if torch.cuda.is_available() else "cpu")

    def mat(frame):
        X = frame[cols].to_numpy(dtype="float32", na_value=float("nan"))
        return torch.as_tensor(X, device=dev) if str(dev).startswith("cuda") else X

    sc = Scorecard(n_fine=args.bins, max_bins=args.max_bins, min_bin_share=args.min_bin_share, l2=args.l2,
                   pdo=args.pdo, base_points=args.base_points, base_odds=args.base_odds)
    sc.fit(mat(df), df[args.label].to_numpy(dtype="float32"), feature_names=cols)
    path = sc.save(args.out)
    sc.points_frame().to_csv(os.path.join(args.out, "scorecard_points.csv"), index=False)
    print(f"[INFO] wrote {path} ({sc.n_kept} of {len(cols)} characteristics, {sc.fit_info['passes']} Newton passes)")
    if args.score:
        rows = pd.read_csv(args.score)
        lacking = [c for c in cols if c not in rows.columns]
        if lacking:
            raise SystemExit(f"{args.score} lacks the columns {lacking}")
        X = mat(rows)
        rows["score"] = sc.score(X)
        rows["prob_default"] = sc.predict_proba(X)[:, 1]
        rs = sc.reasons(X, top=args.top)
        for k in range(rs.shape[1]):
            rows[f"reason_{k + 1}"] = [cols[f] if f >= 0 else "" for f in rs[:, k]]
        out = os.path.join(args.out, "scorecard_scored.csv")
        rows.to_csv(out, index=False)
        print(f"[INFO] wrote {out} ({len(rows)} rows)")
    return 0


def cmd_corr(args) -> int:
    """The correlation matrix (select/collinearity.py) of the numeric columns of TRAIN.csv: the pairs with ``|r|``
    at or above --threshold and the greedy screen on stdout, everything as ``correlation.json`` in --out. With
    --label the screen keeps, of two correlated features, the one with the higher information value."""
    import os

    import pandas as pd
    import torch

    from .select.collinearity import correlation_matrix, drop_correlated

    df = pd.read_csv(args.train)
    if args.label and args.label not in df.columns:
        raise SystemExit(f"{args.train} has no column {args.label!r}")
    cols = [c for c in df.columns if c != args.label and pd.api.types.is_numeric_dtype(df[c])
            and not pd.api.types.is_bool_dtype(df[c])]
    if not cols:
        raise SystemExit("no numeric feature column")
    dev = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    X = df[cols].to_numpy(dtype="float32", na_value=float("nan"))
    X = torch.as_tensor(X, device=dev) if str(dev).startswith("cuda") else X
    rep = correlation_matrix(X, cols, method=args.method, missing=args.missing, min_periods=args.min_periods)
    priority = None
    if args.label:
        from .monitor import information_value

        iv = {r["feature"]: r["iv"] for r in information_value(X, df[args.label].to_numpy(dtype="float32"),
                                                               feature_names=cols)}
        priority = [iv[c] for c in cols]
    screen = drop_correlated(rep, args.threshold, priority=priority)
    pairs = rep.pairs(args.threshold)
    for p in pairs:
        print(f"{p['a']}\t{p['b']}\t{p['r']:+.6f}\t{p['n']}")
    for d in screen.dropped:
        print(f"[DROP] {d['feature']} (r = {d['r']:+.4f} with {d['by']})")
    print(f"[INFO] kept {len(screen.kept)} of {len(cols)} features at |r| < {args.threshold:g}")
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "correlation.json")
    with open(path, "w") as fh:
        json.dump({**rep.to_dict(), "threshold": args.threshold, "pairs": pairs, "screen": screen.to_dict(),
                   "priority": None if priority is None else dict(zip(cols, map(float, priority)))}, fh)
    print(f"[INFO] wrote {path}")
    return 0


def cmd_portfolio_loss(args) -> int:
    """The loss distribution (portfolio/) of the book in SCORES.csv: ``summary()`` on stdout and the whole report
    as ``portfolio_loss.json`` in --out. --lgd and --rho take a number or, for --lgd, a column name."""
    import os

    import pandas as pd
    import torch

    from .portfolio import simulate_losses

    df = pd.read_csv(args.csv)
    try:
        lgd = float(args.lgd)
    except ValueError:
        lgd = None
    for c in [args.pd, args.exposure] + ([args.lgd] if lgd is None else []) + \
            [c for c in (args.segment, args.sector) if c]:
        if c not in df.columns:
            raise SystemExit(f"{args.csv} has no column {c!r}")
    dev = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    rho = [float(v) for v in str(args.rho).split(",")]
    rep = simulate_losses(df[args.pd].to_numpy(dtype="float64"), df[args.exposure].to_numpy(dtype="float64"),
                          lgd if lgd is not None else df[args.lgd].to_numpy(dtype="float64"),
                          rho=rho[0] if len(rho) == 1 else rho,
                          sector=df[args.sector].to_numpy() if args.sector else None,
                          segment=df[args.segment].to_numpy() if args.segment else None,
                          n_scenarios=args.scenarios, seed=args.seed, unit=args.unit,
                          quantiles=tuple(float(q) for q in args.quantiles.split(",")), device=dev)
    print(rep.summary())
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "portfolio_loss.json")
    with open(path, "w") as fh:
        json.dump(rep.to_dict(), fh)
    print(f"[INFO] wrote {path}")
    return 0


def cmd_fairness(args) -> int:
    """The fair-lending audit (fairness/) of SCORES.csv: ``summary()`` on stdout and the whole report as JSON in
    --out. Every --group column is one audited attribute; its values are read as strings."""
    import pandas as pd
    import torch

    from .fairness import fair_lending_audit

    df = pd.read_csv(args.csv)
    for c in [args.score] + list(args.group) + ([args.label] if args.label else []):
        if c not in df.columns:
            raise SystemExit(f"{args.csv} has no column {c!r}")
    dev = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    score = df[args.score].to_numpy(dtype="float32")
    y = df[args.label].to_numpy(dtype="int64") if args.label else None
    if str(dev).startswith("cuda"):
        score = torch.as_tensor(score, device=dev)
        y = None if y is None else torch.as_tensor(y, device=dev)
    groups = {c: df[c].astype(str).to_numpy() for c in args.group}
    reference = {c: args.reference for c in args.group} if args.reference is not None else None
    cutoffs = [float(v) for v in args.cutoffs.split(",")] if args.cutoffs else None
    rep = fair_lending_audit(score, groups, y, cutoff=args.cutoff, reference=reference, cutoffs=cutoffs,
                             n_boot=args.n_boot, alpha=args.alpha, seed=args.seed, air_floor=args.air_floor)
    print(rep.summary())
    with open(args.out, "w") as fh:
        json.dump(rep.to_dict(), fh)
    print(f"[INFO] wrote {args.out}")
    return 0


def main(argv: list[str] | None = None) -> int:
    logging.basicConfig(level=logging.INFO, format="[%(levelname)s] %(message)s")
    p = argparse.ArgumentParser(prog="cobalt_smart_lender_ai_amd")
    p.add_argument("--store", default=None, help="artifact store (dir or s3://bucket)")
    p.add_argument("--device", default=None, help="cuda:N or cpu (default: cuda:0 when available)")
    sub = p.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("synth")
    s.add_argument("--rows", type=int, default=100_000)
    s.add_argument("--seed", type=int, default=0)
    s.add_argument("--full", action="store_true")
    s.add_argument("--both", action="store_true", help="write the same frame under sample and full keys")
    s.set_defaults(fn=cmd_synth)
    s = sub.add_parser("clean")
    s.add_argument("--full", action="store_true")
    s.add_argument("--preset", default="script", choices=["script", "notebook"])
    s.add_argument("--engine", default=None, choices=["device", "pandas"],
                   help="device-resident frame (default on a GPU) or the pandas path")
    s.set_defaults(fn=cmd_clean)
    s = sub.add_parser("features")
    s.add_argument("--reference-date", default=None)
    s.add_argument("--engine", default=None, choices=["device", "pandas"])
    s.set_defaults(fn=cmd_features)
    s = sub.add_parser("train")
    s.add_argument("--local-dir", default="models")
    s.add_argument("--n-iter", type=int, default=None)
    s.add_argument("--gpus", type=int, default=None)
    s.set_defaults(fn=cmd_train)
    s = sub.add_parser("train-nn")
    s.add_argument("--local-dir", default="models")
    s.add_argument("--epochs", type=int, default=50)
    s.add_argument("--use-smote", action="store_true", help="train on the SMOTE-resampled, scaled rows")
    s.add_argument("--explain", type=int, default=0, metavar="N",
                   help="also write shap_importance_nn.json from N validation rows (integrated gradients)")
    s.set_defaults(fn=cmd_train_nn)
    s = sub.add_parser("explain-nn", help="integrated-gradients attributions of the NN challenger for ROWS.csv")
    s.add_argument("model", help="nn_model.safetensors")
    s.add_argument("rows", help="CSV with the model's feature columns")
    s.add_argument("--background", required=True, help="CSV of background rows the attributions are taken against")
    s.add_argument("--scaler", default=None, help="scaler_nn.json: scale both CSVs before the network sees them")
    s.add_argument("--steps", type=int, default=32, help="midpoint steps per (row, background row) pair")
    s.add_argument("--output", default="probability", choices=["raw", "probability"])
    s.set_defaults(fn=cmd_explain_nn)
    s = sub.add_parser("serve")
    s.add_argument("--host", default="0.0.0.0")
    s.add_argument("--port", type=int, default=8000)
    s.add_argument("--workers", type=int, default=int(__import__("os").environ.get("COBALT_SERVE_WORKERS", "1")))
    s.add_argument("--log-level", default="info")
    s.set_defaults(fn=cmd_serve)
    s = sub.add_parser("dvc", help="DVC-compatible data versioning: add | status | push | pull")
    s.add_argument("action", choices=["add", "status", "push", "pull"])
    s.add_argument("targets", nargs="+", help="data files (add) or .dvc pointers")
    s.add_argument("--prefix", default="dataset/", help="remote key prefix (the reference's DVC remote path)")
    s.set_defaults(fn=cmd_dvc)
    s = sub.add_parser("dictionary", help="column descriptions (default: the 20 deployed model features)")
    s.add_argument("--xlsx", required=True, help="path to LCDataDictionary.xlsx")
    s.add_argument("columns", nargs="*")
    s.set_defaults(fn=cmd_dictionary)
    s = sub.add_parser("drift", help="PSI / CSI drift report of CUR.csv against REF.csv")
    s.add_argument("ref")
    s.add_argument("cur")
    s.add_argument("--model", default=None, help="model checkpoint: adds the score row, fixes the columns")
    s.add_argument("--bins", type=int, default=10)
    s.add_argument("--label", default=None, help="label column (adds WoE / IV per side)")
    s.add_argument("--out", default="drift.json")
    s.add_argument("--top", type=int, default=10, help="rows printed")
    s.set_defaults(fn=cmd_drift)
    s = sub.add_parser("bootstrap", help="bootstrap confidence intervals from a CSV of labels and scores")
    s.add_argument("csv")
    s.add_argument("--label", default="label", help="0/1 label column")
    s.add_argument("--score", default="score", help="score column of the model")
    s.add_argument("--score-b", default=None, help="score column of a second model: adds the paired comparison")
    s.add_argument("--metrics", default="auc,ks", help="comma-separated: auc,gini,ks,error,precision,recall,f1,"
                                                       "logloss,brier")
    s.add_argument("--n-boot", type=int, default=1000)
    s.add_argument("--alpha", type=float, default=0.05)
    s.add_argument("--seed", type=int, default=0)
    s.add_argument("--threshold", type=float, default=0.5)
    s.add_argument("--values", action="store_true", help="keep every replicate's value in the JSON")
    s.set_defaults(fn=cmd_bootstrap)
    s = sub.add_parser("calibration", help="reliability report (and a fitted calibrator) from a CSV of labels and "
                                           "probabilities")
    s.add_argument("csv")
    s.add_argument("--label", default="label", help="0/1 label column")
    s.add_argument("--score", default="score", help="probability column of the model")
    s.add_argument("--bins", type=int, default=10)
    s.add_argument("--strategy", default="quantile", choices=["quantile", "uniform"])
    s.add_argument("--fit", default=None, choices=["isotonic", "sigmoid"],
                   help="fit this calibrator on the column's log-odds and report the calibrated scores too")
    s.add_argument("--out", default="calibration.json", help="where --fit writes the calibrator")
    s.set_defaults(fn=cmd_calibration)
    s = sub.add_parser("recourse", help="the nearest change that approves each declined row of ROWS.csv")
    s.add_argument("rows", help="CSV with the model's feature columns")
    s.add_argument("--model", default=None, help="model checkpoint (default: $COBALT_MODEL_PATH)")
    s.add_argument("--cutoff", type=float, default=0.5, help="approve at or below this probability of default")
    s.add_argument("--max-changes", type=int, default=1)
    s.add_argument("--immutable", default=None, help="comma-separated features that never change")
    s.add_argument("--increase-only", default=None, help="comma-separated features that may only grow")
    s.add_argument("--decrease-only", default=None, help="comma-separated features that may only shrink")
    s.add_argument("--out", default=None, help="write JSON records (or CSV, by suffix) here instead of stdout")
    s.set_defaults(fn=cmd_recourse)
    s = sub.add_parser("scorecard", help="fit a WoE points scorecard on TRAIN.csv (and score ROWS.csv with it)")
    s.add_argument("train", help="CSV with the label and the feature columns")
    s.add_argument("--label", default="loan_default", help="0/1 label column (1 = bad)")
    s.add_argument("--features", default=None, help="comma-separated feature columns (default: every numeric one)")
    s.add_argument("--out", default="scorecard", help="directory for scorecard.json and scorecard_points.csv")
    s.add_argument("--score", default=None, help="CSV of rows to score: adds scorecard_scored.csv")
    s.add_argument("--top", type=int, default=4, help="reason codes per scored row (at most 8)")
    s.add_argument("--bins", type=int, default=20, help="fine bins per feature before coarse classing")
    s.add_argument("--max-bins", type=int, default=6)
    s.add_argument("--min-bin-share", type=float, default=0.05)
    s.add_argument("--l2", type=float, default=0.0)
    s.add_argument("--pdo", type=float, default=20.0, help="points that double the odds")
    s.add_argument("--base-points", type=float, default=600.0)
    s.add_argument("--base-odds", type=float, default=50.0, help="odds good:bad at --base-points")
    s.set_defaults(fn=cmd_scorecard)
    s = sub.add_parser("corr", help="correlation matrix, correlated pairs and the collinearity screen of TRAIN.csv")
    s.add_argument("train", help="CSV with the feature columns (and the label, with --label)")
    s.add_argument("--method", default="pearson", choices=["pearson", "spearman"])
    s.add_argument("--missing", default="pairwise", choices=["pairwise", "listwise"])
    s.add_argument("--min-periods", type=int, default=1)
    s.add_argument("--threshold", type=float, default=0.7, help="|r| from which two features count as collinear")
    s.add_argument("--label", default=None, help="0/1 label column: the screen keeps the feature with the higher IV")
    s.add_argument("--out", default="correlation", help="directory for correlation.json")
    s.set_defaults(fn=cmd_corr)
    s = sub.add_parser("portfolio-loss", help="loss distribution, VaR and expected shortfall of a CSV of PDs and "
                                              "exposures")
    s.add_argument("csv", help="CSV with one row per loan")
    s.add_argument("--pd", default="pd", help="column of calibrated default probabilities")
    s.add_argument("--exposure", default="loan_amnt", help="column of exposures at default")
    s.add_argument("--lgd", default="1.0", help="loss given default: a number or a column")
    s.add_argument("--rho", default="0.15", help="asset correlation: a number, or one per sector separated by commas")
    s.add_argument("--sector", default=None, help="column of integer sector ids (one factor each)")
    s.add_argument("--segment", default=None, help="column to break the loss down by")
    s.add_argument("--scenarios", type=int, default=10000)
    s.add_argument("--seed", type=int, default=0)
    s.add_argument("--unit", type=int, default=100, help="integer units per currency unit (100: cents)")
    s.add_argument("--quantiles", default="0.95,0.99,0.999")
    s.add_argument("--out", default=".", help="directory for portfolio_loss.json")
    s.set_defaults(fn=cmd_portfolio_loss)
    s = sub.add_parser("fairness", help="fair-lending audit of a CSV of scores and protected attributes")
    s.add_argument("csv", help="CSV with one row per applicant")
    s.add_argument("--score", default="score", help="column of default probabilities")
    s.add_argument("--group", action="append", required=True, help="protected-attribute column (repeatable)")
    s.add_argument("--label", default=None, help="0/1 outcome column (1 = bad): adds error gaps, calibration, AUC")
    s.add_argument("--cutoff", type=float, default=0.5, help="declined above this probability of default")
    s.add_argument("--cutoffs", default=None, help="comma-separated further cutoffs for the AIR curve")
    s.add_argument("--reference", default=None, help="reference group (default: the highest approval rate)")
    s.add_argument("--n-boot", type=int, default=1000)
    s.add_argument("--alpha", type=float, default=0.05)
    s.add_argument("--seed", type=int, default=0)
    s.add_argument("--air-floor", type=float, default=0.8)
    s.add_argument("--out", default="fairness.json", help="where the report is written")
    s.set_defaults(fn=cmd_fairness)
    args = p.parse_args(argv)
    return args.fn(args)


if __name__ == "__main__":
    sys.exit(main())
