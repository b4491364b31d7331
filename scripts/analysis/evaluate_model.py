#!/usr/bin/env python3
"""Model evaluation -- counterpart of the reference's scripts/analysis/evaluate_model.py (and of the prediction step that
scripts/analysis/generate_km_curves.py leaves unimplemented: "load each model's best-fold checkpoint and predict").

Reference behaviour kept (evaluate_model.py:27-45,57-60,191-225): read results/test_predictions.csv (columns
survival_time, event, risk_score), C-index = concordance_index(survival_time, -risk_score, event), median split into
'High Risk' (score > median) / 'Low Risk', Kaplan-Meier curves per group, results/evaluation_summary.json with the same
keys; the figures results/{kaplan_meier_curves,risk_score_distribution,survival_vs_risk}.png are written when matplotlib
is importable.  Added: the log-rank test between the two risk groups (what generate_km_curves.py imports logrank_test for)
and the Kaplan-Meier tables as CSV.

    python scripts/analysis/evaluate_model.py                            # evaluates an existing results/test_predictions.csv
    python scripts/analysis/evaluate_model.py --predict models/final/fold_1_best.pth --model final --fold 1
    python scripts/analysis/evaluate_model.py --predict models/final/fold_1_best.pth --model final --fold 1 --attribute [--attribute-format nii]
    python scripts/analysis/evaluate_model.py --predict models/final/fold_1_best.pth --model final --fold 1 --genes models/final/fold_1_genes.json
    python scripts/analysis/evaluate_model.py --ensemble models/final/fold_*_best.pth --model final [--combine rank] [--attribute]
    python scripts/analysis/evaluate_model.py --bootstrap 2000 [--seed 0] [--compare other_model/test_predictions.csv ...]

--predict runs the checkpoint's eval-mode forward on the MI355X (the HIP path; no CPU fallback) over the validation split
of that fold of the cohort the training entry points use (data/processed/* under MMS_DATA_ROOT when present, else the seeded
synthetic cohort) and writes results/test_predictions.csv first.  lifelines/seaborn are not needed: the statistics are the
numpy restatements in multimodal_survival_prediction_amd/survival_stats.py.

--genes FILE (with --predict): the checkpoint was trained on per-fold selected genes (MMS_SELECT_GENES; the fold_k_genes.json written next
to it): the model is built at that width and reads the fold's columns of the RNA-seq matrix; --attribute names the genes by their
original identity.  Ensembles of selected-gene models are not supported (every member has its own columns) and are refused.

--bootstrap R adds "c_index_bootstrap" to the summary: the percentile interval of the C-index over R patient resamples (on the MI355X:
multimodal_survival_prediction_amd/bootstrap.py), for a file with risk_fold_* columns each member's C-index and the paired difference
ensemble - member, and with --compare the paired difference of this file's risk_score against every other file's on the same patients.
A `fold` column, when present, stratifies both the pairs and the resampling.  Without --bootstrap nothing changes.

--stratify R [--min-prop 0.1] adds "risk_stratification" to the summary: the log-rank statistic of EVERY admissible cut of risk_score
(cutpoint_scan.csv), the median split's permutation p, the best cut with the ADJUSTED p of the maximally selected statistic over R random
relabellings (on the MI355X: multimodal_survival_prediction_amd/risk_strata.py), Peto hazard ratios, and Greenwood bands on the
Kaplan-Meier figure.  Without --stratify nothing changes.

--horizons H | t1,t2,... adds "prediction_error" to the summary: the risk score becomes a survival curve S(t | x) through the Breslow
baseline hazard of the fit set (--baseline TRAIN.csv; with --predict the fold's training patients are scored into
<outdir>/train_predictions.csv and used), written per patient to survival_curves.csv, and is judged at the horizons by the IPCW Brier
score, its scaled form against the Kaplan-Meier null model (IPA), the cumulative/dynamic AUC (prediction_error.csv, with intervals when
--bootstrap R is given, on the MI355X: multimodal_survival_prediction_amd/absolute_risk.py) and a calibration table at the middle
horizon (calibration.csv).  --compare-curves adds paired IBS / iAUC differences against other runs' survival_curves.csv on the same
patients and horizons.  A file with risk_fold_* member columns has its risk_score evaluated alone.  Without --horizons nothing changes.

    python scripts/analysis/evaluate_model.py --predict models/final/fold_1_best.pth --model final --fold 1 --horizons 16 --bootstrap 2000
    python scripts/analysis/evaluate_model.py --horizons 365,730,1095 --baseline results/train_predictions.csv

--adjust [COVARIATES.csv] adds "multivariable" to the summary: is risk_score an INDEPENDENT prognostic factor once the covariates of
that file (patient_id plus numeric columns; --adjust-columns a,b takes those alone) are in a Cox model?  The file's columns are the base
model, risk_score is added to it, and every --compare file's risk_score is added under that file's stem: adjusted hazard ratios (per
standard deviation and per unit) with Wald intervals, likelihood-ratio tests of base + covariate against base, and with --bootstrap R
percentile intervals over the same patient resamples as the C-index (on the MI355X: multimodal_survival_prediction_amd/multivariable.py);
multivariable.csv has one row per model and coefficient.  With --predict a bare --adjust writes <outdir>/covariates.csv (age of the
predicted patients, empty where the clinical record is missing) and uses it.  Without --adjust nothing changes.

    python scripts/analysis/evaluate_model.py --adjust data/covariates.csv --compare rnaseq/test_predictions.csv --bootstrap 2000
"""
import argparse
import json
import os
import sys

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts", "training"))

from multimodal_survival_prediction_amd import survival_stats as SS  # noqa: E402

# --model -> (class, constructor kwargs, the cohort its training entry point builds: make_cohort kwargs, default patients / folds / batch)
MODELS = {
    "final": ("MultiModalSurvivalNet", lambda c: dict(rna_dim=c["rnaseq"].shape[1]), dict(seed=608, complete=True), 109, 5, 4),
    "partial": ("PartialModalityNet", lambda c: dict(rna_dim=c["rnaseq"].shape[1]), dict(seed=608, complete=False), 608, 3, 8),
    "simple": ("SimpleFusionModel", lambda c: dict(rna_dim=c["rnaseq"].shape[1]), dict(seed=88, complete=True), 88, 3, 8),
    "flexible": ("FlexibleMultimodalModel", lambda c: dict(rna_dim=c["rnaseq"].shape[1]), dict(seed=608, complete=False), 608, 3, 16),
    "simmim": ("SimMLM_SurvivalNet", lambda c: dict(rna_dim=c["rnaseq"].shape[1]), dict(seed=608, complete=False), 608, 3, 8),
    "image_only": ("ImageOnlyModel", lambda c: dict(), dict(seed=608, complete=False), 608, 5, 4),
    "rnaseq": ("RNASeqSurvivalModel", lambda c: dict(input_dim=c["rnaseq"].shape[1]), dict(seed=427, complete=True, dims=(32, 32, 32)), 240, 3, 16),
}


def _cohort_of(kind, device, external=False):
    """-> (cohort, keep): the cohort --model's training entry point builds and the boolean mask of the patients it trains on.
    external: every model class reads data/processed/* under MMS_DATA_ROOT when present (--ensemble: external validation)."""
    import torch  # noqa: F401
    from _common import env_dims, env_int, load_or_make_cohort
    from multimodal_survival_prediction_amd import data
    _, _, ckw, n_default, _, _ = MODELS[kind]
    n = env_int("MMS_PATIENTS", n_default)
    if kind == "image_only":          # image_only_training.py builds its cohort at MMS_VOLUME
        cohort = load_or_make_cohort(device, n=n, dims=env_dims(), **ckw)
    elif kind in ("partial", "simmim") or external:
        cohort = load_or_make_cohort(device, n=n, **ckw)                 # data/processed/* under MMS_DATA_ROOT when present
    else:
        cohort = data.cohort_to(data.make_cohort(n=n, **ckw), device)
    keep = cohort["has_survival"].cpu().bool()
    if kind == "simmim":              # simmlm_training.py's cohort: labelled patients with at least one modality
        keep &= (cohort["mask"].cpu() != 0).any(1)
    if kind == "image_only":          # image_only_training.py's cohort: patients with an image and a label
        keep &= cohort["mask"].cpu()[:, 0] != 0
    return cohort, keep


def save_saliency(attribute_dir, stem, vol, cohort, i, fmt="npy"):
    """One saliency volume (tD, tH, tW) of patient i -> <stem>.npy on the network grid, or (fmt "nii") <stem>.nii.gz: float32 NIfTI whose
    affine is the scan's (cohort["geometry"], kept by load_cohort for NIfTI volumes) times the per-axis scale of the loader's
    align-corners resample (nifti.saliency_affine), so a viewer overlays the map on the scan; identity without geometry."""
    if fmt == "npy":
        np.save(os.path.join(attribute_dir, stem + ".npy"), vol)
        return
    from multimodal_survival_prediction_amd import nifti
    geometry = cohort.get("geometry")
    geo = geometry[i] if geometry is not None else None
    A = nifti.saliency_affine(geo[0], geo[1], vol.shape) if geo is not None else np.eye(4)
    nifti.write_nifti(os.path.join(attribute_dir, stem + ".nii.gz"), np.ascontiguousarray(vol, dtype=np.float32), affine=A)


def predict(checkpoint, kind, fold, n_folds, batch_size, out_csv, attribute_dir=None, top=50, genes=None, train_csv=None, cov_csv=None,
            attribute_format="npy"):
    """Eval-mode log-hazards of the fold's validation patients -> results/test_predictions.csv.  The cohort and the fold split
    are rebuilt exactly as the model's training entry point builds them (scripts/training/<name>.py: same seeds, K-fold over the
    labelled patients with random_state 42), so fold k here is the held-out split of models/<name>/fold_k_best.pth.
    train_csv: also score the fold's TRAINING patients into that file, same columns (the fit set of --horizons' Breslow baseline).
    cov_csv: also write the predicted patients' covariates there (patient_id, age = clinical * 100, empty without a clinical record)."""
    import torch
    from _common import env_dims, env_int, load_or_make_cohort, setup_device
    from multimodal_survival_prediction_amd import data, models
    from multimodal_survival_prediction_amd.engine import engine_of
    _, _, device = setup_device()
    cls, ctor, ckw, n_default, folds_default, batch_default = MODELS[kind]
    n_folds, batch_size = n_folds or env_int("MMS_FOLDS", folds_default), batch_size or env_int("MMS_BATCH_SIZE", batch_default)
    cohort, keep = _cohort_of(kind, device)
    labelled = torch.nonzero(keep).reshape(-1).numpy()
    trn, val = data.kfold_indices(len(labelled), n_folds, seed=42)[fold - 1]
    idx = labelled[val]
    gene_cols = None
    if genes:                                          # per-fold gene selection: the fold's columns, read before the forward pass
        from multimodal_survival_prediction_amd.gene_select import GeneSelection
        if kind == "image_only":
            raise SystemExit("--genes: ImageOnlyModel reads no RNA-seq")
        sel = GeneSelection.load(genes)
        gene_cols = np.asarray(sel.columns[0] if len(sel.columns) == 1 else sel.columns_of(fold - 1), dtype=np.int64)
        if sel.n_genes != cohort["rnaseq"].shape[1]:
            raise SystemExit(f"--genes: {genes} selects among {sel.n_genes} genes, the cohort has {cohort['rnaseq'].shape[1]}")
        cohort = dict(cohort, rnaseq=cohort["rnaseq"][:, torch.as_tensor(gene_cols, device=cohort["rnaseq"].device)].contiguous())
    model = getattr(models, cls)(**ctor(cohort))
    model.load_state_dict(torch.load(checkpoint, map_location="cpu"))
    model.to(device).eval()
    eng = engine_of(model)
    risks = []
    ids = cohort.get("patient_id")
    pid = lambda i: ids[i] if ids is not None else f"SYN-{i:04d}"
    gene_sum, gene_rows = None, 0
    if attribute_dir:
        from multimodal_survival_prediction_amd import attribution
        os.makedirs(attribute_dir, exist_ok=True)
    def forward(ct, rna, clin, mask):
        if kind == "final":
            return eng.forward_eval(ct, rna, clin)[0]
        if kind in ("partial", "simmim"):
            return eng.forward_eval(ct, rna, clin, mask=mask)[0]
        if kind == "simple":
            return eng.forward_eval(ct, rna)[0]
        if kind == "flexible":
            return eng.forward_eval(ct, rna, mask=mask[:, :2])[0]
        if kind == "image_only":
            return eng.forward_eval(ct)[0]
        return eng.forward_eval(None, rna)[0]

    for s in range(0, len(idx), batch_size):
        j = torch.as_tensor(idx[s:s + batch_size], device=device)
        ct, rna, clin, mask = cohort["image"][j], cohort["rnaseq"][j], cohort["clinical"][j], cohort["mask"][j]
        hz = forward(ct, rna, clin, mask)
        risks.append(hz.clone().cpu())
        if attribute_dir:
            has = (mask != 0).cpu().numpy() if mask is not None else np.ones((len(j), 3), bool)
            res = attribution.attribute(model, dict(ct=ct, rna=rna, clinical=clin, mask=mask if kind in ("partial", "flexible") else None))
            if res["ct"] is not None:
                vols = res["ct"][:, 0].cpu().numpy()
                for r, i in enumerate(idx[s:s + batch_size]):
                    if has[r, 0]:
                        save_saliency(attribute_dir, f"{pid(i)}_ct", vols[r], cohort, int(i), attribute_format)
            if res["rna"] is not None and has[:, 1].any():
                g = res["rna"].abs().double().cpu().numpy()[has[:, 1]]
                gene_sum = g.sum(0) if gene_sum is None else gene_sum + g.sum(0)
                gene_rows += len(g)
    if attribute_dir and gene_sum is not None:
        n_all = len(gene_sum) if gene_cols is None else sel.n_genes
        names = cohort.get("gene_names") or [f"g{i}" for i in range(n_all)]
        if gene_cols is not None:                      # the selected columns under their original names
            names = [names[int(c)] for c in gene_cols]
        score = gene_sum / gene_rows
        order = np.argsort(-score, kind="stable")[:top]
        pd.DataFrame({"gene": [names[i] for i in order], "mean_abs_grad": score[order]}).to_csv(
            os.path.join(attribute_dir, "gene_scores.csv"), index=False)
        print(f"wrote {attribute_dir}: saliency volumes and gene_scores.csv ({len(order)} genes over {gene_rows} patients)")
    train_risks = []
    if train_csv:                                      # the fold's training patients, scored by the same forward (after the validation split)
        tidx = labelled[trn]
        for s in range(0, len(tidx), batch_size):
            j = torch.as_tensor(tidx[s:s + batch_size], device=device)
            train_risks.append(forward(cohort["image"][j], cohort["rnaseq"][j], cohort["clinical"][j], cohort["mask"][j]).clone().cpu())
    eng.check_b4()                                     # a timed-out block-4 hand-off must not end up in the predictions file
    lab = cohort["label"].cpu().numpy()[idx]
    df = pd.DataFrame({"patient_id": [pid(i) for i in idx],
                       "survival_time": lab[:, 0], "event": lab[:, 1].astype(int), "risk_score": torch.cat(risks).numpy()})
    os.makedirs(os.path.dirname(out_csv) or ".", exist_ok=True)
    df.to_csv(out_csv, index=False)
    print(f"wrote {out_csv}: {len(df)} patients of fold {fold}/{n_folds} ({cls})")
    if cov_csv:
        age = cohort["clinical"].cpu().numpy()[idx, 0].astype(np.float64) * 100.0
        os.makedirs(os.path.dirname(cov_csv) or ".", exist_ok=True)
        pd.DataFrame({"patient_id": [pid(i) for i in idx],
                      "age": np.where(cohort["mask"].cpu().numpy()[idx, 2] != 0, age, np.nan)}).to_csv(cov_csv, index=False)
        print(f"wrote {cov_csv}: age of {len(idx)} patients")
    if train_csv:
        lab = cohort["label"].cpu().numpy()[tidx]
        os.makedirs(os.path.dirname(train_csv) or ".", exist_ok=True)
        pd.DataFrame({"patient_id": [pid(i) for i in tidx], "survival_time": lab[:, 0], "event": lab[:, 1].astype(int),
                      "risk_score": torch.cat(train_risks).numpy()}).to_csv(train_csv, index=False)
        print(f"wrote {train_csv}: {len(tidx)} training patients of fold {fold}/{n_folds}")
    return df


def predict_ensemble(checkpoints, kind, combine, batch_size, out_csv, attribute_dir=None, top=50, attribute_format="npy"):
    """The K fold checkpoints as one predictor (multimodal_survival_prediction_amd.ensemble.FoldEnsemble) over EVERY labelled patient of
    the loaded cohort -> results/test_predictions.csv with predict's columns (risk_score = the combined score) plus risk_std and
    risk_fold_1..K.  On the cohort the folds were trained on the score is optimistic: each patient was seen by K - 1 members."""
    import torch
    from _common import env_int, setup_device
    from multimodal_survival_prediction_amd import attribution, models
    from multimodal_survival_prediction_amd.ensemble import FoldEnsemble
    _, _, device = setup_device()
    cls, ctor, _, _, _, batch_default = MODELS[kind]
    batch_size = batch_size or env_int("MMS_BATCH_SIZE", batch_default)
    cohort, keep = _cohort_of(kind, device, external=True)
    idx = torch.nonzero(keep).reshape(-1).numpy()
    ens = FoldEnsemble.from_checkpoints(checkpoints, lambda: getattr(models, cls)(**ctor(cohort)), device)
    K = len(ens)
    res = ens.predict_cohort(cohort, idx, batch_size=batch_size, combine=combine)
    ids = cohort.get("patient_id")
    pid = lambda i: ids[i] if ids is not None else f"SYN-{i:04d}"
    if attribute_dir:
        os.makedirs(attribute_dir, exist_ok=True)
        gene_sum, gene_rows = None, 0
        for s in range(0, len(idx), batch_size):
            j = torch.as_tensor(idx[s:s + batch_size], device=device)
            mask = cohort["mask"][j]
            has = (mask != 0).cpu().numpy()
            att = ens.attribute(dict(ct=cohort["image"][j], rna=cohort["rnaseq"][j], clinical=cohort["clinical"][j], mask=mask))
            if att["ct"] is not None:
                vols, stds = att["ct"][:, 0].cpu().numpy(), att["ct_std"][:, 0].cpu().numpy()
                for r, i in enumerate(idx[s:s + batch_size]):
                    if has[r, 0]:
                        save_saliency(attribute_dir, f"{pid(i)}_ct", vols[r], cohort, int(i), attribute_format)
                        save_saliency(attribute_dir, f"{pid(i)}_ct_std", stds[r], cohort, int(i), attribute_format)
            if att["rna"] is not None and has[:, 1].any():
                g = att["rna"].abs().double().cpu().numpy()[has[:, 1]]
                gene_sum = g.sum(0) if gene_sum is None else gene_sum + g.sum(0)
                gene_rows += len(g)
        if gene_sum is not None:
            names = cohort.get("gene_names") or [f"g{i}" for i in range(len(gene_sum))]
            score = gene_sum / gene_rows
            order = np.argsort(-score, kind="stable")[:top]
            pd.DataFrame({"gene": [names[i] for i in order], "mean_abs_grad": score[order]}).to_csv(
                os.path.join(attribute_dir, "gene_scores.csv"), index=False)
        print(f"wrote {attribute_dir}: mean and spread saliency volumes of {K} members, gene_scores.csv")
    lab = cohort["label"].cpu().numpy()[idx]
    cols = {"patient_id": [pid(i) for i in idx], "survival_time": lab[:, 0], "event": lab[:, 1].astype(int),
            "risk_score": res["hazard"].cpu().numpy(), "risk_std": res["hazard_std"].cpu().numpy()}
    hz = res["hazards"].cpu().numpy()
    for g in range(K):
        cols[f"risk_fold_{g + 1}"] = hz[g]
    df = pd.DataFrame(cols)
    os.makedirs(os.path.dirname(out_csv) or ".", exist_ok=True)
    df.to_csv(out_csv, index=False)
    print(f"wrote {out_csv}: {len(df)} labelled patients scored by {K} fold models ({cls}, combine={combine})")
    return df


def bootstrap_summary(df, replicates, seed=0, compare=(), alpha=0.05):
    """-> the "c_index_bootstrap" entry: one paired bootstrap over risk_score, the risk_fold_* members and the --compare files' risk_score."""
    from multimodal_survival_prediction_amd.bootstrap import cindex_bootstrap
    members = sorted((c for c in df.columns if c.startswith("risk_fold_")), key=lambda c: int(c.rsplit("_", 1)[1]))
    rows, others = [df["risk_score"].to_numpy(float)] + [df[c].to_numpy(float) for c in members], []
    for path in compare:
        if "patient_id" not in df.columns:
            raise ValueError("--compare joins on patient_id, which the predictions file does not have")
        o = pd.read_csv(path)
        if o["patient_id"].duplicated().any() or df["patient_id"].duplicated().any() or set(o["patient_id"]) != set(df["patient_id"]):
            raise ValueError(f"{path}: the patient sets differ (a paired comparison scores every model on the same patients)")
        others.append(path)
        rows.append(o.set_index("patient_id").loc[df["patient_id"], "risk_score"].to_numpy(float))
    res = cindex_bootstrap(np.stack(rows), df["survival_time"].to_numpy(float), df["event"].to_numpy(int), R=replicates, seed=seed,
                           strata=df["fold"].to_numpy() if "fold" in df.columns else None, pair_rule="lifelines", alpha=alpha)
    paired = lambda a, b: {"delta": float(res.delta[a, b]), "low": float(res.delta_ci_low[a, b]), "high": float(res.delta_ci_high[a, b]),
                           "p_value": float(res.p_value[a, b])}
    out = {"replicates": int(replicates), "seed": int(seed), "alpha": float(alpha), "low": float(res.ci_low[0]), "high": float(res.ci_high[0]),
           "se": float(res.se[0]), "n_degenerate": int(res.n_degenerate)}
    if members:
        out["members"] = {c: dict(c_index=float(res.c[1 + k]), **paired(0, 1 + k)) for k, c in enumerate(members)}
    if others:
        out["compare"] = {path: dict(c_index=float(res.c[1 + len(members) + k]), **paired(0, 1 + len(members) + k)) for k, path in enumerate(others)}
    return out


def stratification_summary(df, replicates, seed=0, min_prop=0.1, outdir="results", alpha=0.05):
    """-> (the "risk_stratification" entry, the median split's Kaplan-Meier curves with bands); writes <outdir>/cutpoint_scan.csv, the
    log-rank statistic of every admissible cut of risk_score (multimodal_survival_prediction_amd/risk_strata.py, on the GPU)."""
    from multimodal_survival_prediction_amd import risk_strata as RS
    t, e, r = df["survival_time"].to_numpy(float), df["event"].to_numpy(int), df["risk_score"].to_numpy(float)
    res = RS.stratify(r, t, e, R=replicates, seed=seed, min_prop=min_prop, alpha=alpha)
    m = res.models[0]
    pd.DataFrame({"threshold": m.threshold, "n_high": m.n_high, "d_high": m.d_high, "U": m.U, "V": m.V, "chi2": m.chi2,
                  "p_unadjusted": m.p_unadjusted, "median_split": np.arange(len(m.threshold)) == m.median_index,
                  "best": np.arange(len(m.threshold)) == m.best_index}).to_csv(os.path.join(outdir, "cutpoint_scan.csv"), index=False)
    curves = RS.km_groups(t, e, m.high(r, "median"), alpha)
    out = dict(replicates=res.replicates, seed=int(seed), min_prop=float(min_prop), alpha=float(alpha), **m.summary())
    out["km"] = {c.group: {"median": c.median, "median_low": c.median_low, "median_high": c.median_high} for c in curves}
    return out, curves


def parse_horizons(arg, time, event):
    """--horizons: a count H (absolute_risk.default_horizons of this file's patients) or the horizons themselves, comma-separated"""
    from multimodal_survival_prediction_amd import absolute_risk as AR
    if str(arg).strip().isdigit():
        return AR.default_horizons(time, event, int(arg))
    return AR.check_horizons([float(x) for x in str(arg).split(",")])


def curve_columns(horizons):
    """one S_<tau> column name per horizon; repr keeps every digit, so --compare-curves reads the horizons back exactly"""
    return [f"S_{float(x)!r}" for x in horizons]


def prediction_error_summary(df, horizons, baseline, replicates=0, seed=0, compare_curves=(), outdir="results", alpha=0.05):
    """-> (the "prediction_error" entry, what the figures need).  baseline: the fit-set predictions (survival_time, event, risk_score)
    of the Breslow baseline.  Writes <outdir>/survival_curves.csv (S(tau | risk_score) per patient), prediction_error.csv (per horizon
    Brier score, Kaplan-Meier null model, IPA and cumulative/dynamic AUC; with replicates > 0 their bootstrap intervals, on the GPU:
    multimodal_survival_prediction_amd/absolute_risk.py) and calibration.csv (at the middle horizon)."""
    from multimodal_survival_prediction_amd import absolute_risk as AR
    t, e, r = df["survival_time"].to_numpy(float), df["event"].to_numpy(int), df["risk_score"].to_numpy(float)
    if any(c.startswith("risk_fold_") for c in df.columns):
        print("--horizons: the file has risk_fold_* member columns; risk_score alone is evaluated")
    tau = parse_horizons(horizons, t, e)
    base = AR.breslow_baseline(baseline["risk_score"].to_numpy(float), baseline["survival_time"].to_numpy(float), baseline["event"].to_numpy(int))
    surv, cols = base.survival(r, tau), curve_columns(tau)
    keep = [c for c in ("patient_id", "survival_time", "event", "risk_score") if c in df.columns]
    curves = pd.concat([df[keep].reset_index(drop=True), pd.DataFrame(surv, columns=cols)], axis=1)
    curves.to_csv(os.path.join(outdir, "survival_curves.csv"), index=False)
    survs, risks, others = [surv], [r], []
    for path in compare_curves:
        o = pd.read_csv(path)
        if "patient_id" not in df.columns or "patient_id" not in o.columns:
            raise ValueError(f"{path}: --compare-curves joins on patient_id")
        if o["patient_id"].duplicated().any() or df["patient_id"].duplicated().any() or set(o["patient_id"]) != set(df["patient_id"]):
            raise ValueError(f"{path}: the patient sets differ (a paired comparison scores every model on the same patients)")
        if [c for c in o.columns if c.startswith("S_")] != cols:
            raise ValueError(f"{path}: its horizons {[c[2:] for c in o.columns if c.startswith('S_')]} are not this run's {[c[2:] for c in cols]}")
        o = o.set_index("patient_id").loc[df["patient_id"]]
        if not (np.array_equal(o["survival_time"].to_numpy(float), t) and np.array_equal(o["event"].to_numpy(int), e)):
            raise ValueError(f"{path}: survival_time / event differ from this run's for the same patient ids")
        others.append(path); survs.append(o[cols].to_numpy(float)); risks.append(o["risk_score"].to_numpy(float))
    res = AR.prediction_error(np.stack(survs), np.stack(risks), t, e, tau, R=replicates, seed=seed,
                              strata=df["fold"].to_numpy() if "fold" in df.columns else None, alpha=alpha)
    table = {"horizon": tau}
    for name, est in (("brier", res.brier), ("brier_null", res.brier_null), ("ipa", res.ipa), ("auc", res.auc)):
        table[name] = est.value if est.value.ndim == 1 else est.value[0]
    if replicates:
        for name, est in (("brier", res.brier), ("brier_null", res.brier_null), ("ipa", res.ipa), ("auc", res.auc)):
            table[name + "_low"], table[name + "_high"] = (est.low, est.high) if est.low.ndim == 1 else (est.low[0], est.high[0])
    table = pd.DataFrame(table)
    table.to_csv(os.path.join(outdir, "prediction_error.csv"), index=False)
    k = (len(tau) - 1) // 2
    calib = pd.DataFrame(AR.calibration_table(surv[:, k], t, e, tau[k], groups=min(5, len(t)), alpha=alpha))
    calib.insert(0, "horizon", tau[k])
    calib.to_csv(os.path.join(outdir, "calibration.csv"), index=False)
    out = {"horizons": [float(x) for x in tau], "replicates": int(replicates), "seed": int(seed), "alpha": float(alpha),
           "baseline_patients": int(len(baseline)), "ibs": float(res.ibs.value[0]), "iauc": float(res.iauc.value[0]),
           "brier": [float(x) for x in res.brier.value[0]], "brier_null": [float(x) for x in res.brier_null.value],
           "ipa": [float(x) for x in res.ipa.value[0]], "auc": [float(x) for x in res.auc.value[0]], "calibration_horizon": float(tau[k])}
    if replicates:
        out.update(n_degenerate=int(res.n_degenerate), ibs_low=float(res.ibs.low[0]), ibs_high=float(res.ibs.high[0]), ibs_se=float(res.ibs.se[0]),
                   iauc_low=float(res.iauc.low[0]), iauc_high=float(res.iauc.high[0]), iauc_se=float(res.iauc.se[0]))
    if others:
        def paired(d, m):
            p = {"delta": float(d.delta[0, m])}
            if replicates:
                p.update(low=float(d.low[0, m]), high=float(d.high[0, m]), p_value=float(d.p_value[0, m]))
            return p
        out["compare"] = {path: {"ibs": float(res.ibs.value[1 + m]), "iauc": float(res.iauc.value[1 + m]), "ibs_difference": paired(res.ibs_diff, 1 + m),
                                 "iauc_difference": paired(res.iauc_diff, 1 + m)} for m, path in enumerate(others)}
    return out, (table, calib)


def multivariable_summary(df, adjust, adjust_columns=None, compare=(), replicates=0, seed=0, outdir="results", alpha=0.05):
    """-> the "multivariable" entry; writes <outdir>/multivariable.csv (one row per model and coefficient).  adjust: the covariates file
    (or its DataFrame): patient_id plus numeric columns = the base model (adjust_columns: those alone); risk_score and every compare
    file's risk_score (under the file's stem) are the added covariates (multimodal_survival_prediction_amd/multivariable.py, on the GPU)."""
    from multimodal_survival_prediction_amd import multivariable as MV
    cov = pd.read_csv(adjust) if isinstance(adjust, (str, os.PathLike)) else adjust
    if "patient_id" not in df.columns or "patient_id" not in cov.columns:
        raise ValueError("--adjust joins on patient_id, which both files must have")
    if cov["patient_id"].duplicated().any() or df["patient_id"].duplicated().any() or not set(df["patient_id"]) <= set(cov["patient_id"]):
        raise ValueError("--adjust: the covariates must list every predicted patient once")
    cov = cov.set_index("patient_id").loc[df["patient_id"]]
    base = list(adjust_columns) if adjust_columns else [c for c in cov.columns if pd.api.types.is_numeric_dtype(cov[c])]
    missing = [c for c in base if c not in cov.columns or not pd.api.types.is_numeric_dtype(cov[c])]
    if missing or not base:
        raise ValueError(f"--adjust: no numeric column(s) {missing or ''} in the covariates file")
    columns = {c: cov[c].to_numpy(float) for c in base}
    columns["risk_score"] = df["risk_score"].to_numpy(float)
    for path in compare:
        o = pd.read_csv(path)
        if o["patient_id"].duplicated().any() or set(o["patient_id"]) != set(df["patient_id"]):
            raise ValueError(f"{path}: the patient sets differ (a paired comparison scores every model on the same patients)")
        stem = os.path.splitext(os.path.basename(path))[0]
        if stem in columns:
            raise ValueError(f"{path}: the name {stem!r} is taken (a covariate is named after its file's stem)")
        columns[stem] = o.set_index("patient_id").loc[df["patient_id"], "risk_score"].to_numpy(float)
    add = [c for c in columns if c not in base]
    res = MV.analyse(columns, df["survival_time"].to_numpy(float), df["event"].to_numpy(int), base, add, R=replicates, seed=seed,
                     strata=df["fold"].to_numpy() if "fold" in df.columns else None, alpha=alpha)
    rows = []
    for m in res["models"]:
        for name, c in m["coefficients"].items():
            rows.append(dict(model=m["model"], covariate=name, **c, loglik=m["loglik"], aic=m["aic"], c_index=m["c_index"], status=m["status"]))
    pd.DataFrame(rows).to_csv(os.path.join(outdir, "multivariable.csv"), index=False)
    return res


def evaluate(df, outdir="results", plots=True, bootstrap=0, seed=0, compare=(), stratify=0, min_prop=0.1, horizons=None, baseline=None,
             compare_curves=(), adjust=None, adjust_columns=None):
    """-> the evaluation_summary.json dictionary (reference keys + log-rank + per-group statistics; bootstrap > 0: + c_index_bootstrap;
    stratify > 0: + risk_stratification and cutpoint_scan.csv; horizons: + prediction_error, survival_curves.csv, prediction_error.csv
    and calibration.csv, with `baseline` the fit-set predictions of the Breslow baseline; adjust: + multivariable and multivariable.csv,
    with `adjust` the covariates file)."""
    t, e, r = df["survival_time"].to_numpy(float), df["event"].to_numpy(int), df["risk_score"].to_numpy(float)
    c_index = SS.concordance_index(t, -r, e)
    group = SS.risk_groups(r)
    lo, hi = group == "Low Risk", group == "High Risk"
    chi2, p = SS.logrank_test(t[hi], t[lo], e[hi], e[lo]) if hi.any() and lo.any() else (0.0, 1.0)
    summary = {
        "test_patients": int(len(df)), "deaths": int(e.sum()), "censored": int((1 - e).sum()), "c_index": float(c_index),
        "median_survival_time": float(np.median(t)), "median_risk_score": float(np.median(r)),
        "risk_groups": {"low_risk": int(lo.sum()), "high_risk": int(hi.sum())},
        "logrank": {"chi2": chi2, "p_value": p},
        "group_statistics": {},
    }
    os.makedirs(outdir, exist_ok=True)
    km_rows = []
    for name, m in (("Low Risk", lo), ("High Risk", hi)):
        if not m.any():
            continue
        summary["group_statistics"][name] = {
            "patients": int(m.sum()), "deaths": int(e[m].sum()), "censored": int((1 - e[m]).sum()),
            "mean_survival_time": float(t[m].mean()), "median_survival_time": float(np.median(t[m])),
            "km_median_survival_time": SS.median_survival(t[m], e[m]), "mean_risk_score": float(r[m].mean())}
        times, surv, at_risk, deaths = SS.kaplan_meier(t[m], e[m])
        km_rows += [dict(group=name, time=a, survival=b, at_risk=int(c), events=int(d)) for a, b, c, d in zip(times, surv, at_risk, deaths)]
    pd.DataFrame(km_rows).to_csv(os.path.join(outdir, "kaplan_meier_table.csv"), index=False)
    if bootstrap:
        summary["c_index_bootstrap"] = bootstrap_summary(df, bootstrap, seed, compare)
    bands = None
    if stratify:
        summary["risk_stratification"], bands = stratification_summary(df, stratify, seed, min_prop, outdir)
    tables = None
    if horizons:
        summary["prediction_error"], tables = prediction_error_summary(df, horizons, baseline, bootstrap, seed, compare_curves, outdir)
    if adjust is not None:
        summary["multivariable"] = multivariable_summary(df, adjust, adjust_columns, compare, bootstrap, seed, outdir)
    with open(os.path.join(outdir, "evaluation_summary.json"), "w") as f:
        json.dump(summary, f, indent=2)
    if plots:
        _plots(df.assign(risk_group=group), km_rows, summary, outdir, bands)
        if tables:
            _absolute_risk_plots(*tables, outdir)
    return summary


def _absolute_risk_plots(table, calib, outdir):
    """--horizons: Brier score / AUC against time (with the bootstrap intervals when present) and the calibration plot"""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return
    fig, (a0, a1) = plt.subplots(1, 2, figsize=(11, 4.5))
    for ax, names, title in ((a0, (("brier", "Model", "tab:red"), ("brier_null", "Kaplan-Meier null model", "tab:gray")), "IPCW Brier score"),
                             (a1, (("auc", "Model", "tab:blue"),), "Cumulative/dynamic AUC")):
        for col, label, colour in names:
            ax.plot(table["horizon"], table[col], marker="o", label=label, color=colour)
            if col + "_low" in table.columns:
                ax.fill_between(table["horizon"], table[col + "_low"], table[col + "_high"], alpha=0.15, color=colour, linewidth=0)
        ax.set_xlabel("Time (days)"); ax.set_title(title); ax.legend(loc="best"); ax.grid(True, alpha=0.3)
    a1.axhline(0.5, color="black", linestyle="--", linewidth=0.8)
    fig.tight_layout(); fig.savefig(os.path.join(outdir, "prediction_error.png"), dpi=150); plt.close(fig)
    fig, ax = plt.subplots(figsize=(5.5, 5))
    ax.errorbar(calib["predicted"], calib["observed"], yerr=[calib["observed"] - calib["low"], calib["high"] - calib["observed"]], marker="o", capsize=3)
    ax.plot([0, 1], [0, 1], color="black", linestyle="--", linewidth=0.8)
    ax.set_xlabel("Predicted event probability"); ax.set_ylabel("Observed (1 - Kaplan-Meier)")
    ax.set_title(f"Calibration at {calib['horizon'].iloc[0]:g} days"); ax.grid(True, alpha=0.3)
    fig.tight_layout(); fig.savefig(os.path.join(outdir, "calibration.png"), dpi=150); plt.close(fig)


def _plots(df, km_rows, summary, outdir, bands=None):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        print("matplotlib not available: figures skipped")
        return
    km = pd.DataFrame(km_rows)
    fig, ax = plt.subplots(figsize=(7, 5))
    for name, colour in (("Low Risk", "tab:blue"), ("High Risk", "tab:red")):
        g = km[km["group"] == name]
        if len(g):
            ax.step(g["time"], g["survival"], where="post", label=name, color=colour)
    for c in bands or ():                              # --stratify: Greenwood (log-log) bands of the same two groups
        ax.fill_between(c.time, c.low, c.high, step="post", alpha=0.15, color="tab:red" if c.group == "High Risk" else "tab:blue", linewidth=0)
    ax.set_xlabel("Time (days)"); ax.set_ylabel("Survival Probability"); ax.set_ylim(0, 1.02)
    ax.set_title(f"Kaplan-Meier by risk group (log-rank p = {summary['logrank']['p_value']:.3g})")
    ax.legend(loc="best"); ax.grid(True, alpha=0.3)
    fig.tight_layout(); fig.savefig(os.path.join(outdir, "kaplan_meier_curves.png"), dpi=150); plt.close(fig)
    fig, ax = plt.subplots(figsize=(7, 5))
    for name, colour in (("Low Risk", "blue"), ("High Risk", "red")):
        ax.hist(df[df["risk_group"] == name]["risk_score"], bins=15, alpha=0.6, label=name, color=colour)
    ax.axvline(summary["median_risk_score"], color="black", linestyle="--", label="Median")
    ax.set_xlabel("Risk Score"); ax.set_ylabel("Frequency"); ax.set_title("Risk Score Distribution"); ax.legend(); ax.grid(True, alpha=0.3)
    fig.tight_layout(); fig.savefig(os.path.join(outdir, "risk_score_distribution.png"), dpi=150); plt.close(fig)
    fig, ax = plt.subplots(figsize=(8, 5))
    for val, colour, label in ((0, "blue", "Censored"), (1, "red", "Death")):
        m = df["event"] == val
        ax.scatter(df[m]["risk_score"], df[m]["survival_time"], c=colour, alpha=0.6, s=60, label=label, edgecolors="black", linewidths=0.5)
    ax.set_xlabel("Risk Score"); ax.set_ylabel("Survival Time (days)"); ax.set_title("Survival Time vs Risk Score"); ax.legend(); ax.grid(True, alpha=0.3)
    fig.tight_layout(); fig.savefig(os.path.join(outdir, "survival_vs_risk.png"), dpi=150); plt.close(fig)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--predictions", default="results/test_predictions.csv")
    ap.add_argument("--outdir", default="results")
    ap.add_argument("--predict", metavar="CHECKPOINT", help="state_dict written by a training entry point (models/<name>/fold_k_best.pth)")
    ap.add_argument("--model", choices=sorted(MODELS), default="final")
    ap.add_argument("--fold", type=int, default=1)
    ap.add_argument("--n-folds", type=int, default=0, help="default: the training script's N_FOLDS (MMS_FOLDS)")
    ap.add_argument("--batch-size", type=int, default=0, help="default: the training script's BATCH_SIZE (MMS_BATCH_SIZE)")
    ap.add_argument("--no-plots", action="store_true")
    ap.add_argument("--ensemble", metavar="CKPT", nargs="+",
                    help="the fold checkpoints of one model class as ONE predictor over every labelled patient of the loaded cohort (data/processed/* "
                         "under MMS_DATA_ROOT when present: external validation; else the seeded synthetic cohort); adds the columns risk_std and "
                         "risk_fold_1..K.  On the training cohort itself an ensemble's score is optimistic: each patient was seen in training by "
                         "K-1 of the K members")
    ap.add_argument("--combine", choices=("mean", "rank"), default="mean",
                    help="with --ensemble: risk_score = the members' mean log-hazard, or their mean midrank over the predicted patients / N")
    ap.add_argument("--attribute", action="store_true", help="with --predict: write <outdir>/attribution/<patient_id>_ct.npy and gene_scores.csv; "
                    "with --ensemble: the members' mean (<id>_ct.npy) and spread (<id>_ct_std.npy) and the mean gradient's gene_scores.csv")
    ap.add_argument("--attribute-format", choices=("npy", "nii"), default="npy",
                    help="with --attribute: npy = arrays on the network grid; nii = <patient_id>_ct.nii.gz (and _ct_std.nii.gz for ensembles) "
                         "carrying the scan's geometry, for a medical viewer to overlay on the scan")
    ap.add_argument("--genes", metavar="FILE", help="with --predict: the fold's selected gene columns (fold_k_genes.json written by a training entry "
                    "point under MMS_SELECT_GENES); the model is built at that width")
    ap.add_argument("--top", type=int, default=50, help="rows of gene_scores.csv")
    ap.add_argument("--bootstrap", type=int, default=0, metavar="R",
                    help="R bootstrap resamples of the patients (on the GPU): adds c_index_bootstrap {replicates, seed, alpha, low, high, se, "
                         "n_degenerate} to the summary, and for risk_fold_* columns each member's C-index and ensemble - member with CI and p-value")
    ap.add_argument("--seed", type=int, default=0, help="with --bootstrap / --stratify: seed of numpy.random.default_rng")
    ap.add_argument("--stratify", type=int, default=0, metavar="R",
                    help="scan every admissible cut of risk_score with R random relabellings (on the GPU): adds risk_stratification {median: chi2, "
                         "p_asymptotic, p_permutation, hazard_ratio; best: threshold, chi2, p_adjusted, hazard_ratio; km} to the summary, writes "
                         "cutpoint_scan.csv and draws Greenwood bands on the Kaplan-Meier figure")
    ap.add_argument("--min-prop", type=float, default=0.1, help="with --stratify: every cut leaves ceil(min_prop n) patients on each side")
    ap.add_argument("--compare", metavar="OTHER.csv", nargs="+", default=[],
                    help="with --bootstrap: other models' predictions of the SAME patients (joined on patient_id); adds the paired difference "
                         "of this file's risk_score against each, with CI and p-value")
    ap.add_argument("--horizons", metavar="H | t1,t2,...",
                    help="absolute-risk evaluation at H default horizons (equally spaced between the 10th and 90th percentile of the observed event "
                         "times) or at the given times: adds prediction_error {horizons, brier, brier_null, ipa, auc, ibs, iauc} to the summary and "
                         "writes survival_curves.csv, prediction_error.csv and calibration.csv; with --bootstrap R (on the GPU) their intervals")
    ap.add_argument("--baseline", metavar="TRAIN.csv",
                    help="with --horizons: the fit set of the Breslow baseline hazard -- the TRAINING patients scored by the same model, in the "
                         "columns of test_predictions.csv (default with --predict: <outdir>/train_predictions.csv, which --predict then writes)")
    ap.add_argument("--compare-curves", metavar="OTHER/survival_curves.csv", nargs="+", default=[],
                    help="with --horizons: other runs' survival_curves.csv on the SAME patient ids and horizons; adds the paired difference of "
                         "IBS and iAUC against each (with --bootstrap R: interval and p-value)")
    ap.add_argument("--adjust", metavar="COVARIATES.csv", nargs="?", const=True, default=None,
                    help="multivariable Cox analysis (on the GPU): patient_id plus numeric columns = the base model, to which risk_score and every "
                         "--compare file's risk_score are added; adds multivariable {models, lr_tests, n_degenerate, status_counts} to the summary and "
                         "writes multivariable.csv; with --bootstrap R percentile intervals.  Bare, with --predict: <outdir>/covariates.csv (age), "
                         "which --predict then writes")
    ap.add_argument("--adjust-columns", metavar="a,b", help="with --adjust: the columns of the base model (default: every numeric column)")
    a = ap.parse_args(argv)
    if a.adjust is True and not a.predict:
        ap.error("--adjust needs a covariates file (bare --adjust belongs to --predict, which writes <outdir>/covariates.csv)")
    if a.adjust_columns and a.adjust is None:
        ap.error("--adjust-columns belongs to --adjust")
    if (a.baseline or a.compare_curves) and not a.horizons:
        ap.error("--baseline and --compare-curves belong to --horizons")
    if a.horizons and not (a.baseline or a.predict):
        ap.error("--horizons needs the fit set of the baseline hazard: --baseline TRAIN.csv (or --predict, which scores the fold's training patients)")
    if a.compare and not (a.bootstrap or a.adjust is not None):
        ap.error("--compare needs --bootstrap R (the comparison is a paired bootstrap) or --adjust")
    if a.bootstrap < 0:
        ap.error("--bootstrap needs a positive number of replicates")
    if a.stratify < 0 or not 0.0 <= a.min_prop <= 0.5:
        ap.error("--stratify needs a positive number of relabellings and --min-prop a share in [0, 0.5]")
    if a.attribute and not (a.predict or a.ensemble):
        ap.error("--attribute needs --predict CHECKPOINT (the gradients are taken on the checkpoint's model)")
    if a.predict and a.ensemble:
        ap.error("--predict scores one fold's validation split, --ensemble every labelled patient: give one of them")
    if a.genes and a.ensemble:
        ap.error("--genes with --ensemble: ensembles of selected-gene models are not supported (every fold's model reads its own columns; "
                 "score each fold with --predict --genes)")
    if a.genes and not a.predict:
        ap.error("--genes needs --predict CHECKPOINT")
    adir = os.path.join(a.outdir, "attribution") if a.attribute else None
    if a.ensemble:
        df = predict_ensemble(a.ensemble, a.model, a.combine, a.batch_size, a.predictions, adir, a.top, a.attribute_format)
    elif a.predict:
        train_csv = os.path.join(a.outdir, "train_predictions.csv") if a.horizons and not a.baseline else None
        cov_csv = os.path.join(a.outdir, "covariates.csv") if a.adjust is True else None
        df = predict(a.predict, a.model, a.fold, a.n_folds, a.batch_size, a.predictions, adir, a.top, a.genes, train_csv, cov_csv,
                     a.attribute_format)
        a.baseline = a.baseline or train_csv
        a.adjust = cov_csv or a.adjust
    else:
        df = pd.read_csv(a.predictions)
    s = evaluate(df, a.outdir, plots=not a.no_plots, bootstrap=a.bootstrap, seed=a.seed, compare=a.compare, stratify=a.stratify,
                 min_prop=a.min_prop, horizons=a.horizons, baseline=pd.read_csv(a.baseline) if a.horizons else None,
                 compare_curves=a.compare_curves, adjust=a.adjust, adjust_columns=a.adjust_columns.split(",") if a.adjust_columns else None)
    print(f"patients {s['test_patients']} (deaths {s['deaths']}, censored {s['censored']}); C-index {s['c_index']:.4f}; "
          f"median risk {s['median_risk_score']:.4f}; low/high {s['risk_groups']['low_risk']}/{s['risk_groups']['high_risk']}; "
          f"log-rank chi2 {s['logrank']['chi2']:.3f} p {s['logrank']['p_value']:.3g}")
    if a.bootstrap:
        b = s["c_index_bootstrap"]
        print(f"C-index {s['c_index']:.4f}, {100 * (1 - b['alpha']):.0f} % CI {b['low']:.4f}-{b['high']:.4f} (SE {b['se']:.4f}; {b['replicates']} resamples, "
              f"seed {b['seed']}, {b['n_degenerate']} degenerate)")
        for name, m in list(b.get("members", {}).items()) + list(b.get("compare", {}).items()):
            print(f"  vs {name}: C {m['c_index']:.4f}, difference {m['delta']:+.4f} (CI {m['low']:+.4f}..{m['high']:+.4f}, p = {m['p_value']:.3g})")
    if a.stratify:
        rs = s["risk_stratification"]
        print(f"median split: chi2 {rs['median']['chi2']:.3f}, p {rs['median']['p_asymptotic']:.3g} asymptotic / {rs['median']['p_permutation']:.3g} "
              f"permutation, HR {rs['median']['hazard_ratio']:.2f} ({rs['median']['low']:.2f}-{rs['median']['high']:.2f}); best of {rs['n_cuts']} cuts: "
              f"risk > {rs['best']['threshold']:.4f}, chi2 {rs['best']['chi2']:.3f}, adjusted p {rs['best']['p_adjusted']:.3g} "
              f"({rs['replicates']} relabellings, seed {rs['seed']}); saved cutpoint_scan.csv")
    if a.horizons:
        pe = s["prediction_error"]
        ci = lambda k: f" ({100 * (1 - pe['alpha']):.0f} % CI {pe[k + '_low']:.4f}-{pe[k + '_high']:.4f})" if a.bootstrap else ""
        print(f"{len(pe['horizons'])} horizons {pe['horizons'][0]:g}..{pe['horizons'][-1]:g}, baseline on {pe['baseline_patients']} patients: "
              f"IBS {pe['ibs']:.4f}{ci('ibs')}, iAUC {pe['iauc']:.4f}{ci('iauc')}; saved survival_curves.csv, prediction_error.csv, calibration.csv")
        for name, m in pe.get("compare", {}).items():
            tail = lambda d: f" (CI {d['low']:+.4f}..{d['high']:+.4f}, p = {d['p_value']:.3g})" if a.bootstrap else ""
            print(f"  vs {name}: IBS {m['ibs']:.4f}, difference {m['ibs_difference']['delta']:+.4f}{tail(m['ibs_difference'])}; "
                  f"iAUC {m['iauc']:.4f}, difference {m['iauc_difference']['delta']:+.4f}{tail(m['iauc_difference'])}")
    if a.adjust is not None:
        mv = s["multivariable"]
        full = mv["models"][-1]
        print(f"multivariable Cox on {mv['patients']} complete cases ({mv['n_dropped']} dropped), model {' + '.join(full['columns'])}:")
        for name, c in full["coefficients"].items():
            boot = f", bootstrap {c['hr_boot_low']:.3f}-{c['hr_boot_high']:.3f}" if a.bootstrap else ""
            print(f"  {name}: HR {c['hr']:.3f} per SD (Wald {c['hr_low']:.3f}-{c['hr_high']:.3f}{boot}), p = {c['p']:.3g}")
        for name, lr in mv["lr_tests"].items():
            print(f"  likelihood-ratio test, base + {name} against base: chi2 {lr['chi2']:.3f} on {lr['df']} df, p = {lr['p']:.3g}")
        if a.bootstrap:
            print(f"  {mv['replicates']} resamples, seed {mv['seed']}, {mv['n_degenerate']} degenerate; saved multivariable.csv")
    print(f"saved {os.path.join(a.outdir, 'evaluation_summary.json')}, kaplan_meier_table.csv" + ("" if a.no_plots else ", figures"))
    return s


if __name__ == "__main__":
    main()
