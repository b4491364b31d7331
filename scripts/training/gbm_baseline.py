#!/usr/bin/env python3
"""Gradient-boosted Cox trees baseline on the genes, nested K-fold cross-validation -- the third classical point on the reference's
"simple is better for small datasets" / "RNA-only wins" axis (final_comparison.py:301-335), next to cox_baseline.py's linear one and
rsf_baseline.py's bagged one.

Same conventions as rsf_baseline.py: the seeded synthetic cohort (MMS_PATIENTS), MMS_FOLDS folds from kfold_indices(seed=42),
MMS_SELECT_GENES (per-fold gene selection; each fold's problems are then their own lock-step call on that fold's genes).  Every outer
fold has MMS_GBM_INNER (5) inner folds; MMS_GBM_ROUNDS (300) rounds of one tree each; MMS_GBM_LR (0.1) and MMS_GBM_DEPTH (2) may be comma
lists, whose product is the grid; MMS_GBM_MIN_LEAF (10), MMS_GBM_L2 (1.0), MMS_GBM_SUBSAMPLE (1.0), MMS_GBM_COLSAMPLE (1.0), MMS_GBM_BINS
(32); hash streams from MMS_GBM_SEED (0).  All K (J + 1) |grid| boosters advance in lock-step
(multimodal_survival_prediction_amd/boosting.py); the (grid point, round count) of an outer fold is the one with the best mean
inner-fold C-index, and the validation fold is scored once at that choice.

Writes results/gbm_baseline/cv_results.json in the RNA-only schema -- best_c_index is the validation C-index at the choice made inside
the training patients (nested cross-validation, unlike the networks' maximum over epochs on the validation fold), best_epoch the chosen
round count, num_epochs the rounds run -- plus per fold fold_{k}_predictions.csv (patient_id, survival_time, event, risk_score = F: what
evaluate_model.py --bootstrap --compare reads), fold_{k}_survival_curves.csv (the same columns and one S_<tau> column per horizon, from
absolute_risk.breslow_baseline on the training patients' F: --compare-curves joins it), fold_{k}_importance.csv (index, column, gene,
splits, gain_sum of the chosen booster's chosen rounds: gene_set_enrichment.py --scores ... --score-column gain_sum reads it) and
fold_{k}_curves.csv (per grid point and round count: every inner fold's C-index, their mean, and the validation fold's own C-index,
which is recorded and never consulted).
MMS_GBM_SHAP=1 (default 0: nothing more is computed or written) adds the TreeSHAP values (Booster.shap) of every fold's chosen booster at
its chosen round count on that fold's VALIDATION patients: fold_{k}_shap.npz (patient_id, genes = source columns, phi [patients, genes],
base; F = base + phi.sum(1), exp(phi) a gene's hazard-ratio multiplier for that patient), fold_{k}_shap_importance.csv (index, column,
gene, mean_abs_shap, mean_shap) and the pooled shap_importance.csv (gene, score = the mean |phi| over all out-of-fold patients, 0 for a
gene never split on: gene_set_enrichment.py --scores reads it by its default column)."""
import os
import time

import numpy as np

from _common import env_float, env_int, gene_hparams, save_json, select_genes, setup_device

RESULTS_DIR = "results/gbm_baseline"
N_FOLDS = env_int("MMS_FOLDS", 3)
N_PATIENTS = env_int("MMS_PATIENTS", 240)
ROUNDS = env_int("MMS_GBM_ROUNDS", 300)
LR = [float(v) for v in os.environ.get("MMS_GBM_LR", "0.1").split(",")]
DEPTH = [int(v) for v in os.environ.get("MMS_GBM_DEPTH", "2").split(",")]
MIN_LEAF = env_int("MMS_GBM_MIN_LEAF", 10)
L2 = env_float("MMS_GBM_L2", 1.0)
SUBSAMPLE = env_float("MMS_GBM_SUBSAMPLE", 1.0)
COLSAMPLE = env_float("MMS_GBM_COLSAMPLE", 1.0)
BINS = env_int("MMS_GBM_BINS", 32)
INNER = env_int("MMS_GBM_INNER", 5)
SEED = env_int("MMS_GBM_SEED", 0)
SHAP = env_int("MMS_GBM_SHAP", 0)


def curve_columns(horizons):
    """evaluate_model.py's curve_columns: repr keeps every digit, so --compare-curves reads the horizons back exactly"""
    return [f"S_{float(x)!r}" for x in horizons]


def curves_frame(r):
    """One row per (grid point, round count) of an outer fold's result (boosting.nested_cv): the inner folds' C-index, their mean, the
    validation fold's own curve, and whether the row is the one chosen."""
    import pandas as pd
    G, J, M = r["inner"].shape
    rows = []
    for g in range(G):
        for m in range(M):
            row = {"grid_index": g, "learning_rate": r["grid"][g]["learning_rate"], "max_depth": r["grid"][g]["max_depth"], "rounds": m + 1}
            row.update({f"inner_{j + 1}": r["inner"][g, j, m] for j in range(J)})
            row.update(inner_mean=r["inner_mean"][g, m], outer=r["outer_curve"][g, m], chosen=int(g == r["grid_index"] and m + 1 == r["rounds"]))
            rows.append(row)
    return pd.DataFrame(rows)


def write_outputs(results, label, folds, horizons, out_dir=RESULTS_DIR, gene_names=None, patient_ids=None, sel=None, hyper=None, seconds=None):
    """results: boosting.nested_cv's list (with `grid`: the grid points, added by main); label: [N, 2] (time, event) of the cohort.
    Writes every file of the module docstring -> the cv_results.json dict."""
    import pandas as pd
    from multimodal_survival_prediction_amd import absolute_risk, tree_shap
    os.makedirs(out_dir, exist_ok=True)
    fold_results, shap_folds = [], []
    for f, r in enumerate(results):
        fold = f + 1
        rows = np.asarray(r["val_rows"])
        base = {"patient_id": [patient_ids[i] if patient_ids is not None else f"SYN-{i:04d}" for i in rows], "survival_time": label[rows, 0],
                "event": label[rows, 1].astype(int), "risk_score": r["val_F"]}
        pd.DataFrame(base).to_csv(os.path.join(out_dir, f"fold_{fold}_predictions.csv"), index=False)
        tr = np.asarray(r["train_rows"])
        bl = absolute_risk.breslow_baseline(r["train_F"], label[tr, 0], label[tr, 1])
        S = bl.survival(r["val_F"], horizons)
        pd.DataFrame({**base, **{c: S[:, h] for h, c in enumerate(curve_columns(horizons))}}).to_csv(
            os.path.join(out_dir, f"fold_{fold}_survival_curves.csv"), index=False)
        counts, gain = r["importance"]
        used = np.nonzero(counts)[0]
        used = used[np.argsort(-gain[used], kind="stable")]
        src = used if sel is None else np.asarray(sel.columns[f])[used]
        pd.DataFrame({"index": used, "column": src, "gene": [str(gene_names[int(j)]) if gene_names is not None else f"gene_{int(j)}" for j in src],
                      "splits": counts[used], "gain_sum": gain[used]}).to_csv(os.path.join(out_dir, f"fold_{fold}_importance.csv"), index=False)
        curves_frame(r).to_csv(os.path.join(out_dir, f"fold_{fold}_curves.csv"), index=False)
        if "shap" in r:
            shap_folds.append(tree_shap.write_fold(out_dir, fold, r["shap"], base["patient_id"], None if sel is None else sel.columns[f], gene_names))
        print(f"fold {fold} | grid point {r['grid_index']} {r['grid_point']['learning_rate']}/{r['grid_point']['max_depth']} | rounds {r['rounds']} | "
              f"Val C-index: {r['c_index']:.4f} | inner mean C-index: {r['inner_mean'][r['grid_index'], r['rounds'] - 1]:.4f}", flush=True)
        fold_results.append({"fold": fold, "best_c_index": float(r["c_index"]), "best_epoch": int(r["rounds"]), "train_size": int(len(folds[f][0])),
                             "val_size": int(len(folds[f][1])), "grid_index": int(r["grid_index"]),
                             "learning_rate": float(r["grid_point"]["learning_rate"]), "max_depth": int(r["grid_point"]["max_depth"]),
                             "inner_c_index": float(r["inner_mean"][r["grid_index"], r["rounds"] - 1]), "genes_split_on": int(len(used))})
    if shap_folds:
        tree_shap.write_pooled(out_dir, shap_folds, results[0]["booster"].p if sel is None else sel.n_genes, gene_names)
    c = [r["best_c_index"] for r in fold_results]
    cv = {"model": "Gradient-boosted Cox trees", "n_folds": len(results), "num_epochs": int(results[0]["inner"].shape[2]) if results else 0,
          "c_index_mean": float(np.mean(c)), "c_index_std": float(np.std(c)), "fold_results": fold_results,
          "hyperparameters": {**(hyper or {}), "horizons": [float(h) for h in horizons], **gene_hparams(sel)}}
    if seconds is not None:
        cv["seconds"] = float(seconds)
    save_json(os.path.join(out_dir, "cv_results.json"), cv)
    return cv


def main():
    from multimodal_survival_prediction_amd import boosting, data, survival_forest
    world, rank, device = setup_device()
    if rank != 0:                                                  # one lock-step call holds every problem: nothing to spread over ranks
        return
    os.makedirs(RESULTS_DIR, exist_ok=True)
    cohort = data.cohort_to(data.make_cohort(n=N_PATIENTS, dims=(32, 32, 32), seed=427, complete=True), device)   # volumes unused
    folds = data.kfold_indices(cohort["n"], N_FOLDS, seed=42)
    sel = select_genes(cohort, [tr for tr, _ in folds], lambda name: os.path.join(RESULTS_DIR, f"best_model_fold{name}.pth"), rank=rank)
    grid = boosting.default_grid(LR, DEPTH)
    t0 = time.perf_counter()
    res = boosting.nested_cv(cohort, folds, inner=INNER, rounds=ROUNDS, grid=grid, seed=SEED, min_leaf=MIN_LEAF, l2=L2, subsample=SUBSAMPLE,
                             colsample=COLSAMPLE, bins=BINS, shap=SHAP > 0)
    dt = time.perf_counter() - t0
    for r in res:
        r["grid"] = grid
    label = cohort["label"].cpu().numpy()
    horizons = survival_forest.default_horizons(label[:, 0], label[:, 1])
    hyper = {"rounds": ROUNDS, "learning_rate": LR, "max_depth": DEPTH, "min_leaf": MIN_LEAF, "l2": L2, "subsample": SUBSAMPLE,
             "colsample": COLSAMPLE, "bins": BINS, "inner_folds": INNER, "seed": SEED}
    cv = write_outputs(res, label, folds, horizons, RESULTS_DIR, cohort.get("gene_names"), cohort.get("patient_id"), sel, hyper, dt)
    print(f"C-index: {cv['c_index_mean']:.4f} +/- {cv['c_index_std']:.4f} (validation folds at the choice of the inner folds; {dt:.2f} s for "
          f"{len(folds) * (INNER + 1) * len(grid)} boosters x {ROUNDS} rounds); saved {RESULTS_DIR}/cv_results.json")


if __name__ == "__main__":
    main()
