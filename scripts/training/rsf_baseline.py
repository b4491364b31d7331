#!/usr/bin/env python3
"""Random survival forest baseline on the genes, K-fold cross-validation -- the nonlinear, non-deep point on the reference's "simple is
better for small datasets" / "RNA-only wins" axis (final_comparison.py:301-335), next to cox_baseline.py's linear one.

Same conventions as cox_baseline.py: the seeded synthetic cohort (MMS_PATIENTS), MMS_FOLDS folds from kfold_indices(seed=42),
MMS_SELECT_GENES (per-fold gene selection; each fold's trees then read that fold's genes).  Every fold grows MMS_RSF_TREES (500) trees on
bootstrap samples of its training patients; a node tries MMS_RSF_MTRY (0 = ceil(sqrt(genes))) random genes with MMS_RSF_NSPLIT (10)
random thresholds each, splits by the log-rank statistic while both children keep MMS_RSF_MIN_LEAF (15) patients, down to MMS_RSF_DEPTH
(10) levels; hash streams from MMS_RSF_SEED (0).  All trees of all folds grow in lock-step
(multimodal_survival_prediction_amd/survival_forest.py).

Writes results/rsf_baseline/cv_results.json in the RNA-only schema -- best_c_index is the validation C-index of the forest as specified
(nothing is tuned on the validation fold, unlike the networks' maximum over epochs), oob_c_index beside it is the out-of-bag C-index of
the fold's training patients; num_epochs / best_epoch have no meaning here and are 0 -- plus per fold fold_{k}_predictions.csv
(patient_id, survival_time, event, risk_score = ensemble mortality: what evaluate_model.py --bootstrap --compare reads),
fold_{k}_survival_curves.csv (the same columns and one S_<tau> column per horizon, the layout of evaluate_model.py's survival_curves.csv:
--compare-curves joins it) and fold_{k}_importance.csv (gene column, name, splits, summed chi2; the genes some tree split on).
MMS_RSF_VIMP = R > 0 (default 0: nothing more is computed or written) adds the out-of-bag permutation importance with R repeats, one
launch for all folds: fold_{k}_vimp.csv (index, column, gene, splits, chi2_sum, vimp = the drop in the fold's out-of-bag C-index when the
gene is shuffled, vimp_sd over the repeats; the same genes, sorted by vimp) and "vimp_repeats" among the hyperparameters.
MMS_RSF_SHAP=1 (default 0: nothing more is computed or written) adds the TreeSHAP values (Forest.shap) of every fold's trees on that
fold's VALIDATION patients: fold_{k}_shap.npz (patient_id, genes = source columns, phi [patients, genes], base; mortality = base +
phi.sum(1)), fold_{k}_shap_importance.csv (index, column, gene, mean_abs_shap, mean_shap) and the pooled shap_importance.csv (gene, score =
the mean |phi| over all out-of-fold patients, 0 for a gene never split on: gene_set_enrichment.py --scores reads it by its default
column)."""
import os
import time

import numpy as np

from _common import env_int, gene_hparams, save_json, select_genes, setup_device

from multimodal_survival_prediction_amd import data, survival_forest, tree_shap

RESULTS_DIR = "results/rsf_baseline"
N_FOLDS = env_int("MMS_FOLDS", 3)
N_PATIENTS = env_int("MMS_PATIENTS", 240)
TREES = env_int("MMS_RSF_TREES", 500)
MTRY = env_int("MMS_RSF_MTRY", 0)
NSPLIT = env_int("MMS_RSF_NSPLIT", 10)
MIN_LEAF = env_int("MMS_RSF_MIN_LEAF", 15)
DEPTH = env_int("MMS_RSF_DEPTH", 10)
SEED = env_int("MMS_RSF_SEED", 0)
VIMP = env_int("MMS_RSF_VIMP", 0)
SHAP = env_int("MMS_RSF_SHAP", 0)


def curve_columns(horizons):
    """evaluate_model.py's curve_columns: repr keeps every digit, so --compare-curves reads the horizons back exactly"""
    return [f"S_{float(x)!r}" for x in horizons]


def main():
    import pandas as pd
    world, rank, device = setup_device()
    if rank != 0:                                                  # one lock-step call holds every fold: nothing to spread over ranks
        return
    os.makedirs(RESULTS_DIR, exist_ok=True)
    cohort = data.cohort_to(data.make_cohort(n=N_PATIENTS, dims=(32, 32, 32), seed=427, complete=True), device)   # volumes unused
    folds = data.kfold_indices(cohort["n"], N_FOLDS, seed=42)
    sel = select_genes(cohort, [tr for tr, _ in folds], lambda name: os.path.join(RESULTS_DIR, f"best_model_fold{name}.pth"), rank=rank)
    t0 = time.perf_counter()
    res = survival_forest.cross_validate(cohort, folds, n_trees=TREES, mtry=MTRY or None, nsplit=NSPLIT, min_leaf=MIN_LEAF, max_depth=DEPTH,
                                         seed=SEED, vimp=VIMP, shap=SHAP > 0)
    dt = time.perf_counter() - t0
    names, ids = cohort.get("gene_names"), cohort.get("patient_id")
    label = cohort["label"].cpu().numpy()
    fold_results, shap_folds = [], []
    for f, r in enumerate(res):
        fold = f + 1
        rows = r["val_rows"]
        base = {"patient_id": [ids[i] if ids is not None else f"SYN-{i:04d}" for i in rows], "survival_time": label[rows, 0],
                "event": label[rows, 1].astype(int), "risk_score": r["val_mortality"]}
        pd.DataFrame(base).to_csv(os.path.join(RESULTS_DIR, f"fold_{fold}_predictions.csv"), index=False)
        pd.DataFrame({**base, **{c: r["val_survival"][:, h] for h, c in enumerate(curve_columns(r["horizons"]))}}).to_csv(
            os.path.join(RESULTS_DIR, f"fold_{fold}_survival_curves.csv"), index=False)
        counts, chi2 = r["importance"]
        used = np.nonzero(counts)[0]
        used = used[np.argsort(-chi2[used], kind="stable")]
        src = used if sel is None else np.asarray(sel.columns[f])[used]
        pd.DataFrame({"index": used, "column": src, "gene": [str(names[int(j)]) if names is not None else f"gene_{int(j)}" for j in src],
                      "splits": counts[used], "chi2_sum": chi2[used]}).to_csv(os.path.join(RESULTS_DIR, f"fold_{fold}_importance.csv"), index=False)
        if VIMP > 0:
            by = np.nonzero(counts)[0]
            by = by[np.argsort(-r["vimp"][by], kind="stable")]
            col = by if sel is None else np.asarray(sel.columns[f])[by]
            pd.DataFrame({"index": by, "column": col, "gene": [str(names[int(j)]) if names is not None else f"gene_{int(j)}" for j in col],
                          "splits": counts[by], "chi2_sum": chi2[by], "vimp": r["vimp"][by], "vimp_sd": r["vimp_reps"][:, by].std(0)}).to_csv(
                os.path.join(RESULTS_DIR, f"fold_{fold}_vimp.csv"), index=False)
        if "shap" in r:
            shap_folds.append(tree_shap.write_fold(RESULTS_DIR, fold, r["shap"], base["patient_id"], None if sel is None else sel.columns[f], names))
        print(f"fold {fold} | trees {TREES} | Val C-index: {r['c_index']:.4f} | OOB C-index: {r['oob_c_index']:.4f} "
              f"({r['oob_missing']} training patients never out of bag)", flush=True)
        fold_results.append({"fold": fold, "best_c_index": float(r["c_index"]), "best_epoch": 0, "train_size": int(len(folds[f][0])),
                             "val_size": int(len(folds[f][1])), "oob_c_index": float(r["oob_c_index"]), "oob_missing": int(r["oob_missing"]),
                             "genes_split_on": int(len(used))})
    if shap_folds:
        tree_shap.write_pooled(RESULTS_DIR, shap_folds, res[0]["forest"].p if sel is None else sel.n_genes, names)
    c = [r["best_c_index"] for r in fold_results]
    hyper = res[0]["forest"].hyper if res else {}
    save_json(os.path.join(RESULTS_DIR, "cv_results.json"), {
        "model": "Random survival forest", "n_folds": N_FOLDS, "num_epochs": 0,
        "c_index_mean": float(np.mean(c)), "c_index_std": float(np.std(c)), "fold_results": fold_results,
        "hyperparameters": {"n_trees": TREES, **hyper, "horizons": [float(h) for h in (res[0]["horizons"] if res else [])],
                            **({"vimp_repeats": VIMP} if VIMP > 0 else {}), **gene_hparams(sel)}})
    print(f"C-index: {np.mean(c):.4f} +/- {np.std(c):.4f} (validation folds, nothing tuned on them; {dt:.2f} s for all trees); "
          f"saved {RESULTS_DIR}/cv_results.json")


if __name__ == "__main__":
    main()
