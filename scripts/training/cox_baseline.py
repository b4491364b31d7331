#!/usr/bin/env python3
"""Elastic-net Cox regression baseline on the genes, nested cross-validation -- the linear point on the reference's "simple is better for
small datasets" / "RNA-only wins" axis (final_comparison.py:301-335), which the reference itself does not have.

Same conventions as train_rnaseq_only.py: the seeded synthetic cohort (MMS_PATIENTS), MMS_FOLDS outer folds from kfold_indices(seed=42),
MMS_SELECT_GENES (per-fold gene selection; each outer fold's fits then read that fold's genes).  Inside each outer fold's training patients
MMS_COX_INNER (5) inner folds choose lambda among MMS_COX_NLAMBDA (30) log-spaced values down to 0.05 lambda_max by MMS_COX_CRITERION
("cindex": mean inner-validation C-index; "pl": cross-validated partial likelihood) at elastic-net mixing MMS_COX_ALPHA (0.5), inner folds
drawn from MMS_COX_SEED (0).  All fits of all folds advance in lock-step (multimodal_survival_prediction_amd/coxnet.py).

Writes results/cox_baseline/cv_results.json in the RNA-only schema -- best_c_index is the OUTER validation C-index at the lambda chosen
inside the fold, so unlike the networks' (a maximum over epochs on the validation fold) it has not seen the validation patients;
num_epochs / best_epoch have no meaning here and are 0 -- plus fold_{k}_coefficients.json (the non-zero genes, their names when known,
lambda) and fold_{k}_predictions.csv (patient_id, survival_time, event, risk_score: what evaluate_model.py --bootstrap --compare reads)."""
import os
import time

import numpy as np

from _common import env_float, env_int, gene_hparams, save_json, select_genes, setup_device

from multimodal_survival_prediction_amd import coxnet, data

RESULTS_DIR = "results/cox_baseline"
N_FOLDS = env_int("MMS_FOLDS", 3)
N_PATIENTS = env_int("MMS_PATIENTS", 240)
ALPHA = env_float("MMS_COX_ALPHA", 0.5)
N_LAMBDA = env_int("MMS_COX_NLAMBDA", 30)
INNER = env_int("MMS_COX_INNER", 5)
CRITERION = os.environ.get("MMS_COX_CRITERION", "cindex")
SEED = env_int("MMS_COX_SEED", 0)


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
    res = coxnet.nested_cv(cohort, folds, alpha=ALPHA, n_lambda=N_LAMBDA, inner=INNER, criterion=CRITERION, seed=SEED)
    dt = time.perf_counter() - t0
    names, ids = cohort.get("gene_names"), cohort.get("patient_id")
    label = cohort["label"].cpu().numpy()
    fold_results = []
    for f, r in enumerate(res):
        fold = f + 1
        cols = None if sel is None else sel.columns[f]
        coxnet.save_coefficients(os.path.join(RESULTS_DIR, f"fold_{fold}_coefficients.json"), r, ALPHA, gene_names=names, columns=cols)
        rows = r["val_rows"]
        pd.DataFrame({"patient_id": [ids[i] if ids is not None else f"SYN-{i:04d}" for i in rows], "survival_time": label[rows, 0],
                      "event": label[rows, 1].astype(int), "risk_score": r["val_eta"]}).to_csv(
            os.path.join(RESULTS_DIR, f"fold_{fold}_predictions.csv"), index=False)
        print(f"fold {fold} | lambda {r['lambda_']:.4g} (index {r['lambda_index']} of {N_LAMBDA}) | non-zero genes "
              f"{int(np.count_nonzero(r['coef']))} | Val C-index: {r['c_index']:.4f}", flush=True)
        fold_results.append({"fold": fold, "best_c_index": float(r["c_index"]), "best_epoch": 0, "train_size": int(len(folds[f][0])),
                             "val_size": int(len(folds[f][1])), "lambda": r["lambda_"], "lambda_index": r["lambda_index"],
                             "nonzero": int(np.count_nonzero(r["coef"])), "converged": bool(r["status"] == 1)})
    c = [r["best_c_index"] for r in fold_results]
    save_json(os.path.join(RESULTS_DIR, "cv_results.json"), {
        "model": "Cox elastic net", "n_folds": N_FOLDS, "num_epochs": 0,
        "c_index_mean": float(np.mean(c)), "c_index_std": float(np.std(c)), "fold_results": fold_results,
        "hyperparameters": {"alpha": ALPHA, "n_lambda": N_LAMBDA, "inner_folds": INNER, "criterion": CRITERION, "seed": SEED,
                            **gene_hparams(sel)}})
    print(f"C-index: {np.mean(c):.4f} +/- {np.std(c):.4f} (nested CV, {dt:.2f} s for all fits); saved {RESULTS_DIR}/cv_results.json")


if __name__ == "__main__":
    main()
