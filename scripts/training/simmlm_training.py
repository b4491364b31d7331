#!/usr/bin/env python3
"""SimMLM_SurvivalNet training (gated mixture of modality experts, R/scripts/analysis/generate_km_curves.py:158-281) on the
MI355X.  The reference ships the model and its results (results/simmim/cv_results.json) but no training script; this entry point
has the shape of the others: defaults from the reference's JSON (3 folds, batch 8, lr 1e-4, MMS_EPOCHS = 50 epochs of one stage),
K-fold over the cohort, fold groups by default, distributed.folds_of_rank, MMS_* environment overrides.

The objective is this project's own (the reference's two-stage schedule and MoFe loss are not in the reference):
    L = cox(ensemble; has_survival) + EXPERT_LAMBDA * sum_m cox(h_m; has_survival and mask_m),   EXPERT_LAMBDA default 0.1.
Cohort: the patients with a survival label and at least one modality (a patient without any has a NaN ensemble hazard); the number
dropped is reported.  Writes results/simmim/cv_results.json and models/simmim/fold_{k}_best.pth (the checkpoint path
generate_km_curves.py:380 names).
"""
import os
import time

import numpy as np
import torch

from _common import Transfer, augment_hparams, augment_spec, cv_lockstep, env_dims, env_float, env_int, gene_hparams, load_or_make_cohort, lockstep_enabled, rna_width, save_json, select_genes, setup_device

from multimodal_survival_prediction_amd import data, distributed as D
from multimodal_survival_prediction_amd.models import SimMLM_SurvivalNet
from multimodal_survival_prediction_amd.training import FusedOptimizer, ReduceLROnPlateau
from multimodal_survival_prediction_amd.training import train_epoch_simmlm as train_epoch
from multimodal_survival_prediction_amd.training import validate_simmlm as validate

SEED = 42
BATCH_SIZE = env_int("MMS_BATCH_SIZE", 8)
LEARNING_RATE = env_float("MMS_LR", 1e-4)
NUM_EPOCHS = env_int("MMS_EPOCHS", 50)
N_FOLDS = env_int("MMS_FOLDS", 3)
PATIENCE = env_int("MMS_PATIENCE", 15)
EXPERT_LAMBDA = env_float("MMS_EXPERT_LAMBDA", 0.1)
N_PATIENTS = env_int("MMS_PATIENTS", 608)
AUGMENT = augment_spec("simmlm")        # MMS_AUGMENT: GPU batch augmentation of the training loaders (unset: off)


def main():
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    world, rank, device = setup_device()
    cohort = load_or_make_cohort(device, n=N_PATIENTS, dims=env_dims(), seed=608, complete=False)      # data/processed/* in the cwd, else synthetic
    has_surv = cohort["has_survival"].cpu().numpy().astype(bool)
    any_mod = (cohort["mask"].cpu().numpy() != 0).any(1)
    usable = np.nonzero(has_surv & any_mod)[0]
    dropped = int(len(has_surv) - len(usable))
    if rank == 0:
        print(f"SimMLM cohort: {len(usable)} of {len(has_surv)} patients (dropped {dropped}: {int((~has_surv).sum())} without a survival "
              f"label, {int((has_surv & ~any_mod).sum())} labelled without any modality)", flush=True)
    folds = data.kfold_indices(len(usable), N_FOLDS, seed=SEED)
    os.makedirs("models/simmim", exist_ok=True)
    ckpt = lambda name: f"models/simmim/fold_{name}_best.pth"
    sel = select_genes(cohort, [usable[tr] for tr, _ in folds], ckpt, rank=rank)        # MMS_SELECT_GENES (unset: off)
    xfer = Transfer(cohort, sel, rank)        # MMS_PRETRAINED / MMS_PRETRAINED_GENES / MMS_FINETUNE (unset: off)
    kw = dict(lr=LEARNING_RATE, weight_decay=1e-4, adamw=False, expert_weight=EXPERT_LAMBDA)
    local = []
    my_folds = list(D.folds_of_rank(N_FOLDS, world, rank))
    if lockstep_enabled(len(my_folds)):
        splits = [(usable[folds[f][0]], usable[folds[f][1]]) for f in my_folds]
        loaders = [(data.BatchLoader(cohort, tr, BATCH_SIZE, shuffle=True, seed=SEED + f, augment=AUGMENT, augment_style="simmlm", fold=f),
                    data.BatchLoader(cohort, va, BATCH_SIZE, shuffle=False, fold=f)) for f, (tr, va) in zip(my_folds, splits)]
        models = [SimMLM_SurvivalNet(**rna_width(sel)).to(device) for _ in my_folds]
        res = cv_lockstep("simmlm", models, loaders, kw, NUM_EPOCHS, PATIENCE,
                          lambda o: ReduceLROnPlateau(o, mode="max", factor=0.5, patience=5),
                          ckpt, device, rank, [f + 1 for f in my_folds], fold_ids=my_folds, transfer=xfer)
        local = [{"fold": f + 1, "best_c_index": r["best_c_index"], "train_size": int(len(tr)), "val_size": int(len(va)),
                  "patients_per_sec": r["patients_per_sec"], "epochs_run": r["epochs_run"]}
                 for f, r, (tr, va) in zip(my_folds, res, splits)]
        my_folds = []
    for fold in my_folds:
        tr, va = usable[folds[fold][0]], usable[folds[fold][1]]
        train_loader = data.BatchLoader(cohort, tr, BATCH_SIZE, shuffle=True, seed=SEED + fold, augment=AUGMENT, augment_style="simmlm", fold=fold)
        val_loader = data.BatchLoader(cohort, va, BATCH_SIZE, shuffle=False, fold=fold)
        model = SimMLM_SurvivalNet(**rna_width(sel)).to(device)
        xfer.apply(model, fold + 1, fold)
        optimizer = FusedOptimizer(model, **kw, **xfer.engine_kw)
        scheduler = ReduceLROnPlateau(optimizer, mode="max", factor=0.5, patience=5)
        best_c_index, patience_counter, t_train, n_train, epochs_run = 0, 0, 0.0, 0, 0
        for epoch in range(NUM_EPOCHS):
            epochs_run = epoch + 1
            torch.cuda.synchronize(); t0 = time.perf_counter()
            train_loss = train_epoch(model, train_loader, optimizer, device)
            torch.cuda.synchronize(); t_train += time.perf_counter() - t0; n_train += len(tr)
            val_loss, val_c_index = validate(model, val_loader, device)
            scheduler.step(val_c_index)
            if (epoch + 1) % 5 == 0 or epoch == 0:
                print(f"[rank {rank}] fold {fold + 1} epoch {epoch + 1:3d}: L={train_loss:.4f}, Val Loss={val_loss:.4f}, "
                      f"C-index={val_c_index:.4f}", flush=True)
            if val_c_index > best_c_index:
                best_c_index, patience_counter = val_c_index, 0
                torch.save(model.state_dict(), f"models/simmim/fold_{fold + 1}_best.pth")
            else:
                patience_counter += 1
                if patience_counter >= PATIENCE:
                    break
        local.append({"fold": fold + 1, "best_c_index": best_c_index, "train_size": int(len(tr)), "val_size": int(len(va)),
                      "patients_per_sec": n_train / t_train, "epochs_run": epochs_run})
    cv_results = D.gather_fold_results(local, world)
    if rank == 0:
        c = [r["best_c_index"] for r in cv_results]
        save_json("results/simmim/cv_results.json", {
            "model": "SimMLM", "c_index_mean": float(np.mean(c)), "c_index_std": float(np.std(c)), "fold_results": cv_results,
            "patients": int(len(usable)), "patients_dropped": dropped,
            "hyperparameters": {"batch_size": BATCH_SIZE, "learning_rate": LEARNING_RATE, "epochs": NUM_EPOCHS, "n_folds": N_FOLDS,
                                "expert_lambda": EXPERT_LAMBDA,
                                **augment_hparams(AUGMENT), **gene_hparams(sel)}, **xfer.record()})
        print(f"C-index: {np.mean(c):.4f} +/- {np.std(c):.4f}; saved results/simmim/cv_results.json")


if __name__ == "__main__":
    main()
