#!/usr/bin/env python3
"""ImageOnlyModel training (the CT-only baseline, R/scripts/analysis/generate_km_curves.py:28-54) on the MI355X.  The reference ships
the class and its results (results/image_only/cv_results.json: 5 folds, 142 patients) but no training script; this entry point has the
shape of the others and the settings of final_multimodal.py: 5-fold KFold(shuffle=True, random_state=42), Adam lr 1e-4 / weight decay
1e-4, ReduceLROnPlateau('max', 0.5, 5), patience 15, 50 epochs, batch 4; fold groups by default, distributed.folds_of_rank, MMS_*
environment overrides.

The loop is training.train_epoch_image / validate_image (final_multimodal.py:238-305 on the image alone).
Cohort: the patients that have both an image and a survival label (142 of the reference's 608).  Writes
results/image_only/cv_results.json (reference keys c_index_mean, c_index_std, fold_results[{fold, best_c_index}] + extras) and
models/image_only/fold_{k}_best.pth.
"""
import os
import time

import numpy as np
import torch

from _common import Transfer, augment_hparams, augment_spec, cv_lockstep, env_dims, env_float, env_int, load_or_make_cohort, lockstep_enabled, save_json, setup_device

from multimodal_survival_prediction_amd import data, distributed as D
from multimodal_survival_prediction_amd.models import ImageOnlyModel
from multimodal_survival_prediction_amd.training import FusedOptimizer, ReduceLROnPlateau
from multimodal_survival_prediction_amd.training import train_epoch_image as train_epoch
from multimodal_survival_prediction_amd.training import validate_image as validate

SEED = 42
BATCH_SIZE = env_int("MMS_BATCH_SIZE", 4)
LEARNING_RATE = env_float("MMS_LR", 1e-4)
NUM_EPOCHS = env_int("MMS_EPOCHS", 50)
N_FOLDS = env_int("MMS_FOLDS", 5)
PATIENCE = env_int("MMS_PATIENCE", 15)
N_PATIENTS = env_int("MMS_PATIENTS", 608)
AUGMENT = augment_spec("image")        # MMS_AUGMENT: GPU batch augmentation of the training loaders (unset: off)


def main():
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    world, rank, device = setup_device()
    cohort = load_or_make_cohort(device, n=N_PATIENTS, dims=env_dims(), seed=608, complete=False)      # data/processed/* in the cwd, else synthetic
    has_surv = cohort["has_survival"].cpu().numpy().astype(bool)
    has_img = cohort["mask"].cpu().numpy()[:, 0] != 0
    usable = np.nonzero(has_surv & has_img)[0]
    if rank == 0:
        print(f"Image-only cohort: {len(usable)} of {len(has_surv)} patients have an image and a survival label", flush=True)
    folds = data.kfold_indices(len(usable), N_FOLDS, seed=SEED)
    xfer = Transfer(cohort, None, rank)        # MMS_PRETRAINED / MMS_PRETRAINED_GENES / MMS_FINETUNE (unset: off)
    os.makedirs("models/image_only", exist_ok=True)
    kw = dict(lr=LEARNING_RATE, weight_decay=1e-4, adamw=False)
    local = []
    my_folds = list(D.folds_of_rank(N_FOLDS, world, rank))
    if lockstep_enabled(len(my_folds), BATCH_SIZE):
        splits = [(usable[folds[f][0]], usable[folds[f][1]]) for f in my_folds]
        loaders = [(data.BatchLoader(cohort, tr, BATCH_SIZE, shuffle=True, seed=SEED + f, augment=AUGMENT, augment_style="image"),
                    data.BatchLoader(cohort, va, BATCH_SIZE, shuffle=False)) for f, (tr, va) in zip(my_folds, splits)]
        models = [ImageOnlyModel().to(device) for _ in my_folds]
        res = cv_lockstep("image", models, loaders, kw, NUM_EPOCHS, PATIENCE,
                          lambda o: ReduceLROnPlateau(o, mode="max", factor=0.5, patience=5),
                          lambda name: f"models/image_only/fold_{name}_best.pth", device, rank, [f + 1 for f in my_folds], transfer=xfer)
        local = [{"fold": f + 1, "best_c_index": r["best_c_index"], "train_size": int(len(tr)), "val_size": int(len(va)),
                  "patients_per_sec": r["patients_per_sec"], "epochs_run": r["epochs_run"]}
                 for f, r, (tr, va) in zip(my_folds, res, splits)]
        my_folds = []
    for fold in my_folds:
        tr, va = usable[folds[fold][0]], usable[folds[fold][1]]
        train_loader = data.BatchLoader(cohort, tr, BATCH_SIZE, shuffle=True, seed=SEED + fold, augment=AUGMENT, augment_style="image")
        val_loader = data.BatchLoader(cohort, va, BATCH_SIZE, shuffle=False)
        model = ImageOnlyModel().to(device)
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
                print(f"[rank {rank}] fold {fold + 1} epoch {epoch + 1:3d}: Train Loss={train_loss:.4f}, Val Loss={val_loss:.4f}, "
                      f"C-index={val_c_index:.4f}", flush=True)
            if val_c_index > best_c_index:
                best_c_index, patience_counter = val_c_index, 0
                torch.save(model.state_dict(), f"models/image_only/fold_{fold + 1}_best.pth")
            else:
                patience_counter += 1
                if patience_counter >= PATIENCE:
                    break
        local.append({"fold": fold + 1, "best_c_index": best_c_index, "train_size": int(len(tr)), "val_size": int(len(va)),
                      "patients_per_sec": n_train / t_train, "epochs_run": epochs_run})
    cv_results = D.gather_fold_results(local, world)
    if rank == 0:
        c = [r["best_c_index"] for r in cv_results]
        save_json("results/image_only/cv_results.json", {
            "model": "Image-Only", "c_index_mean": float(np.mean(c)), "c_index_std": float(np.std(c)), "fold_results": cv_results,
            "patients": int(len(usable)),
            "hyperparameters": {"batch_size": BATCH_SIZE, "learning_rate": LEARNING_RATE, "epochs": NUM_EPOCHS, "n_folds": N_FOLDS,
                                **augment_hparams(AUGMENT)}, **xfer.record()})
        print(f"C-index: {np.mean(c):.4f} +/- {np.std(c):.4f}; saved results/image_only/cv_results.json")


if __name__ == "__main__":
    main()
