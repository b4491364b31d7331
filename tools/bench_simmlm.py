#!/usr/bin/env python3
"""Patients/s of a 5-fold LOCK-STEP training epoch of SimMLM_SurvivalNet and of PartialModalityNet at BASELINE config 3's layout
(608 synthetic patients with the cohort's modality masks, 64x64x32 volumes, batch 8): one FoldGroupEngine per model class, the
folds advanced by training.train_epoch_lockstep (3 HIP streams, batches assembled by the loaders for both), fused HIP-graph steps.
Cohort: the patients with a survival label and at least one modality (SimMLM's cohort), the same for both models.  The two legs
are interleaved and repeated (--reps), after one warm-up epoch each (graph capture); prints one JSON line with every epoch time.
    python tools/bench_simmlm.py [--patients 608] [--folds 5] [--batch 8] [--reps 3] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patients", type=int, default=608)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from multimodal_survival_prediction_amd import data, models, training as T
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    dev = torch.device("cuda:0")
    c = data.cohort_to(data.make_cohort(n=a.patients, dims=(64, 64, 32), rna_dim=5005, seed=608, complete=False), dev)
    keep = (c["has_survival"].cpu() & (c["mask"].cpu() != 0).any(1)).numpy()
    usable = np.nonzero(keep)[0]
    folds = data.kfold_indices(len(usable), a.folds, seed=42)
    legs = {}
    for cls, style in (("PartialModalityNet", "partial"), ("SimMLM_SurvivalNet", "simmlm")):
        ms = []
        for k in range(a.folds):
            torch.manual_seed(100 + k)
            ms.append(getattr(models, cls)(rna_dim=5005).to(dev))
        group = FoldGroupEngine(ms, lr=1e-4, weight_decay=1e-4, adamw=False)
        loaders = [data.BatchLoader(c, usable[folds[k][0]], a.batch, shuffle=True, seed=7 + k) for k in range(a.folds)]
        legs[cls] = (group, loaders, style, sum(len(folds[k][0]) for k in range(a.folds)))
        T.train_epoch_lockstep(group, loaders, style, concurrent=3)          # warm-up: graph capture of every (sub-)group shape
    torch.cuda.synchronize()
    times = {cls: [] for cls in legs}
    for _ in range(a.reps):
        for cls, (group, loaders, style, n) in legs.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            T.train_epoch_lockstep(group, loaders, style, concurrent=3)
            torch.cuda.synchronize()
            times[cls].append(time.perf_counter() - t0)
    out = dict(tool="bench_simmlm", patients=int(len(usable)), dropped=int(a.patients - len(usable)), folds=a.folds, batch=a.batch,
               reps=a.reps, order="interleaved: PartialModalityNet, SimMLM_SurvivalNet per repetition")
    for cls, (_, _, _, n) in legs.items():
        med = float(np.median(times[cls]))
        out[cls] = dict(patients_per_s=round(n / med, 1), epoch_s_median=round(med, 4), epoch_s=[round(x, 4) for x in times[cls]],
                        train_patients_per_epoch=n)
    out["simmlm_step_cost_ratio"] = round(out["SimMLM_SurvivalNet"]["epoch_s_median"] / out["PartialModalityNet"]["epoch_s_median"], 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
