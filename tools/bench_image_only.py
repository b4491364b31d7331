#!/usr/bin/env python
"""ImageOnlyModel (CT-only baseline: 3-conv encoder at 16 / 32 / 64 channels + two Linear layers) K-fold training step, three layouts.

The reference's image-only cohort: 142 patients with an image and a survival label, 5 folds, batch 4, 64x64x32 volumes.  Three legs,
interleaved round by round in one process (same cohort, same loaders' batch order, each leg its own copies of the five fold models):
  sequential       five SurvivalEngines stepped one after another (train_epoch_image; scalar single-model kernels)
  group            the five folds as ONE lock-step FoldGroupEngine group (train_epoch_lockstep, one stream; fp32-MFMA group kernels)
  group_indexed    batches named by index (one gather launch per step), sub-groups 2 + 2 + 1 on three streams
  group_fused, group_indexed_fused    the two lock-step legs with the fused tail (FoldGroupEngine(fused_tail=True): BN3 + ReLU + pool and both
                   Linear layers in one launch per pass) -- the A/B behind FoldGroupEngine.FUSED_IMG_TAIL
Writes ms per lock-step position (= one batch of every fold), patients/s and the ratios to --out as JSON and prints the same line."""
import argparse
import copy
import itertools
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=28, help="batch positions per leg and round (a fold's training split has 28 whole batches)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--patients", type=int, default=142)
    ap.add_argument("--volume", type=int, nargs=3, default=[64, 64, 32])
    ap.add_argument("--out", default=os.path.join("profiles", "image_only_bench.json"))
    args = ap.parse_args()

    import torch
    from multimodal_survival_prediction_amd import data, models
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    from multimodal_survival_prediction_amd.training import FusedOptimizer, train_epoch_image, train_epoch_lockstep

    dev = torch.device("cuda:0")
    B, K, dims = 4, 5, tuple(args.volume)
    cohort = data.cohort_to(data.make_cohort(n=args.patients, dims=dims, rna_dim=8, seed=142, complete=True), dev)      # every patient: image + label
    folds = data.kfold_indices(args.patients, K, seed=42)
    train_sets = [f[0] for f in folds]
    steps = min(args.steps, min(len(t) for t in train_sets) // B)         # whole batches only: no ragged tail inside the timed region

    def loaders(lazy):
        kw = dict(lazy=True, with_valid=True) if lazy else {}
        return [data.BatchLoader(cohort, t, B, shuffle=True, seed=42 + k, **kw) for k, t in enumerate(train_sets)]

    base = []
    for k in range(K):
        torch.manual_seed(42 + k)
        base.append(models.ImageOnlyModel())
    hyper = dict(lr=1e-4, weight_decay=1e-4, adamw=False)
    seq_models = [copy.deepcopy(m).to(dev).train() for m in base]
    seq_opts = [FusedOptimizer(m, **hyper) for m in seq_models]
    group = lambda fused: FoldGroupEngine([copy.deepcopy(m).to(dev).train() for m in base], fused_tail=fused, **hyper)
    grp, grp_ix, grp_f, grp_ix_f = group(False), group(False), group(True), group(True)
    ld_seq, ld_grp, ld_ix, ld_grp_f, ld_ix_f = loaders(False), loaders(False), loaders(True), loaders(False), loaders(True)
    cut = lambda ls: [itertools.islice(l, steps) for l in ls]

    def leg_sequential():
        for m, o, l in zip(seq_models, seq_opts, cut(ld_seq)):
            train_epoch_image(m, l, o, dev)

    legs = {"sequential": leg_sequential,
            "group": lambda: train_epoch_lockstep(grp, cut(ld_grp), "image"),
            "group_fused": lambda: train_epoch_lockstep(grp_f, cut(ld_grp_f), "image"),
            "group_indexed": lambda: train_epoch_lockstep(grp_ix, cut(ld_ix), "image", concurrent=3),
            "group_indexed_fused": lambda: train_epoch_lockstep(grp_ix_f, cut(ld_ix_f), "image", concurrent=3)}
    ms = {k: [] for k in legs}
    for r in range(args.rounds + 1):                # round 0: warm-up (plans, graph capture), not recorded
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"config": "image-only cohort: %d patients, ImageOnlyModel, %d folds, batch %d, %dx%dx%d" % (args.patients, K, B, dims[0], dims[1], dims[2]),
           "device": torch.cuda.get_device_name(0), "steps_per_round": steps, "rounds": args.rounds,
           "ms_per_step": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "ms_per_step_median": {k: round(v, 4) for k, v in med.items()},
           "patients_per_s": {k: round(K * B / v * 1e3, 1) for k, v in med.items()},
           "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
           "speedup_group": round(med["sequential"] / med["group"], 3),
           "speedup_group_indexed": round(med["sequential"] / med["group_indexed"], 3),
           "fused_tail_gain": {"group": round(med["group"] / med["group_fused"], 4),
                               "group_indexed": round(med["group_indexed"] / med["group_indexed_fused"], 4)}}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
