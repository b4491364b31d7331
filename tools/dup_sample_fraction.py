"""Share of a training run's sample-volumes that the forward has to compute when the identical all-zero volumes of a (model, batch) pair are
computed once (MmsDnOpts.dup_zero): every sample with a CT plus one representative of the zero samples.  Counted on the CPU over three
epochs of bench.py's flagship workload -- the cohort, folds, loaders and seeds bench.py builds; the volumes' size does not enter, so tiny
ones are made.
    python tools/dup_sample_fraction.py"""
import os, sys, collections, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_survival_prediction_amd import data
B, dims, K, EPOCHS = 4, (8, 8, 8), 5, 3
c = data.make_cohort(n=608, dims=dims, rna_dim=16, seed=608, complete=False)
ct = c["mask"][:, 0].numpy() > 0
print("patients", len(ct), "with a CT", int(ct.sum()))
has = c["has_survival"].numpy()
surv, non = np.nonzero(has)[0], np.nonzero(~has)[0]
folds = data.kfold_indices(len(surv), K, seed=42)
tr = [np.concatenate([surv[f[0]], non]) for f in folds]
hist = collections.Counter()
rows = comp = pairs = 0
for ep in range(EPOCHS):
    for k, t in enumerate(tr):
        L = data.BatchLoader(c, t, B, shuffle=True, seed=42 + k, lazy=True, with_valid=True)
        for _ in range(ep + 1):                      # the loader reshuffles per pass: epoch ep is its pass ep + 1
            batches = list(L)
        for b in batches:
            idx = b["index"]
            idx = np.asarray(idx.cpu() if hasattr(idx, "cpu") else idx).reshape(-1)
            n, r = len(idx), int(ct[idx].sum())
            hist[(n, r)] += 1
            pairs += 1; rows += n; comp += r + (1 if n > r else 0)
print("(model, batch) pairs", pairs)
print("full batches of %d by samples with a CT:" % B, {r: hist[(B, r)] for r in range(B + 1)})
print("ragged tails:", {k: v for k, v in sorted(hist.items()) if k[0] != B})
print("sample-volumes %d, computed %d (%.1f %%), repeats %.1f %%" % (rows, comp, 100.0 * comp / rows, 100.0 * (rows - comp) / rows))
