"""What the backward of block 1's conv2 has to compute when the identical gradient rows of a (model, batch) pair's absent CTs are computed
once (MmsDnOpts.dup_zero_bwd): every sample with a CT plus one representative of the absent ones -- their rows of dout are zero under the
modality mask.  Counted on the CPU over three epochs of bench.py's flagship workload (the cohort, folds, loaders, seeds and rna_dim bench.py
builds; the volumes' size does not enter, so tiny ones are made), per (model, step) pair and per launch of the lock-step sub-groups 2 + 2 + 1,
where a launch lasts as long as its slowest member:
  weight gradient: rows of the slowest live member;
  backward-data:   tile rounds of the slowest CU -- a member of an n-model launch has 256 / n CUs (n = 1, 2), a sample 64 tiles of 32 rows.
    python tools/dup_sample_fraction_bwd.py"""
import os, sys, collections, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_survival_prediction_amd import data
B, dims, K, EPOCHS, TPS = 4, (8, 8, 8), 5, 3, 64
GROUPS = ((0, 1), (2, 3), (4,))
c = data.make_cohort(n=608, dims=dims, rna_dim=5005, seed=608, complete=False)
ct = c["mask"][:, 0].numpy() > 0
print("patients", len(ct), "with a CT", int(ct.sum()))
has = c["has_survival"].numpy()
surv, non = np.nonzero(has)[0], np.nonzero(~has)[0]
folds = data.kfold_indices(len(surv), K, seed=42)
tr = [np.concatenate([surv[f[0]], non]) for f in folds]
hist = collections.Counter()
pairs = live = rows = dup = 0
w_before = w_after = d_before = d_after = launches = 0
for ep in range(EPOCHS):
    per_model = []
    for k, t in enumerate(tr):
        L = data.BatchLoader(c, t, B, shuffle=True, seed=42 + k, lazy=True, with_valid=True)
        for _ in range(ep + 1):                      # the loader reshuffles per pass: epoch ep is its pass ep + 1
            batches = list(L)
        nr = []
        for b in batches:
            idx = b["index"]
            idx = np.asarray(idx.cpu() if hasattr(idx, "cpu") else idx).reshape(-1)
            nr.append((len(idx), int(ct[idx].sum())))
        per_model.append(nr)
    for nr in per_model:
        for n, r in nr:
            pairs += 1
            hist[(n, r)] += 1
            if r > 0:
                live += 1; rows += n; dup += max(0, n - r - 1)
    for grp in GROUPS:
        for step in range(max(len(per_model[k]) for k in grp)):
            mem = [per_model[k][step] for k in grp if step < len(per_model[k])]
            mem = [(n, r) for n, r in mem if r > 0]                  # a dead member's workgroups return at once
            if not mem:
                continue
            launches += 1
            cus = 256 // len(grp)
            comp = [(n, r + (1 if n > r else 0)) for n, r in mem]
            w_before += max(n for n, _ in comp); w_after += max(m for _, m in comp)
            d_before += max(-(-n * TPS // cus) for n, _ in comp); d_after += max(-(-m * TPS // cus) for _, m in comp)
print("(model, step) pairs", pairs, "live (at least one CT)", live)
print("full batches of %d by samples with a CT:" % B, {r: hist[(B, r)] for r in range(B + 1)})
print("ragged tails:", {k: v for k, v in sorted(hist.items()) if k[0] != B})
print("live pairs: sample-volumes %d, repeating another absent sample of the batch %d (%.1f %%)" % (rows, dup, 100.0 * dup / rows))
print("live launches of the sub-groups 2 + 2 + 1:", launches)
print("  weight gradient, rows of the slowest member: %.3f of today's" % (w_after / w_before))
print("  backward-data, tile rounds of the slowest CU: %.3f of today's" % (d_after / d_before))
