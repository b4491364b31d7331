"""Fraction of conv0's boxes whose staged input region is all zero (MmsDnOpts.c0_zero_skip) over one training epoch of bench.py's flagship
workload: the cohort, folds and training sets bench.py builds, on the CPU (no GPU, no loaders: every training patient of a fold is seen
once per epoch, so the shuffle does not enter).
    python tools/conv0_zero_fraction.py"""
import os, sys, math, numpy as np, torch, torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_survival_prediction_amd import data
B, dims, K = 4, (64, 64, 32), 5
c = data.make_cohort(n=608, dims=dims, rna_dim=5005, seed=608, complete=False)
img = c["image"]
print("image", tuple(img.shape), "mask cols", tuple(c["mask"].shape))
x = img.reshape(608, 1, *dims).abs()
xp = F.pad(x, (3, 3, 3, 3, 3, 3))
zf = (F.max_pool3d(xp, (13, 13, 13), stride=8) == 0).flatten(1)        # forward boxes
zw = (F.max_pool3d(xp, (9, 13, 13), stride=(4, 8, 8)) == 0).flatten(1)  # weight-gradient boxes
print("boxes per sample", zf.shape[1], zw.shape[1])
present = (x.flatten(1).amax(1) > 0)
print("patients with a non-zero volume", int(present.sum()), "mask says", int((c["mask"][:, 0] > 0).sum()))
print("zero boxes inside present volumes: fwd %.4f wgrad %.4f" % (float(zf[present].float().mean()), float(zw[present].float().mean())))
has = c["has_survival"].numpy()
surv, non = np.nonzero(has)[0], np.nonzero(~has)[0]
folds = data.kfold_indices(len(surv), K, seed=42)
tr = [np.concatenate([surv[f[0]], non]) for f in folds]
tot = sum(len(t) for t in tr)
nf = sum(float(zf[t].float().sum()) for t in tr); nw = sum(float(zw[t].float().sum()) for t in tr)
print("training patients per epoch", tot, "with CT", sum(int(present[t].sum()) for t in tr))
print("zero fraction over the epoch: fwd %.4f (%d of %d)  wgrad %.4f (%d of %d)" % (nf / (tot * zf.shape[1]), nf, tot * zf.shape[1], nw / (tot * zw.shape[1]), nw, tot * zw.shape[1]))
print("steps per epoch", max(math.ceil(len(t) / B) for t in tr), [len(t) for t in tr])
