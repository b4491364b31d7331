"""TreeSHAP of the two tree baselines: which genes pushed ONE patient's prediction up or down, and by how much.

Booster.importance and Forest.importance / vimp are global and unsigned.  The path-dependent Shapley values (Lundberg et al. 2018/2020,
Algorithm 2's value function; the contract: include/mmsurv.h, TreeShapP; the kernel: csrc/tree_shap.hip; the numpy replica:
tests/tree_shap_ref.py) split a row's prediction into base + sum_g phi_g.  For the boosted Cox trees F = base + sum phi is a log-hazard,
so exp(phi_g) is gene g's hazard-ratio multiplier for that patient; for the forest the same holds for the ensemble mortality.

Both baselines keep heap-indexed [T, nn] tables feat / thr / leaf value / cover and route with x[feat] <= thr -> left, so ONE kernel
serves both: Booster.shap and Forest.shap gather their trees into groups (one per problem / per set) and call ops.tree_shap.  This
module holds the host-side pieces that need no GPU: the output columns of a group (slots), the table checks the launch cannot make,
and the result type."""
from dataclasses import dataclass

import numpy as np

from .risk_sets import to_numpy


def split_nodes(feat):
    """feat [T, nn] (numpy or torch) -> bool [T, (nn - 1) // 2]: node s splits (feat >= 0 and both children exist, 2s + 2 < nn)"""
    ns = (feat.shape[1] - 1) // 2
    return feat[:, :ns] >= 0


def check_tables(feat, cover):
    """The cover rule of the TreeSHAP contract, on numpy arrays or torch tensors [T, nn]: at every split node both children's covers
    are > 0 and sum to the node's (z = cover[child] / cover[node] is the kernel's only division).  ValueError otherwise."""
    split = split_nodes(feat)
    ns = split.shape[1]
    if ns == 0:
        return
    wide = (lambda a: a.long()) if hasattr(cover, "long") else (lambda a: a.astype(np.int64))
    left, right, node = wide(cover[:, 1:2 * ns + 1:2]), wide(cover[:, 2:2 * ns + 1:2]), wide(cover[:, :ns])
    bad = split & ((left <= 0) | (right <= 0) | (left + right != node))
    if bool(bad.any()):
        raise ValueError("the covers of a split node's children must be > 0 and sum to the node's (%d nodes do not)" % int(bad.sum()))


def slots(feat, goff):
    """feat [T, nn] tree tables, goff [G + 1] ascending tree offsets -> (slot int32 [T, nn], genes: list of G ascending int64 arrays).
    genes[g] = the genes group g's trees split on; slot = the position of feat in its group's genes at split nodes, 0 elsewhere.  The
    output of a launch has U = max(1, max len(genes)) columns; a group's columns past len(genes[g]) are padding (zeros)."""
    feat = np.asarray(to_numpy(feat))
    goff = np.asarray(goff, np.int64).reshape(-1)
    T, nn = feat.shape
    if len(goff) < 1 or goff[0] != 0 or goff[-1] != T or (np.diff(goff) < 0).any():
        raise ValueError("goff must ascend from 0 to T = %d" % T)
    split = np.zeros((T, nn), bool)
    split[:, :(nn - 1) // 2] = split_nodes(feat)
    slot, genes = np.zeros((T, nn), np.int32), []
    for g in range(len(goff) - 1):
        fg, sg = feat[goff[g]:goff[g + 1]], split[goff[g]:goff[g + 1]]
        genes.append(np.unique(fg[sg]).astype(np.int64))
        slot[goff[g]:goff[g + 1]][sg] = np.searchsorted(genes[-1], fg[sg])
    return slot, genes


def n_slots(genes):
    return max([1] + [len(g) for g in genes])


@dataclass
class ShapValues:
    genes: list               # per group: ascending int64 [U_g] columns of the matrix handed in
    phi: list                 # per group: float64 [R, U_g]
    base: list                # per group: float64 [R]

    def dense(self, g, p):
        """-> float64 [R, p]: phi of group g scattered to all p columns (0 for genes never split on; NaN rows stay NaN)"""
        out = np.zeros((self.phi[g].shape[0], int(p)))
        out[:, self.genes[g]] = self.phi[g]
        out[np.isnan(self.base[g])] = np.nan
        return out

    def mean_abs(self, g):
        """-> float64 [U_g]: the mean |phi| over the rows that have a value (NaN rows are skipped; no such row: 0)"""
        ok = ~np.isnan(self.base[g])
        return np.abs(self.phi[g][ok]).mean(0) if ok.any() else np.zeros(len(self.genes[g]))

    def top(self, g, row, k=10):
        """-> [(gene, phi)] the k genes with the largest |phi| of one row, largest first (ties: the lower gene first)"""
        v = self.phi[g][int(row)]
        order = np.lexsort((self.genes[g], -np.abs(v)))[:int(k)]
        return [(int(self.genes[g][i]), float(v[i])) for i in order]


def from_launch(phi, base, genes, count=None):
    """The device result of ops.tree_shap (phi [G, U, R] slot-major, base [G, R]) -> ShapValues.  count [G, R] (numpy): the sums are
    divided by it (a forest's admitted-tree count), NaN where it is 0."""
    phi, base = phi.cpu().numpy(), base.cpu().numpy()
    out = ShapValues([np.asarray(g, np.int64) for g in genes], [], [])
    for g, gg in enumerate(genes):
        ph, b = np.ascontiguousarray(phi[g, :len(gg)].T), base[g].copy()
        if count is not None:
            with np.errstate(invalid="ignore", divide="ignore"):
                c = np.asarray(count[g], np.float64)
                ph, b = np.where(c[:, None] > 0, ph / c[:, None], np.nan), np.where(c > 0, b / c, np.nan)
        out.phi.append(ph); out.base.append(b)
    return out


def write_fold(out_dir, fold, sv, patient_ids, columns=None, gene_names=None, g=0):
    """The per-fold files of gbm_baseline.py / rsf_baseline.py for group g of sv (a fold's out-of-fold values): fold_{fold}_shap.npz
    (patient_id, genes = the SOURCE columns of the values' columns, phi [R, U], base [R]) and fold_{fold}_shap_importance.csv (index,
    column, gene, mean_abs_shap, mean_shap; sorted by mean_abs_shap).  columns: the source column of every column of the fold's matrix
    (per-fold gene selection), None: the identity.  -> (source columns int64 [U], phi [R, U], base [R]): what write_pooled takes"""
    import os
    import pandas as pd
    idx = sv.genes[g]
    src = idx if columns is None else np.asarray(columns, np.int64)[idx]
    phi, base = sv.phi[g], sv.base[g]
    np.savez(os.path.join(out_dir, "fold_%d_shap.npz" % fold), patient_id=np.asarray(patient_ids), genes=src, phi=phi, base=base)
    ok = ~np.isnan(base)
    mean = phi[ok].mean(0) if ok.any() else np.zeros(len(idx))
    by = np.argsort(-sv.mean_abs(g), kind="stable")
    pd.DataFrame({"index": idx[by], "column": src[by], "gene": [str(gene_names[int(j)]) if gene_names is not None else "gene_%d" % int(j) for j in src[by]],
                  "mean_abs_shap": sv.mean_abs(g)[by], "mean_shap": mean[by]}).to_csv(os.path.join(out_dir, "fold_%d_shap_importance.csv" % fold), index=False)
    return src, phi, base


def write_pooled(out_dir, folds, p, gene_names=None):
    """shap_importance.csv (gene, score): score = the mean |phi| over ALL out-of-fold patients of all folds, a gene a fold never split on
    counting 0 for that fold's patients, patients without a value (base NaN) left out; every one of the p source genes has a row (what
    gene_set_enrichment.py --scores reads by its default column).  folds: write_fold's returns.  -> score float64 [p]"""
    import os
    import pandas as pd
    total, rows = np.zeros(int(p)), 0
    for src, phi, base in folds:
        ok = ~np.isnan(base)                                        # a patient no tree admits has no value: not in the mean
        total[src] += np.abs(phi[ok]).sum(0)
        rows += int(ok.sum())
    score = total / max(rows, 1)
    pd.DataFrame({"gene": [str(gene_names[j]) if gene_names is not None else "gene_%d" % j for j in range(int(p))], "score": score}).to_csv(
        os.path.join(out_dir, "shap_importance.csv"), index=False)
    return score


def launch(x, feat, thr, value, cover, goff, use=None, timings=None):
    """Slots, checks and one launch for device tables [T, nn] -> (phi [G, U, R], base [G, R] device, genes).  timings: a list that
    receives ("launch", milliseconds) from HIP events (tools/bench_tree_shap.py)."""
    import torch
    from . import ops
    slot, genes = slots(feat, goff)
    slot_d = torch.from_numpy(slot).to(x.device)
    U = n_slots(genes)
    if timings is None:
        phi, base = ops.tree_shap(x, feat, thr, value, cover, goff, slot_d, U, use=use)
    else:
        plan = ops.tree_shap(x, feat, thr, value, cover, goff, slot_d, U, use=use, plan_only=True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if plan[0] is not None:
            ops.call("mms_tree_shap", plan[0])
        e1.record()
        e1.synchronize()
        timings.append(("launch", e0.elapsed_time(e1)))
        phi, base = plan[2], plan[3]
    return phi, base, genes
