"""Random survival forest (Ishwaran et al. 2008) as the nonlinear, non-deep baseline: all trees of a cross-validation in lock-step.

The K T trees of a K-fold cross-validation read ONE patient x gene matrix and differ only in their multiplicity vectors (a bootstrap
sample of the fold's training patients: 0 = out of bag, > 1 = a repeat, which counts as a separate subject) and their hash streams.  They
grow level by level together: one launch per level scores mtry * nsplit random (gene, threshold) candidates of every live node of every
tree with the two-group log-rank statistic, keeps the best and routes the node's patients to its children (include/mmsurv.h: RsfSplitP;
csrc/rsf.hip).  One more launch turns every leaf into a Nelson-Aalen cumulative hazard H -- kept as the ensemble mortality (the sum of H
over the distinct event times of the tree's own training set) and as H at the caller's horizons -- and one launch drops rows down all
trees and averages over the trees a byte mask admits (out-of-bag and fold-validation prediction are two masks).  There is no CPU
fallback.

The hash contract (restated in tests/rsf_ref.py, which replicates all of this in numpy): with h = csrc/common.h's hash_u32 and
mulhi(a, k) = (a * k) >> 32,
    tree key  ht = h(seed ^ (id * 0x85ebca6b))              id = the tree's number in the whole forest (fold * T + j)
    draw k    of a bootstrap sample of m patients: member mulhi(h((k + 1) * 0x9E3779B9 + h(ht ^ 0xB5297A4D)), m), k = 0..m-1
    node key  hn = h((s + 1) * 0x9E3779B9 + ht),   feature j: hf = h((j + 1) * 0x9E3779B9 + hn), f = mulhi(hf, p)
    threshold q of feature j: x[f] of the node's in-bag member mulhi(h((q + 1) * 0x85ebca6b + hf), members), members counted without
    repeats in time-descending order (the stable order of risk_sets.descending_groups)."""
from dataclasses import dataclass, field

import numpy as np

from .risk_sets import descending_groups, to_numpy

GOLDEN, STREAM, DRAW = 0x9E3779B9, 0x85EBCA6B, 0xB5297A4D
_M32 = np.uint64(0xFFFFFFFF)


def hash_u32(x):
    """csrc/common.h hash_u32 on uint32 arrays (computed in uint64, masked)"""
    x = np.asarray(x, dtype=np.uint64) & _M32
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def tree_key(seed, tree_id):
    return hash_u32((np.uint64(int(seed) & 0xFFFFFFFF)) ^ ((np.asarray(tree_id, dtype=np.uint64) * np.uint64(STREAM)) & _M32))


def bootstrap_draws(seed, tree_id, m):
    """The m draws (members 0..m-1 of a training set of m patients) of tree `tree_id`."""
    k = np.arange(int(m), dtype=np.uint64)
    h = hash_u32(((k + np.uint64(1)) * np.uint64(GOLDEN) + hash_u32(tree_key(seed, tree_id) ^ np.uint64(DRAW))) & _M32)
    return ((h * np.uint64(int(m))) >> np.uint64(32)).astype(np.int64)


def bootstrap_mults(folds, n, n_trees, seed=0):
    """-> uint8 [K * n_trees, n]: tree fold * n_trees + j draws len(train) patients with replacement from fold `fold`'s training rows
    (folds: [(train, val)] or [train] index arrays into 0..n-1); every other row is 0.  A multiplicity above 255 raises."""
    K, T = len(folds), int(n_trees)
    out = np.zeros((K * T, int(n)), dtype=np.uint8)
    for f, fold in enumerate(folds):
        tr = np.asarray(fold[0] if isinstance(fold, (tuple, list)) and len(fold) == 2 and np.ndim(fold[0]) == 1 else fold, dtype=np.int64)
        if len(tr) == 0:
            raise ValueError("fold %d has no training row" % f)
        for j in range(T):
            cnt = np.bincount(tr[bootstrap_draws(seed, f * T + j, len(tr))], minlength=int(n))
            if cnt.max() > 255:
                raise ValueError("a bootstrap multiplicity above 255")
            out[f * T + j] = cnt
    return out


def mortality_weights(time, event, masks):
    """weight[w][i] = the number of distinct event times of training set w (masks [F, n] bool) that are >= time[i]"""
    time, event = np.asarray(time, np.float64), np.asarray(event) != 0
    out = np.zeros((len(masks), len(time)))
    for w, mk in enumerate(masks):
        u = np.unique(time[np.asarray(mk, bool) & event])
        out[w] = len(u) - np.searchsorted(u, time, side="left")
    return out


@dataclass
class Forest:
    feat: object              # int32 [T, nn] device: split feature, -1 = leaf or absent
    thr: object               # float32 [T, nn]
    stat: object              # float64 [T, nn] the winning chi2
    n_node: object            # int32 [T, nn] weighted patients
    d_node: object            # int32 [T, nn] weighted events
    mort: object              # float64 [T, nn] leaf mortality
    H: object                 # float64 [T, nn, nh] leaf cumulative hazard at the horizons
    horizons: np.ndarray
    p: int
    hyper: dict = field(default_factory=dict)      # mtry, nsplit, min_leaf, max_depth, seed
    tree_id: np.ndarray = None
    node: object = None       # int32 [T, n] the final node of every in-bag training row, in the rows' order of fit (not saved)

    @property
    def n_trees(self):
        return int(self.feat.shape[0])

    def predict(self, x, use=None):
        """x: fp32 [R, p] device matrix; use: [T, R] mask (bool / uint8; host or device) of the trees each row may use, None = all.
        -> dict(mortality [R], survival [R, nh] = exp(-H), hazard [R, nh], count [R]) numpy; NaN where no tree is admitted."""
        import torch
        from . import ops
        if use is not None:
            use = torch.as_tensor(np.ascontiguousarray(to_numpy(use)).astype(np.uint8) if not torch.is_tensor(use) else use)
            use = use.to(device=x.device, dtype=torch.uint8).contiguous()
        m, H, c = ops.rsf_predict(x, self.feat, self.thr, self.mort, self.H.contiguous(), use=use)
        H = H.cpu().numpy()
        return dict(mortality=m.cpu().numpy(), hazard=H, survival=np.exp(-H), count=c.cpu().numpy())

    def importance(self, trees=None):
        """-> (split counts int64 [p], summed chi2 float64 [p]) over the trees (`trees`: an index array, None = all), from the tables."""
        feat, stat = to_numpy(self.feat), to_numpy(self.stat)
        if trees is not None:
            feat, stat = feat[np.asarray(trees)], stat[np.asarray(trees)]
        ok = feat >= 0
        return (np.bincount(feat[ok], minlength=self.p).astype(np.int64), np.bincount(feat[ok], weights=stat[ok], minlength=self.p))

    def save(self, path):
        np.savez(path, **{k: to_numpy(getattr(self, k)) for k in ("feat", "thr", "stat", "n_node", "d_node", "mort", "H")},
                 horizons=np.asarray(self.horizons, np.float64), p=np.int64(self.p),
                 tree_id=np.asarray(self.tree_id if self.tree_id is not None else np.arange(self.n_trees), np.int64),
                 hyper_keys=np.array(sorted(self.hyper)), hyper_values=np.array([int(self.hyper[k]) for k in sorted(self.hyper)], np.int64))


def load(path, device="cuda"):
    import torch
    with np.load(path if str(path).endswith(".npz") else str(path) + ".npz") as z:
        t = {k: torch.from_numpy(z[k]).to(device) for k in ("feat", "thr", "stat", "n_node", "d_node", "mort", "H")}
        return Forest(**t, horizons=z["horizons"], p=int(z["p"]), tree_id=z["tree_id"],
                      hyper={str(k): int(v) for k, v in zip(z["hyper_keys"], z["hyper_values"])})


def save(forest, path):
    forest.save(path)


def fit(x, time, event, mults, *, mtry=None, nsplit=10, min_leaf=15, max_depth=10, seed=0, horizons=None, train_sets=None, tree_ids=None,
        candidates_level=None, timings=None):
    """Grow len(mults) trees in lock-step.  x: fp32 [n, p] device matrix; time / event: [n]; mults: [T, n] multiplicities 0..255 over
    x's rows.  train_sets = (masks bool [F, n], set int [T]): the training set whose distinct event times each tree's mortality sums
    over (None: one set, every row).  tree_ids: the hash stream of each tree (None: 0..T-1).  horizons: up to 32 times.
    candidates_level = L: stop after level L and also return that launch's candidate tables (tests).  timings: a list that receives
    (launch name, milliseconds) of every launch, from HIP events (tools/bench_rsf.py; it synchronises after each).  -> Forest (, tables)."""
    import torch
    from . import _lib, ops
    lim = _lib.defines("MMS_RSF_")
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise TypeError("x must be a float32 [n, p] device tensor")
    n, p = int(x.shape[0]), int(x.shape[1])
    time, ev = to_numpy(time, "time").astype(np.float64).reshape(-1), to_numpy(event).reshape(-1) != 0
    mults = np.asarray(to_numpy(mults))
    if mults.ndim != 2 or mults.shape[1] != n or len(time) != n or len(ev) != n:
        raise ValueError("time / event must be [n] and mults [T, n] for x [n, p]")
    if mults.size and (mults.min() < 0 or mults.max() > 255):
        raise ValueError("multiplicities must lie in 0..255")
    T = len(mults)
    mtry = int(np.ceil(np.sqrt(p))) if mtry is None else int(mtry)
    nsplit, min_leaf, max_depth = int(nsplit), int(min_leaf), int(max_depth)
    if not (1 <= n <= lim["MAX_N"]) or not (0 <= max_depth <= lim["MAX_DEPTH"]) or T > lim["MAX_T"]:
        raise ValueError("n must be in 1..%d, max_depth in 0..%d, trees <= %d" % (lim["MAX_N"], lim["MAX_DEPTH"], lim["MAX_T"]))
    if mtry < 1 or nsplit < 1 or min_leaf < 1 or mtry * nsplit > lim["MAX_C"]:
        raise ValueError("mtry, nsplit, min_leaf must be >= 1 and mtry * nsplit <= %d" % lim["MAX_C"])
    horizons = np.zeros(0) if horizons is None else np.asarray(horizons, np.float64).reshape(-1)
    if len(horizons) > lim["MAX_H"]:
        raise ValueError("at most %d horizons" % lim["MAX_H"])
    ids = np.arange(T, dtype=np.int64) if tree_ids is None else np.asarray(tree_ids, np.int64).reshape(-1)
    if len(ids) != T:
        raise ValueError("tree_ids must name one hash stream per tree")
    if train_sets is None:
        masks, wset = np.ones((1, n), bool), np.zeros(T, np.int64)
    else:
        masks, wset = np.asarray(train_sets[0], bool).reshape(-1, n), np.asarray(train_sets[1], np.int64).reshape(-1)
        if len(wset) != T or (T and (wset.min() < 0 or wset.max() >= len(masks))):
            raise ValueError("train_sets = (masks [F, n], one set index per tree)")
    dev = x.device
    order, _, gid, _, _ = descending_groups(time)
    inv = np.empty(n, np.int64); inv[order] = np.arange(n)
    od = torch.from_numpy(order).to(dev)
    xt = x[od].t().contiguous()                                     # feature-major [p, n] in position order, built once
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dt)
    mult_d = up(mults[:, order].astype(np.uint8), torch.uint8).reshape(T, n)
    event_d, tgroup_d = up(ev[order].astype(np.int32), torch.int32), up(gid.astype(np.int32), torch.int32)
    tid_d = up(ids.astype(np.int32), torch.int32)
    nn = (2 << max_depth) - 1
    node = torch.zeros(T, n, dtype=torch.int32, device=dev)
    tab = dict(feat=torch.full((T, nn), -1, dtype=torch.int32, device=dev), thr=torch.zeros(T, nn, dtype=torch.float32, device=dev),
               stat=torch.zeros(T, nn, dtype=torch.float64, device=dev), n_node=torch.zeros(T, nn, dtype=torch.int32, device=dev),
               d_node=torch.zeros(T, nn, dtype=torch.int32, device=dev))
    cand = None

    def timed(name, fn):
        if timings is None:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        timings.append((name, e0.elapsed_time(e1)))
        return out

    if max_depth == 0 and T:                                        # stumps without a split launch: the root's counts on the host
        tab["n_node"][:, 0] = up(mults.sum(1).astype(np.int32), torch.int32)
        tab["d_node"][:, 0] = up((mults * ev[None, :]).sum(1).astype(np.int32), torch.int32)
    for level in range(max_depth):
        want = candidates_level is not None and level == int(candidates_level)
        c = timed("split_level_%d" % level, lambda: ops.rsf_split(xt, mult_d, event_d, tgroup_d, node, tab, level, mtry, nsplit, min_leaf, seed,
                                                                   tree_id=tid_d, candidates=want))
        if want:
            cand = c
            break
        lo = (1 << level) - 1
        if T == 0 or not bool((tab["feat"][:, lo:2 * lo + 1] >= 0).any()):     # no node of the level split: the trees are complete
            break
    weight = mortality_weights(time[order], ev[order], masks[:, order])
    hpos = np.array([(time > h).sum() for h in horizons], dtype=np.int32)
    weight_d, wset_d, hpos_d = up(weight, torch.float64).reshape(len(masks), n), up(wset.astype(np.int32), torch.int32), up(hpos, torch.int32)
    mort, H = timed("leaves", lambda: ops.rsf_leaves(mult_d, event_d, tgroup_d, node, tab["feat"], tab["n_node"], weight_d, wset_d, hpos_d))
    forest = Forest(tab["feat"], tab["thr"], tab["stat"], tab["n_node"], tab["d_node"], mort, H.contiguous(), horizons, p,
                    dict(mtry=mtry, nsplit=nsplit, min_leaf=min_leaf, max_depth=max_depth, seed=int(seed)), ids,
                    node[:, torch.from_numpy(inv).to(dev)] if T else node)
    return (forest, cand) if candidates_level is not None else forest


def default_horizons(time, event, k=3):
    """k horizons at equally spaced quantiles of the observed event times (the quartiles for k = 3)"""
    t = np.asarray(time, np.float64)[np.asarray(event) != 0]
    return np.unique(np.quantile(t, np.arange(1, k + 1) / (k + 1.0))) if len(t) else np.zeros(0)      # (ties may merge two)


def cross_validate(cohort, folds, n_trees=500, *, mtry=None, nsplit=10, min_leaf=15, max_depth=10, seed=0, horizons=None, x=None):
    """K-fold cross-validation of the forest: all K * n_trees trees grow in ONE launch sequence (one per fold when the cohort carries
    per-fold gene matrices, gene_select.fold_matrix; the trees keep their forest-wide hash streams).  Rows: coxnet.risk_rows(cohort),
    the eligible patients.  Higher mortality = higher risk: C = survival_stats.concordance_index(time, -mortality, event).
    -> list per fold of dict(fold, c_index, oob_c_index, oob_missing (training rows no tree left out), val_rows, val_mortality,
    val_survival [n_val, nh], horizons, importance = (counts, chi2 sums) of the fold's trees, n_train, n_val, forest, trees)."""
    import torch
    from . import coxnet, gene_select
    from .survival_stats import concordance_index
    rr = coxnet.risk_rows(cohort)
    n, K, T = len(rr), len(folds), int(n_trees)
    N = int(to_numpy(cohort["label"]).shape[0])
    pos = [(rr.positions(gene_select.eligible_rows(cohort, tr), N), rr.positions(gene_select.eligible_rows(cohort, va), N)) for tr, va in folds]
    mults = bootstrap_mults([p[0] for p in pos], n, T, seed)
    masks = np.zeros((K, n), bool)
    for f, (tr, _) in enumerate(pos):
        masks[f, tr] = True
    tree_fold = np.repeat(np.arange(K), T)
    horizons = default_horizons(rr.time, rr.event) if horizons is None else np.asarray(horizons, np.float64)
    per_fold = "rnaseq_folds" in cohort and x is None
    groups = [[f] for f in range(K)] if per_fold else [list(range(K))]
    kw = dict(mtry=mtry, nsplit=nsplit, min_leaf=min_leaf, max_depth=max_depth, seed=seed, horizons=horizons)
    results = [None] * K
    for grp in groups:
        xg = gene_select.fold_matrix(cohort, grp[0] if per_fold else None) if x is None else x
        xe = xg[torch.as_tensor(rr.rows, device=xg.device)].contiguous()
        trees = np.concatenate([np.arange(f * T, (f + 1) * T) for f in grp])
        forest = fit(xe, rr.time, rr.event, mults[trees], train_sets=(masks, tree_fold[trees]), tree_ids=trees, **kw)
        val = np.zeros((len(trees), n), np.uint8)
        for i, f in enumerate(grp):
            val[i * T:(i + 1) * T, pos[f][1]] = 1
        oob = ((mults[trees] == 0) & masks[tree_fold[trees]]).astype(np.uint8)
        pv = forest.predict(xe, use=val)
        for i, f in enumerate(grp):
            tr, va = pos[f]
            use = np.zeros_like(oob)                                # fold f's out-of-bag mean is over fold f's trees alone
            use[i * T:(i + 1) * T] = oob[i * T:(i + 1) * T]
            om = forest.predict(xe, use=use)["mortality"][tr]
            ok = ~np.isnan(om)
            results[f] = dict(fold=f, c_index=float(concordance_index(rr.time[va], -pv["mortality"][va], rr.event[va])),
                              oob_c_index=float(concordance_index(rr.time[tr][ok], -om[ok], rr.event[tr][ok])) if ok.sum() > 1 else float("nan"),
                              oob_missing=int((~ok).sum()), val_rows=rr.rows[va], val_mortality=pv["mortality"][va],
                              val_survival=pv["survival"][va], horizons=horizons, importance=forest.importance(np.arange(i * T, (i + 1) * T)),
                              n_train=int(len(tr)), n_val=int(len(va)), forest=forest, trees=np.arange(i * T, (i + 1) * T))
    return results
