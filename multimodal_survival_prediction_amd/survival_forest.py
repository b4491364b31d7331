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
    repeats in time-descending order (the stable order of risk_sets.descending_groups).
Permutation importance (include/mmsurv.h: RsfVimpP) adds, per tree and repeat r, over the ROWS i of the matrix handed in:
    hp = h((r + 1) * 0x85EBCA6B + h(ht ^ 0x68E31DA4)),   k_i = h((i + 1) * 0x9E3779B9 + hp);
    the rows the tree admits, ascending, receive the same rows sorted by (k, i) as donors; any other row is its own donor."""
from dataclasses import dataclass, field

import numpy as np

from .risk_sets import descending_groups, to_numpy

GOLDEN, STREAM, DRAW, PERMUTE = 0x9E3779B9, 0x85EBCA6B, 0xB5297A4D, 0x68E31DA4
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


def _hash_t(x):
    """hash_u32 on torch int64 tensors holding uint32 values (products wrap mod 2^64, which keeps the low 32 bits)"""
    x = x & 0xFFFFFFFF
    x = x ^ (x >> 16); x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x = x ^ (x >> 15); x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def permutation_donors(seed, tree_ids, use, nperm):
    """-> int32 [R, T, n] donor rows of R = nperm repeats (the contract: include/mmsurv.h, RsfVimpP): within each tree's admitted rows
    (use [T, n] != 0) a permutation keyed by (seed, tree id, repeat), the identity elsewhere.  Computed with torch on use's device --
    int64 arithmetic masked to 32 bits and two stable sorts; a device tensor when use is one, else a numpy array."""
    import torch
    as_numpy = not torch.is_tensor(use)
    use = torch.as_tensor(np.ascontiguousarray(to_numpy(use)) != 0) if as_numpy else use != 0
    T, n = use.shape
    R = int(nperm)
    ids = np.asarray(tree_ids, np.int64).reshape(-1)
    if len(ids) != T or R < 1:
        raise ValueError("one tree id per row of use, and at least one repeat")
    hp = hash_u32(((np.arange(1, R + 1, dtype=np.uint64)[:, None] * np.uint64(STREAM)) & _M32)
                  + hash_u32(tree_key(seed, ids) ^ np.uint64(PERMUTE))[None, :])                     # [R, T] (hash_u32 masks its input)
    dev = use.device
    hp = torch.from_numpy(hp.astype(np.int64)).to(dev)
    k = _hash_t(torch.arange(1, n + 1, dtype=torch.int64, device=dev) * GOLDEN + hp[:, :, None])     # [R, T, n]
    by_key = torch.sort(torch.where(use[None], k, torch.full_like(k, 1 << 32)), dim=2, stable=True).indices      # s_0, s_1, ..., then the rest
    rows = torch.sort((~use).to(torch.uint8), dim=1, stable=True).indices                             # a_0, a_1, ..., then the rest
    donor = torch.empty(R, T, n, dtype=torch.int64, device=dev)
    donor.scatter_(2, rows[None].expand(R, T, n), by_key)
    donor = donor.to(torch.int32)
    return donor.numpy() if as_numpy else donor


def problem_table(feat, sets=None, p=None):
    """The (set, gene) problems of the forest tables feat [T, nn] (a tensor on any device, or an array): every pair for which some tree of
    the set (sets [T], None: one set) splits on the gene at some node, sorted by (set, gene), with its trees ascending and without
    repeats.  -> dict(set, gene [P], off [P + 1], tree [off[P]]) int32 tensors on feat's device."""
    import torch
    feat = torch.as_tensor(to_numpy(feat)) if not torch.is_tensor(feat) else feat
    T = feat.shape[0]
    dev = feat.device
    p = int(p) if p is not None else (int(feat.max()) + 1 if feat.numel() else 1)
    sets_t = torch.zeros(T, dtype=torch.int64, device=dev) if sets is None else torch.as_tensor(np.asarray(to_numpy(sets), np.int64)).to(dev)
    t, s = torch.nonzero(feat >= 0, as_tuple=True)
    key = torch.unique((sets_t[t] * max(p, 1) + feat[t, s].to(torch.int64)) * max(T, 1) + t)           # sorted, one per (set, gene, tree)
    prob, count = torch.unique_consecutive(torch.div(key, max(T, 1), rounding_mode="floor"), return_counts=True)
    off = torch.zeros(len(prob) + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(count, 0)
    i32 = lambda a: a.to(torch.int32)
    return dict(set=i32(torch.div(prob, max(p, 1), rounding_mode="floor")), gene=i32(prob % max(p, 1)), off=i32(off), tree=i32(key % max(T, 1)))


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

    def vimp(self, x, time, event, use, sets=None, nperm=1, return_delta=False, timings=None):
        """Out-of-bag permutation importance (ensemble VIMP; include/mmsurv.h: RsfVimpP): the drop in the C-index of the rows `use` admits
        when a gene's values are shuffled among each tree's admitted rows, all (set, gene, repeat) problems in ONE launch.
        x: fp32 [n, p] device matrix; time / event: [n] of its rows; use: [T, n] mask (the out-of-bag rows of every tree, or a
        validation mask); sets: [T] the set (fold) of each tree, None = one set: a set's C-index is over ITS trees' predictions.
        -> dict(vimp [F, p] = c_base - the mean over repeats, vimp_reps [F, R, p], c_base [F], conc2 / comparable int64 [P, R] and
        base_conc2 / base_comparable [F] (when a launch ran), problems = dict(set, gene [P], off [P + 1], tree), n_rows [F] rows some tree admits; with
        return_delta also D and M float64 [P, R, n]).  A gene no tree of a set splits on has importance exactly 0.0 and no problem.
        ValueError when a set has no comparable pair among its admitted rows.  timings: a list that receives (name, milliseconds)."""
        import time as _time
        import torch
        from . import ops
        from .survival_stats import concordance_index
        dev = x.device
        n, T, R = int(x.shape[0]), self.n_trees, int(nperm)
        tm, ev = to_numpy(time, "time").astype(np.float64).reshape(-1), to_numpy(event).reshape(-1) != 0
        use = torch.as_tensor(np.ascontiguousarray(to_numpy(use)).astype(np.uint8) if not torch.is_tensor(use) else use)
        use = (use.to(dev) != 0).to(torch.uint8).contiguous()
        sets = np.zeros(T, np.int64) if sets is None else np.asarray(to_numpy(sets), np.int64).reshape(-1)
        if tuple(use.shape) != (T, n) or len(tm) != n or len(ev) != n or len(sets) != T or (T and sets.min() < 0):
            raise ValueError("use must be [T, n], time / event [n] and sets [T] for x [n, p]")
        F = int(sets.max()) + 1 if T else 1
        sets_d = torch.from_numpy(sets).to(dev)
        M0, cnt = torch.zeros(F, n, dtype=torch.float64, device=dev), torch.zeros(F, n, dtype=torch.int32, device=dev)
        for f in range(F):                                          # what mms_rsf_predict returns for the set's trees and the mask
            m, _, c = ops.rsf_predict(x, self.feat, self.thr, self.mort, self.H.contiguous(), use=use * (sets_d == f).to(torch.uint8)[:, None])
            M0[f], cnt[f] = m, c
        cnt_h = cnt.cpu().numpy()
        order, _, gid, _, _ = descending_groups(tm)
        tg = np.empty(n, np.int32); tg[order] = gid                 # per row; a larger number is a shorter time
        t0 = _time.perf_counter()
        prob = problem_table(self.feat, sets, self.p)
        P = len(prob["set"])
        out = dict(vimp=np.zeros((F, self.p)), vimp_reps=np.zeros((F, R, self.p)), n_rows=(cnt_h > 0).sum(1),
                   problems={k: v.cpu().numpy() for k, v in prob.items()})
        if P == 0:                                                  # stumps: nothing to permute and nothing to launch
            M0_h = M0.cpu().numpy()
            try:
                out["c_base"] = np.array([concordance_index(tm[cnt_h[f] > 0], -M0_h[f][cnt_h[f] > 0], ev[cnt_h[f] > 0]) for f in range(F)])
            except ZeroDivisionError:
                raise ValueError("a set has no comparable pair among its admitted rows") from None
            out.update(conc2=np.zeros((0, R), np.int64), comparable=np.zeros((0, R), np.int64))
            if return_delta:
                out.update(D=np.zeros((0, R, n)), M=np.zeros((0, R, n)))
            return out
        ids = self.tree_id if self.tree_id is not None else np.arange(T)
        donor = permutation_donors(self.hyper.get("seed", 0), ids, use, R)
        # the base C-index rides in the launch: F more problems with an empty tree list count M0 itself
        i32 = lambda a: torch.as_tensor(a, dtype=torch.int32, device=dev)
        pset, pgene = torch.cat([prob["set"], i32(np.arange(F))]), torch.cat([prob["gene"], i32(np.zeros(F))])
        poff = torch.cat([prob["off"], prob["off"][-1:].expand(F)])
        if timings is not None:
            torch.cuda.synchronize()
            timings.append(("tables", (_time.perf_counter() - t0) * 1e3))
        args = (x, self.feat, self.thr, self.mort, use, donor, M0, cnt, i32(ev.astype(np.int32)), i32(tg), pset, pgene, poff, prob["tree"])
        if timings is None:
            got = ops.rsf_vimp(*args, delta=return_delta)
        else:
            plan = ops.rsf_vimp(*args, delta=return_delta, plan_only=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.call("mms_rsf_vimp", plan[0])
            e1.record()
            e1.synchronize()
            timings.append(("launch", e0.elapsed_time(e1)))
            got = plan[2]
        got = {k: v.cpu().numpy() for k, v in got.items()}
        conc2, comp = got["conc2"], got["comparable"]
        if (comp[P:, 0] == 0).any():
            raise ValueError("a set has no comparable pair among its admitted rows")
        c_base = conc2[P:, 0] / (2.0 * comp[P:, 0])
        ps, pg = out["problems"]["set"], out["problems"]["gene"]
        total = np.zeros(P)
        for r in range(R):                                          # the mean over repeats: a sequential sum, then one division
            c_perm = conc2[:P, r] / (2.0 * comp[:P, r])
            out["vimp_reps"][ps, r, pg] = c_base[ps] - c_perm
            total = total + c_perm
        out["vimp"][ps, pg] = c_base[ps] - total / R
        out.update(c_base=c_base, conc2=conc2[:P], comparable=comp[:P], base_conc2=conc2[P:, 0], base_comparable=comp[P:, 0])
        if return_delta:
            out.update(D=got["D"][:P], M=got["M"][:P])
        return out

    def shap(self, x, use=None, sets=None, trees=None, timings=None):
        """Path-dependent TreeSHAP of the ensemble mortality for the rows x: fp32 [R, p] device.  use: [T, R] mask as in predict (None:
        every tree); sets: [T] the set (fold) of each tree, None = one set: one group per set 0..max, over ITS trees; trees: an index
        array of the trees that take part (None = all, as in importance; use and sets stay indexed by the forest's trees).  A
        contiguous run of trees is read in place, anything else is gathered.  The kernel's sums are divided by the admitted-tree
        count (the set's tree count, or use.sum(0) over its trees); NaN where that is 0, as in predict.
        -> tree_shap.ShapValues with one group per set: base[g] + phi[g].sum(1) == predict(x, use)["mortality"] to rounding when the
        set holds all trees.  timings: receives ("launch", milliseconds)."""
        import torch
        from . import tree_shap
        T, R, dev = self.n_trees, int(x.shape[0]), x.device
        sets = np.zeros(T, np.int64) if sets is None else np.asarray(to_numpy(sets), np.int64).reshape(-1)
        idx = np.arange(T) if trees is None else np.asarray(trees, np.int64).reshape(-1)
        if len(sets) != T or (T and sets.min() < 0) or (len(idx) and (idx.min() < 0 or idx.max() >= T)):
            raise ValueError("sets must name one set >= 0 per tree and trees lie in 0..%d" % (T - 1))
        G = int(sets[idx].max()) + 1 if len(idx) else 1
        order = idx[np.argsort(sets[idx], kind="stable")]
        goff = np.concatenate([[0], np.cumsum(np.bincount(sets[idx], minlength=G))])
        if len(order) and (order == np.arange(order[0], order[0] + len(order))).all():
            take = slice(int(order[0]), int(order[0]) + len(order))                     # a view: nothing is copied or uploaded
        else:
            take = torch.from_numpy(order).to(dev)
        tab = [t[take].contiguous() for t in (self.feat, self.thr, self.mort, self.n_node)]
        if use is not None:
            use = torch.as_tensor(np.ascontiguousarray(to_numpy(use)).astype(np.uint8) if not torch.is_tensor(use) else use)
            use = (use.to(dev) != 0).to(torch.uint8)
            if tuple(use.shape) != (T, R):
                raise ValueError("use must be [T, R]")
            use = use[take].contiguous()
            count = torch.stack([use[goff[g]:goff[g + 1]].sum(0, dtype=torch.int64) for g in range(G)]).cpu().numpy()
        else:
            count = np.repeat(np.diff(goff)[:, None], R, axis=1)
        phi, base, genes = tree_shap.launch(x, *tab, goff, use=use, timings=timings)
        return tree_shap.from_launch(phi, base, genes, count=count)

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


def cross_validate(cohort, folds, n_trees=500, *, mtry=None, nsplit=10, min_leaf=15, max_depth=10, seed=0, horizons=None, x=None, vimp=0, shap=False):
    """K-fold cross-validation of the forest: all K * n_trees trees grow in ONE launch sequence (one per fold when the cohort carries
    per-fold gene matrices, gene_select.fold_matrix; the trees keep their forest-wide hash streams).  Rows: coxnet.risk_rows(cohort),
    the eligible patients.  Higher mortality = higher risk: C = survival_stats.concordance_index(time, -mortality, event).
    -> list per fold of dict(fold, c_index, oob_c_index, oob_missing (training rows no tree left out), val_rows, val_mortality,
    val_survival [n_val, nh], horizons, importance = (counts, chi2 sums) of the fold's trees, n_train, n_val, forest, trees).
    vimp = R > 0 adds the out-of-bag permutation importance of every fold over its own trees (Forest.vimp, R repeats; one launch for all
    folds, one per fold with per-fold matrices): vimp float64 [p] and vimp_reps [R, p].
    shap=True adds `shap`: the TreeSHAP values (Forest.shap -> tree_shap.ShapValues, one group) of the fold's own trees on that fold's
    VALIDATION rows only (Forest.shap(trees=the fold's)), in val_rows' order: out-of-fold, so honest; one launch per fold."""
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
        vi = forest.vimp(xe, rr.time, rr.event, oob, sets=np.repeat(np.arange(len(grp)), T), nperm=int(vimp)) if int(vimp) > 0 else None
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
            if vi is not None:
                results[f].update(vimp=vi["vimp"][i], vimp_reps=vi["vimp_reps"][i])
            if shap:
                results[f]["shap"] = forest.shap(xe[torch.as_tensor(va, device=xe.device)].contiguous(), trees=np.arange(i * T, (i + 1) * T))
    return results
