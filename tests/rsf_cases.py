"""The cases of the random survival forest tests and what the numpy replica (tests/rsf_ref.py) says about them -- shared by
test_cpu_survival_forest.py (which asserts on the CPU that the replica shows no ambiguous node and no pair of mortalities close enough
to flip) and test_gpu_survival_forest.py.  Each reference is computed once."""
import functools

import numpy as np

import rsf_ref as REF

TREES_SEED = 56            # chosen on the CPU: no node of the replica's seven trees has a rival within the rounding bound (asserted)
CV_SEED = 3                # chosen on the CPU: no two validation / out-of-bag mortalities of the replica are close enough to flip (asserted)
PLANTED = 7


def labels(kind, n, seed):
    """times from 8 distinct values (heavy ties: events and censorings share times)"""
    rng = np.random.default_rng([seed, n])
    t = rng.integers(1, 9, n).astype(np.float64)
    e = (rng.random(n) < 0.6).astype(np.int64)
    if kind == "lonely":                                             # the latest time has one patient: Y = 1 at the first tie group
        t[n // 2], e[n // 2] = 20.0, 1
    if kind == "noevent":
        e[:] = 0
    return t, e


def level0_case(kind, n=67, p=37, seed=0):
    """-> X [n, p] fp32, time, event, mults [3, n] in 0..3 (rows of x, not positions).  kind: base | lonely | noevent | constant"""
    rng = np.random.default_rng([seed, n, p])
    X = np.round(rng.normal(size=(n, p)), 1).astype(np.float32)      # rounded: values repeat, thresholds meet equal values
    if kind == "constant":
        X[:] = 1.5
    t, e = labels(kind, n, seed)
    mults = rng.integers(0, 4, (3, n))
    if kind == "lonely":
        mults[:, n // 2] = 1
    return X, t, e, mults


def in_positions(X, time, ev, mults):
    order, gid = REF.positions(time)
    return X[order], np.asarray(time, np.float64)[order], np.asarray(ev)[order].astype(np.int64), gid, np.asarray(mults)[:, order], order


@functools.lru_cache(maxsize=None)
def trees_case():
    """Seven trees of two overlapping training sets over 150 patients, 40 genes; min_leaf 5, max_depth 5, 3 horizons.  Everything in ROW
    order of X except the replica's trees, which live in position order (order: position -> row)."""
    n, p, T = 150, 40, 7
    rng = np.random.default_rng(TREES_SEED)
    X = rng.normal(size=(n, p)).astype(np.float32)
    time = np.round(rng.exponential(30.0, n) * np.exp(-0.8 * X[:, 3] + 0.5 * np.abs(X[:, 5])), 0) + 1.0      # ties
    ev = (rng.random(n) < 0.7).astype(np.int64)
    trains = [np.arange(0, 110), np.arange(30, 140)]                 # rows 140..149 are in no training set
    mults = REF.bootstrap_mults(trains, n, 4, seed=5)[:T]
    wset = np.array([0, 0, 0, 0, 1, 1, 1])
    masks = np.zeros((2, n), bool)
    masks[0, trains[0]] = True; masks[1, trains[1]] = True
    hz = np.quantile(time[ev != 0], [0.25, 0.5, 0.75])
    kw = dict(mtry=7, nsplit=10, min_leaf=5, max_depth=5, seed=5)
    Xp, tp, ep, gid, mp, order = in_positions(X, time, ev, mults)
    trees, morts, Hs = REF.forest(Xp, tp, ep, gid, mp, np.arange(T), kw["seed"], kw["mtry"], kw["nsplit"], kw["min_leaf"], kw["max_depth"],
                                  masks[:, order], wset, hz)
    return dict(X=X, time=time, ev=ev, mults=mults, wset=wset, masks=masks, hz=hz, kw=kw, trains=trains, Xp=Xp, tp=tp, ep=ep, gid=gid,
                mp=mp, order=order, trees=trees, morts=morts, Hs=Hs)


def cindex(time, risk, event):
    """the pair rule of survival_stats.concordance_index(time, -risk, event), restated: comparable when the shorter time is an event (equal
    times: event against censored); concordant when the shorter time has the higher risk; risk ties 1/2"""
    num = den = 0.0
    for i in range(len(time)):
        for j in range(len(time)):
            if event[i] and (time[i] < time[j] or (time[i] == time[j] and not event[j])):
                den += 1
                num += 1.0 if risk[i] > risk[j] else 0.5 if risk[i] == risk[j] else 0.0
    return num / den


@functools.lru_cache(maxsize=None)
def cv_case():
    """90 patients, 30 genes, gene PLANTED with a non-monotone effect (both tails die early: no linear model sees it); 3 folds x 20 trees.
    -> the cohort's arrays, the folds, and the replica's cross-validation: per fold mortalities, C-indices, importance."""
    from multimodal_survival_prediction_amd import data
    N, p, K, T = 90, 30, 3, 20
    rng = np.random.default_rng(CV_SEED)
    X = rng.normal(size=(N, p)).astype(np.float32)
    time = np.round(rng.exponential(40.0, N) * np.exp(-2.0 * (np.abs(X[:, PLANTED]) - 0.8)), 1) + 1.0
    ev = (rng.random(N) < 0.75).astype(np.int64)
    folds = data.kfold_indices(N, K, seed=42)
    kw = dict(mtry=6, nsplit=5, min_leaf=8, max_depth=4, seed=3)
    order, gid = REF.positions(time)
    inv = np.empty(N, np.int64); inv[order] = np.arange(N)
    Xp, tp, ep = X[order], time[order], ev[order]
    pos = [(inv[np.asarray(tr)], inv[np.asarray(va)]) for tr, va in folds]
    mults = REF.bootstrap_mults([tr for tr, _ in pos], N, T, kw["seed"])
    masks = np.zeros((K, N), bool)
    for f, (tr, _) in enumerate(pos):
        masks[f, tr] = True
    wset = np.repeat(np.arange(K), T)
    hz = np.quantile(time[ev != 0], [0.25, 0.5, 0.75])
    trees, morts, Hs = REF.forest(Xp, tp, ep, gid, mults, np.arange(K * T), kw["seed"], kw["mtry"], kw["nsplit"], kw["min_leaf"],
                                  kw["max_depth"], masks, wset, hz)
    leaf = np.array([[REF.drop(t, Xp[r]) for r in range(N)] for t in trees])          # [KT, N]
    out = []
    for f, (tr, va) in enumerate(pos):
        sl = slice(f * T, (f + 1) * T)
        use_v = np.zeros((K * T, N), bool); use_v[sl, va] = True
        use_o = np.zeros((K * T, N), bool); use_o[sl] = (mults[sl] == 0) & masks[f]
        mv, Hv, _ = REF.predict(trees, morts, Hs, Xp, use_v)
        mo, _, co = REF.predict(trees, morts, Hs, Xp, use_o)
        ok = tr[co[tr] > 0]
        cnt, chi = np.zeros(p, np.int64), np.zeros(p)
        for t in trees[sl]:
            for s in np.nonzero(t["feat"] >= 0)[0]:
                cnt[t["feat"][s]] += 1; chi[t["feat"][s]] += t["stat"][s]
        out.append(dict(val_pos=va, val_rows=order[va], val_mort=mv[va], val_H=Hv[va], c_index=cindex(tp[va], mv[va], ep[va]),
                        oob_pos=ok, oob_mort=mo[ok], oob_c_index=cindex(tp[ok], mo[ok], ep[ok]), oob_missing=int(len(tr) - len(ok)),
                        counts=cnt, chi2=chi, leaves_val=leaf[sl][:, va], leaves_oob=np.where(use_o[sl][:, ok], leaf[sl][:, ok], -1)))
    margins = [t["margins"] for t in trees]
    return dict(X=X, time=time, ev=ev, folds=folds, kw=kw, T=T, hz=hz, order=order, folds_ref=out, trees=trees, margins=margins)


def flip_gap(mort, leaves):
    """The smallest relative gap between two different mortalities (inf: none), and whether every pair of EQUAL mortalities comes from
    identical leaves in every admitted tree (then both sides sum the same numbers in the same order: equal on the GPU too)."""
    gap, same_ok = np.inf, True
    for i in range(len(mort)):
        for j in range(i + 1, len(mort)):
            if mort[i] == mort[j]:
                same_ok &= bool((leaves[:, i] == leaves[:, j]).all())
            else:
                gap = min(gap, abs(mort[i] - mort[j]) / max(abs(mort[i]), abs(mort[j])))
    return gap, same_ok
