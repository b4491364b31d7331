"""The cases of the boosting tests and what the numpy replica (tests/gbm_ref.py) says about them -- shared by test_cpu_boosting.py (which
asserts on the CPU that no node of the replica's trees needs the near-tie excuse) and test_gpu_boosting.py.

A case: X [n, p] fp32 with repeated values (gene 0 constant, gene 1 with two distinct values: empty bins at any B > 2), times from a
few distinct values (ties between events and censorings), multiplicities 0..3, and P problems that differ in depth, sample rates,
min_leaf, l2 and id.  Problem 1 (when P > 1) has no event among its training rows -- its gradient is 0 and every tree a single leaf of
value 0 --, problem 2 a min_leaf that blocks every cut, problem 3 a colsample low enough to admit no gene in some round."""
import functools

import numpy as np

import gbm_ref as REF

ROUNDS = 4
SEED = 11                  # chosen on the CPU: no node of any case's replica trees is within the near-tie excuse (asserted)
# (n, p, B, P, depths): the kernels' edges -- n past one 256-position chunk, p not a multiple of the 32-gene tile and more than one
# tile, B at the ends and the default, D = 1, 3 and the deepest
SHAPES = {"tiny": (67, 5, 4, 1, (1,)), "wide": (300, 70, 32, 24, (1, 3, 2)), "bins64": (67, 70, 64, 24, (3,)), "one": (300, 5, 32, 1, (3,)),
          "deep": (300, 70, 64, 1, (6,))}


def make_data(n, p, seed):
    rng = np.random.default_rng([seed, n, p])
    X = np.round(rng.normal(size=(n, p)), 1).astype(np.float32)
    X[:, 0] = 1.5
    if p > 1:
        X[:, 1] = (rng.random(n) < 0.4).astype(np.float32)
    t = rng.integers(1, 12, n).astype(np.float64)
    score = X[:, min(2, p - 1)] - 0.7 * np.abs(X[:, min(3, p - 1)])
    t = np.maximum(1.0, np.round(t * np.exp(-0.6 * score)))
    e = (rng.random(n) < 0.65).astype(np.int64)
    return X, t, e


def make_problems(n, P, depths, e, seed):
    rng = np.random.default_rng([seed, n, P, 7])
    mults = rng.integers(0, 4, (P, n))
    masks = mults == 0
    prm = dict(learning_rate=np.full(P, 0.1), max_depth=np.array([depths[q % len(depths)] for q in range(P)]), min_leaf=np.full(P, 3),
               l2=np.full(P, 1.0), min_gain=np.zeros(P), subsample=np.ones(P), colsample=np.ones(P))
    ids = np.arange(P) * 3 + 5
    if P > 1:
        mults[1, e != 0] = 0                                           # no event in training
        masks[1] = mults[1] == 0
        prm["min_leaf"][2] = 10 * n                                    # blocks every cut
        prm["colsample"][3] = 0.02
        for q in range(4, P):
            prm["subsample"][q] = (1.0, 0.7, 0.5)[q % 3]
            prm["colsample"][q] = (1.0, 0.5)[q % 2]
            prm["l2"][q] = (1.0, 0.0, 3.5)[q % 3]
            prm["learning_rate"][q] = (0.1, 0.05)[q % 2]
            prm["min_leaf"][q] = (3, 8)[(q // 2) % 2]
            prm["min_gain"][q] = (0.0, 0.05)[(q // 3) % 2]
    return mults, masks, prm, ids


def edges_of(X, B):
    """numpy restatement of boosting.quantile_edges (linear interpolation in fp32 is the package's; the tests take the package's edges for
    the fit and use this one only where no device is involved)"""
    q = np.arange(1, B, dtype=np.float64) / B
    return np.ascontiguousarray(np.quantile(X.astype(np.float64), q, axis=0).T.astype(np.float32))


def bins_of(X, edges):
    """[p, R] bins: the number of the gene's edges < x"""
    return np.stack([np.searchsorted(edges[f], X[:, f], side="left") for f in range(X.shape[1])]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(name):
    n, p, B, P, depths = SHAPES[name]
    X, t, e = make_data(n, p, SEED)
    mults, masks, prm, ids = make_problems(n, P, depths, e, SEED)
    return dict(name=name, n=n, p=p, B=B, P=P, X=X, time=t, event=e, mults=mults, masks=masks, prm=prm, ids=ids, seed=SEED, rounds=ROUNDS,
                nn=(2 << int(prm["max_depth"].max())) - 1)


def replica(c, edges=None, problems=None):
    """The replica's fit of the case's problems (all, or the listed ones) on the given edges (None: edges_of) -> list of REF.boost dicts;
    everything in position order."""
    edges = edges_of(c["X"], c["B"]) if edges is None else np.asarray(edges, np.float32)
    order, gid = REF.positions(c["time"])
    xb = bins_of(c["X"][order], edges)
    ev = c["event"][order]
    out = []
    for q in (range(c["P"]) if problems is None else problems):
        prm = c["prm"]
        out.append(REF.boost(xb, edges, ev, gid, order, c["mults"][q][order], c["B"], c["rounds"], lr=float(prm["learning_rate"][q]),
                             depth=int(prm["max_depth"][q]), min_leaf=int(prm["min_leaf"][q]), l2=float(prm["l2"][q]),
                             min_gain=float(prm["min_gain"][q]), subsample=REF.threshold(prm["subsample"][q]),
                             colsample=REF.threshold(prm["colsample"][q]), pid=int(c["ids"][q]), seed=c["seed"], nn=c["nn"],
                             mask=c["masks"][q][order]))
    return out


@functools.lru_cache(maxsize=None)
def replica_cached(name):
    return replica(case(name))
