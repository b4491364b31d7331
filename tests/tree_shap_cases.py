"""The cases of the TreeSHAP tests and what the numpy replica (tests/tree_shap_ref.py) says about them -- shared by
test_cpu_tree_shap.py and test_gpu_tree_shap.py.  The tables are hand-built from a seed (no fit): covers and leaf values are drawn, about
half of the thresholds are set equal to a row's value of the split gene, so x == thr occurs and must go left.  Each reference is computed
once, on all R_MAX rows; a test with fewer rows takes the first ones (a row's result depends on no other row)."""
import functools

import numpy as np

import tree_shap_ref as REF

R_MAX = 257
ROWS = (1, 64, 65, 257)
SEED = 23
NAMES = ("stump", "rootleaf", "repeat", "gbm6", "chain12", "groups")


class _Tables:
    def __init__(self, T, nn, p, rng, x):
        self.feat = np.full((T, nn), -1, np.int32)
        self.thr = np.zeros((T, nn), np.float32)
        self.value = np.zeros((T, nn), np.float64)
        self.cover = np.zeros((T, nn), np.int32)
        self.nn, self.p, self.rng, self.x = nn, p, rng, x

    def split(self, t, s, gene, left_share=None):
        """make node s of tree t a split on `gene`; left_share: the left child's part of the cover (None: drawn)"""
        rng, n = self.rng, int(self.cover[t, s])
        assert n >= 2 and 2 * s + 2 < self.nn
        self.feat[t, s] = gene
        self.thr[t, s] = self.x[rng.integers(len(self.x)), gene] if rng.random() < 0.5 else np.float32(rng.normal())
        l = int(rng.integers(1, n)) if left_share is None else min(max(int(n * left_share), 1), n - 1)
        self.cover[t, 2 * s + 1], self.cover[t, 2 * s + 2] = l, n - l

    def leaf(self, t, s):
        self.value[t, s] = self.rng.normal()

    def bushy(self, t, depth, genes, root=4000, p_split=0.85):
        """a random tree of at most `depth` levels of splits on the given genes"""
        self.cover[t, 0] = root

        def grow(s, d):
            if d < depth and self.cover[t, s] >= 2 and 2 * s + 2 < self.nn and (d == 0 or self.rng.random() < p_split):
                self.split(t, s, int(self.rng.choice(genes)))
                grow(2 * s + 1, d + 1); grow(2 * s + 2, d + 1)
            else:
                self.leaf(t, s)

        grow(0, 0)

    def chain(self, t, genes, root=60000):
        """len(genes) splits down one path: at each the side that goes on is drawn and keeps most of the cover"""
        self.cover[t, 0] = root
        s = 0
        for gene in genes:
            on_left = self.rng.random() < 0.5
            share = self.rng.uniform(0.55, 0.9)
            self.split(t, s, gene, share if on_left else 1.0 - share)
            self.leaf(t, 2 * s + 2 if on_left else 2 * s + 1)
            s = 2 * s + 1 if on_left else 2 * s + 2
        self.leaf(t, s)


def _build(name):
    rng = np.random.default_rng([SEED, NAMES.index(name)])
    p = dict(stump=1, rootleaf=3, repeat=2, gbm6=9, chain12=13, groups=7)[name]
    x = np.round(rng.normal(size=(R_MAX, p)), 1).astype(np.float32)
    if name == "stump":
        tb = _Tables(1, 3, p, rng, x)
        tb.bushy(0, 1, [0])
        goff = [0, 1]
    elif name == "rootleaf":
        tb = _Tables(2, 7, p, rng, x)
        tb.cover[0, 0] = 50; tb.leaf(0, 0)                           # the root is the leaf
        tb.bushy(1, 2, [0, 1, 2], p_split=1.0)
        goff = [0, 2]
    elif name == "repeat":
        tb = _Tables(2, 31, p, rng, x)
        tb.bushy(0, 4, [0, 1], p_split=1.0)                          # the same gene up to 4 times on a path
        tb.bushy(1, 4, [1], p_split=0.9)
        goff = [0, 2]
    elif name == "gbm6":
        tb = _Tables(6, 127, p, rng, x)
        for t in range(6):
            tb.bushy(t, 6, list(range(p)), p_split=0.95)
        goff = [0, 6]
    elif name == "chain12":
        tb = _Tables(3, 8191, p, rng, x)
        tb.chain(0, [int(g) for g in rng.permutation(p)[:12]])       # 12 splits on 12 distinct genes
        tb.chain(1, [5] * 12)                                        # 12 splits on ONE gene
        tb.bushy(2, 5, list(range(p)))
        goff = [0, 3]
    else:
        tb = _Tables(9, 15, p, rng, x)                               # G = 4 with (3, 0, 1, 5) trees and different gene sets
        for t, genes in enumerate([[0, 1, 2]] * 3 + [[6]] + [[1, 3, 4, 5, 6]] * 5):
            tb.bushy(t, 3, genes)
        goff = [0, 3, 3, 4, 9]
    T = tb.feat.shape[0]
    use = (rng.random((T, R_MAX)) < 0.6).astype(np.uint8)
    use[:, 0] = 0                                                    # row 0: no tree admits it
    use[:, 1] = 1                                                    # row 1: all do
    return dict(name=name, p=p, x=x, feat=tb.feat, thr=tb.thr, value=tb.value, cover=tb.cover, goff=np.asarray(goff, np.int64), use=use,
                T=T, nn=tb.nn)


@functools.lru_cache(maxsize=None)
def case(name):
    return _build(name)


def tables(c):
    return c["feat"], c["thr"], c["value"], c["cover"], c["goff"]


@functools.lru_cache(maxsize=None)
def reference(name, masked=False):
    """the replica's (phi [G, R_MAX, p], base [G, R_MAX]) of the case, with or without its use mask"""
    c = case(name)
    return REF.shap(c["x"], *tables(c), c["use"] if masked else None)


@functools.lru_cache(maxsize=None)
def tolerance(name):
    c = case(name)
    return REF.tolerance(c["feat"], c["value"], c["goff"])


def subgroup(c, g):
    """group g of a case as a case of its own (its trees alone)"""
    a, b = int(c["goff"][g]), int(c["goff"][g + 1])
    return dict(c, feat=c["feat"][a:b], thr=c["thr"][a:b], value=c["value"][a:b], cover=c["cover"][a:b], use=c["use"][a:b],
                goff=np.array([0, b - a], np.int64), T=b - a)


def random_small(seed, n=12):
    """n random trees of depth <= 3 on <= 4 genes, one group each, with 6 rows -- for the brute-force comparison"""
    rng = np.random.default_rng([SEED, 99, seed])
    p = int(rng.integers(1, 5))
    x = np.round(rng.normal(size=(6, p)), 1).astype(np.float32)
    tb = _Tables(n, 15, p, rng, x)
    for t in range(n):
        tb.bushy(t, int(rng.integers(1, 4)), list(range(p)), root=int(rng.integers(40, 100)), p_split=0.8)
    return dict(p=p, x=x, feat=tb.feat, thr=tb.thr, value=tb.value, cover=tb.cover, goff=np.arange(n + 1, dtype=np.int64), T=n, nn=15)
