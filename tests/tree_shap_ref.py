"""numpy replica of the TreeSHAP contract (include/mmsurv.h: TreeShapP; csrc/tree_shap.hip) and an independent brute-force Shapley value
to hold it against.  Both read the kernel's table format: feat (< 0: leaf or absent), thr, value, cover [T, nn] heap-indexed, a row goes
LEFT iff x[feat] <= thr, a node is a leaf iff feat < 0 or 2s + 2 >= nn; goff [G + 1] groups of trees; use [T, R] or None.
Everything in float64; phi comes back DENSE over the p columns of x: [G, R, p], base [G, R]."""
import itertools
import math

import numpy as np


def is_leaf(feat_t, s):
    return feat_t[s] < 0 or 2 * s + 2 >= len(feat_t)


def leaves(feat_t, cover_t=None):
    """-> [(leaf node, [(split node, feature, zero fraction, child is left)])] depth-first, left-first (without covers: fraction None)"""
    out = []

    def walk(s, path):
        if is_leaf(feat_t, s):
            out.append((s, path))
            return
        for c, left in ((2 * s + 1, True), (2 * s + 2, False)):
            walk(c, path + [(s, int(feat_t[s]), None if cover_t is None else float(cover_t[c]) / float(cover_t[s]), left)])

    walk(0, [])
    return out


def weights(u):
    return [math.factorial(k) * math.factorial(u - k - 1) / math.factorial(u) for k in range(u)]


def shap(x, feat, thr, value, cover, goff, use=None):
    """The literal per-leaf form of the contract.  x [R, p] -> (phi [G, R, p], base [G, R])"""
    x = np.asarray(x)
    R, p = x.shape
    G = len(goff) - 1
    phi, base = np.zeros((G, R, p)), np.zeros((G, R))
    for g in range(G):
        for t in range(int(goff[g]), int(goff[g + 1])):
            adm = np.ones(R, bool) if use is None else np.asarray(use[t]) != 0
            zero = np.zeros(R)
            for s, path in leaves(feat[t], cover[t]):                # every quantity below is a vector over the rows
                v = float(value[t][s])
                fs, zs, os_ = [], [], []
                for node, f, z, left in path:
                    o = (x[:, f] <= thr[t][node]) == left
                    if f in fs:
                        i = fs.index(f); zs[i] *= z; os_[i] = os_[i] & o
                    else:
                        fs.append(f); zs.append(z); os_.append(o)
                u = len(fs)
                zall = 1.0
                for z in zs:
                    zall *= z
                base[g, adm] += v * zall if u else v
                w = weights(u) if u else []
                for j in range(u):
                    poly = [np.ones(R)]
                    for m in range(u):
                        if m != j:
                            om = os_[m].astype(np.float64)
                            poly = [(poly[k] if k < len(poly) else zero) * zs[m] + (poly[k - 1] * om if k >= 1 else zero) for k in range(len(poly) + 1)]
                    tot = np.zeros(R)
                    for k in range(u):
                        tot = tot + poly[k] * w[k]
                    term = (v * (os_[j].astype(np.float64) - zs[j])) * tot
                    phi[g, adm, fs[j]] += term[adm]
    return phi, base


def reached(x, feat, thr, value, goff, use=None):
    """-> [G, R]: the sum of the leaf values each row reaches over the trees that admit it (what local accuracy must reproduce)"""
    x = np.asarray(x)
    R, G = x.shape[0], len(goff) - 1
    out = np.zeros((G, R))
    for g in range(G):
        for t in range(int(goff[g]), int(goff[g + 1])):
            for r in range(R):
                if use is not None and not use[t][r]:
                    continue
                s = 0
                while not is_leaf(feat[t], s):
                    s = 2 * s + 1 + (0 if x[r, feat[t][s]] <= thr[t][s] else 1)
                out[g, r] += value[t][s]
    return out


def _expect(xr, S, feat_t, thr_t, value_t, cover_t, s=0):
    """the path-dependent expectation of the tree given the features in S"""
    if is_leaf(feat_t, s):
        return float(value_t[s])
    l, r = 2 * s + 1, 2 * s + 2
    if int(feat_t[s]) in S:
        return _expect(xr, S, feat_t, thr_t, value_t, cover_t, l if xr[feat_t[s]] <= thr_t[s] else r)
    return (cover_t[l] * _expect(xr, S, feat_t, thr_t, value_t, cover_t, l) + cover_t[r] * _expect(xr, S, feat_t, thr_t, value_t, cover_t, r)) / cover_t[s]


def shapley_bruteforce(x, feat, thr, value, cover, goff, use=None):
    """Shapley values by subset enumeration over the recursive path-dependent expectation, tree by tree (only for trees with <= 8
    distinct features).  Same result format as shap."""
    x = np.asarray(x)
    R, p = x.shape
    G = len(goff) - 1
    phi, base = np.zeros((G, R, p)), np.zeros((G, R))
    for g in range(G):
        for t in range(int(goff[g]), int(goff[g + 1])):
            used = sorted({int(feat[t][s]) for s in range(len(feat[t])) if _on_tree(feat[t], s) and not is_leaf(feat[t], s)})
            assert len(used) <= 8
            u = len(used)
            args = (feat[t], thr[t], value[t], cover[t])
            for r in range(R):
                if use is not None and not use[t][r]:
                    continue
                base[g, r] += _expect(x[r], set(), *args)
                for j in used:
                    rest = [f for f in used if f != j]
                    for k in range(len(rest) + 1):
                        w = math.factorial(k) * math.factorial(u - k - 1) / math.factorial(u)
                        for S in itertools.combinations(rest, k):
                            phi[g, r, j] += w * (_expect(x[r], set(S) | {j}, *args) - _expect(x[r], set(S), *args))
    return phi, base


def _on_tree(feat_t, s):
    """node s is reachable from the root through split nodes"""
    while s > 0:
        s = (s - 1) >> 1
        if is_leaf(feat_t, s):
            return False
    return True


def tolerance(feat, value, goff):
    """The derived bound of the device tests per group: (256 + L) 2^-52 A, L = the group's leaf count, A = the sum of |leaf value| over
    its trees.  sum_k w_k e_k <= 1 (w_k = 1 / (u C(u-1, k)), e_k <= C(u-1, k)), so a leaf term is at most |v|; it takes at most
    2d + u^2 + u + 4 <= 184 roundings at d = u = 12, and L further additions accumulate it."""
    return np.array([(256 + L) * 2.0 ** -52 * A for L, A in leaf_stats(feat, value, goff)])


def leaf_stats(feat, value, goff):
    """-> per group (L, A): the leaf count and the sum of |leaf value| over its trees"""
    out = []
    for g in range(len(goff) - 1):
        L, A = 0, 0.0
        for t in range(int(goff[g]), int(goff[g + 1])):
            for s, _ in leaves(feat[t]):
                L += 1; A += abs(float(value[t][s]))
        out.append((L, A))
    return out

