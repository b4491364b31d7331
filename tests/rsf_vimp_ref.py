"""numpy replica of the forest's permutation importance (include/mmsurv.h: RsfVimpP; survival_forest.permutation_donors / Forest.vimp) --
test infrastructure, written the slow, obvious way and sharing no code with the package: donor tables, the problem table, the substituted
walk, the sequential delta sum D, M = M0 + D / cnt, and the pair counts of the C-index.

The contract (restated).  h = rsf_ref.h32, ht = rsf_ref.tree_key(seed, id); ROWS i are rows of the matrix handed in, not time positions.
    hp = h((r + 1) * 0x85EBCA6B + h(ht ^ 0x68E31DA4));   k_i = h((i + 1) * 0x9E3779B9 + hp)       (mod 2^32)
    a_0 < a_1 < ... the rows tree `id` admits, s_0, s_1, ... the same rows sorted by (k, i):  donor[a_j] = s_j; any other row: itself.
Problem (f, g): the trees of set f that split on g at any node, ascending, each once.  For a row i with cnt[f][i] > 0, over those trees
that admit i, in that order, D_i += mort_t(leaf') - mort_t(leaf) as one sequential float64 sum from 0.0; leaf' is reached reading
x[donor_t(i)][g] in place of x[i][g] at every node on g; the walk stops at feat < 0 or 2 s + 2 >= nn.  M_i = M0[f][i] + D_i / cnt[f][i].
Over the rows with cnt > 0, with risk M: the ordered pair (i, j) is comparable when i is an event and time_i < time_j, or the times are
equal and j is censored; conc2 = sum over comparable pairs of 2 [M_i > M_j] + [M_i == M_j].  C = conc2 / (2 comparable).
VIMP[f][g] = C_base[f] - (C_perm[f][g][0] + ... + C_perm[f][g][R - 1]) / R, the sum taken in that order; exactly 0.0 without a problem."""
import numpy as np

import rsf_ref as REF

M32 = 0xFFFFFFFF


def donors(seed, tid, r, admitted):
    """-> int64 [n]: the donor row of every row for tree `tid`, repeat r; admitted: bool [n]"""
    hp = REF.h32(((r + 1) * 0x85EBCA6B + REF.h32(REF.tree_key(int(seed), int(tid)) ^ 0x68E31DA4)) & M32)
    n = len(admitted)
    k = [REF.h32(((i + 1) * 0x9E3779B9 + hp) & M32) for i in range(n)]
    a = [i for i in range(n) if admitted[i]]
    s = sorted(a, key=lambda i: (k[i], i))
    out = list(range(n))
    for aj, sj in zip(a, s):
        out[aj] = sj
    return np.array(out, dtype=np.int64)


def donor_table(seed, tree_ids, use, R):
    """-> int64 [R, T, n]"""
    return np.array([[donors(seed, tid, r, np.asarray(use[t]) != 0) for t, tid in enumerate(tree_ids)] for r in range(R)], dtype=np.int64)


def problem_table(feat, sets=None):
    """-> list of (set, gene, [trees ascending, each once]) sorted by (set, gene); feat: [T, nn]"""
    feat = np.asarray(feat)
    sets = np.zeros(len(feat), np.int64) if sets is None else np.asarray(sets)
    table = {}
    for t in range(len(feat)):
        for g in sorted(set(int(v) for v in feat[t] if v >= 0)):
            table.setdefault((int(sets[t]), g), []).append(t)
    return [(f, g, table[(f, g)]) for f, g in sorted(table)]


def walk(feat, thr, x, g=None, xg=None):
    """the leaf of row x in one tree (feat, thr: [nn]); with g, every node on gene g reads xg instead of x[g]"""
    s, nn = 0, len(feat)
    while not (feat[s] < 0 or 2 * s + 2 >= nn):
        v = xg if feat[s] == g else x[feat[s]]
        s = 2 * s + 1 + (0 if v <= thr[s] else 1)
    return s


def delta(X, feat, thr, mort, use, donor_r, trees, g, cnt):
    """D [n] of one problem under one repeat's donors donor_r [T, n]"""
    D = np.zeros(len(X))
    for i in range(len(X)):
        if cnt[i] <= 0:
            continue
        d = 0.0
        for t in trees:
            if not use[t][i]:
                continue
            l0 = walk(feat[t], thr[t], X[i])
            l1 = walk(feat[t], thr[t], X[i], g, X[donor_r[t][i]][g])
            d = d + (float(mort[t][l1]) - float(mort[t][l0]))
        D[i] = d
    return D


def pair_counts(time, event, M, rows):
    """-> (conc2, comparable) of the rows `rows` (bool [n]) with risk M, as exact Python ints"""
    t, e, m = np.asarray(time, np.float64)[rows], np.asarray(event)[rows] != 0, np.asarray(M, np.float64)[rows]
    ti, tj = t[:, None], t[None, :]
    comp = ((ti < tj) & e[:, None]) | ((ti == tj) & e[:, None] & ~e[None, :])
    mi, mj = m[:, None], m[None, :]
    return 2 * int(((mi > mj) & comp).sum()) + int(((mi == mj) & comp).sum()), int(comp.sum())


def vimp(X, time, event, feat, thr, mort, use, sets, M0, cnt, seed, tree_ids, R, p=None):
    """The whole method on host arrays.  X [n, p]; feat / thr / mort [T, nn]; use [T, n]; sets [T] or None; M0 float64, cnt int [F, n].
    -> dict(problems, D, M [P, R, n], conc2, comparable int64 [P, R], base_conc2, base_comparable [F], c_base [F], vimp [F, p],
    vimp_reps [F, R, p])."""
    X, feat, thr, mort, use = np.asarray(X), np.asarray(feat), np.asarray(thr), np.asarray(mort), np.asarray(use) != 0
    M0, cnt = np.asarray(M0, np.float64), np.asarray(cnt)
    F, n = M0.shape
    p = X.shape[1] if p is None else p
    probs = problem_table(feat, sets)
    don = donor_table(seed, tree_ids, use, R)
    P = len(probs)
    D, Mo = np.zeros((P, R, n)), np.zeros((P, R, n))
    conc2, comp = np.zeros((P, R), np.int64), np.zeros((P, R), np.int64)
    base = [pair_counts(time, event, M0[f], cnt[f] > 0) for f in range(F)]
    c_base = np.array([b[0] / (2.0 * b[1]) if b[1] else np.nan for b in base])
    out_v, out_r = np.zeros((F, p)), np.zeros((F, R, p))
    for q, (f, g, trees) in enumerate(probs):
        total = 0.0
        for r in range(R):
            D[q, r] = delta(X, feat, thr, mort, use, don[r], trees, g, cnt[f])
            rows = cnt[f] > 0
            Mo[q, r] = M0[f]
            Mo[q, r][rows] = M0[f][rows] + D[q, r][rows] / cnt[f][rows].astype(np.float64)
            conc2[q, r], comp[q, r] = pair_counts(time, event, Mo[q, r], rows)
            c_perm = conc2[q, r] / (2.0 * comp[q, r]) if comp[q, r] else np.nan
            out_r[f, r, g] = c_base[f] - c_perm
            total = total + c_perm
        out_v[f, g] = c_base[f] - total / R
    return dict(problems=probs, D=D, M=Mo, conc2=conc2, comparable=comp, base_conc2=np.array([b[0] for b in base], np.int64),
                base_comparable=np.array([b[1] for b in base], np.int64), c_base=c_base, vimp=out_v, vimp_reps=out_r, donor=don)
