"""numpy float64 restatement of the univariate Cox score screen (include/mmsurv.h: GeneScreenP) -- written from the definitions, without
the package's own coefficient code:
  * risk_set_score: the brute-force risk-set definition (U = sum over events of x_i - mean over R(t_i), V = sum of var over R(t_i));
  * coefficients / closed_form: the per-position form the kernel evaluates, with O(n^2) comparisons instead of the package's scan;
  * screen / select: what gene_select.cox_score_screen / select_genes must return."""
import numpy as np


def risk_order(time, rows):
    """positions into rows, time descending, equal times in list order"""
    t = np.asarray(time, dtype=np.float64)[np.asarray(rows, dtype=np.int64)]
    return np.argsort(-t, kind="stable")


def risk_set_score(x, time, event, rows):
    """x: [N, G]; -> (U, V) float64 [G] of the problem `rows` straight from the risk sets (Breslow: every event tied at u sees R(u))."""
    rows = np.asarray(rows, dtype=np.int64)
    X = np.asarray(x, dtype=np.float64)[rows]
    t, e = np.asarray(time, dtype=np.float64)[rows], np.asarray(event)[rows] != 0
    G = X.shape[1]
    U, V = np.zeros(G), np.zeros(G)
    for i in np.nonzero(e)[0]:
        R = X[t >= t[i]]
        m = R.mean(0)
        U += X[i] - m
        V += ((R - m) ** 2).mean(0)
    return U, V


def coefficients(time, event, rows):
    """-> (order, a, b, q) per position of the risk order, by direct comparison of every pair of positions."""
    rows = np.asarray(rows, dtype=np.int64)
    order = risk_order(time, rows)
    t = np.asarray(time, dtype=np.float64)[rows][order]
    e = (np.asarray(event)[rows][order] != 0).astype(np.float64)
    n = len(t)
    a, b, q = np.zeros(n), np.zeros(n), np.zeros(n)
    if n == 0:
        return order, a, b, q
    n_at = (t[None, :] >= t[:, None]).sum(1).astype(np.float64)          # |R(t_i)|
    for k in range(n):
        ev = (e != 0) & (t <= t[k])
        b[k] = (1.0 / n_at[ev]).sum()
        if k == n - 1 or t[k + 1] != t[k]:
            tie = (e != 0) & (t == t[k])
            q[k] = (1.0 / n_at[tie] ** 2).sum()
    a = e - b
    return order, a, b, q


def closed_form(x, time, event, rows):
    """-> (U, V, bound_U, bound_V): the per-position sums in float64 and the magnitudes the parity bound scales with
    (sum |a x|;  sum b x^2 + sum q S1^2)."""
    rows = np.asarray(rows, dtype=np.int64)
    order, a, b, q = coefficients(time, event, rows)
    X = np.asarray(x, dtype=np.float64)[rows[order]]
    S1 = np.cumsum(X, 0)
    U = (a[:, None] * X).sum(0)
    vb, vq = (b[:, None] * X * X).sum(0), (q[:, None] * S1 * S1).sum(0)
    return U, vb - vq, (np.abs(a)[:, None] * np.abs(X)).sum(0), vb + vq


def statistic(U, V):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(V > 0, U * U / np.where(V > 0, V, 1.0), 0.0)


def screen(x, time, event, index_lists):
    G = np.asarray(x).shape[1]
    U, V = np.zeros((len(index_lists), G)), np.zeros((len(index_lists), G))
    for p, rows in enumerate(index_lists):
        U[p], V[p], _, _ = closed_form(x, time, event, rows)
    return U, V, statistic(U, V)


def top_k(stat, k):
    """rank order of the k largest, lower index first among equals"""
    idx = sorted(range(len(stat)), key=lambda j: (-float(stat[j]), j))
    return np.asarray(idx[:k], dtype=np.int64)


def eligible(cohort, idx):
    idx = np.asarray(idx, dtype=np.int64)
    ok = cohort["has_survival"].cpu().numpy().astype(bool) & (cohort["mask"].cpu().numpy()[:, 1] != 0)
    return idx[ok[idx]]


def resamples(n, R, seed, fold):
    """[R] index arrays into a fold's n eligible rows: numpy.random.default_rng([seed, fold]), replicate after replicate one call
    integers(0, n, size=n); a resample lists every row as often as it was drawn (ascending position)."""
    rng = np.random.default_rng([int(seed), int(fold)])
    return [np.sort(rng.integers(0, n, size=n)) for _ in range(R)]


def select(cohort, train_indices_per_fold, k, stability=0, seed=0):
    """-> (columns per fold ascending, frequency per fold or None, full-sample stat per fold, problems per fold)"""
    x = cohort["rnaseq"].cpu().numpy()
    lab = cohort["label"].cpu().numpy()
    G = x.shape[1]
    cols, freqs, stats, probs = [], [], [], []
    for f, idx in enumerate(train_indices_per_fold):
        rows = eligible(cohort, idx)
        lists = [rows] + [rows[r] for r in resamples(len(rows), stability, seed, f)]
        _, _, st = screen(x, lab[:, 0], lab[:, 1], lists)
        freq = None
        if stability:
            keep = [s for s in st[1:] if (s > 0).any()]
            freq = np.zeros(G)
            for s in keep:
                freq[top_k(s, k)] += 1.0
            freq = freq / len(keep) if keep else freq
            win = sorted(range(G), key=lambda j: (-freq[j], -st[0][j], j))[:k]
        else:
            win = top_k(st[0], k)
        cols.append(np.sort(np.asarray(win, dtype=np.int64)))
        freqs.append(freq); stats.append(st[0]); probs.append(lists)
    return cols, (freqs if stability else None), stats, probs
