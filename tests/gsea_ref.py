"""A literal numpy replica of the gene-set enrichment statistic (multimodal_survival_prediction_amd/enrichment.py's docstring and
include/mmsurv.h: GseaScoreP, GseaEsP), written from those definitions with loops; it shares no code with the package."""
import numpy as np


def null_residuals(time, event, rows=None):
    """m_i = delta_i - sum over the event times u <= t_i of d_u / n_u (Breslow), per list position"""
    time, event = np.asarray(time, dtype=np.float64), np.asarray(event) != 0
    rows = np.arange(len(time)) if rows is None else np.asarray(rows, dtype=np.int64)
    t, e = time[rows], event[rows]
    m = np.zeros(len(rows))
    for i in range(len(rows)):
        H = 0.0
        for u in np.unique(t[e]):
            if u <= t[i]:
                H += float((e & (t == u)).sum()) / float((t >= u).sum())
        m[i] = float(e[i]) - H
    return m


def scores(x, rows, m, perm):
    """x: [N, G] (any float type; widened to float64), rows [n], m [n], perm [R1, n] -> (scale [G], Z [R1, G])"""
    X = np.asarray(x, dtype=np.float64)[np.asarray(rows, dtype=np.int64)]
    m = np.asarray(m, dtype=np.float64)
    n = len(m)
    css = ((X - X.mean(0)) ** 2).sum(0)
    sm2 = float((m * m).sum())
    scale = np.zeros(X.shape[1])
    ok = (css > 0) & (sm2 > 0)
    scale[ok] = 1.0 / np.sqrt(sm2 / (n - 1) * css[ok])
    Z = np.zeros((len(perm), X.shape[1]))
    for r in range(len(perm)):
        Z[r] = scale * (m[np.asarray(perm[r], dtype=np.int64)] @ X)
    Z[:, ~ok] = 0.0
    return scale, Z


def abs_sums(x, rows, m, perm):
    """-> [R1, G]: sum_i |m[perm[r][i]]| |x[rows[i]][g]|, the absolute sum behind the rounding bound of Z"""
    X = np.abs(np.asarray(x, dtype=np.float64)[np.asarray(rows, dtype=np.int64)])
    m = np.abs(np.asarray(m, dtype=np.float64))
    return np.stack([m[np.asarray(p, dtype=np.int64)] @ X for p in perm])


def ranking(z):
    z = np.asarray(z, dtype=np.float64)
    return np.lexsort((np.arange(len(z)), -z))


def es_one(z, members, weight=1, detail=False):
    """-> (es, peak) of one set in one replicate by a cumulative sum over the ranking.  detail: -> (es, peak, gap, run, order), gap = the
    distance of the winning extreme to the best value of the same kind at any OTHER position: how far rounding is from moving the peak.
    With unit weights (weight 0, or members whose weights add up to 0) the running sum is exact and gap = inf."""
    z = np.asarray(z, dtype=np.float64)
    G = len(z)
    order = ranking(z)
    member = np.zeros(G, dtype=bool)
    member[np.asarray(members, dtype=np.int64)] = True
    k = int(member.sum())
    assert 1 <= k <= G - 1 and k == len(members)
    hit = member[order]
    w = np.abs(z[order]) if weight == 1 else np.ones(G)
    NR = w[hit].sum()
    unit = weight == 0 or not NR > 0
    if unit:                    # steps of 1 / k and 1 / (G - k): an integer cumulative sum over the common denominator, so ties are ties
        run = np.cumsum(np.where(hit, G - k, -k)).astype(np.float64) / float(k * (G - k))
    else:
        run = np.cumsum(np.where(hit, w / NR, -1.0 / (G - k)))
    hi, lo = run.max(), run.min()
    if hi >= -lo:
        es, peak = hi, int(np.argmax(run))
        gap = hi - np.delete(run, peak).max()
    else:
        es, peak = lo, int(np.argmin(run))
        gap = np.delete(run, peak).min() - lo
    if unit:
        gap = np.inf            # exact arithmetic decides every position
    return (es, peak, gap, run, order) if detail else (es, peak)


def es_all(Z, set_off, set_gene, weight=1, gperm=None):
    """-> (es [R1, S], peak [R1, S], gap [R1, S]); with gperm [R, G]: Z is one row and replicate r >= 1 ranks Z[0][gperm[r - 1]]"""
    Z = np.asarray(Z, dtype=np.float64).reshape(-1, np.asarray(Z).shape[-1])
    R1 = len(Z) if gperm is None else len(gperm) + 1
    S = len(set_off) - 1
    es, peak, gap = np.zeros((R1, S)), np.zeros((R1, S), dtype=np.int64), np.zeros((R1, S))
    for r in range(R1):
        z = Z[r] if gperm is None else (Z[0] if r == 0 else Z[0][np.asarray(gperm[r - 1], dtype=np.int64)])
        for s in range(S):
            es[r, s], peak[r, s], gap[r, s] = es_one(z, set_gene[set_off[s]:set_off[s + 1]], weight, detail=True)[:3]
    return es, peak, gap


def leading_edge(z, members, es, peak):
    order = ranking(z)
    member = np.zeros(len(order), dtype=bool)
    member[np.asarray(members, dtype=np.int64)] = True
    pos = range(0, peak + 1) if es >= 0 else range(peak + 1, len(order))
    return [int(order[i]) for i in pos if member[order[i]]]


def summarise(es):
    """es [R + 1, S] -> dict(es, nes, p, fdr, fwer) by the documented formulas, set by set"""
    es = np.asarray(es, dtype=np.float64)
    obs, null = es[0], es[1:]
    R, S = null.shape
    p, nes, nnes = np.zeros(S), np.full(S, np.nan), np.full((R, S), np.nan)
    for j in range(S):
        col = null[:, j]
        pos = col >= 0
        mp = np.mean(col[pos]) if pos.any() else np.nan
        mn = np.mean(-col[~pos]) if (~pos).any() else np.nan
        same = col[pos] if obs[j] >= 0 else col[~pos]
        p[j] = (1.0 + (np.abs(same) >= abs(obs[j])).sum()) / (1.0 + len(same))
        with np.errstate(divide="ignore", invalid="ignore"):
            nes[j] = obs[j] / (mp if obs[j] >= 0 else mn)
            nnes[:, j] = col / np.where(pos, mp, mn)
    null_pos = np.array([nnes[r, j] for r in range(R) for j in range(S) if null[r, j] >= 0 and not np.isnan(nnes[r, j])])
    null_neg = np.array([nnes[r, j] for r in range(R) for j in range(S) if null[r, j] < 0 and not np.isnan(nnes[r, j])])
    obs_pos = np.array([nes[j] for j in range(S) if obs[j] >= 0 and not np.isnan(nes[j])])
    obs_neg = np.array([nes[j] for j in range(S) if obs[j] < 0 and not np.isnan(nes[j])])
    fdr, fwer = np.full(S, np.nan), np.full(S, np.nan)
    for j in range(S):
        if np.isnan(nes[j]):
            continue
        if obs[j] >= 0:
            num, den = (null_pos >= nes[j]).sum() / len(null_pos), (obs_pos >= nes[j]).sum() / len(obs_pos)
        else:
            num, den = (null_neg <= nes[j]).sum() / len(null_neg), (obs_neg <= nes[j]).sum() / len(obs_neg)
        fdr[j] = min(1.0, num / den)
        count = 0
        for r in range(R):
            row = np.abs(nnes[r][~np.isnan(nnes[r])])
            if len(row) and row.max() >= abs(nes[j]):
                count += 1
        fwer[j] = (1.0 + count) / (R + 1.0)
    return dict(es=obs.copy(), nes=nes, p=p, fdr=fdr, fwer=fwer)
