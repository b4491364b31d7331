"""numpy replica of the gradient-boosted Cox trees contract (include/mmsurv.h: GbmGradP, GbmSplitP, GbmUpdateP, GbmPredictP; boosting.py)
-- test infrastructure, written the slow, obvious way and sharing no code with the package: hashes, gradient, quantisation, histograms,
cuts, leaves, update, pair counts, predict.

Everything here works on arrays in POSITION order: patients sorted by time descending with a stable sort; rowid[i] = the row of the
caller's matrix at position i.  Hash contract (restated): h = the 32-bit mixer below,
    hk = h(seed ^ (id * 0x85ebca6b));  hm = h((m + 1) * 0x85ebca6b + hk)
    row r is in round m's sample iff h((r + 1) * 0x9E3779B9 + hm) <= subsample;  gene j iff h((j + 1) * 0x9E3779B9 + (hm ^ 0xB5297A4D)) <= colsample."""
import numpy as np

M32 = 0xFFFFFFFF
QSCALE = 2.0 ** 32
U = 2.0 ** -53


def h32(x):
    x &= M32
    x ^= x >> 16; x = (x * 0x7FEB352D) & M32
    x ^= x >> 15; x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def round_key(seed, pid, m):
    hk = h32((seed & M32) ^ ((pid * 0x85EBCA6B) & M32))
    return h32(((m + 1) * 0x85EBCA6B + hk) & M32)


def rows_in(seed, pid, m, rowid, thr):
    hm = round_key(seed, pid, m)
    return np.array([h32(((int(r) + 1) * 0x9E3779B9 + hm) & M32) <= thr for r in rowid], dtype=bool)


def genes_in(seed, pid, m, p, thr):
    hm = round_key(seed, pid, m) ^ 0xB5297A4D
    return np.array([h32(((j + 1) * 0x9E3779B9 + hm) & M32) <= thr for j in range(p)], dtype=bool)


def threshold(rate):
    return min(int(np.floor(rate * 4294967296.0)), M32)


def positions(time):
    time = np.asarray(time, np.float64)
    order = np.argsort(-time, kind="stable")
    ts = time[order]
    gid = np.concatenate([[0], np.cumsum(ts[1:] != ts[:-1])]).astype(np.int64) if len(ts) else np.zeros(0, np.int64)
    return order, gid


def loglik(F, w, ev, gid):
    """Breslow log partial likelihood of F over the rows with w > 0 (w multiplicities), positions time-descending, gid tie groups"""
    w = np.asarray(w, np.float64)
    tr = w > 0
    if not tr.any():
        return 0.0
    c = F[tr].max()
    e = np.where(tr, w * np.exp(np.where(tr, F - c, 0.0)), 0.0)
    ll = float((w * ev * np.where(tr, F - c, 0.0)).sum())
    for u in np.unique(gid):
        d = float((w * ev)[gid == u].sum())
        if d > 0:
            ll -= d * np.log(e[gid <= u].sum())
    return ll


def gradient(F, w, ev, gid):
    """-> dict(g, h: per unit weight, 0 where w = 0; eL = e Lambda, e2Q = e^2 Q; loglik; ll_mag, ll_d for the bound)"""
    n = len(F)
    w = np.asarray(w, np.float64)
    tr = w > 0
    out = dict(g=np.zeros(n), h=np.zeros(n), eL=np.zeros(n), e2Q=np.zeros(n), loglik=0.0, ll_mag=0.0, ll_d=0.0)
    if not tr.any():
        return out
    c = F[tr].max()
    e = np.where(tr, np.exp(np.where(tr, F - c, 0.0)), 0.0)
    groups = np.unique(gid)
    a, b = np.zeros(len(groups)), np.zeros(len(groups))
    ll = float((w * ev * np.where(tr, F - c, 0.0)).sum())
    mag = float(np.abs(w * ev * np.where(tr, F - c, 0.0)).sum())
    dsum = 0.0
    for k, u in enumerate(groups):
        d = float((w * ev)[gid == u].sum())
        if d > 0:
            S = float((w * e)[gid <= u].sum())
            a[k], b[k] = d / S, d / S / S
            ll -= d * np.log(S); mag += d * abs(np.log(S)); dsum += d
    lam = np.array([a[k:].sum() for k in range(len(groups))])      # groups from k's own to the last (shortest) time
    Q = np.array([b[k:].sum() for k in range(len(groups))])
    pos = np.searchsorted(groups, gid)
    eL, e2Q = e * lam[pos], e * e * Q[pos]
    out.update(g=np.where(tr, ev - eL, 0.0), h=np.where(tr, eL - e2Q, 0.0), eL=np.where(tr, eL, 0.0), e2Q=np.where(tr, e2Q, 0.0),
               loglik=ll, ll_mag=mag, ll_d=dsum)
    return out


def quantise(g, h):
    """int64 fixed point: rint (ties to even, what llrint does) of the clamped value times 2^32"""
    return (np.rint(np.clip(g, -256.0, 1.0) * QSCALE).astype(np.int64), np.rint(np.clip(h, 0.0, 256.0) * QSCALE).astype(np.int64))


def bound_q(gr, n):
    """|q_gpu - q_ref| <= 1 + 2^32 bound, bound per position for (g, h).  u = 2^-53.  F - c is exact on both sides (c is a maximum, one
    subtraction of the same operands).  exp is within 2 ulp on either side: 4 u relative.  S_k sums at most n non-negative products
    mult * e (one rounding each) in some order: relative error <= (n + 5) u.  a = d / S adds u, b = a / S another (n + 6) u.  Lambda and Q
    sum at most n non-negative a's / b's: <= (2 n + 7) u and (3 n + 14) u; the products e Lambda and (e e) Q add the errors of e and their
    own roundings: <= (2 n + 12) u and (3 n + 24) u.  The last subtraction rounds once more: u (1 + e Lambda).  Per side, first order;
    two sides and a factor 2 of slack: bound_g = 4 (2 n + 16) u (1 + e Lambda), bound_h = 4 (3 n + 24) u (e Lambda + e^2 Q).  Clamping
    moves nothing apart; the two roundings to an integer are the 1."""
    return 4.0 * (2 * n + 16) * U * (1.0 + gr["eL"]), 4.0 * (3 * n + 24) * U * (gr["eL"] + gr["e2Q"])


def bound_loglik(gr, n):
    """log S carries S's relative error (n + 5) u as an absolute one, times d; every other term is a product and a sum of at most n + K
    terms of magnitude ll_mag in total.  Two sides, slack 2."""
    return 4.0 * U * ((2 * n + 8) * gr["ll_mag"] + (n + 5) * gr["ll_d"]) + 1e-300


def term(G, H, lam):
    """(g g) / (h + lambda) of int64 sums, g = G 2^-32 (conversion rounds to nearest, scaling exact); 0 when h + lambda <= 0"""
    g = np.asarray(G, np.int64).astype(np.float64) * 2.0 ** -32
    h = np.asarray(H, np.int64).astype(np.float64) * 2.0 ** -32 + lam
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(h > 0, (g * g) / np.where(h > 0, h, 1.0), 0.0)


def ratio(G, H, lam):
    g = float(np.int64(G)) * 2.0 ** -32
    h = float(np.int64(H)) * 2.0 ** -32 + lam
    return g / h if h > 0 else 0.0


def grow(xb, edges, qg, qh, wt, B, depth, min_leaf, l2, min_gain, lr, admitted, nn):
    """One tree from quantised gradients.  xb [p, n] bins, edges [p, B - 1], qg / qh int64 [n], wt int64 [n] (0 = not in the sample),
    admitted bool [p].  -> dict(feat, bin, thr, gain, value, n_node, G, H [nn]; node [n]: the final node of EVERY position; levels: per
    level dict(n, G, H) [2^level, p, B] prefixed histograms (zero for dead nodes and genes not admitted); excused: the nodes whose
    runner-up is within 16 * 2^-53 * (the three terms' magnitudes) of the winner)."""
    p, n = xb.shape
    t = dict(feat=np.full(nn, -1, np.int64), bin=np.zeros(nn, np.int64), thr=np.zeros(nn, np.float32), gain=np.zeros(nn), value=np.zeros(nn),
             n_node=np.zeros(nn, np.int64), G=np.zeros(nn, np.int64), H=np.zeros(nn, np.int64))
    wt, qg, qh = np.asarray(wt, np.int64), np.asarray(qg, np.int64), np.asarray(qh, np.int64)
    node = np.zeros(n, np.int64)
    t["n_node"][0], t["G"][0], t["H"][0] = wt.sum(), (wt * qg).sum(), (wt * qh).sum()
    levels, excused = [], []
    rows = np.arange(p)[:, None]
    for level in range(depth):
        nl = 1 << level
        lv = dict(n=np.zeros((nl, p, B), np.int64), G=np.zeros((nl, p, B), np.int64), H=np.zeros((nl, p, B), np.int64))
        for k in range(nl):
            s = nl - 1 + k
            if s > 0 and t["feat"][(s - 1) // 2] < 0:
                continue
            if t["n_node"][s] < 2 * min_leaf:
                continue
            idx = np.nonzero((node == s) & (wt > 0))[0]
            hn, hG, hH = np.zeros((p, B), np.int64), np.zeros((p, B), np.int64), np.zeros((p, B), np.int64)
            if len(idx):
                np.add.at(hn, (rows, xb[:, idx]), wt[idx][None, :])
                np.add.at(hG, (rows, xb[:, idx]), (wt * qg)[idx][None, :])
                np.add.at(hH, (rows, xb[:, idx]), (wt * qh)[idx][None, :])
            nL, GL, HL = np.cumsum(hn, 1), np.cumsum(hG, 1), np.cumsum(hH, 1)
            nL[~admitted], GL[~admitted], HL[~admitted] = 0, 0, 0
            lv["n"][k], lv["G"][k], lv["H"][k] = nL, GL, HL
            nT, GT, HT = t["n_node"][s], t["G"][s], t["H"][s]
            a, b, c = term(GL[:, :B - 1], HL[:, :B - 1], l2), term(GT - GL[:, :B - 1], HT - HL[:, :B - 1], l2), term(GT, HT, l2)
            gain = a + b - c
            adm = admitted[:, None] & (nL[:, :B - 1] >= min_leaf) & (nT - nL[:, :B - 1] >= min_leaf)
            score = np.where(adm & (gain > 0), gain, 0.0)
            if score.size == 0 or not (score.max() > min_gain):
                continue
            f, bb = np.unravel_index(int(np.argmax(score)), score.shape)          # row-major argmax: smallest gene, then smallest bin
            # a cut with the winner's left sums, or with the winner's RIGHT sums on its left, runs the winner's arithmetic on either side
            # (a + b commutes exactly): an exact tie there and here, which the smallest index keeps -- no rival
            # (the gain is a function of G_L and H_L alone: members with zero gradient and curvature move n_L only)
            same = (GL[:, :B - 1] == GL[f, bb]) & (HL[:, :B - 1] == HL[f, bb])
            same |= (GL[:, :B - 1] == GT - GL[f, bb]) & (HL[:, :B - 1] == HT - HL[f, bb])
            rival = np.where(same, 0.0, score)
            tol = 16.0 * U * (a[f, bb] + b[f, bb] + c)
            if score[f, bb] - rival.max() <= tol or abs(score[f, bb] - min_gain) <= tol:
                excused.append(s)
            t["feat"][s], t["bin"][s], t["thr"][s], t["gain"][s] = f, bb, edges[f, bb], gain[f, bb]
            t["n_node"][2 * s + 1], t["G"][2 * s + 1], t["H"][2 * s + 1] = nL[f, bb], GL[f, bb], HL[f, bb]
            t["n_node"][2 * s + 2], t["G"][2 * s + 2], t["H"][2 * s + 2] = nT - nL[f, bb], GT - GL[f, bb], HT - HL[f, bb]
            node = np.where(node == s, 2 * s + 1 + (xb[f] > bb), node)
        levels.append(lv)
    for s in range(nn):
        exists = s == 0 or t["feat"][(s - 1) // 2] >= 0
        if exists and t["feat"][s] < 0:
            t["value"][s] = lr * ratio(t["G"][s], t["H"][s], l2)
    t.update(node=node, levels=levels, excused=excused)
    return t


def pair_counts(F, ev, gid, mask):
    """(conc2 = 2 concordant + ties, comparable) of concordance_index(time, -F, event) over the masked positions: (i, j) comparable when i
    is an event and its time is shorter (gid larger), or equal with j censored"""
    c2 = cm = 0
    idx = np.nonzero(mask)[0]
    for i in idx:
        if not ev[i]:
            continue
        for j in idx:
            if gid[i] > gid[j] or (gid[i] == gid[j] and not ev[j]):
                cm += 1
                c2 += 2 if F[i] > F[j] else 1 if F[i] == F[j] else 0
    return c2, cm


def drop(tree, x):
    s = 0
    while tree["feat"][s] >= 0:
        s = 2 * s + 1 + (0 if x[tree["feat"][s]] <= tree["thr"][s] else 1)
    return s


def predict(trees, X, at):
    """trees: the rounds' trees of ONE problem; X raw [R, p]; at: ascending round counts -> [K, R]: sequential sums in round order"""
    F = np.zeros(len(X))
    out = np.zeros((len(at), len(X)))
    for m in range(len(trees) + 1):
        for k, a in enumerate(at):
            if a == m:
                out[k] = F
        if m < len(trees):
            F = F + np.array([trees[m]["value"][drop(trees[m], X[r])] for r in range(len(X))])
    return out


def boost(xb, edges, ev, gid, rowid, mult, B, rounds, *, lr, depth, min_leaf, l2, min_gain, subsample, colsample, pid, seed, nn, mask=None):
    """One problem start to finish -> dict(trees, F [n], loglik [M + 1], conc2, comparable [M], qg, qh [M, n], excused)"""
    p, n = xb.shape
    F = np.zeros(n)
    out = dict(trees=[], loglik=[], conc2=[], comparable=[], qg=[], qh=[], excused=0, empty_rounds=0)
    for m in range(rounds):
        gr = gradient(F, mult, ev, gid)
        qg, qh = quantise(gr["g"], gr["h"])
        wt = np.where(rows_in(seed, pid, m, rowid, subsample), mult, 0)
        adm = genes_in(seed, pid, m, p, colsample)
        out["empty_rounds"] += int(not adm.any())
        t = grow(xb, edges, qg, qh, wt, B, depth, min_leaf, l2, min_gain, lr, adm, nn)
        F = F + t["value"][t["node"]]
        out["trees"].append(t); out["loglik"].append(gr["loglik"]); out["qg"].append(qg); out["qh"].append(qh)
        out["excused"] += len(t["excused"])
        if mask is not None:
            c2, cm = pair_counts(F, ev, gid, mask)
            out["conc2"].append(c2); out["comparable"].append(cm)
    out["loglik"].append(gradient(F, mult, ev, gid)["loglik"])
    out["F"] = F
    return out
