"""numpy float64 replica of the random survival forest contract (include/mmsurv.h: RsfSplitP; survival_forest.py) -- test infrastructure,
written the slow, obvious way and sharing no code with the package: hash, bootstrap draws, candidates, statistic, ties, leaves,
mortality, prediction.

Hash contract (restated): h = the 32-bit mixer below, mulhi(a, k) = (a * k) >> 32,
    ht = h(seed ^ (id * 0x85ebca6b));  draw k of m: member mulhi(h((k + 1) * 0x9E3779B9 + h(ht ^ 0xB5297A4D)), m)
    hn = h((s + 1) * 0x9E3779B9 + ht);  hf = h((j + 1) * 0x9E3779B9 + hn), feature mulhi(hf, p)
    threshold q: x[feature] of in-node in-bag member mulhi(h((q + 1) * 0x85ebca6b + hf), members) in time-descending (stable) order.
Everything here works on arrays in POSITION order: patients sorted by time descending with a stable sort."""
import numpy as np

M = 0xFFFFFFFF


def h32(x):
    x &= M
    x ^= x >> 16; x = (x * 0x7FEB352D) & M
    x ^= x >> 15; x = (x * 0x846CA68B) & M
    x ^= x >> 16
    return x


def tree_key(seed, tid):
    return h32((seed & M) ^ ((tid * 0x85EBCA6B) & M))


def draws(seed, tid, m):
    base = h32(tree_key(seed, tid) ^ 0xB5297A4D)
    return np.array([(h32(((k + 1) * 0x9E3779B9 + base) & M) * m) >> 32 for k in range(m)], dtype=np.int64)


def bootstrap_mults(trains, n, n_trees, seed):
    out = np.zeros((len(trains) * n_trees, n), dtype=np.int64)
    for f, tr in enumerate(trains):
        tr = np.asarray(tr, dtype=np.int64)
        for j in range(n_trees):
            for k in draws(seed, f * n_trees + j, len(tr)):
                out[f * n_trees + j, tr[k]] += 1
    return out


def positions(time):
    """-> (order: stable time-descending, gid: tie group number per position)"""
    time = np.asarray(time, np.float64)
    order = np.argsort(-time, kind="stable")
    ts = time[order]
    gid = np.concatenate([[0], np.cumsum(ts[1:] != ts[:-1])]).astype(np.int64) if len(ts) else np.zeros(0, np.int64)
    return order, gid


def logrank_uv(w, e, g, left):
    """The statistic of one candidate over a node's members in position order (w multiplicities, e events, g tie groups, left flags):
    U = sum (d_L - d Y_L / Y), V = sum d (Y - d) Y_L (Y - Y_L) / (Y^2 (Y - 1)) over the tie groups with events (V's term 0 at Y = 1).
    -> (U, V, n_L, d_L, terms K, magnitude D_L + sum d Y_L / Y)"""
    U = V = mag = 0.0
    K = 0
    for u in np.unique(g):
        at = g <= u                                   # time >= the group's
        here = g == u
        d = float((w * e)[here].sum())
        if d == 0:
            continue
        Y, YL = float(w[at].sum()), float(w[at & left].sum())
        dL = float((w * e)[here & left].sum())
        U += dL - d * YL / Y
        mag += dL + d * YL / Y
        if Y > 1:
            V += d * (Y - d) * YL * (Y - YL) / (Y * Y * (Y - 1.0))
        K += 1
    return U, V, int(w[left].sum()), int((w * e)[left].sum()), K, mag


def candidates(X, ev, gid, mult, member, s, tid, seed, mtry, nsplit, min_leaf):
    """Every candidate of node s of tree tid.  X [n, p] float32 in position order; member: bool [n], the node's in-bag positions.
    -> dict of arrays over c = j * nsplit + q: feat, thr, U, V, chi2, n_left, d_left, adm, K, mag; and best (-1: a leaf), n, d."""
    idx = np.nonzero(member)[0]
    m, p = len(idx), X.shape[1]
    w, e, g = mult[idx].astype(np.int64), ev[idx].astype(np.int64), gid[idx]
    n_node, d_node = int(w.sum()), int((w * e).sum())
    C = mtry * nsplit
    out = dict(feat=np.zeros(C, np.int64), thr=np.zeros(C, np.float32), U=np.zeros(C), V=np.zeros(C), chi2=np.zeros(C),
               n_left=np.zeros(C, np.int64), d_left=np.zeros(C, np.int64), adm=np.zeros(C, bool), K=np.zeros(C, np.int64), mag=np.zeros(C))
    hn = h32(((s + 1) * 0x9E3779B9 + tree_key(seed, tid)) & M)
    for j in range(mtry):
        hf = h32(((j + 1) * 0x9E3779B9 + hn) & M)
        for q in range(nsplit):
            r = (h32(((q + 1) * 0x85EBCA6B + hf) & M) * m) >> 32
            out["feat"][j * nsplit + q] = (hf * p) >> 32
            out["thr"][j * nsplit + q] = X[idx[r], (hf * p) >> 32]
    if C and m:
        # logrank_uv for all candidates at once: the same sums, the groups as columns (sequential cumsum along the groups)
        left = X[idx][:, out["feat"]].T <= out["thr"][:, None]                  # [C, m]
        last = np.concatenate([g[1:] != g[:-1], [True]])
        we = w * e
        Y, dc = np.cumsum(w)[last].astype(np.float64), np.cumsum(we)[last]
        d = np.diff(dc, prepend=0).astype(np.float64)
        YL = np.cumsum(left * w, axis=1)[:, last].astype(np.float64)
        dL = np.diff(np.cumsum(left * we, axis=1)[:, last], prepend=0, axis=1).astype(np.float64)
        sel = d > 0
        Y, d, YL, dL = Y[sel], d[sel], YL[:, sel], dL[:, sel]
        if sel.any():
            exp = d * YL / Y
            out["U"] = np.cumsum(dL - exp, axis=1)[:, -1]
            out["mag"] = np.cumsum(dL + exp, axis=1)[:, -1]
            with np.errstate(invalid="ignore", divide="ignore"):
                tv = np.where(Y > 1, d * (Y - d) * YL * (Y - YL) / (Y * Y * (Y - 1.0)), 0.0)
            out["V"] = np.cumsum(tv, axis=1)[:, -1]
        out["K"][:] = int(sel.sum())
        out["seq"] = np.concatenate([YL, dL], axis=1)                              # what the statistic is a function of
        out["n_left"], out["d_left"] = (left * w).sum(1), (left * we).sum(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["chi2"] = np.where(out["V"] > 0, out["U"] * out["U"] / out["V"], 0.0)
        out["adm"] = (out["n_left"] >= min_leaf) & (n_node - out["n_left"] >= min_leaf)
    score = np.where(out["adm"], out["chi2"], 0.0)
    best = int(np.argmax(score)) if C and score.max() > 0 else -1          # argmax: the first (smallest c) of equal maxima
    out.update(best=best, n=n_node, d=d_node)
    return out


def bound_uv(K, mag, V):
    """|U_gpu - U_ref| and |V_gpu - V_ref| bounds.  Either side forms each of K terms with at most 4 roundings (a quotient, products, the
    fused or plain add) and adds it to a running sum whose magnitude never exceeds `mag` = D_L + sum d Y_L / Y (U) or V (all of V's terms
    are >= 0): at most (K + 4) unit roundoffs 2^-53 of that magnitude per side; both sides and a factor 2 of slack: 4 (K + 4) 2^-53."""
    eps = 4.0 * (K + 4) * 2.0 ** -53
    return eps * mag, eps * V


def chi2_rel_bound(c, i):
    """relative bound on chi2 = U^2 / V of candidate i of candidates() output c: 2 |dU| / |U| + dV / V (+ 3 roundings)"""
    bu, bv = bound_uv(c["K"][i], c["mag"][i], c["V"][i])
    if c["V"][i] <= 0 or c["U"][i] == 0:
        return 0.0
    return 2.0 * bu / abs(c["U"][i]) + bv / c["V"][i] + 3 * 2.0 ** -53


def grow(X, ev, gid, mult, tid, seed, mtry, nsplit, min_leaf, max_depth):
    """One tree -> dict(feat, thr, stat, n_node, d_node [nn], node [n] (final node of in-bag positions, -1 out of bag), margin: the
    smallest relative gap between a node's winner and its best admissible rival of another (feat, thr), with the rival's bound)"""
    nn = (2 << max_depth) - 1
    t = dict(feat=np.full(nn, -1, np.int64), thr=np.zeros(nn, np.float32), stat=np.zeros(nn), n_node=np.zeros(nn, np.int64),
             d_node=np.zeros(nn, np.int64))
    node = np.where(mult > 0, 0, -1)
    t["n_node"][0], t["d_node"][0] = int(mult.sum()), int((mult * ev).sum())
    margins = []
    for s in range((1 << max_depth) - 1):
        if s > 0 and t["feat"][(s - 1) // 2] < 0:
            continue
        member = node == s
        if t["n_node"][s] < 2 * min_leaf or not member.any():
            continue
        c = candidates(X, ev, gid, mult, member, s, tid, seed, mtry, nsplit, min_leaf)
        b = c["best"]
        if b < 0:
            continue
        margins.append(node_margin(c))
        f, thr = int(c["feat"][b]), c["thr"][b]
        t["feat"][s], t["thr"][s], t["stat"][s] = f, thr, c["chi2"][b]
        t["n_node"][2 * s + 1], t["d_node"][2 * s + 1] = c["n_left"][b], c["d_left"][b]
        t["n_node"][2 * s + 2], t["d_node"][2 * s + 2] = c["n"] - c["n_left"][b], c["d"] - c["d_left"][b]
        node = np.where(member, 2 * s + 1 + (X[:, f] > thr), node)
    t["node"], t["margins"] = node, margins
    return t


def node_margin(c):
    """(relative gap between the winner's chi2 and the best admissible candidate whose left counts differ at some tie group, the sum of
    both candidates' relative bounds).  The gap is inf without such a rival."""
    b = c["best"]
    score = np.where(c["adm"], c["chi2"], 0.0)
    # a candidate with the winner's Y_L and d_L at every tie group with events runs the winner's arithmetic on either side: an exact tie
    # there and here, which the smallest index keeps -- no rival
    same = (c["seq"] == c["seq"][b]).all(1)
    rival = np.where(same, -1.0, score)
    if rival.max() <= 0:
        return np.inf, chi2_rel_bound(c, b)
    r = int(np.argmax(rival))
    return (score[b] - rival[r]) / score[b], chi2_rel_bound(c, b) + chi2_rel_bound(c, r)


def leaf_hazard(time_pos, ev, mult, member):
    """Nelson-Aalen of a leaf's members -> (event times u ascending, increments d_u / Y_u)"""
    w, e, t = mult[member].astype(np.float64), ev[member].astype(np.float64), time_pos[member]
    us = np.unique(t[(e > 0)])
    return us, np.array([(w * e)[t == u].sum() / w[t >= u].sum() for u in us])


def leaves(time_pos, ev, mult, tree, train_mask, horizons):
    """-> (mort [nn], H [nn, nh]) of one grown tree: H(t) = sum_{u <= t} d_u / Y_u, mort = sum of H over the distinct event times of the
    tree's training set (train_mask over positions)."""
    nn = len(tree["feat"])
    mort, H = np.zeros(nn), np.zeros((nn, len(horizons)))
    tj = np.unique(time_pos[train_mask & (ev != 0)])
    for s in range(nn):
        if tree["feat"][s] >= 0 or tree["n_node"][s] <= 0:
            continue
        us, inc = leaf_hazard(time_pos, ev, mult, tree["node"] == s)
        mort[s] = sum(inc[us <= t].sum() for t in tj)
        H[s] = [inc[us <= h].sum() for h in horizons]
    return mort, H


def drop(tree, x):
    s = 0
    while tree["feat"][s] >= 0:
        s = 2 * s + 1 + (0 if x[tree["feat"][s]] <= tree["thr"][s] else 1)
    return s


def predict(trees, morts, Hs, X, use=None):
    """-> (mortality [R], H [R, nh], count [R]): means over the trees use[t, r] admits (None: all), in ascending tree order; NaN without
    a tree."""
    R, nh = len(X), Hs[0].shape[1]
    mo, H, cnt = np.zeros(R), np.zeros((R, nh)), np.zeros(R, np.int64)
    for r in range(R):
        for t, tree in enumerate(trees):
            if use is not None and not use[t, r]:
                continue
            s = drop(tree, X[r])
            mo[r] += morts[t][s]; H[r] += Hs[t][s]; cnt[r] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, mo / cnt, np.nan), np.where(cnt[:, None] > 0, H / cnt[:, None], np.nan), cnt


def forest(X, time_pos, ev, gid, mults, tids, seed, mtry, nsplit, min_leaf, max_depth, train_masks, wset, horizons):
    """Grow and finish every tree -> (trees, morts, Hs)"""
    trees = [grow(X, ev, gid, mults[i], int(tids[i]), seed, mtry, nsplit, min_leaf, max_depth) for i in range(len(mults))]
    fin = [leaves(time_pos, ev, mults[i], trees[i], train_masks[wset[i]], horizons) for i in range(len(mults))]
    return trees, [f[0] for f in fin], [f[1] for f in fin]
