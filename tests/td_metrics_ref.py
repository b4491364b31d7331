"""numpy float64 reference of the absolute-risk metrics (mms_td_metrics, absolute_risk.prediction_error), written the slow, obvious way
from the definitions: the two product-limit estimates loop over the distinct times and count from the raw arrays, cases and controls
are masks on the raw times, and the AUC numerator is the O(n^2) sum over (case, control) pairs.  Nothing of the kernel's form (sorted
positions, running sums, tie-group commits in risk order) is used.  With every sum comes the sum of its absolute terms: the tests'
tolerances are relative to those.  `metrics` is the literal loop form; `metrics_vec` states the same sums as array expressions (the
pair sum as a product with the n x n comparison matrix) and is what the larger GPU cases and tools/bench_td_metrics.py use -- the CPU
tests hold the two together."""
import numpy as np

REL = 1e-10        # allowed error of a sum relative to the sum of its absolute terms (the criterion of test_gpu_gene_screen.py)
EPS = 2.0 ** -53


def product_limits(t, e, w):
    """-> (u, G, KM, nfac): the distinct times ascending, G(u) and KM(u) right after each (lists of floats) and the number of factors
    multiplied so far.  G: factor (n_u - c_u) / n_u where n_u = sum w [t >= u] - sum w [t = u, e] > 0; KM: (a_u - d_u) / a_u where
    a_u = sum w [t >= u] > 0.  ONE float division of two integers per factor."""
    u = np.unique(t)
    g, km, G, KM = 1.0, 1.0, [], []
    for v in u:
        at = int(w[t >= v].sum())
        d = int(w[(t == v) & e].sum())
        c = int(w[(t == v) & ~e].sum())
        nu = at - d
        if at > 0:
            km *= float(at - d) / float(at)
        if nu > 0:
            g *= float(nu - c) / float(nu)
        G.append(g)
        KM.append(km)
    return u, G, KM


def _upto(u, vals, x, strict):
    """the product over u <= x (strict: u < x): 1.0 before the first time"""
    k = int(np.searchsorted(u, x, side="left" if strict else "right"))
    return (1.0 if k == 0 else vals[k - 1]), k


def _labels(time, event, w):
    t = np.asarray(time, dtype=np.float64).reshape(-1)
    e = np.asarray(event).reshape(-1) != 0
    w = np.ones(len(t), np.int64) if w is None else np.asarray(w).astype(np.int64).reshape(-1)
    return t, e, w


def _omega(u, G, t, e, w):
    """case weights w_i / G(t_i-) of the drawn events, 0 elsewhere"""
    om = np.zeros(len(t))
    for i in range(len(t)):
        if e[i] and w[i] > 0:
            om[i] = w[i] / _upto(u, G, t[i], True)[0]
    return om


def metrics(time, event, risk, surv, horizons, w=None):
    """One replicate, literally.  risk [M, n], surv [M, n, H], horizons [H], w [n] integer multiplicities (None: all ones) -> dict of
    G, km, wcase, wctrl [H], nfac [H] (the factors in G(tau_h) / KM(tau_h)), brier, auc_num [M, H] and abs_wcase / abs_brier /
    abs_auc_num (the sums of the absolute terms; every term here is non-negative), plus W = sum w."""
    t, e, w = _labels(time, event, w)
    risk, surv, tau = np.atleast_2d(np.asarray(risk, dtype=np.float64)), np.asarray(surv, dtype=np.float64), np.asarray(horizons, dtype=np.float64)
    M, n, H = surv.shape
    u, G, KM = product_limits(t, e, w)
    om = _omega(u, G, t, e, w)
    W = int(w.sum())
    out = dict(G=np.zeros(H), km=np.zeros(H), wcase=np.zeros(H), wctrl=np.zeros(H), nfac=np.zeros(H, np.int64), brier=np.zeros((M, H)),
               auc_num=np.zeros((M, H)), W=W)
    for h in range(H):
        gt, k = _upto(u, G, tau[h], False)
        out["G"][h], out["km"][h], out["nfac"][h] = gt, _upto(u, KM, tau[h], False)[0], k
        case = [i for i in range(n) if t[i] <= tau[h] and e[i]]
        ctrl = [j for j in range(n) if t[j] > tau[h]]
        out["wcase"][h] = sum(om[i] for i in case)
        out["wctrl"][h] = sum(int(w[j]) for j in ctrl)
        for m in range(M):
            a = sum(om[i] * surv[m, i, h] ** 2 for i in case)
            b = sum(w[j] * (1.0 - surv[m, j, h]) ** 2 for j in ctrl)
            out["brier"][m, h] = (a + (b / gt if out["wctrl"][h] > 0 else 0.0)) / W
            s = 0.0
            for i in case:
                for j in ctrl:
                    s += om[i] * w[j] * (1.0 if risk[m, i] > risk[m, j] else 0.5 if risk[m, i] == risk[m, j] else 0.0)
            out["auc_num"][m, h] = s
    out.update(abs_wcase=out["wcase"].copy(), abs_brier=out["brier"].copy(), abs_auc_num=out["auc_num"].copy())
    return out


def metrics_vec(time, event, risk, surv, horizons, w=None):
    """metrics as array expressions (the product-limit loop stays): masks [H, n] and the pair sum as A K B' with K the n x n comparison
    matrix [eta_i > eta_j] + 1/2 [eta_i = eta_j]."""
    t, e, w = _labels(time, event, w)
    risk, surv, tau = np.atleast_2d(np.asarray(risk, dtype=np.float64)), np.asarray(surv, dtype=np.float64), np.asarray(horizons, dtype=np.float64)
    u, G, KM = product_limits(t, e, w)
    Ga, KMa = np.concatenate([[1.0], G]), np.concatenate([[1.0], KM])
    with np.errstate(divide="ignore"):
        om = np.where(e & (w > 0), w / np.where(e & (w > 0), Ga[np.searchsorted(u, t, side="left")], 1.0), 0.0)
    k = np.searchsorted(u, tau, side="right")
    gt, W = Ga[k], int(w.sum())
    A = np.where((t[None, :] <= tau[:, None]) & e[None, :], om[None, :], 0.0)            # [H, n] case weights
    B = np.where(t[None, :] > tau[:, None], w[None, :], 0).astype(np.float64)            # [H, n] control weights
    wcase, wctrl = A.sum(1), B.sum(1)
    S = np.moveaxis(surv, 2, 1)                                                          # [M, H, n]
    with np.errstate(divide="ignore", invalid="ignore"):
        second = np.where(wctrl > 0, (B * (1.0 - S) ** 2).sum(2) / np.where(wctrl > 0, gt, 1.0), 0.0)
    brier = ((A * S * S).sum(2) + second) / W
    K = (risk[:, :, None] > risk[:, None, :]) + 0.5 * (risk[:, :, None] == risk[:, None, :])     # [M, n, n]
    num = ((A[None] @ K) * B[None]).sum(2)
    return dict(G=gt, km=KMa[k], wcase=wcase, wctrl=wctrl, nfac=k.astype(np.int64), brier=brier, auc_num=num, W=W, abs_wcase=wcase.copy(),
                abs_brier=brier.copy(), abs_auc_num=num.copy())


def resampled(time, event, risk, surv, w):
    """the arrays of the literal resample that draws patient i w_i times -> (time, event, risk, surv)"""
    idx = np.repeat(np.arange(len(w)), np.asarray(w).astype(np.int64))
    return np.asarray(time)[idx], np.asarray(event)[idx], np.atleast_2d(risk)[:, idx], np.asarray(surv)[:, idx, :]


def trapezoid_mean(y, x):
    """sum of the trapezoids of y over x / (x[-1] - x[0]) along the last axis; y itself for a single point"""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    if len(x) == 1:
        return y[..., 0]
    tot = np.zeros(y.shape[:-1])
    for k in range(len(x) - 1):
        tot = tot + (x[k + 1] - x[k]) * (y[..., k] + y[..., k + 1]) / 2.0
    return tot / (x[-1] - x[0])


def derived(m):
    """one replicate's metrics -> auc [M, H] (NaN without a case or a control), brier_null [H], ipa [M, H]"""
    with np.errstate(divide="ignore", invalid="ignore"):
        den = m["wcase"] * m["wctrl"]
        auc = np.where(den > 0, m["auc_num"] / np.where(den > 0, den, 1.0), np.nan)
        ctrl = np.where(m["wctrl"] > 0, m["wctrl"] * (1 - m["km"]) ** 2 / np.where(m["wctrl"] > 0, m["G"], 1.0), 0.0)
        null = (m["wcase"] * m["km"] ** 2 + ctrl) / m["W"]
        return auc, null, 1.0 - m["brier"] / null
