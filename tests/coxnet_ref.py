"""float64 reference of the elastic-net Cox objective, written from the definitions (include/mmsurv.h: CoxnetP), not from the kernel.

A problem: X [n, G] (the list rows' genes, already divided by the per-gene scale), time [n] (any order for the mask form, descending for the
cumulative form), event [n], integer multiplicities m [n], lam, alpha.
    F(beta) = (1/n_p) [ -sum m e eta + sum_u d_u log S0_u ] + lam (alpha |beta|_1 + (1 - alpha)/2 |beta|^2),   n_p = sum m
    r_k = m_k e_k - m_k exp(eta_k) c_k,  c_k = sum_{u <= t_k} d_u / S0_u;  gradient of the smooth part: -X'r / n_p + lam (1 - alpha) beta
Every function also returns the SUM OF ABSOLUTE TERMS of what it computes: the tests' tolerances are 1e-10 times those."""
import numpy as np

MASK_MAX = 300


def _shift(eta, m):
    on = m > 0
    return float(eta[on].max()) if on.any() else 0.0


def loss_resid_mask(eta, time, event, m):
    """Explicit risk sets, O(n^2) -> (loss, r, |loss| terms, |r| terms [n])."""
    eta, time, m = np.asarray(eta, np.float64), np.asarray(time, np.float64), np.asarray(m, np.float64)
    e = (np.asarray(event) != 0).astype(np.float64)
    on = m > 0
    d = np.where(on, eta - _shift(eta, m), 0.0)
    w = np.where(on, m * np.exp(d), 0.0)
    me = np.where(on, m * e, 0.0)
    us = np.unique(time[me > 0])
    risk = time[None, :] >= us[:, None]                      # [u, k]: k is at risk at u
    S0 = (risk * w[None, :]).sum(1)
    du = ((time[None, :] == us[:, None]) * me[None, :]).sum(1)
    loss = -(me * d).sum() + (du * np.log(S0)).sum()
    labs = np.abs(me * d).sum() + np.abs(du * np.log(S0)).sum()
    c = ((us[:, None] <= time[None, :]) * (du / S0)[:, None]).sum(0)
    r = np.where(on, me - w * c, 0.0)
    return loss, r, labs, np.where(on, me + w * c, 0.0)


def loss_resid_cum(eta, time, event, m):
    """Cumulative sums over a time-descending list -> the same four results."""
    eta, time, m = np.asarray(eta, np.float64), np.asarray(time, np.float64), np.asarray(m, np.float64)
    n = len(time)
    if n == 0:
        return 0.0, np.zeros(0), 0.0, np.zeros(0)
    assert (np.diff(time) <= 0).all(), "time descending"
    e = (np.asarray(event) != 0).astype(np.float64)
    on = m > 0
    d = np.where(on, eta - _shift(eta, m), 0.0)
    w = np.where(on, m * np.exp(d), 0.0)
    me = np.where(on, m * e, 0.0)
    first = np.concatenate([[True], time[1:] != time[:-1]])
    gid = np.cumsum(first) - 1
    last = np.concatenate([np.nonzero(first)[0][1:] - 1, [n - 1]])
    S0 = np.cumsum(w)[last]
    du = np.bincount(gid, weights=me, minlength=len(last))
    ev = du > 0
    logS = np.log(np.where(ev, S0, 1.0))
    h = np.where(ev, du / np.where(ev, S0, 1.0), 0.0)
    loss = -(me * d).sum() + (du * logS).sum()
    labs = np.abs(me * d).sum() + np.abs(du * logS).sum()
    c = np.cumsum(h[::-1])[::-1][gid]
    r = np.where(on, me - w * c, 0.0)
    return loss, r, labs, np.where(on, me + w * c, 0.0)


def loss_resid(eta, time, event, m):
    return (loss_resid_mask if len(time) <= MASK_MAX else loss_resid_cum)(eta, time, event, m)


def evaluate(X, time, event, m, lam, alpha, beta):
    """-> dict: eta, r, loss (not divided by n), n, grad, f (smooth part), obj, kkt and the term bounds eta_abs, r_abs, loss_abs, grad_abs."""
    X, beta, m = np.asarray(X, np.float64), np.asarray(beta, np.float64), np.asarray(m, np.float64)
    eta = X @ beta
    loss, r, labs, rabs = loss_resid(eta, time, event, m)
    n = m.sum()
    invn = 1.0 / n if n > 0 else 0.0
    l1, l2 = lam * alpha, lam * (1.0 - alpha)
    g = -(X.T @ r) * invn + l2 * beta
    f = loss * invn + 0.5 * l2 * (beta * beta).sum()
    return dict(eta=eta, r=r, loss=loss, n=n, grad=g, f=f, obj=f + l1 * np.abs(beta).sum(), kkt=kkt(beta, g, l1),
                eta_abs=np.abs(X) @ np.abs(beta), r_abs=rabs, loss_abs=labs,
                grad_abs=(np.abs(X).T @ rabs) * invn + np.abs(l2 * beta))


def kkt(beta, g, l1):
    rho = np.where(beta != 0, np.abs(g + l1 * np.sign(beta)), np.maximum(np.abs(g) - l1, 0.0))
    return float(rho.max()) if len(rho) else 0.0


def soft(z, t):
    return np.sign(z) * np.maximum(np.abs(z) - t, 0.0)


def solve(X, time, event, m, lam, alpha, beta0=None, tol=1e-6, max_iter=5000, floor=False):
    """Replica of the solver: monotone proximal gradient, step 1 at the start, x 1.25 on accept, / 2 on reject, accept iff
    f(trial) <= f + <g, D> + |D|^2 / (2 s) + 1e-12 max(1, |f|); converged when the KKT residual of the kept pair is <= tol.
    -> dict(beta, grad, f, obj, kkt, iters, status (1 converged / 2 max_iter), step).  floor=True: ignore tol, run max_iter iterations and
    report the smallest KKT residual seen as `kkt_floor`."""
    X = np.asarray(X, np.float64)
    l1 = lam * alpha
    beta = np.zeros(X.shape[1]) if beta0 is None else np.asarray(beta0, np.float64).copy()
    ev = evaluate(X, time, event, m, lam, alpha, beta)
    f, g, s, it = ev["f"], ev["grad"], 1.0, 0
    rho = kkt(beta, g, l1)
    best = rho
    status = 1 if (rho <= tol and not floor) else 0
    while status == 0:
        trial = soft(beta - s * g, s * l1)
        ev = evaluate(X, time, event, m, lam, alpha, trial)
        dlt = trial - beta
        it += 1
        if ev["f"] <= f + g @ dlt + (dlt @ dlt) / (2.0 * s) + 1e-12 * max(1.0, abs(f)):
            beta, g, f, s = trial, ev["grad"], ev["f"], s * 1.25
            rho = kkt(beta, g, l1)
            best = min(best, rho)
            if rho <= tol and not floor:
                status = 1
                break
        else:
            s *= 0.5
        if it >= max_iter:
            status = 2
    return dict(beta=beta, grad=g, f=f, obj=f + l1 * np.abs(beta).sum(), kkt=rho, iters=it, status=status, step=s, kkt_floor=best)


class Backend:
    """coxnet.py's backend interface on the host: the same problems through this reference (x: numpy [N, G])."""

    def _X(self, x, rr, scale, p):
        X = np.asarray(x, np.float64)[rr.rows]
        return X if scale is None else X / scale[p][None, :]

    def __init__(self):
        self.cache = {}                                             # fits by problem: the two criteria of a test share them

    def fit(self, x, rr, mult, lam, alpha, scale=None, beta=None, tol=1e-6, max_iter=5000):
        key = tuple(np.ascontiguousarray(a).tobytes() for a in (rr.rows, mult, lam, alpha) + (() if scale is None else (scale,))) + (tol, max_iter)
        if beta is None and key in self.cache:
            return self.cache[key]
        out = [solve(self._X(x, rr, scale, p), rr.time, rr.event, mult[p], float(lam[p]), float(alpha[p]),
                     None if beta is None else beta[p], tol, max_iter) for p in range(len(mult))]
        res = {k: np.array([o[k] for o in out]) for k in ("beta", "grad", "f", "obj", "kkt", "iters", "status", "step")}
        if beta is None:
            self.cache[key] = res
        return res

    def evaluate(self, x, rr, mult, lam, alpha, beta, scale=None):
        out = [evaluate(self._X(x, rr, scale, p), rr.time, rr.event, mult[p], float(lam[p]), float(alpha[p]), beta[p])
               for p in range(len(mult))]
        return {k: np.array([o[k] for o in out]) for k in ("eta", "r", "loss", "n", "grad", "f", "obj", "kkt")}
