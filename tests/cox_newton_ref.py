"""numpy float64 reference of the multivariable Cox fit (mms_cox_newton, multivariable.cox_fit / analyse), written the slow, obvious way
from the definitions: `evaluate` loops over the distinct event times and forms every risk set as a mask on the raw times (O(n^2)),
nothing of the kernel's form (sorted positions, running sums, tie-group flags) is used, and `fit` is the solver of include/mmsurv.h
(CoxNewtonP) written literally.  With every sum comes the sum of its absolute terms: the tests' tolerances are relative to those.
`fit` also reports the MARGIN of its decisions -- the smallest factor by which the two sides of any comparison it took were apart -- so a
test can tell a decision that rounding could flip from one it cannot.  `evaluate_cumsum` states the same sums as cumulative sums over
the time-descending order; tools/bench_cox_newton.py times it as the CPU form, and the CPU tests hold the two together."""
import numpy as np

REL = 1e-10        # allowed error of a sum relative to the sum of its absolute terms (the criterion of tests/td_metrics_ref.py)
EPS = 2.0 ** -53
PIVOT = 1e-10      # a pivot must exceed PIVOT * the largest diagonal entry
SLACK = 1e-12      # a step is accepted when l does not fall by more than SLACK * max(1, |l|)
HALVINGS = 20
STATUS = {1: "converged", 2: "max_iter", 3: "singular", 4: "monotone likelihood", 5: "no step accepted", 6: "no events"}


def _arrays(x, time, event, w):
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(len(x), -1)
    t = np.asarray(time, dtype=np.float64).reshape(-1)
    e = np.asarray(event).reshape(-1) != 0
    w = np.ones(len(t), np.int64) if w is None else np.asarray(w).astype(np.int64).reshape(-1)
    return x, t, e, w


def _eta(x, w, beta, cols):
    """x beta over the model's columns, shifted by its maximum over the drawn rows; r = w exp(eta)"""
    eta = np.zeros(len(x))
    for a in cols:
        eta = eta + x[:, a] * beta[a]
    if (w > 0).any():
        eta = eta - eta[w > 0].max()
    return eta, np.where(w > 0, w * np.exp(eta), 0.0)


def evaluate(x, time, event, w, beta, cols):
    """One evaluation at beta [p] (zero outside cols) -> dict(l, g [p], I [p, p], abs_l, abs_g, abs_I, d): Breslow ties, a multiplicity
    is a repeat.  Entries outside cols are 0.  d = sum w e."""
    x, t, e, w = _arrays(x, time, event, w)
    p = x.shape[1]
    beta = np.asarray(beta, dtype=np.float64)
    eta, r = _eta(x, w, beta, cols)
    cols = list(cols)
    l = al = 0.0
    g, ag, I, aI = np.zeros(len(cols)), np.zeros(len(cols)), np.zeros((len(cols),) * 2), np.zeros((len(cols),) * 2)
    for u in np.unique(t[e]):
        grp = (t == u) & e
        d = int(w[grp].sum())
        if d == 0:
            continue
        risk = t >= u                                                       # the risk set, from the raw times
        rk, xk, wg, xg = r[risk], x[risk][:, cols], w[grp], x[grp][:, cols]
        S0 = float(rk.sum())
        S1, A1 = (rk[:, None] * xk).sum(0), (rk[:, None] * np.abs(xk)).sum(0)
        S2 = (rk[:, None, None] * xk[:, :, None] * xk[:, None, :]).sum(0)
        A2 = (rk[:, None, None] * np.abs(xk[:, :, None] * xk[:, None, :])).sum(0)
        l += float((wg * eta[grp]).sum()) - d * np.log(S0)
        al += float((wg * np.abs(eta[grp])).sum()) + d * abs(np.log(S0))
        g += (wg[:, None] * xg).sum(0) - d * S1 / S0
        ag += (wg[:, None] * np.abs(xg)).sum(0) + d * A1 / S0
        I += d * (S2 / S0 - S1[:, None] * S1[None, :] / S0 ** 2)
        aI += d * (A2 / S0 + A1[:, None] * A1[None, :] / S0 ** 2)
    full = lambda v: _scatter(v, cols, p)
    return dict(l=l, g=full(g), I=full(I), abs_l=al, abs_g=full(ag), abs_I=full(aI), d=int((w * e).sum()))


def _scatter(v, cols, p):
    """a vector / matrix on cols -> its place among p columns, zero elsewhere"""
    out = np.zeros((p,) * v.ndim)
    out[np.ix_(*([cols] * v.ndim))] = v
    return out


def evaluate_cumsum(x, time, event, w, beta, cols):
    """evaluate's l, g, I as cumulative sums over the patients in time-descending order (no absolute sums)"""
    x, t, e, w = _arrays(x, time, event, w)
    p = x.shape[1]
    cols = list(cols)
    o = np.argsort(-t, kind="stable")
    xs, ts, es, ws = x[o][:, cols], t[o], e[o], w[o]
    eta, r = _eta(xs, ws, np.asarray(beta, dtype=np.float64)[cols], range(len(cols)))
    last = np.concatenate([ts[1:] != ts[:-1], [True]])
    S0 = np.cumsum(r)[last]
    S1 = np.cumsum(r[:, None] * xs, 0)[last]
    S2 = np.cumsum(r[:, None, None] * xs[:, :, None] * xs[:, None, :], 0)[last]
    gid = np.concatenate([[0], np.cumsum(last)[:-1]])
    we = np.where(es, ws, 0).astype(np.float64)
    d = np.bincount(gid, we, minlength=len(S0))
    k = d > 0
    m = S1[k] / S0[k, None]
    l = float((we * eta).sum() - (d[k] * np.log(S0[k])).sum())
    gc = (we[:, None] * xs).sum(0) - (d[k, None] * m).sum(0)
    Ic = (d[k, None, None] * (S2[k] / S0[k, None, None] - m[:, :, None] * m[:, None, :])).sum(0)
    g, I = np.zeros(p), np.zeros((p, p))
    g[cols] = gc
    I[np.ix_(cols, cols)] = Ic
    return dict(l=l, g=g, I=I, d=int(we.sum()))


def cholesky(I, cols):
    """Left-looking I = L L' on cols -> (L or None when a pivot is not > PIVOT * the largest diagonal entry, margin of the pivot tests)"""
    A = I[np.ix_(cols, cols)]
    m = len(cols)
    thr = PIVOT * max([A[j, j] for j in range(m)] + [0.0])
    L = np.zeros((m, m))
    margin = np.inf
    for j in range(m):
        piv = A[j, j] - sum(L[j, k] ** 2 for k in range(j))
        if not piv > thr:
            return None, min(margin, thr / piv if piv > 0 else np.inf)
        margin = min(margin, piv / thr if thr > 0 else np.inf)
        L[j, j] = np.sqrt(piv)
        for i in range(j + 1, m):
            L[i, j] = (A[i, j] - sum(L[i, k] * L[j, k] for k in range(j))) / L[j, j]
    return L, margin


def newton_step(I, g, cols):
    """-> (delta [p], se [p] (NaN outside cols), pivot margin), or (None, None, margin) when I is singular on cols"""
    p = len(g)
    L, margin = cholesky(I, cols)
    if L is None:
        return None, None, margin
    Z = np.linalg.solve(L, np.eye(len(cols))) if len(cols) else np.zeros((0, 0))       # L^-1; I^-1 = Z' Z
    delta, se = np.zeros(p), np.full(p, np.nan)
    delta[cols] = Z.T @ (Z @ g[cols])
    se[cols] = np.sqrt((Z * Z).sum(0))
    return delta, se, margin


def _apart(a, b):
    """the factor by which two non-negative numbers are apart"""
    lo, hi = min(a, b), max(a, b)
    return np.inf if lo <= 0 else hi / lo


def fit(x, time, event, w=None, cols=None, tol=1e-9, max_iter=30, beta_max=30.0, evaluate=evaluate):
    """The solver of CoxNewtonP, literally -> dict(beta, se, loglik, loglik0, iters, status, info, margins, margin).  margins: per kind
    of decision (convergence, pivot, acceptance, bound) the smallest factor by which the two sides of such a comparison were apart;
    margin: the smallest of them.  (A convergence decision that rounding flips costs or saves one iteration; only the other three,
    or max_iter, can change the status.)"""
    x, t, e, w = _arrays(x, time, event, w)
    p = x.shape[1]
    cols = list(range(p)) if cols is None else sorted(cols)
    beta, nan = np.zeros(p), np.full(p, np.nan)
    ev = evaluate(x, t, e, w, beta, cols)
    mg = dict(convergence=np.inf, pivot=np.inf, acceptance=np.inf, bound=np.inf)
    def note(kind, factor):
        mg[kind] = min(mg[kind], factor)
    out = lambda status, se, it: dict(beta=beta, se=se, loglik=ev["l"], loglik0=l0, iters=it, status=status, info=ev["I"], margins=mg,
                                      margin=min(mg.values()))
    l0, iters = ev["l"], 0
    if ev["d"] == 0:
        return out(6, nan, 0)
    while True:
        delta, se, m = newton_step(ev["I"], ev["g"], cols)
        note("pivot", m)
        if delta is None:
            return out(3, nan, iters)
        md = float(np.abs(delta).max()) if p else 0.0
        note("convergence", _apart(md, tol))
        if md <= tol:
            return out(1, se, iters)
        slack, accepted = SLACK * max(1.0, abs(ev["l"])), None
        for h in range(HALVINGS + 1):
            trial = beta + 2.0 ** -h * delta
            et = evaluate(x, t, e, w, trial, cols)
            fall = ev["l"] - et["l"]                     # accepted iff fall <= slack (NaN: not)
            if fall <= slack:
                note("acceptance", _apart(max(fall, 0.0), slack))
                accepted = et
                break
            note("acceptance", _apart(fall, slack) if np.isfinite(fall) else np.inf)
        if accepted is None:
            return out(5, nan, iters)
        beta, ev, iters = trial, accepted, iters + 1
        mb = float(np.abs(beta).max())
        note("bound", _apart(mb, beta_max))
        if mb > beta_max:
            return out(4, nan, iters)
        if iters == max_iter:
            return out(2, nan, iters)


def resampled(x, time, event, w):
    """the arrays of the literal resample that draws patient i w_i times -> (x, time, event)"""
    idx = np.repeat(np.arange(len(w)), np.asarray(w).astype(np.int64))
    x = np.asarray(x, dtype=np.float64)
    return x.reshape(len(x), -1)[idx], np.asarray(time)[idx], np.asarray(event)[idx]


def mask_columns(mask, p):
    return [a for a in range(p) if (int(mask) >> a) & 1]


def cohort(n, p, seed, censor_all=False):
    """The tests' cohort: integer times 1..11 with ties shared by events and censorings, about 60 % events, x rounded to two decimals,
    column 0 binary, a planted signal (hazard rises with 0.7 x_0 + 0.5 x_1 - 0.4 x_2 as far as the columns exist) -> (x, time, event)."""
    rng = np.random.default_rng(seed)
    x = np.round(rng.normal(size=(n, p)), 2)
    x[:, 0] = rng.integers(0, 2, size=n)
    coef = np.array([0.7, 0.5, -0.4] + [0.0] * p)[:p]
    lat = rng.exponential(size=n) * np.exp(-(x @ coef))
    time = np.clip(np.ceil(lat * 4.0), 1, 11)
    event = (rng.random(n) < 0.6) & (not censor_all)
    return x, time, event.astype(np.int64)
