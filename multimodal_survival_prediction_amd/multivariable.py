"""Multivariable Cox analysis: is a model's risk score an INDEPENDENT prognostic factor once other covariates (age, another model's
score) are in the model?  Adjusted hazard ratios with Wald and bootstrap percentile intervals, and likelihood-ratio tests of nested
models.

The fit is the classical low-dimensional one -- Newton-Raphson on the Breslow partial likelihood with the observed information
(include/mmsurv.h: CoxNewtonP) -- and it runs many times: every bootstrap replicate of every nested covariate subset is its own fit.
All of them are ONE launch of mms_cox_newton, one workgroup per fit, under the multiplicity rows of bootstrap.replicate_rows -- the rows
cindex_bootstrap and absolute_risk.prediction_error use, so the intervals of one evaluation describe the same resamples.  Everything
after the launch (z, p-values, likelihood-ratio tests; bootstrap intervals: bootstrap.estimate) is float64 host arithmetic on a few
thousand numbers.  There is no CPU fallback for the fits, like the rest of the package.

A fit's status (ops.COX_NEWTON_STATUS): 1 converged, 2 max_iter, 3 singular information (a column constant in the resample, or
collinear), 4 monotone likelihood (a separating covariate: |beta| passed beta_max; reported, not repaired), 5 no step accepted,
6 no events.  Not covered: Efron ties, the score test, optimism correction, bootstrap-t, strata, time-varying
covariates, offsets, Firth's correction."""
from dataclasses import dataclass

import numpy as np
from scipy import stats

from .bootstrap import estimate, multiplicity_rows, replicate_rows
from .risk_sets import descending_groups, to_numpy

MAX_P, MAX_S = 16, 64          # MMS_COXNEWTON_MAX_P / _MAX_S of include/mmsurv.h


@dataclass
class Design:
    X: np.ndarray                # [n, p] float64 design matrix of the complete cases
    names: list                  # [p] column names
    keep: np.ndarray             # bool [n_all]: the complete cases among the rows given
    n_dropped: int
    center: np.ndarray           # [p] subtracted (0 for a column left as it is)
    scale: np.ndarray            # [p] divided by (1 for a column left as it is): beta / scale is the coefficient per unit


def design(columns, standardize=True):
    """columns: dict name -> [n] numbers.  Complete cases only (a row with a NaN in any column is dropped and counted in n_dropped).  With
    standardize every column is centred and scaled by its standard deviation (ddof 1) over the complete cases, except a column with
    exactly two distinct values (an indicator), which is left as it is; the scales are kept.  A column that is constant over the
    complete cases, or holds an infinity, raises."""
    names = list(columns)
    if not names:
        raise ValueError("no columns")
    raw = np.stack([np.asarray(to_numpy(columns[k]), dtype=np.float64).reshape(-1) for k in names], axis=1)
    if np.isinf(raw).any():
        raise ValueError("non-finite values in column(s) %s" % [k for k, c in zip(names, raw.T) if np.isinf(c).any()])
    keep = ~np.isnan(raw).any(axis=1)
    X = raw[keep]
    if len(X) < 2:
        raise ValueError("fewer than two complete cases")
    center, scale = np.zeros(len(names)), np.ones(len(names))
    for a, k in enumerate(names):
        distinct = len(np.unique(X[:, a]))
        if distinct < 2:
            raise ValueError("column %r is constant over the complete cases" % k)
        if standardize and distinct > 2:
            center[a], scale[a] = X[:, a].mean(), X[:, a].std(ddof=1)
    return Design(X=(X - center) / scale, names=names, keep=keep, n_dropped=int((~keep).sum()), center=center, scale=scale)


def launch_order(time):
    """-> (order, glast): the patients in time-descending order (stable) and the flag at the last position of every group of equal times
    (risk_sets.descending_groups)"""
    order, _, _, _, glast = descending_groups(time)
    return order, glast.astype(np.int32)


def subset_masks(subsets, p):
    """subsets: lists of column indices -> int64 [S] bit masks (bit a = column a); an empty or repeated subset, or an index outside
    [0, p), raises"""
    masks = []
    for s in subsets:
        cols = [int(a) for a in s]
        if not cols or len(set(cols)) != len(cols) or min(cols) < 0 or max(cols) >= p:
            raise ValueError("a subset must name at least one of the %d columns, each once: %r" % (p, list(s)))
        masks.append(sum(1 << a for a in cols))
    if len(set(masks)) != len(masks):
        raise ValueError("a subset is given twice")
    return np.asarray(masks, dtype=np.int64)


def model_subsets(base, add):
    """The nested models of analyse -> list of (label, tuple of names): base, each added name alone, base + each added name, base + all;
    duplicates merged (the first label stays), an empty base left out."""
    base, add = list(base), list(add)
    if len(set(base + add)) != len(base + add) or not add:
        raise ValueError("base and add must be disjoint lists of distinct names, add not empty")
    models = []
    def put(label, cols):
        if cols and tuple(cols) not in [m[1] for m in models]:
            models.append((label, tuple(cols)))
    put("base", base)
    for k in add:
        put(k, [k])
    for k in add:
        put("base+" + k, base + [k])
    put("base+all", base + add)
    return models


def _run(X, time, event, w, masks, tol, max_iter, beta_max):
    """One launch: X [n, p], w int8 [R, n] in the patients' own order -> dict of host arrays beta, se [R, S, p], loglik, loglik0, iters,
    status [R, S]"""
    from . import ops
    order, glast = launch_order(time)
    e = (np.asarray(event).reshape(-1) != 0).astype(np.int32)
    out = ops.cox_newton(np.ascontiguousarray(X[order]), np.asarray(time, dtype=np.float64).reshape(-1)[order], e[order], glast,
                         np.ascontiguousarray(w[:, order]), masks, tol=tol, max_iter=max_iter, beta_max=beta_max)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _checked(X, time, event):
    X = np.asarray(to_numpy(X, "X"), dtype=np.float64)
    X = X.reshape(len(X), -1)
    t, e = np.asarray(to_numpy(time, "time"), dtype=np.float64).reshape(-1), to_numpy(event, "event").reshape(-1)
    n, p = X.shape
    if n < 1 or not 1 <= p <= MAX_P or len(t) != n or len(e) != n or not np.isfinite(X).all() or not np.isfinite(t).all():
        raise ValueError("X must be finite [n, p] with 1 <= p <= %d and time / event [n], finite" % MAX_P)
    return X, t, (e != 0).astype(np.int64)


def coefficient_table(beta, se, cols, alpha=0.05):
    """Wald statistics of one fit's coefficients on cols -> dict of [len(cols)] arrays beta, se, z, p, hr, hr_low, hr_high"""
    b, s = np.asarray(beta, dtype=np.float64)[list(cols)], np.asarray(se, dtype=np.float64)[list(cols)]
    with np.errstate(divide="ignore", invalid="ignore"):
        z = b / s
    q = stats.norm.ppf(1.0 - alpha / 2.0)
    return dict(beta=b, se=s, z=z, p=2.0 * stats.norm.sf(np.abs(z)), hr=np.exp(b), hr_low=np.exp(b - q * s), hr_high=np.exp(b + q * s))


def _apparent_c(X, t, e, beta):
    from .survival_stats import concordance_index
    try:
        return float(concordance_index(t, -(X @ beta), e))
    except ZeroDivisionError:
        return float("nan")


def point_fits(raw_point, X, time, event, subsets, alpha=0.05):
    """The per-subset results of cox_fit from one row of the launch's outputs: raw_point = dict(beta, se [S, p], loglik, loglik0, iters,
    status [S]); subsets: lists of column indices.  Pure host arithmetic."""
    fits = []
    for s, cols in enumerate(subsets):
        cols = list(cols)
        f = coefficient_table(raw_point["beta"][s], raw_point["se"][s], cols, alpha)
        ll = float(raw_point["loglik"][s])
        f.update(columns=cols, loglik=ll, loglik0=float(raw_point["loglik0"][s]), aic=2.0 * len(cols) - 2.0 * ll,
                 status=int(raw_point["status"][s]), iters=int(raw_point["iters"][s]),
                 c_index=_apparent_c(X, time, event, np.asarray(raw_point["beta"][s], dtype=np.float64)))
        fits.append(f)
    return fits


def cox_fit(X, time, event, weights=None, subsets=None, tol=1e-9, max_iter=30, beta_max=30.0, alpha=0.05):
    """Cox regression of (time, event) on the columns of X [n, p] (p <= 16), one fit per subset of columns (lists of column indices;
    None: all columns).  weights: [n] integer multiplicities 0..127 (a multiplicity is a repeat; None: all ones; checked by
    bootstrap.multiplicity_rows).  Breslow ties.
    -> list, per subset, of dict(columns, beta, se, z, p (Wald, two-sided), hr, hr_low, hr_high (Wald, level 1 - alpha), loglik,
    loglik0, aic = 2 k - 2 loglik, status, iters, c_index = the apparent C-index of X beta, survival_stats.concordance_index on the
    patients as given).  Runs on the current GPU."""
    X, t, e = _checked(X, time, event)
    n, p = X.shape
    subsets = [list(range(p))] if subsets is None else [list(s) for s in subsets]
    masks = subset_masks(subsets, p)
    w = np.ones((1, n), np.int8) if weights is None else multiplicity_rows(to_numpy(weights).reshape(1, -1), n)
    raw = _run(X, t, e, w, masks, tol, max_iter, beta_max)
    return point_fits({k: v[0] for k, v in raw.items()}, X, t, e, subsets, alpha)


def lr_test(loglik_full, loglik_nested, df):
    """likelihood-ratio test of nested models -> dict(chi2, df, p)"""
    chi2 = max(0.0, 2.0 * (float(loglik_full) - float(loglik_nested)))
    return dict(chi2=chi2, df=int(df), p=float(stats.chi2.sf(chi2, int(df))))


def analyse_statistics(raw, X, time, event, names, models, base, add, alpha=0.05, scale=None):
    """The statistics layer of analyse on the launch's raw outputs (host arrays; row 0 = the all-ones weights, rows 1.. = the R
    replicates): raw = dict(beta, se [1 + R, S, p], loglik, loglik0, iters, status [1 + R, S]); models = model_subsets(base, add), in
    the order of the launch's subsets; names = the columns of X.  Pure float64 host arithmetic.  A replicate whose status is not 1 in
    ANY subset is counted in n_degenerate and left out of every quantile; when all are, every bootstrap interval is NaN."""
    names = list(names)
    col = {k: a for a, k in enumerate(names)}
    subsets = [[col[k] for k in m[1]] for m in models]
    beta, status = np.asarray(raw["beta"], dtype=np.float64), np.asarray(raw["status"])
    R = beta.shape[0] - 1
    scale = np.ones(len(names)) if scale is None else np.asarray(scale, dtype=np.float64)
    ok = (status[1:] == 1).all(axis=1)
    fits = point_fits({k: np.asarray(v)[0] for k, v in raw.items()}, X, time, event, subsets, alpha)
    fitted = [(s, col[k]) for s, m in enumerate(models) for k in m[1]]                        # the coefficients that exist, in output order
    rl = np.ascontiguousarray(np.moveaxis(beta, 0, -1)[tuple(zip(*fitted))])                  # [len(fitted), 1 + R]: replicates last and contiguous
    b_est, hr_est = estimate(rl, ok, alpha), estimate(np.exp(rl), ok, alpha)
    out_models = []
    for s, ((label, cols), f) in enumerate(zip(models, fits)):
        coefs = {}
        for j, k in enumerate(cols):
            c = {key: float(f[key][j]) for key in ("beta", "se", "z", "p", "hr", "hr_low", "hr_high")}
            c["scale"] = float(scale[col[k]])
            c["hr_per_unit"] = float(np.exp(f["beta"][j] / scale[col[k]]))
            if R:
                a = fitted.index((s, col[k]))
                c.update(beta_boot_low=float(b_est.low[a]), beta_boot_high=float(b_est.high[a]), hr_boot_low=float(hr_est.low[a]),
                         hr_boot_high=float(hr_est.high[a]), beta_boot_se=float(b_est.se[a]))
            coefs[k] = c
        out_models.append(dict(model=label, columns=list(cols), coefficients=coefs, loglik=f["loglik"], loglik0=f["loglik0"], aic=f["aic"],
                               status=f["status"], iters=f["iters"], c_index=f["c_index"]))
    index = {m[1]: s for s, m in enumerate(models)}
    base, add = tuple(base), list(add)
    ll = lambda cols: fits[index[tuple(cols)]]["loglik"] if cols else fits[0]["loglik0"]      # (the null model's l is every fit's loglik0)
    tests = {k: lr_test(ll(base + (k,)), ll(base), 1) for k in add}
    tests["all"] = lr_test(ll(base + tuple(add)), ll(base), len(add))
    counts = {int(v): int(c) for v, c in zip(*np.unique(status[1:], return_counts=True))} if R else {}
    return dict(columns=names, patients=int(len(X)), events=int(np.asarray(event).astype(bool).sum()), base=list(base), add=add,
                replicates=int(R), alpha=float(alpha), models=out_models, lr_tests=tests, n_degenerate=int(R - ok.sum()),
                status_counts=counts)


def analyse(columns, time, event, base, add, R=2000, seed=0, strata=None, alpha=0.05, tol=1e-9, max_iter=30, beta_max=30.0,
            weights=None):
    """Adjusted hazard ratios of the `add` covariates over the `base` model, with bootstrap intervals and likelihood-ratio tests.

    columns: dict name -> [n] numbers holding every name of base and add (design: complete cases, standardised; a hazard ratio is per
    standard deviation, hr_per_unit per unit of the column).  The models are model_subsets(base, add).  One launch fits all of them
    under bootstrap.replicate_rows(n, R, seed, strata, weights) over the n complete cases; R = 0 gives the point estimates alone.
    -> the dictionary of analyse_statistics plus n_dropped, seed and the design's center / scale.  Runs on the current GPU."""
    models = model_subsets(base, add)
    names = list(base) + list(add)
    missing = [k for k in names if k not in columns]
    if missing:
        raise ValueError("columns has no %s" % missing)
    if len(names) > MAX_P or len(models) > MAX_S:
        raise ValueError("at most %d covariates and %d models in one analysis" % (MAX_P, MAX_S))
    t_all, e_all = np.asarray(to_numpy(time), dtype=np.float64).reshape(-1), np.asarray(to_numpy(event), dtype=np.float64).reshape(-1)
    cols = {k: np.asarray(to_numpy(columns[k]), dtype=np.float64).reshape(-1) for k in names}
    if any(len(c) != len(t_all) for c in cols.values()) or len(e_all) != len(t_all):
        raise ValueError("every column, time and event must have the same n entries")
    keep = ~np.isnan(np.stack(list(cols.values()) + [t_all, e_all], axis=1)).any(axis=1)      # (a patient without a label is no complete case)
    d = design({k: c[keep] for k, c in cols.items()})
    X, t, e = _checked(d.X, t_all[keep], e_all[keep])
    n = len(X)
    w = replicate_rows(n, R, seed, None if strata is None else np.asarray(strata).reshape(-1)[keep], weights)      # (over the complete cases)
    col = {k: a for a, k in enumerate(names)}
    masks = subset_masks([[col[k] for k in m[1]] for m in models], len(names))
    raw = _run(X, t, e, w, masks, tol, max_iter, beta_max)
    out = analyse_statistics(raw, X, t, e, names, models, base, add, alpha, d.scale)
    out.update(n_dropped=int((~keep).sum()), seed=int(seed), center=[float(v) for v in d.center], scale=[float(v) for v in d.scale])
    return out
