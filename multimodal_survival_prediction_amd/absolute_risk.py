"""Absolute-risk evaluation: from a log-hazard to a survival probability, and how far that probability can be trusted.

The networks output a risk score; the C-index (bootstrap.py) and the cut-point scan (risk_strata.py) judge its ORDER only.  This module
adds what judges the predicted probabilities themselves:

  * breslow_baseline: the Breslow cumulative baseline hazard of a fit set, which turns a risk score into a curve
    S(t | eta) = exp(-H0(t) e^eta);
  * prediction_error: the IPCW Brier score BS(tau) with its integral (IBS) and its scaled form against the Kaplan-Meier null model
    (IPA = 1 - BS / BS_null), and the cumulative/dynamic AUC(tau) of Uno / Hung-Chiang with its integral (iAUC), each with bootstrap
    percentile intervals, and PAIRED differences of IBS and iAUC between models scored on the same patients;
  * calibration_table: mean predicted event probability against 1 - KM(tau) per prediction group.

Definitions (n patients (t_i, e_i), integer multiplicities w_i, horizons tau_1 < ... < tau_H; at equal times events precede censorings):
  censoring distribution (reverse Kaplan-Meier)  G(t) = prod_{u <= t} (n_u - c_u) / n_u over the distinct times u with n_u > 0,
      c_u = sum w_i [t_i = u, e_i = 0],  n_u = sum w_i [t_i >= u] - sum w_i [t_i = u, e_i = 1];  G(t-) is the product over u < t;
  case at tau: t_i <= tau and e_i = 1, weight omega_i = 1 / G(t_i-);  control at tau: t_i > tau;
  BS(tau)  = [ sum_cases w_i omega_i S_i(tau)^2 + sum_controls w_i (1 - S_i(tau))^2 / G(tau) ] / sum w_i   (the second term 0 without a control),
  BS_null  = the same with S_i = the weighted Kaplan-Meier estimate KM(tau),   IPA = 1 - BS / BS_null,
  AUC(tau) = sum_{i case, j control} w_i omega_i w_j ([eta_i > eta_j] + 1/2 [eta_i = eta_j]) / (sum_cases w_i omega_i  sum_controls w_j),
      NaN without a case or without a control,
  IBS / iAUC = the trapezoid integral over the horizons / (tau_H - tau_1) (the value itself when H = 1).
These are the conventions of lifelines / scikit-survival with ONE difference: a case is weighted by the LEFT limit G(t_i-), after Graf
et al. (1999); scikit-survival uses G(t_i).

All replicates of all models at all horizons are ONE launch of mms_td_metrics (include/mmsurv.h: TdMetricsP) under the multiplicity
rows of bootstrap.replicate_rows.  Everything after it (ratios and integrals: prediction_error_statistics; intervals and p-values:
bootstrap.estimate / paired) is float64 host arithmetic.  There is no CPU fallback for the launch, like the rest of the package.

With strata (pooled out-of-fold predictions) only the RESAMPLING is stratified.  The pooled Brier score is meaningful when each fold's
predictions came from that fold's own baseline; the pooled AUC assumes that the folds' risk scores are on a comparable scale.  Out of
scope: an AUC stratified across folds, competing risks, time-varying predictions and censoring models that depend on covariates."""
from dataclasses import dataclass

import numpy as np

from .bootstrap import Estimate, Paired, estimate, paired, replicate_rows
from .risk_sets import risk_matrix, run_flags, to_numpy


# ---- Breslow baseline ---------------------------------------------------------------------------------------------------------------
@dataclass
class Baseline:
    time: np.ndarray             # distinct event times of the fit set, ascending
    hazard: np.ndarray           # cumulative baseline hazard at those times, of the SHIFTED scores eta - shift
    shift: float                 # the fit set's largest eta

    @property
    def H0(self):
        """the cumulative baseline hazard H0 at `time` (of the unshifted scores: hazard e^-shift)"""
        return self.hazard * np.exp(-self.shift)

    def _steps(self, t):
        t = np.asarray(t, dtype=np.float64)
        k = np.searchsorted(self.time, t, side="right")
        return np.where(k > 0, self.hazard[np.maximum(k - 1, 0)] if len(self.hazard) else 0.0, 0.0)

    def cumulative_hazard(self, t):
        """H0(t): the right-continuous step function (0 before the first event time)"""
        return self._steps(t) * np.exp(-self.shift)

    def survival(self, risk, horizons):
        """S(tau | eta) = exp(-H0(tau) e^eta) -> [..., H] for risk [...]"""
        eta = np.asarray(to_numpy(risk, "risk"), dtype=np.float64)
        return np.exp(-self._steps(horizons) * np.exp(eta - self.shift)[..., None])


def breslow_baseline(risk, time, event):
    """Breslow's estimate of the cumulative baseline hazard on a fit set (a fold's training patients scored by the model that predicts):
    H0(t) = sum over the event times u <= t of d_u / sum_{j: t_j >= u} exp(eta_j), d_u the events at u; computed on eta - max eta."""
    eta = np.asarray(to_numpy(risk, "risk"), dtype=np.float64).reshape(-1)
    t, e = np.asarray(to_numpy(time, "time"), dtype=np.float64).reshape(-1), np.asarray(to_numpy(event, "event")).reshape(-1) != 0
    if len(eta) < 1 or len(t) != len(eta) or len(e) != len(eta):
        raise ValueError("risk, time and event must have the same n >= 1 entries")
    shift = float(eta.max())
    x = np.exp(eta - shift)
    u = np.unique(t[e])
    d = np.array([np.count_nonzero(e & (t == v)) for v in u], dtype=np.float64)
    s0 = np.array([x[t >= v].sum() for v in u])
    return Baseline(time=u, hazard=np.cumsum(d / s0) if len(u) else np.zeros(0), shift=shift)


# ---- horizons -----------------------------------------------------------------------------------------------------------------------
def check_horizons(horizons):
    h = np.asarray(horizons, dtype=np.float64).reshape(-1)
    if len(h) < 1 or not np.isfinite(h).all() or (h <= 0).any() or (np.diff(h) <= 0).any():
        raise ValueError("horizons must be finite, positive and strictly ascending")
    return h


def default_horizons(time, event, H=16):
    """H equally spaced times from the 10th to the 90th percentile (numpy.quantile) of the observed event times"""
    t, e = np.asarray(time, dtype=np.float64).reshape(-1), np.asarray(event).reshape(-1) != 0
    if int(H) < 1 or not e.any():
        raise ValueError("default horizons need H >= 1 and at least one observed event")
    lo, hi = np.quantile(t[e], [0.1, 0.9])
    return check_horizons(np.linspace(lo, hi, int(H)) if hi > lo else [lo])


# ---- host side of the launch --------------------------------------------------------------------------------------------------------
def metric_inputs(risk, time, event, horizons):
    """-> (order, trank, event, hcut, rord) of TdMetricsP: order = the patients time ascending, events before censorings at equal
    times (stable); trank / event per position of that order; hcut[h] = positions with t <= tau_h; rord[m] = 2 * position + [last of
    its group of equal risks], the positions of model m (risk: [M, n]) in risk-ascending order.  (Tie flags: risk_sets.run_flags.)"""
    t, e = np.asarray(time, dtype=np.float64).reshape(-1), (np.asarray(event).reshape(-1) != 0).astype(np.int32)
    order = np.lexsort((1 - e, t))
    ts = t[order]
    trank = (np.cumsum(run_flags(ts)[0]) - 1).astype(np.int32)
    hcut = np.searchsorted(ts, np.asarray(horizons, dtype=np.float64), side="right").astype(np.int32)
    rord = []
    for r in np.asarray(risk):
        rp = r[order]
        ro = np.argsort(rp, kind="stable")
        rord.append(2 * ro + run_flags(rp[ro])[1])
    return order, trank, e[order], hcut, np.stack(rord).astype(np.int32)


def _trapezoid_mean(y, x):
    """trapezoid integral of y over x along the last axis / (x[-1] - x[0]); y itself when there is one point"""
    if len(x) == 1:
        return y[..., 0]
    return np.sum(0.5 * (y[..., 1:] + y[..., :-1]) * np.diff(x), axis=-1) / (x[-1] - x[0])


# ---- statistics layer ---------------------------------------------------------------------------------------------------------------
@dataclass
class PredictionErrorResult:
    horizons: np.ndarray         # [H]
    brier: Estimate              # [M, H]
    brier_null: Estimate         # [H] the Kaplan-Meier null model
    ipa: Estimate                # [M, H] 1 - brier / brier_null
    ibs: Estimate                # [M]
    auc: Estimate                # [M, H]
    iauc: Estimate               # [M]
    ibs_diff: Paired
    iauc_diff: Paired
    n_degenerate: int            # replicates with an undefined AUC at some horizon (left out of every quantile)
    replicates: int = 0
    seed: int = 0
    alpha: float = 0.05


def prediction_error_statistics(raw, horizons, alpha=0.05, seed=0):
    """The statistics layer on the launch's raw outputs (host arrays; row 0 = the all-ones weights, rows 1.. = the R replicates):
    raw = dict(G, km, wcase, wctrl [1 + R, H], brier, auc_num [1 + R, M, H], wsum [1 + R] = each row's sum of multiplicities).
    Pure float64 host arithmetic.  A replicate whose AUC is undefined at some horizon (no case or no control drawn there) has a NaN
    iAUC, is counted in n_degenerate and left out of every quantile; when all are degenerate every interval is NaN."""
    tau = check_horizons(horizons)
    f = lambda k: np.asarray(raw[k], dtype=np.float64)
    G, km, wcase, wctrl, brier, num, wsum = f("G"), f("km"), f("wcase"), f("wctrl"), f("brier"), f("auc_num"), f("wsum")
    R = brier.shape[0] - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        ctrl = np.where(wctrl > 0, wctrl * (1.0 - km) ** 2 / np.where(wctrl > 0, G, 1.0), 0.0)
        null = (wcase * km * km + ctrl) / wsum[:, None]                          # [1 + R, H]
        ipa = 1.0 - brier / null[:, None, :]
        den = (wcase * wctrl)[:, None, :]
        auc = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)       # [1 + R, M, H]
    ibs, iauc = _trapezoid_mean(brier, tau), _trapezoid_mean(auc, tau)           # [1 + R, M]
    ok = ~np.isnan(auc[1:]).any(axis=(1, 2))
    mv = lambda x: np.moveaxis(x, 0, -1)                                         # replicates last
    e_ibs, e_iauc = estimate(mv(ibs), ok, alpha), estimate(mv(iauc), ok, alpha)
    return PredictionErrorResult(horizons=tau, brier=estimate(mv(brier), ok, alpha), brier_null=estimate(mv(null), ok, alpha),
                                 ipa=estimate(mv(ipa), ok, alpha), ibs=e_ibs, auc=estimate(mv(auc), ok, alpha), iauc=e_iauc,
                                 ibs_diff=paired(e_ibs, ok, alpha), iauc_diff=paired(e_iauc, ok, alpha), n_degenerate=int(R - ok.sum()),
                                 replicates=int(R), seed=seed, alpha=float(alpha))


def prediction_error(surv, risk, time, event, horizons, R=2000, seed=0, strata=None, weights=None, alpha=0.05):
    """IPCW Brier score, IPA and cumulative/dynamic AUC of M models scored on the same n patients, with bootstrap intervals and paired
    model comparison -> PredictionErrorResult (the module docstring has the definitions and the caveats of pooled predictions).

    surv: [n, H] or [M, n, H] predicted survival probabilities at the horizons (Baseline.survival), risk: [n] or [M, n] (higher = higher
    risk; orders the AUC), time / event: [n], horizons: [H] finite, positive, strictly ascending.  The multiplicity rows are
    bootstrap.replicate_rows(n, R, seed, strata, weights); R = 0 gives the point estimates alone.  Runs on the current GPU."""
    from . import ops
    tau = check_horizons(horizons)
    risk, t, e = risk_matrix(risk, time, event)
    risk = np.asarray(risk, dtype=np.float64)
    surv = np.asarray(to_numpy(surv, "surv"), dtype=np.float64)
    surv = surv[None] if surv.ndim == 2 else surv
    M, n = risk.shape
    if surv.shape != (M, n, len(tau)):
        raise ValueError("surv must be [n, H] or [M, n, H] with H = len(horizons)")
    if not np.isfinite(surv).all() or surv.min() < 0 or surv.max() > 1:
        raise ValueError("surv must hold probabilities in [0, 1]")
    w = replicate_rows(n, R, seed, strata, weights)
    order, trank, es, hcut, rord = metric_inputs(risk, t, e, tau)
    out = ops.td_metrics(trank, es, hcut, rord, np.ascontiguousarray(surv[:, order, :]), np.ascontiguousarray(w[:, order]))
    raw = {k: v.cpu().numpy() for k, v in out.items()}
    raw["wsum"] = w.sum(1, dtype=np.int64)
    return prediction_error_statistics(raw, tau, alpha=alpha, seed=seed)


# ---- calibration --------------------------------------------------------------------------------------------------------------------
def calibration_table(surv_tau, time, event, tau, groups=5, alpha=0.05):
    """Calibration at one horizon: the patients are ordered by their predicted event probability 1 - S_i(tau) (stable) and cut at its
    quantiles into `groups` groups of equal size (to within one patient); per group -> dict(group, patients, predicted = the mean
    predicted event probability, observed = 1 - KM(tau) of the group, low, high = the Greenwood log-log band of risk_strata.km_curve).
    Host arithmetic, point estimates only."""
    from .risk_strata import km_curve
    p = 1.0 - np.asarray(to_numpy(surv_tau, "surv_tau"), dtype=np.float64).reshape(-1)
    t, e = np.asarray(time, dtype=np.float64).reshape(-1), np.asarray(event).reshape(-1) != 0
    groups = int(groups)
    if not 1 <= groups <= len(p) or len(t) != len(p) or len(e) != len(p):
        raise ValueError("surv_tau, time and event must have the same n entries and 1 <= groups <= n")
    rows = []
    for g, idx in enumerate(np.array_split(np.argsort(p, kind="stable"), groups)):
        c = km_curve(t[idx], e[idx], alpha)
        k = int(np.searchsorted(c.time, float(tau), side="right")) - 1          # (c.time starts at 0: k >= 0 for tau >= 0)
        rows.append(dict(group=g + 1, patients=int(len(idx)), predicted=float(p[idx].mean()), observed=float(1.0 - c.survival[k]),
                         low=float(1.0 - c.high[k]), high=float(1.0 - c.low[k])))
    return rows
