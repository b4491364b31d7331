"""Risk-group stratification: the log-rank statistic of EVERY admissible cut of a risk score, with permutation p-values.

The reference's last analysis step (scripts/analysis/generate_km_curves.py) splits each model's patients into a high- and a low-risk
group, draws the two Kaplan-Meier curves and tests them with a log-rank test.  A single median split with an asymptotic p is what
survival_stats offers; this module adds what small cohorts and honest cut-point selection need:

  * the cut table: the two-group log-rank statistic at every cut between distinct risk values that leaves ceil(min_prop n) patients on
    each side (the median split of survival_stats.risk_groups is always in the table);
  * the maximally selected statistic (Lausen & Schumacher; R's maxstat): the largest chi2 over the table, referred to the distribution
    of that same maximum under random relabelling -- the ADJUSTED p of the best cut;
  * a permutation p for the median split, which does not lean on the chi2(1) approximation;
  * Peto's one-step hazard ratio exp(U / V) with exp(U / V +- z / sqrt(V)), and per-group Kaplan-Meier tables with Greenwood bands.

All cuts of all M models under all R relabellings are ONE launch of mms_logrank_scan (include/mmsurv.h: LogrankScanP); the observed
rank vectors are a second, tiny launch that also returns the full tables.  Everything after the launches (p-values, hazard ratios,
Kaplan-Meier bands) is float64 host arithmetic on a few thousand numbers.  There is no CPU fallback for the scan, like the rest of the
package.

Reproducibility contract of the relabellings (draw_permutations): the generator is numpy.random.default_rng(seed); replicates are drawn
in order r = 0..R-1, ONE call rng.permutation(n) each.  Replicate r gives patient i (input order) the risk rank of patient perm[r][i];
the same permutation is applied to every model's ranks.  The identity permutation reproduces the observed statistics bit for bit.

Left out: three or more groups, a log-rank test stratified across folds, bootstrap multiplicities, and the closed-form
Lausen-Schumacher approximation of the adjusted p (the permutation distribution is exact and cheap here)."""
import math
from dataclasses import dataclass, field

import numpy as np
from scipy import stats

from .risk_sets import risk_matrix, risk_set_table, score_chi2 as chi2_of, to_numpy


def logrank_coefficients(time, event):
    """-> (order, a, h, c, pflag) of the shared labels.  order: the patients time descending (stable); per position of that order,
    with d_u events and n_u patients at risk (t >= u) at time u:  h = d_u / n_u and c = d_u (n_u - d_u) / (n_u^2 (n_u - 1)) (c: when
    n_u >= 2, else 0) at the LAST position of time u's tie group, 0 elsewhere;  a = e - sum_{u <= t} d_u / n_u (the per-patient term of
    observed - expected: U = sum over the high group of a);  pflag = [e] | 2 [h or c is not 0] (LogrankScanP).  logrank_test skips a
    time with n_u < 2; its O - E term is identically 0 there (the one patient at risk is the one event: a's two parts cancel), and it
    has no variance term (c = 0).  (n_u, d_u, h and the sum inside a: risk_sets.risk_set_table.)"""
    order, e, _, last, n_u, d_u, h_u, b = risk_set_table(time, event)
    cu = np.where((d_u > 0) & (n_u >= 2), d_u * (n_u - d_u) / (n_u * n_u * np.maximum(n_u - 1.0, 1.0)), 0.0)
    h, c = np.zeros(len(e)), np.zeros(len(e))
    h[last], c[last] = h_u, cu
    pflag = (e != 0).astype(np.int32) | (((h != 0) | (c != 0)).astype(np.int32) << 1)
    return order, e - b, h, c, pflag


def prefix_statistic(high, a, c):
    """The formulation the kernel evaluates, as three numpy lines: high = the group's mask over the time-descending positions ->
    (U, V) = (sum_i [high_i] a_i, sum_i c_i G_i (i + 1 - G_i)) with G the running count of high.  It states the definition for the CPU
    tests (against survival_stats.logrank_test); stratify never calls it -- the scan itself has no host path."""
    high = np.asarray(high, dtype=bool)
    G = np.cumsum(high).astype(np.float64)
    return float(np.sum(np.where(high, a, 0.0))), float(np.sum(c * G * (np.arange(1, len(G) + 1) - G)))


def min_group(n, min_prop):
    """ceil(min_prop n), the smallest admissible group (a product that lands a rounding error above an integer is that integer)"""
    return int(math.ceil(float(min_prop) * int(n) - 1e-9))


@dataclass
class CutSet:
    rank: np.ndarray         # int32 [n] dense ranks of the risk (0 = lowest)
    cut: np.ndarray          # int32 [C] ascending cut ranks: high group iff rank >= cut
    threshold: np.ndarray    # float64 [C] the same cuts as risk values: high group iff risk > threshold
    median_index: int        # the cut that is survival_stats.risk_groups' median split


def admissible_cuts(risk, min_prop=0.1):
    """The cut set of one model's risk scores [n].  A cut lies between two adjacent distinct risk values (patients with equal risk are
    never split) and leaves at least min_group(n, min_prop) patients on each side; its threshold is the lower of the two values (high
    group iff risk > threshold, the convention of survival_stats.risk_groups).  The median split of risk_groups is always in the set,
    whatever its group sizes -- when more than half of the patients share the largest risk it is the cut above every value, whose high
    group is empty (chi2 0)."""
    r = np.asarray(risk, dtype=np.float64).reshape(-1)
    n = len(r)
    uniq, rank = np.unique(r, return_inverse=True)
    rank = rank.reshape(-1).astype(np.int32)
    k = len(uniq)
    n_high = n - np.cumsum(np.bincount(rank, minlength=k))[:-1]          # of cut rank j = 1..k-1: patients with rank >= j
    m = min_group(n, min_prop)
    j = np.arange(1, k)
    ok = (n_high >= m) & (n - n_high >= m)
    jmed = int(np.searchsorted(uniq, np.median(r), side="right"))        # risk > median  <=>  rank >= jmed
    cut = np.union1d(j[ok], [jmed]).astype(np.int32)
    return CutSet(rank=rank, cut=cut, threshold=uniq[cut - 1], median_index=int(np.searchsorted(cut, jmed)))


def draw_permutations(n, R, seed=0):
    """-> int64 [R, n]: replicate r = the r-th call rng.permutation(n) of numpy.random.default_rng(seed) (the module docstring)."""
    n, R = int(n), int(R)
    if n < 1 or R < 0:
        raise ValueError("n must be >= 1 and R >= 0")
    rng = np.random.default_rng(seed)
    out = np.empty((R, n), dtype=np.int64)
    for r in range(R):
        out[r] = rng.permutation(n)
    return out


def permutation_p(obs, perm):
    """(1 + #{r: perm[..., r] >= obs[...]}) / (R + 1) along the last axis of perm"""
    perm = np.asarray(perm, dtype=np.float64)
    obs = np.asarray(obs, dtype=np.float64)
    return (1.0 + np.count_nonzero(perm >= obs[..., None], axis=-1)) / (perm.shape[-1] + 1.0)


def first_argmax(x):
    """index of the first largest element, -1 for an empty array"""
    x = np.asarray(x)
    return int(np.argmax(x)) if len(x) else -1


def peto_hazard_ratio(U, V, alpha=0.05):
    """Peto's one-step estimate of the hazard ratio high : low, exp(U / V), with exp(U / V +- z / sqrt(V)) -> (hr, low, high); NaN when
    V <= 0 (one group is empty or there is no event)."""
    if not V > 0:
        return float("nan"), float("nan"), float("nan")
    z = float(stats.norm.ppf(1 - alpha / 2))
    b, s = U / V, z / math.sqrt(V)
    return float(math.exp(b)), float(math.exp(b - s)), float(math.exp(b + s))


def strata_statistics(chi2_max_obs, chi2_at_obs, chi2_max_perm, chi2_at_perm):
    """The statistics layer on the launches' numbers: observed [M] and replicate [M, R] maxima and median-split statistics ->
    (p_adjusted [M], p_median_permutation [M]), both (1 + #{r: chi2_r >= chi2_obs}) / (R + 1)."""
    return permutation_p(chi2_max_obs, chi2_max_perm), permutation_p(chi2_at_obs, chi2_at_perm)


@dataclass
class ModelStrata:
    threshold: np.ndarray        # [C] cut table: high group iff risk > threshold
    n_high: np.ndarray           # int [C]
    d_high: np.ndarray           # int [C] events in the high group
    U: np.ndarray                # [C] observed - expected events of the high group
    V: np.ndarray                # [C] its hypergeometric variance
    chi2: np.ndarray             # [C]
    p_unadjusted: np.ndarray     # [C] chi2(1) tail of each cut ALONE: not a p-value of the best one
    median_index: int
    median_chi2: float
    median_p_asymptotic: float
    median_p_permutation: float
    median_hazard_ratio: tuple   # (hr, low, high)
    best_index: int
    best_threshold: float
    best_chi2: float
    p_adjusted: float            # of the maximally selected statistic
    best_hazard_ratio: tuple
    chi2_max_perm: np.ndarray = field(default=None, repr=False)      # [R]
    chi2_median_perm: np.ndarray = field(default=None, repr=False)   # [R]

    def high(self, risk, which="median"):
        """boolean high-risk mask of `risk` at the median or the best cut"""
        thr = self.threshold[self.median_index if which == "median" else self.best_index]
        return np.asarray(risk, dtype=np.float64) > thr

    def summary(self):
        hr = lambda t: dict(hazard_ratio=t[0], low=t[1], high=t[2])
        return dict(n_cuts=int(len(self.threshold)),
                    median=dict(threshold=float(self.threshold[self.median_index]), n_high=int(self.n_high[self.median_index]),
                                chi2=self.median_chi2, p_asymptotic=self.median_p_asymptotic, p_permutation=self.median_p_permutation,
                                **hr(self.median_hazard_ratio)),
                    best=dict(threshold=self.best_threshold, n_high=int(self.n_high[self.best_index]), chi2=self.best_chi2,
                              p_unadjusted=float(self.p_unadjusted[self.best_index]), p_adjusted=self.p_adjusted, **hr(self.best_hazard_ratio)))


@dataclass
class StrataResult:
    models: list                 # ModelStrata per model
    n: int
    replicates: int
    seed: int
    min_prop: float
    alpha: float

    def summary(self):
        return dict(patients=self.n, replicates=self.replicates, seed=self.seed, min_prop=self.min_prop, alpha=self.alpha,
                    models=[m.summary() for m in self.models])


def assemble(cutsets, tables, chi2_max, arg_max, chi2_at, chi2_max_perm, chi2_at_perm, n, seed=0, min_prop=0.1, alpha=0.05):
    """StrataResult from the two launches' outputs (host arrays): tables = dict of [M, C] U, V, n_high, d_high of the observed rank
    vectors, chi2_max / arg_max / chi2_at [M] of the same launch, chi2_max_perm / chi2_at_perm [M, R] of the replicates."""
    p_adj, p_med = strata_statistics(chi2_max, chi2_at, chi2_max_perm, chi2_at_perm)
    models = []
    for m, cs in enumerate(cutsets):
        C = len(cs.cut)
        U, V = np.asarray(tables["U"][m][:C], dtype=np.float64), np.asarray(tables["V"][m][:C], dtype=np.float64)
        chi2 = chi2_of(U, V)
        im, ib = cs.median_index, int(arg_max[m])
        models.append(ModelStrata(
            threshold=cs.threshold, n_high=np.asarray(tables["n_high"][m][:C]).astype(np.int64),
            d_high=np.asarray(tables["d_high"][m][:C]).astype(np.int64), U=U, V=V, chi2=chi2, p_unadjusted=stats.chi2.sf(chi2, 1),
            median_index=im, median_chi2=float(chi2_at[m]), median_p_asymptotic=float(stats.chi2.sf(chi2_at[m], 1)),
            median_p_permutation=float(p_med[m]), median_hazard_ratio=peto_hazard_ratio(U[im], V[im], alpha),
            best_index=ib, best_threshold=float(cs.threshold[ib]), best_chi2=float(chi2_max[m]), p_adjusted=float(p_adj[m]),
            best_hazard_ratio=peto_hazard_ratio(U[ib], V[ib], alpha),
            chi2_max_perm=np.asarray(chi2_max_perm[m]), chi2_median_perm=np.asarray(chi2_at_perm[m])))
    return StrataResult(models=models, n=int(n), replicates=int(np.shape(chi2_max_perm)[1]), seed=seed, min_prop=float(min_prop),
                        alpha=float(alpha))


def scan_inputs(risk, time, event, min_prop=0.1):
    """-> (order, pflag, coef [n, 2], cutsets, coff, cut, at): the host side of both launches (risk: [M, n])."""
    order, _, h, c, pflag = logrank_coefficients(time, event)
    cutsets = [admissible_cuts(r, min_prop) for r in risk]
    coff = np.concatenate([[0], np.cumsum([len(cs.cut) for cs in cutsets])]).astype(np.int64)
    cut = np.concatenate([cs.cut for cs in cutsets]) if cutsets else np.zeros(0, np.int32)
    at = np.array([cs.median_index for cs in cutsets], dtype=np.int64)
    return order, pflag, np.stack([h, c], 1), cutsets, coff, cut, at


def stratify(risk, time, event, R=10000, seed=0, min_prop=0.1, permutations=None, alpha=0.05):
    """Cut-point scan with permutation p-values of M models scored on the same n patients -> StrataResult.

    risk: [n] or [M, n] (numpy or torch, any float dtype; higher = higher risk; NaN raises), time / event: [n].  min_prop: every
    admissible cut leaves ceil(min_prop n) patients on each side (admissible_cuts).  The R relabellings are draw_permutations(n, R, seed):
    numpy.random.default_rng(seed), one rng.permutation(n) per replicate, in order; replicate r gives patient i the risk rank of patient
    perm[r][i], the same permutation for every model.  permutations: int [R, n] to use instead of the draw (each row a permutation of
    0..n-1).  Both permutation p-values are (1 + #{r: chi2_r >= chi2_obs}) / (R + 1): p_adjusted compares the replicates' MAXIMA over all
    cuts with the observed maximum, median_p_permutation the statistics at the median cut.  Runs on the current GPU: one launch of
    mms_logrank_scan for the M observed rank vectors (with the cut tables) and one for the M R replicates."""
    import torch
    from . import ops
    risk, t, e = risk_matrix(risk, time, event)
    if not 0.0 <= float(min_prop) <= 0.5:
        raise ValueError("min_prop must lie in [0, 0.5]")
    M, n = risk.shape
    if permutations is None:
        perm = draw_permutations(n, R, seed)
    else:
        perm = np.asarray(to_numpy(permutations, "permutations"))
        if perm.ndim != 2 or perm.shape[1] != n or perm.dtype.kind not in "iu" or not (np.sort(perm, 1) == np.arange(n)).all():
            raise ValueError("permutations must be integer [R, n], every row a permutation of 0..n-1")
        perm = perm.astype(np.int64)
    R = perm.shape[0]
    order, pflag, coef, cutsets, coff, cut, at = scan_inputs(risk, t, e, min_prop)
    dev = torch.device("cuda")
    rank = torch.from_numpy(np.stack([cs.rank for cs in cutsets])).to(dev)                      # [M, n] input order
    obs = ops.logrank_scan(rank[:, torch.from_numpy(order).to(dev)].contiguous(), pflag, coef, coff, cut, at=at, tables=True)
    if R:
        idx = torch.from_numpy(np.ascontiguousarray(perm[:, order])).to(dev)                    # [R, n] positions -> patients
        rep = ops.logrank_scan(rank[:, idx].reshape(M * R, n), pflag, coef, coff, cut, cset=np.repeat(np.arange(M), R), at=at)
        pmax, pat = rep["chi2_max"].cpu().numpy().reshape(M, R), rep["chi2_at"].cpu().numpy().reshape(M, R)
    else:
        pmax, pat = np.zeros((M, 0)), np.zeros((M, 0))
    host = {k: v.cpu().numpy() for k, v in obs.items()}
    return assemble(cutsets, host, host["chi2_max"], host["arg_max"], host["chi2_at"], pmax, pat, n, seed=seed, min_prop=min_prop, alpha=alpha)


# ---- group curves ------------------------------------------------------------------------------------------------------------------
@dataclass
class KMCurve:
    group: str
    time: np.ndarray             # distinct observed times, 0 first
    survival: np.ndarray
    at_risk: np.ndarray
    events: np.ndarray
    variance: np.ndarray         # Greenwood: S^2 sum d / (n (n - d)); inf once nobody is left
    low: np.ndarray              # log-log ("exponential Greenwood") band
    high: np.ndarray
    median: float                # smallest time with S <= 0.5, inf if never
    median_low: float            # the same read off the band's lower curve
    median_high: float           # ... and off its upper curve

    def rows(self):
        return [dict(group=self.group, time=float(a), survival=float(b), at_risk=int(c), events=int(d), variance=float(v), low=float(l),
                     high=float(h)) for a, b, c, d, v, l, h in zip(self.time, self.survival, self.at_risk, self.events, self.variance,
                                                                    self.low, self.high)]


def _first_at_most_half(times, curve):
    hit = np.nonzero(curve <= 0.5)[0]
    return float(times[hit[0]]) if len(hit) else float("inf")


def km_curve(durations, event_observed, alpha=0.05, group=""):
    """Kaplan-Meier table of one group with Greenwood's variance and the log-log interval lifelines draws by default:
    with s2 = sum_{u <= t} d_u / (n_u (n_u - d_u)) and v = log S,  S^exp(-+ z sqrt(s2) / v), i.e. exp(-exp(log(-v) +- z sqrt(s2) / v)).
    Where S = 1 the band is [1, 1]; where S = 0 it is [0, 0].  The median's interval is read off the band: the first time its lower
    (upper) curve is <= 0.5."""
    from .survival_stats import kaplan_meier
    times, surv, at_risk, deaths = kaplan_meier(durations, event_observed)
    nn, dd = at_risk.astype(np.float64), deaths.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        s2 = np.cumsum(np.where(dd > 0, dd / (nn * (nn - dd)), 0.0))
        var = surv * surv * s2
        var = np.where(surv > 0, var, np.inf)
        z = float(stats.norm.ppf(1 - alpha / 2))
        v = np.log(surv)
        w = z * np.sqrt(s2) / v
        lo, hi = np.exp(-np.exp(np.log(-v) - w)), np.exp(-np.exp(np.log(-v) + w))
    inner = (surv > 0) & (surv < 1)
    lo, hi = np.where(inner, lo, surv), np.where(inner, hi, surv)
    return KMCurve(group=group, time=times, survival=surv, at_risk=at_risk, events=deaths, variance=var, low=lo, high=hi,
                   median=_first_at_most_half(times, surv), median_low=_first_at_most_half(times, lo),
                   median_high=_first_at_most_half(times, hi))


def km_groups(time, event, high, alpha=0.05, names=("Low Risk", "High Risk")):
    """Per-group Kaplan-Meier curves of a two-group split: high = boolean mask of the high-risk patients -> [KMCurve] (low first; an
    empty group is left out)."""
    t, e, high = np.asarray(time, dtype=np.float64).reshape(-1), np.asarray(event).reshape(-1), np.asarray(high).reshape(-1).astype(bool)
    return [km_curve(t[m], e[m], alpha, name) for name, m in ((names[0], ~high), (names[1], high)) if m.any()]
