"""Nonparametric bootstrap of Harrell's C: percentile intervals for one model and PAIRED comparison of several models scored on the same
patients -- every replicate resamples the patients once and all models are scored on that resample.

A replicate's pair counts are bilinear forms in its multiplicity vector w (how often each patient was drawn): 2*concordant + tied = w'Sw and
comparable = w'Pw (include/mmsurv.h: CbootP), so all R replicates of all M models are ONE launch sequence of mms_cindex_boot on the int8 matrix
cores; the counts are exact integers and everything after them (C = (w'Sw) / (2 w'Pw), quantiles, p-values) is float64 host arithmetic on a
few thousand numbers.  There is no CPU fallback for the counts, like the rest of the package.

Reproducibility contract of the draws (bootstrap_indices): the generator is numpy.random.default_rng(seed); replicates are drawn in order
r = 0..R-1; within a replicate the strata are visited in ascending label order; for a stratum of n_s patients ONE call
rng.integers(0, n_s, size=n_s) draws positions into that stratum's patients taken in input order.  Without strata all patients form one stratum.
A replicate's row lists its draws stratum after stratum in that order."""
from dataclasses import dataclass

import numpy as np

from .risk_sets import risk_matrix, to_numpy

PAIR_RULES = {"harrell": 0, "lifelines": 1, 0: 0, 1: 1}


def _strata_positions(n, strata):
    if strata is None:
        return [np.arange(n)]
    s = np.asarray(strata).reshape(-1)
    if len(s) != n:
        raise ValueError("strata must have n = %d entries" % n)
    return [np.nonzero(s == u)[0] for u in np.unique(s)]


def bootstrap_indices(n, R, seed, strata=None):
    """-> int64 [R, n]: the patients drawn by each of R bootstrap replicates (draw order: the module docstring).  With strata every replicate
    draws n_s patients from each stratum of n_s patients, so stratum sizes are kept."""
    n, R = int(n), int(R)
    if n < 1 or R < 1:
        raise ValueError("n and R must be >= 1")
    rng = np.random.default_rng(seed)
    pos = _strata_positions(n, strata)
    out = np.empty((R, n), dtype=np.int64)
    for r in range(R):
        o = 0
        for p in pos:
            out[r, o:o + len(p)] = p[rng.integers(0, len(p), size=len(p))]
            o += len(p)
    return out


def bootstrap_weights(n, R, seed, strata=None):
    """-> int8 [R, n]: how often each patient was drawn by each replicate of bootstrap_indices(n, R, seed, strata) (the bincount of its rows).
    A multiplicity above 127 (never seen in practice: the largest of 300 draws at n = 8192 was 9) raises OverflowError."""
    idx = bootstrap_indices(n, R, seed, strata)
    w = np.bincount((idx + np.arange(idx.shape[0], dtype=np.int64)[:, None] * n).ravel(), minlength=idx.shape[0] * n).reshape(idx.shape[0], n)
    if w.max() > 127:
        raise OverflowError("a patient was drawn %d times: multiplicities are int8 (<= 127)" % int(w.max()))
    return w.astype(np.int8)


def multiplicity_rows(weights, n):
    """The one check of a caller's own multiplicities -> int8 [R, n]: 2-D with n columns, integral, 0..127 (NaN raises); R = 0 is fine."""
    w = to_numpy(weights, "weights")
    if w.ndim != 2 or w.shape[1] != n or (w.size and (w.min() < 0 or w.max() > 127 or (w != np.round(w)).any())):
        raise ValueError("weights must be [R, %d] integer multiplicities in 0..127" % n)
    return w.astype(np.int8)


def replicate_rows(n, R, seed, strata=None, weights=None):
    """-> int8 [1 + R, n], the multiplicity rows of one launch: an all-ones row (the point estimates come out of the same launch), then
    bootstrap_weights(n, R, seed, strata) -- or the caller's own `weights` [R, n] (multiplicity_rows).  R = 0 gives the ones row alone.
    Every analysis of an evaluation calls this, so the same seed and strata resample the same patients in all of them."""
    if weights is not None:
        w = multiplicity_rows(weights, n)
    else:
        w = bootstrap_weights(n, R, seed, strata) if R else np.zeros((0, n), np.int8)
    return np.concatenate([np.ones((1, n), np.int8), w])


def dense_ranks(x):
    """-> int32 dense ranks (0 = smallest) of x along its last axis, at x's OWN precision: equal values share a rank, nothing is rounded."""
    x = np.asarray(x)
    if x.ndim == 1:
        return np.unique(x, return_inverse=True)[1].reshape(-1).astype(np.int32)
    return np.stack([dense_ranks(row) for row in x])


@dataclass
class BootstrapResult:
    c: np.ndarray                # [M] point estimates (the all-ones weight row of the same launch)
    c_boot: np.ndarray           # [M, R]; NaN for a replicate without comparable pairs
    se: np.ndarray               # [M] standard deviation (ddof 1) of the non-degenerate replicates
    ci_low: np.ndarray           # [M] percentile interval
    ci_high: np.ndarray
    delta: np.ndarray            # [M, M] c[a] - c[b]
    delta_ci_low: np.ndarray     # [M, M] percentile interval of the paired replicate differences
    delta_ci_high: np.ndarray
    p_value: np.ndarray          # [M, M] two-sided, min(1, 2 min((#{d <= 0} + 1) / (R' + 1), (#{d >= 0} + 1) / (R' + 1)))
    n_degenerate: int            # replicates without comparable pairs (left out of every quantile)
    counts: np.ndarray           # int64 [M + 1, R + 1] raw counts; column 0 = all-ones weights, row M = comparable pairs
    alpha: float = 0.05
    replicates: int = 0
    seed: int = 0


@dataclass
class Estimate:
    value: np.ndarray            # point estimate (the all-ones row)
    low: np.ndarray              # percentile interval over the non-degenerate replicates
    high: np.ndarray
    se: np.ndarray               # their standard deviation (ddof 1)
    boot: np.ndarray = None      # [..., R] replicate values (NaN where undefined)


@dataclass
class Paired:
    delta: np.ndarray            # [M, M] value[a] - value[b]
    low: np.ndarray              # percentile interval of the paired replicate differences
    high: np.ndarray
    p_value: np.ndarray          # two-sided, min(1, 2 min((#{d <= 0} + 1) / (R' + 1), (#{d >= 0} + 1) / (R' + 1)))


def estimate(all_, ok, alpha):
    """all_: [..., 1 + R] (index 0 = the point estimate) -> Estimate over the R' replicates ok [R]: NaN intervals for R' = 0, a NaN se
    for R' = 1"""
    value, boot = all_[..., 0].copy(), all_[..., 1:].copy()
    good = boot[..., ok]
    nan = np.full(value.shape, np.nan)
    lo, hi, se = nan.copy(), nan.copy(), nan.copy()
    if good.shape[-1] > 0:
        lo, hi = np.quantile(good, [alpha / 2, 1 - alpha / 2], axis=-1)
        if good.shape[-1] > 1:
            se = good.std(axis=-1, ddof=1)
    return Estimate(value=value, low=lo, high=hi, se=se, boot=boot)


def paired(est, ok, alpha):
    """the paired differences of an [M] Estimate over the same replicates ok [R] -> Paired"""
    M = len(est.value)
    good = est.boot[:, ok]
    Rp = good.shape[1]
    lo, hi, pv = np.full((M, M), np.nan), np.full((M, M), np.nan), np.full((M, M), np.nan)
    if Rp > 0:
        for a in range(M):
            for b in range(M):
                d = good[a] - good[b]
                lo[a, b], hi[a, b] = np.quantile(d, [alpha / 2, 1 - alpha / 2])
                pv[a, b] = min(1.0, 2.0 * min((np.count_nonzero(d <= 0) + 1) / (Rp + 1), (np.count_nonzero(d >= 0) + 1) / (Rp + 1)))
    return Paired(delta=est.value[:, None] - est.value[None, :], low=lo, high=hi, p_value=pv)


def bootstrap_statistics(counts, alpha=0.05, seed=0):
    """The statistics layer on raw counts: int64 [M + 1, 1 + R], column 0 the point estimate's, rows m < M = 2*concordant + tied of model m,
    row M = comparable pairs.  Pure float64 host arithmetic (estimate / paired); replicates with zero comparable pairs are NaN in c_boot,
    counted in n_degenerate and left out of every quantile; when all are degenerate every statistic is NaN."""
    counts = np.asarray(counts, dtype=np.int64)
    M, R = counts.shape[0] - 1, counts.shape[1] - 1
    num, den = counts[:M].astype(np.float64), counts[M].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        c_all = np.where(den > 0, num / (2.0 * den), np.nan)
    ok = den[1:] > 0
    c = estimate(c_all, ok, alpha)
    d = paired(c, ok, alpha)
    return BootstrapResult(c=c.value, c_boot=c.boot, se=c.se, ci_low=c.low, ci_high=c.high, delta=d.delta, delta_ci_low=d.low,
                           delta_ci_high=d.high, p_value=d.p_value, n_degenerate=R - int(ok.sum()), counts=counts, alpha=float(alpha),
                           replicates=R, seed=seed)


def cindex_bootstrap(risk, time, event, R=2000, seed=0, strata=None, pair_rule="lifelines", alpha=0.05, weights=None):
    """Bootstrap distribution of Harrell's C of M models scored on the same n patients.

    risk: [n] or [M, n] (numpy or torch, any float dtype; higher = higher risk; NaN raises), time / event: [n] (risk_sets.risk_matrix).
    strata: [n] labels -- pairs count only inside one stratum and the resampling keeps every stratum's size (out-of-fold predictions of
    K folds' models).  pair_rule: "lifelines" (survival_stats.concordance_index: at equal times an (event, censored) pair is comparable)
    or "harrell" (ops.cindex_counts: strictly later times only).  The multiplicity rows are replicate_rows(n, R, seed, strata, weights),
    R >= 1.  Runs on the current GPU."""
    import torch
    from . import ops
    if pair_rule not in PAIR_RULES:
        raise ValueError("pair_rule must be one of %s" % sorted(map(str, PAIR_RULES)))
    risk, t, e = risk_matrix(risk, time, event)
    n = risk.shape[1]
    if weights is None and int(R) < 1:
        raise ValueError("n and R must be >= 1")
    w = replicate_rows(n, R, seed, strata, weights)
    trank = dense_ranks(t)
    order = np.argsort(trank, kind="stable")          # time-sorted columns let the kernel skip the tiles without comparable pairs
    dev = torch.device("cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    srank = None if strata is None else up(dense_ranks(np.asarray(strata).reshape(-1))[order])
    out = ops.cindex_boot(up(dense_ranks(risk)[:, order]), up(trank[order]), up((e != 0).astype(np.int32)[order]), up(w[:, order]),
                          stratum=srank, pair_rule=PAIR_RULES[pair_rule])
    return bootstrap_statistics(out.cpu().numpy(), alpha=alpha, seed=seed)
