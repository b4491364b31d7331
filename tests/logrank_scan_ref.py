"""numpy float64 reference of the cut-point log-rank scan (mms_logrank_scan, risk_strata.stratify), written the slow, obvious way: for
every cut the two groups are built and the arithmetic of survival_stats.logrank_test runs on them -- at every distinct event time u the
patients at risk and the events of each group are counted from the raw times, n < 2 is skipped, O - E and the hypergeometric variance are
summed.  Nothing of the kernel's prefix form (running counts over a time-sorted order, per-position coefficients) is used.  The sums of
the absolute terms come back with U and V: the tests' tolerances are relative to them."""
import math

import numpy as np

REL = 1e-10        # allowed error of U and V relative to the sum of their absolute terms (the criterion of test_gpu_gene_screen.py)


class Labels:
    """The per-time tables of logrank_test for one cohort: at_risk[u, i] = [t_i >= u], died[u, i] = [t_i == u and e_i] over the distinct
    event times u, so that a group's n_a(u) and d_a(u) are sums of its members' columns."""

    def __init__(self, time, event):
        self.t = np.asarray(time, dtype=np.float64).reshape(-1)
        self.e = np.asarray(event).reshape(-1).astype(bool)
        self.u = np.unique(self.t[self.e])
        self.at_risk = (self.t[None, :] >= self.u[:, None]).astype(np.float64)
        self.died = ((self.t[None, :] == self.u[:, None]) & self.e[None, :]).astype(np.float64)
        self.n = self.at_risk.sum(1)
        self.d = self.died.sum(1)


def logrank_groups(lab, high):
    """logrank_test's arithmetic for the groups a = high, b = the rest; high: bool [..., n] -> dict of arrays [...]: U (O - E of the high
    group), V, absU, absV (the sums of the absolute terms), n_high, d_high, chi2."""
    high = np.asarray(high, dtype=bool)
    hf = high.astype(np.float64)
    na, da = hf @ lab.at_risk.T, hf @ lab.died.T                    # [..., times]
    n, d = lab.n, lab.d
    nb = n - na
    ok = n >= 2
    nn, n1 = np.where(ok, n, 1.0), np.where(ok, n - 1, 1.0)
    exp = d * na / nn
    tu = np.where(ok, da - exp, 0.0)
    au = np.where(ok, da + exp, 0.0)
    tv = np.where(ok, d * (na / nn) * (nb / nn) * (n - d) / n1, 0.0)
    U, V = tu.sum(-1), tv.sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        chi2 = np.where(V > 0, U * U / np.where(V > 0, V, 1.0), 0.0)
    return dict(U=U, V=V, absU=au.sum(-1), absV=np.abs(tv).sum(-1), chi2=chi2, n_high=high.sum(-1).astype(np.int64),
                d_high=(high & lab.e).sum(-1).astype(np.int64))


def chi2_tolerance(ref, rel=REL):
    """|d chi2| for errors rel * absU in U and rel * absV in V, to first order: 2 |U| dU / V + U^2 dV / V^2 (0 where V <= 0: chi2 is 0
    there by definition); one extra ulp-scale term covers the division itself."""
    U, V = ref["U"], ref["V"]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (2 * np.abs(U) * rel * ref["absU"] + (rel * ref["absU"]) ** 2) / V + U * U * rel * ref["absV"] / (V * V) + 1e-15 * ref["chi2"]
    return np.where(V > 0, t, 0.0)


def scan(time, event, rank, cuts):
    """One problem in the patients' own order: rank [n], cuts [C] -> logrank_groups of high = rank >= cut for every cut."""
    rank, cuts = np.asarray(rank).reshape(-1), np.asarray(cuts).reshape(-1)
    return logrank_groups(Labels(time, event), rank[None, :] >= cuts[:, None])


def thresholds(risk, min_prop):
    """The admissible cuts of one risk vector as risk values (high iff risk > threshold), found by trying every distinct value but the
    largest, plus the median split -> (thresholds ascending, index of the median split)."""
    r = np.asarray(risk, dtype=np.float64).reshape(-1)
    n = len(r)
    m = int(math.ceil(min_prop * n - 1e-9))
    vals = sorted(set(r.tolist()))
    keep = [v for v in vals[:-1] if (r > v).sum() >= m and (r <= v).sum() >= m]
    med = max(v for v in vals if v <= np.median(r))                 # the same groups as risk > median
    keep = sorted(set(keep) | {med})
    return np.array(keep), keep.index(med)


def stratify(risk, time, event, perms, min_prop=0.1):
    """The statistics of risk_strata.stratify on given permutations (replicate r scores patient i with risk[perm[r][i]]) -> per model a
    dict: thresholds, median_index, the observed table (logrank_groups), chi2_max_perm / chi2_median_perm [R], p_adjusted, p_median, and
    near = the number of replicate-vs-observed comparisons whose two values lie within their summed tolerances (a p-value is only
    comparable exactly when this is 0)."""
    risk = np.atleast_2d(np.asarray(risk, dtype=np.float64))
    perms = np.asarray(perms, dtype=np.int64)
    lab = Labels(time, event)
    R = len(perms)
    out = []
    for r in risk:
        thr, im = thresholds(r, min_prop)
        obs = logrank_groups(lab, r[None, :] > thr[:, None])
        rep = logrank_groups(lab, r[perms][:, None, :] > thr[None, :, None])        # [R, C]
        tol_o, tol_r = chi2_tolerance(obs), chi2_tolerance(rep)
        ib = int(np.argmax(obs["chi2"]))
        mx, jr = rep["chi2"].max(1), rep["chi2"].argmax(1)
        near = int((np.abs(mx - obs["chi2"][ib]) <= tol_r[np.arange(R), jr] + tol_o[ib]).sum())
        near += int((np.abs(rep["chi2"][:, im] - obs["chi2"][im]) <= tol_r[:, im] + tol_o[im]).sum())
        out.append(dict(thresholds=thr, median_index=im, obs=obs, chi2_max_perm=mx, chi2_median_perm=rep["chi2"][:, im],
                        p_adjusted=(1 + int((mx >= obs["chi2"][ib]).sum())) / (R + 1),
                        p_median=(1 + int((rep["chi2"][:, im] >= obs["chi2"][im]).sum())) / (R + 1), near=near))
    return out
