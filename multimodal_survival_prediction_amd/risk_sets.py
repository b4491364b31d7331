"""Shared host layer of the evaluation modules, part one: input normalisation and the label-only tables of a risk-set analysis.

bootstrap, gene_select, risk_strata, absolute_risk, multivariable and coxnet each wrap a kernel of their own; what they do to the
labels BEFORE the launch is the same few steps, and lives here once: tensor-or-array to numpy (to_numpy), the [M, n] / [n] / [n]
shape contract of the model-comparison entry points (risk_matrix), the groups of equal times of a sorted list (run_flags,
descending_groups) and the Breslow risk-set table over them (risk_set_table).  The replicate rows of a launch and the summaries of its
replicates are bootstrap.py's.  Pure numpy, float64; nothing here touches the GPU."""
from typing import NamedTuple

import numpy as np


def to_numpy(x, what=None):
    """A torch tensor (any device; bfloat16 has no numpy type: float32 holds it exactly) or anything array-like -> numpy.  With `what`
    a NaN raises ValueError naming it; without, nothing is checked."""
    if hasattr(x, "detach"):
        x = x.detach().cpu()
        x = (x.float() if str(x.dtype) == "torch.bfloat16" else x).numpy()
    x = np.asarray(x)
    if what is not None and x.dtype.kind == "f" and np.isnan(x).any():
        raise ValueError("%s contains NaN" % what)
    return x


def risk_matrix(risk, time, event):
    """risk: [n] or [M, n], time / event: [n] (numpy or torch; NaN raises) -> (risk [M, n] at its own precision, t [n], e [n]);
    M >= 1 and n >= 1."""
    risk = to_numpy(risk, "risk")
    risk = risk.reshape(1, -1) if risk.ndim == 1 else risk
    t, e = to_numpy(time, "time").reshape(-1), to_numpy(event, "event").reshape(-1)
    if risk.ndim != 2 or risk.shape[0] < 1 or risk.shape[1] < 1 or len(t) != risk.shape[1] or len(e) != risk.shape[1]:
        raise ValueError("risk must be [n] or [M, n] with n >= 1 and time / event [n]")
    return risk, t, e


def run_flags(x):
    """x: [n], sorted so that equal values are neighbours -> (first, last): bool [n], set at the first / the last position of every
    run of equal values."""
    x = np.asarray(x).reshape(-1)
    change = x[1:] != x[:-1]
    return np.concatenate([[True], change])[:len(x)], np.concatenate([change, [True]])[:len(x)]


def descending_groups(t):
    """-> (order, first, gid, last, glast).  order: the stable time-descending order of t [n]; per position of that order, first /
    glast: bool flags of the first / last position of its group of equal times, gid: the group's number (0 = the latest time); last
    [groups]: the position at which each group ends.  Everything is empty for n = 0."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    order = np.argsort(-t, kind="stable")
    first, glast = run_flags(t[order])
    return order, first, np.cumsum(first) - 1, np.nonzero(glast)[0], glast


class RiskSetTable(NamedTuple):
    order: np.ndarray            # int64 [n] positions into `rows`, time descending (stable)
    e: np.ndarray                # float64 [n] event flags (0 / 1) per position of that order
    gid: np.ndarray              # int64 [n] the position's group of equal times
    last: np.ndarray             # int64 [groups] the last position of every group
    n_u: np.ndarray              # float64 [groups] at risk at the group's time u (t >= u): everything up to the group's last position
    d_u: np.ndarray              # float64 [groups] events at u
    h_u: np.ndarray              # float64 [groups] d_u / n_u, the Breslow hazard increment
    b: np.ndarray                # float64 [n] sum of h_u over the event times u <= t_k: the groups from k's own onwards


def risk_set_table(time, event, rows=None):
    """The risk sets of one problem -> RiskSetTable.  time / event: per-patient arrays; rows: the problem's patient rows (repeats
    allowed: a row listed twice is a tie; None = all patients once).  Equal times keep their order in `rows`."""
    t_all, e_all = np.asarray(time, dtype=np.float64).reshape(-1), np.asarray(event).reshape(-1) != 0
    rows = np.arange(len(t_all)) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    order, _, gid, last, _ = descending_groups(t_all[rows])
    e = e_all[rows][order].astype(np.float64)
    n_u = (last + 1).astype(np.float64)
    d_u = np.bincount(gid, weights=e, minlength=len(last))
    h_u = d_u / n_u
    return RiskSetTable(order, e, gid, last, n_u, d_u, h_u, np.cumsum(h_u[::-1])[::-1][gid])


def score_chi2(U, V):
    """U^2 / V where V > 0, else 0 (a constant covariate, an empty group, no event): the score / log-rank chi-square, 1 dof."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(V > 0, U * U / np.where(V > 0, V, 1.0), 0.0)
