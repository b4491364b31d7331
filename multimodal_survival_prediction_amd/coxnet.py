"""Elastic-net Cox regression (glmnet's "Coxnet") as a baseline for the networks: penalty paths of many fits in lock-step.

Neither the reference nor its dependencies here have one (final_comparison.py:301-335 concludes "simple is better for small datasets" and
stops at the networks).  An honest baseline needs nested cross-validation: K outer folds, each with J inner folds and a full-training fit,
each over a path of L penalties -- K (J + 1) L independent convex problems over ONE patient x gene matrix.  They differ in which patients
count (an integer multiplicity per patient: 0 = left out, > 1 = a bootstrap repeat) and in lambda, so they are advanced together: the
linear predictors of all of them are one matrix product, their gradients another (include/mmsurv.h: CoxnetP; csrc/coxnet.hip, both on the
fp64 matrix cores).  There is no CPU fallback for the fits.

Objective, residual, solver and convergence test: the comment of CoxnetP.  All problems of a call share risk_rows(cohort): the eligible
patients (RNA-seq and a survival label) in stable time-descending order; a patient outside it is never read."""
import json
from dataclasses import dataclass

import numpy as np

from . import gene_select
from .risk_sets import descending_groups, to_numpy

TOL = 1e-6
MAX_ITER = 5000


@dataclass
class RiskRows:
    rows: np.ndarray          # int64 [n] patient rows, time descending (stable)
    time: np.ndarray          # float64 [n]
    event: np.ndarray         # bool [n]
    glast: np.ndarray         # bool [n]: the last position of a group of equal times

    def __len__(self):
        return len(self.rows)

    def positions(self, patients, n_patients):
        """List positions of `patients` (-1 where a patient is not in the list)."""
        pos = np.full(int(n_patients), -1, dtype=np.int64)
        pos[self.rows] = np.arange(len(self.rows))
        return pos[np.asarray(patients, dtype=np.int64)]

    def mult_of(self, patients, n_patients):
        """Multiplicity vector over the list that counts every listed patient of `patients` as often as it is named."""
        p = self.positions(patients, n_patients)
        return np.bincount(p[p >= 0], minlength=len(self.rows)).astype(np.int32)


def risk_rows(cohort, indices=None):
    """The row list of a call: cohort's eligible patients (gene_select.eligible_rows; of `indices` when given) in stable time-descending
    order (risk_sets.descending_groups), their event flags and the tie-group end flags."""
    label = to_numpy(cohort["label"]).astype(np.float64)
    idx = np.arange(len(label)) if indices is None else indices
    rows = gene_select.eligible_rows(cohort, idx)
    order, _, _, _, glast = descending_groups(label[rows, 0])
    rows = rows[order]
    return RiskRows(rows.astype(np.int64), label[rows, 0], label[rows, 1] != 0, glast)


def rows_as_list(rows):
    """A row list for prediction alone (mms_coxnet_eval's product reads nothing but the rows): any order, no events."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    return RiskRows(rows, np.zeros(len(rows)), np.zeros(len(rows), bool), np.ones(len(rows), bool))


class HipBackend:
    """The fits and evaluations on the GPU (ops.coxnet_fit / ops.coxnet_eval); x: the fp32 device matrix."""

    def fit(self, x, rr, mult, lam, alpha, scale=None, beta=None, tol=TOL, max_iter=MAX_ITER):
        from . import ops
        return ops.coxnet_fit(x, rr.rows, rr.event, rr.glast, mult, lam, alpha, scale=scale, beta=beta, tol=tol, max_iter=max_iter)

    def evaluate(self, x, rr, mult, lam, alpha, beta, scale=None):
        from . import ops
        return ops.coxnet_eval(x, rr.rows, rr.event, rr.glast, mult, lam, alpha, beta, scale=scale)


def problem_scales(x, rr, mults):
    """Per-problem, per-gene weighted standard deviation over the problem's own m > 0 rows (no centring of the data: the partial
    likelihood is shift-invariant) -> (scale float64 [F, G], constant bool [F, G]).  A constant gene gets scale 1."""
    X = to_numpy(x[_index(x, rr.rows)] if hasattr(x, "detach") else np.asarray(x)[rr.rows]).astype(np.float64)
    m = np.asarray(mults, dtype=np.float64)
    n = np.maximum(m.sum(1, keepdims=True), 1.0)
    mean = (m @ X) / n
    msq = (m @ (X * X)) / n
    var = msq - mean * mean
    const = var <= 1e-12 * np.maximum(msq, 1e-300)
    return np.where(const, 1.0, np.sqrt(np.where(const, 1.0, var))), const


def _index(x, rows):
    import torch
    return torch.as_tensor(np.asarray(rows), device=x.device, dtype=torch.long)


def lambda_max_from_score(U, scale, n, alpha):
    """The smallest lambda at which beta = 0 is optimal, from the score U = x'r at beta = 0: max_j |U_j / scale_j| / (n alpha); alpha = 0
    takes alpha = 1e-3 for the path's top, as glmnet does."""
    a = np.maximum(np.asarray(alpha, dtype=np.float64), 1e-3)
    u = np.abs(np.asarray(U, dtype=np.float64) / (1.0 if scale is None else scale)).max(-1)
    return u / (np.maximum(np.asarray(n, dtype=np.float64), 1.0) * a)


def log_path(lam_max, n_lambda=30, ratio=0.05):
    """-> [..., L] log-spaced from lam_max down to ratio * lam_max."""
    lam_max = np.asarray(lam_max, dtype=np.float64)
    w = np.linspace(0.0, 1.0, int(n_lambda)) if n_lambda > 1 else np.zeros(1)
    return lam_max[..., None] * np.float64(ratio) ** w


def lambda_path(x, cohort, rr, mults, alpha, n_lambda=30, ratio=0.05, scale=None):
    """lambda_max of every multiplicity vector from gene_select.cox_score_screen's U (one launch: a problem is its rows repeated by their
    multiplicity) -> (lambdas [F, L] descending, lambda_max [F])."""
    label = to_numpy(cohort["label"])
    mults = np.asarray(mults)
    U, _, _ = gene_select.cox_score_screen(x, label[:, 0], label[:, 1], [np.repeat(rr.rows, m) for m in mults])
    lmax = lambda_max_from_score(U, scale, mults.sum(1), alpha)
    return log_path(lmax, n_lambda, ratio), lmax


def pair_cindex(h, event, time):
    """Harrell C by the pair rule of the entry points' validation (losses.calculate_cindex): pairs (i, j) with e_i and t_j > t_i, concordant
    when h_i > h_j, half credit for tied scores.  NaN without a comparable pair."""
    h, time = np.asarray(h, np.float64), np.asarray(time, np.float64)
    e = np.asarray(event) != 0
    comp = e[:, None] & (time[None, :] > time[:, None])
    tot = comp.sum()
    if tot == 0:
        return float("nan")
    return float(((h[:, None] > h[None, :]) & comp).sum() + 0.5 * ((h[:, None] == h[None, :]) & comp).sum()) / float(tot)


@dataclass
class CoxPath:
    coef: np.ndarray          # [F, L, G] coefficients on the ORIGINAL gene scale
    lambdas: np.ndarray       # [F, L]
    alpha: float
    objective: np.ndarray     # [F, L]
    iterations: np.ndarray    # [F, L]
    kkt: np.ndarray           # [F, L] KKT residual (on the scaled genes)
    status: np.ndarray        # [F, L] 1 converged, 2 max_iter reached: not a fit
    scale: np.ndarray = None  # [F, G] or None

    def converged(self):
        return self.status == 1

    def predict(self, x, rows, backend=None):
        """Linear predictors of patients `rows` under every fit -> [F, L, len(rows)], through mms_coxnet_eval's product."""
        F, L, G = self.coef.shape
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        if len(rows) == 0:
            return np.zeros((F, L, 0))
        return predict(x, self.coef.reshape(F * L, G), rows, backend).reshape(F, L, len(rows))


def predict(x, coef, rows, backend=None):
    """x[rows] . coef' for coef [P, G] on the original gene scale -> [P, len(rows)] (mms_coxnet_eval's product)."""
    coef = np.asarray(coef, dtype=np.float64)
    rl = rows_as_list(rows)
    P = len(coef)
    out = (backend or HipBackend()).evaluate(x, rl, np.ones((P, len(rl)), np.int32), np.zeros(P), np.zeros(P), coef)
    return out["eta"]


def cox_path(x, cohort, mults, lambdas, alpha, standardize=True, rr=None, tol=TOL, max_iter=MAX_ITER, backend=None):
    """Fit every (multiplicity vector, lambda) pair in one lock-step call.  mults: [F, n] over risk_rows(cohort) (or the given rr);
    lambdas: [L] or [F, L].  standardize: every problem runs on x_j / scale_j, its weighted standard deviation over its own m > 0 rows; a
    constant gene gets scale 1 and coefficient 0.  -> CoxPath."""
    rr = risk_rows(cohort) if rr is None else rr
    mults = np.asarray(mults).reshape(-1, len(rr))
    F = len(mults)
    lambdas = np.broadcast_to(np.asarray(lambdas, dtype=np.float64), (F,) + np.shape(lambdas)[-1:]).copy()
    L = lambdas.shape[1]
    G = int(x.shape[1])
    scale, const = problem_scales(x, rr, mults) if standardize else (None, None)
    rep = lambda a: None if a is None else np.repeat(a, L, axis=0)
    out = (backend or HipBackend()).fit(x, rr, rep(mults), lambdas.reshape(-1), np.full(F * L, float(alpha)), scale=rep(scale),
                                        tol=tol, max_iter=max_iter)
    coef = out["beta"].reshape(F, L, G)
    if standardize:
        coef = np.where(const[:, None, :], 0.0, coef / scale[:, None, :])
    sh = lambda a: np.asarray(a).reshape(F, L)
    return CoxPath(coef, lambdas, float(alpha), sh(out["obj"]), sh(out["iters"]), sh(out["kkt"]), sh(out["status"]), scale)


def inner_seed(seed, fold):
    """The inner folds of outer fold `fold` are data.kfold_indices(n, inner, seed=this): one integer drawn from SeedSequence([seed, fold])."""
    return int(np.random.SeedSequence([int(seed), int(fold)]).generate_state(1)[0] % (2 ** 31))


def nested_problems(cohort, folds, inner, seed, rr=None):
    """The multiplicity vectors of nested cross-validation over one row list -> (rr, mults [K, J + 1, n], plan).  mults[f, j], j < J: outer
    fold f's eligible training patients without inner fold j; mults[f, J]: all of them.  plan[f] = dict(train, val, inner_val): patient
    rows (eligible ones only).  An outer validation patient has multiplicity 0 in every problem of its fold, an inner validation patient
    in the fit that is scored on it."""
    from . import data
    rr = risk_rows(cohort) if rr is None else rr
    N = int(to_numpy(cohort["label"]).shape[0])
    J = int(inner)
    mults, plan = np.zeros((len(folds), J + 1, len(rr)), np.int32), []
    for f, (tr, va) in enumerate(folds):
        tr, va = gene_select.eligible_rows(cohort, tr), gene_select.eligible_rows(cohort, va)
        if len(tr) < J:
            raise ValueError("outer fold %d has %d eligible training patients for %d inner folds" % (f, len(tr), J))
        cuts = data.kfold_indices(len(tr), J, seed=inner_seed(seed, f))
        inner_val = [tr[v] for _, v in cuts]
        for j, (t, _) in enumerate(cuts):
            mults[f, j] = rr.mult_of(tr[t], N)
        mults[f, J] = rr.mult_of(tr, N)
        plan.append(dict(train=tr, val=va, inner_val=inner_val))
    return rr, mults, plan


def _fittable(rr, m):
    return bool((rr.event & (m > 0)).any())


def nested_cv(cohort, folds, alpha=0.5, n_lambda=30, inner=5, criterion="cindex", seed=0, ratio=0.05, standardize=True, tol=TOL,
              max_iter=MAX_ITER, backend=None, x=None):
    """Nested cross-validation of the elastic-net Cox model: all K (J + 1) L problems in ONE lock-step call (one call per outer fold when the
    cohort carries per-fold gene matrices, gene_select.fold_matrix).  Each outer fold has one lambda path, from the lambda_max of its
    full-training problem.  criterion "cindex": mean inner-validation C-index (pair_cindex); "pl": Verweij-van Houwelingen, the sum over
    the inner folds of l_all(beta_-j) - l_train(beta_-j).  A problem without events in its fit, or an inner fold without a comparable pair,
    is left out of the criterion; ties go to the larger lambda.  backend / x: the solver and the matrix it reads (tests run the same
    problems through the float64 reference).  -> list per outer fold of dict(fold, lambda_index, lambda_, lambdas, c_index, coef [G]
    (original scale), curve [L], inner [J, L], n_train, n_val, status, iterations, kkt, val_rows, val_eta)."""
    if criterion not in ("cindex", "pl"):
        raise ValueError("criterion must be 'cindex' or 'pl'")
    be = backend or HipBackend()
    label = to_numpy(cohort["label"]).astype(np.float64)
    rr, mults, plan = nested_problems(cohort, folds, inner, seed)
    K, J1, n = mults.shape
    J, L = J1 - 1, int(n_lambda)
    per_fold = "rnaseq_folds" in cohort and x is None
    groups = [[f] for f in range(K)] if per_fold else [list(range(K))]
    results = [None] * K
    for grp in groups:
        xg = gene_select.fold_matrix(cohort, grp[0] if per_fold else None) if x is None else x
        G = int(xg.shape[1])
        m = mults[grp].reshape(-1, n)                                           # [k (J + 1), n]
        scale, const = problem_scales(xg, rr, m) if standardize else (None, None)
        full = np.arange(len(grp)) * J1 + J
        if backend is None:
            _, lmax = lambda_path(xg, cohort, rr, m[full], alpha, L, ratio, None if scale is None else scale[full])
        else:                                                                   # the score on the host: U = x'(e - b) at beta = 0
            ev = be.evaluate(xg, rr, m[full], np.zeros(len(full)), np.zeros(len(full)), np.zeros((len(full), G)), scale=None)
            U = -ev["grad"] * ev["n"][:, None]
            lmax = lambda_max_from_score(U, None if scale is None else scale[full], m[full].sum(1), alpha)
        lams = np.repeat(log_path(lmax, L, ratio), J1, axis=0)                  # [k (J + 1), L]: a fold's path for all its problems
        rep = lambda a: None if a is None else np.repeat(a, L, axis=0)
        al = np.full(len(m) * L, float(alpha))
        fit = be.fit(xg, rr, rep(m), lams.reshape(-1), al, scale=rep(scale), tol=tol, max_iter=max_iter)
        beta = fit["beta"]
        need = be.evaluate(xg, rr, rep(m), lams.reshape(-1), al, beta, scale=rep(scale))      # eta of EVERY list row at the fits
        eta = need["eta"].reshape(len(grp), J1, L, n)
        ok = (np.asarray(fit["status"]).reshape(len(grp), J1, L) == 1)
        if criterion == "pl":
            m_all = np.repeat(m[full], J1, axis=0)                              # the fold's full training set, for every inner problem
            l_all = -be.evaluate(xg, rr, rep(m_all), lams.reshape(-1), al, beta, scale=rep(scale))["loss"].reshape(len(grp), J1, L)
            l_tr = -need["loss"].reshape(len(grp), J1, L)
        N = len(label)
        for i, f in enumerate(grp):
            inner_c = np.full((J, L), np.nan)
            for j in range(J):
                if not _fittable(rr, mults[f, j]):
                    continue
                if criterion == "cindex":
                    pos = rr.positions(plan[f]["inner_val"][j], N)
                    for l in range(L):
                        if ok[i, j, l]:
                            inner_c[j, l] = pair_cindex(eta[i, j, l, pos], rr.event[pos], rr.time[pos])
                else:
                    inner_c[j] = np.where(ok[i, j], l_all[i, j] - l_tr[i, j], np.nan)
            with np.errstate(invalid="ignore"):
                cnt = (~np.isnan(inner_c)).sum(0)
                tot = np.nansum(inner_c, 0)
                curve = np.where(cnt > 0, tot / np.maximum(cnt, 1) if criterion == "cindex" else tot, -np.inf)
            best = int(np.argmax(curve))                                        # first maximum = the larger lambda
            pf = (i * J1 + J) * L + best
            b = beta[pf]
            coef = b if scale is None else np.where(const[i * J1 + J], 0.0, b / scale[i * J1 + J])
            pos = rr.positions(plan[f]["val"], N)
            val_eta = eta[i, J, best, pos]
            results[f] = dict(fold=f, lambda_index=best, lambda_=float(lams[i * J1 + J, best]), lambdas=lams[i * J1 + J].copy(),
                              c_index=pair_cindex(val_eta, rr.event[pos], rr.time[pos]), coef=coef, curve=curve, inner=inner_c,
                              n_train=int(len(plan[f]["train"])), n_val=int(len(plan[f]["val"])), status=int(fit["status"][pf]),
                              iterations=np.asarray(fit["iters"]).reshape(len(grp), J1, L)[i], kkt=float(fit["kkt"][pf]),
                              val_rows=plan[f]["val"], val_eta=val_eta)
    return results


def save_coefficients(path, result, alpha, gene_names=None, columns=None):
    """fold_{k}_coefficients.json: the non-zero genes of one outer fold's chosen fit -- their column in the matrix the fit read, their
    column in the cohort's full matrix when the fold had its own (columns), their names when known, the coefficients, lambda, alpha."""
    coef = np.asarray(result["coef"], dtype=np.float64)
    nz = np.nonzero(coef)[0]
    src = nz if columns is None else np.asarray(columns)[nz]
    d = dict(fold=int(result["fold"]), lambda_=float(result["lambda_"]), lambda_index=int(result["lambda_index"]), alpha=float(alpha),
             n_genes=int(len(coef)), index=[int(j) for j in nz], column=[int(j) for j in src], coef=[float(coef[j]) for j in nz])
    if gene_names is not None:
        d["genes"] = [str(gene_names[int(j)]) for j in src]
    with open(path, "w") as f:
        json.dump(d, f, indent=2)


def load_coefficients(path):
    """-> (dense coefficient vector [n_genes] over the matrix the fit read, the file's dict)."""
    with open(path) as f:
        d = json.load(f)
    coef = np.zeros(int(d["n_genes"]))
    coef[np.asarray(d["index"], dtype=np.int64)] = np.asarray(d["coef"], dtype=np.float64)
    return coef, d
