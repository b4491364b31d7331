"""The problems of the elastic-net Cox tests, built on the host: tests/test_cpu_coxnet.py measures the float64 replica on them (its KKT floor
is what `tol` rests on), tests/test_gpu_coxnet.py runs the same problems through the kernels.  The replica's fits are computed once."""
import functools

import numpy as np

import coxnet_ref as REF
from multimodal_survival_prediction_amd import coxnet as CX

ALPHAS = (0.0, 0.5, 1.0)
N_LAMBDA, RATIO = 6, 0.05
FIT_SIZES = ((120, 40), (240, 130))


def make_cohort(N, ld, seed, planted=None, ties=True, ineligible=7):
    """A host cohort dict (numpy): x [N, ld] fp32 with a sparse signal, times with ties, every `ineligible`-th patient without RNA-seq or
    without a label (alternating).  planted: a gene that orders the times exactly."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (N, ld)).astype(np.float32)
    w = np.zeros(ld)
    w[:min(5, ld)] = rng.normal(0.0, 0.7, min(5, ld))
    t = rng.exponential(60.0, N) * np.exp(-(x.astype(np.float64) @ w))
    time = np.floor(t) + 1.0 if ties else t + 1.0 + np.arange(N) * 1e-6
    if planted is not None:
        x[:, planted] = (-np.argsort(np.argsort(time, kind="stable")) / N * 3.0).astype(np.float32)      # high value = early time
    event = rng.random(N) < 0.6
    has = np.ones(N, bool)
    mask = np.ones((N, 3), np.float32)
    if ineligible:
        has[ineligible - 1::2 * ineligible] = False
        mask[2 * ineligible - 1::2 * ineligible, 1] = 0.0
    return dict(rnaseq=x, label=np.stack([np.where(has, time, 0.0), np.where(has, event, 0.0)], 1), has_survival=has, mask=mask, n=N)


@functools.lru_cache(maxsize=None)
def fit_case(N, G):
    """Three fold multiplicity vectors and one bootstrap resample, alpha in ALPHAS, a 6-point path to 0.05 lambda_max each:
    4 x 3 x 6 = 72 problems over one row list.  -> dict(cohort, rr, X (float64 [n, G] list rows), mult, lam, alpha [72], lmax [72])"""
    cohort = make_cohort(N, G + 6, seed=1000 + N)
    rr = CX.risk_rows(cohort)
    n = len(rr)
    rng = np.random.default_rng(N)
    fold = rng.permutation(n) % 3
    base = [(fold != k).astype(np.int32) for k in range(3)]
    boot = np.bincount(rng.integers(0, n, n), minlength=n).astype(np.int32) * base[0]
    X = cohort["rnaseq"][rr.rows, :G].astype(np.float64)
    mult, lam, alpha, lmax = [], [], [], []
    for m in base + [boot]:
        U = -REF.evaluate(X, rr.time, rr.event, m, 0.0, 0.0, np.zeros(G))["grad"] * m.sum()
        for a in ALPHAS:
            top = float(CX.lambda_max_from_score(U, None, m.sum(), a))
            for lv in CX.log_path(np.float64(top), N_LAMBDA, RATIO):
                mult.append(m); lam.append(float(lv)); alpha.append(a); lmax.append(top)
    return dict(cohort=cohort, rr=rr, X=X, G=G, mult=np.array(mult), lam=np.array(lam), alpha=np.array(alpha), lmax=np.array(lmax))


@functools.lru_cache(maxsize=None)
def fit_reference(N, G, tol=CX.TOL, max_iter=CX.MAX_ITER):
    """The replica's fit of every problem of fit_case(N, G) -> list of REF.solve results."""
    c = fit_case(N, G)
    return [REF.solve(c["X"], c["rr"].time, c["rr"].event, c["mult"][p], c["lam"][p], c["alpha"][p], tol=tol, max_iter=max_iter)
            for p in range(len(c["lam"]))]
