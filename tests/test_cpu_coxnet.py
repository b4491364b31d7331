"""The float64 reference of the elastic-net Cox fits (tests/coxnet_ref.py) against itself, finite differences and scipy; the host side of
multimodal_survival_prediction_amd/coxnet.py (problems of nested cross-validation, lambda_max, the JSON files).  No GPU."""
import numpy as np
import pytest

import coxnet_cases as CASES
import coxnet_ref as REF
from multimodal_survival_prediction_amd import coxnet as CX, data


def _problem(n, G, seed, heavy_ties=True):
    rng = np.random.default_rng(seed)
    X = rng.normal(0, 1, (n, G))
    time = np.sort(rng.integers(1, 60, n) if heavy_ties else rng.permutation(n) + 1.0)[::-1].astype(np.float64)
    event = rng.random(n) < 0.55
    m = rng.integers(0, 4, n)
    return X, time, event, m


@pytest.mark.parametrize("n", [1, 2, 17, 64, 257, 300])
def test_mask_form_equals_cumulative_form(n):
    X, time, event, m = _problem(n, 5, n)
    eta = X @ np.random.default_rng(n + 1).normal(0, 1.5, 5)
    l0, r0, la0, ra0 = REF.loss_resid_mask(eta, time, event, m)
    l1, r1, la1, ra1 = REF.loss_resid_cum(eta, time, event, m)
    assert abs(l0 - l1) <= 1e-12 * max(la0, 1.0)
    assert (np.abs(r0 - r1) <= 1e-12 * np.maximum(ra0, 1.0)).all() and (r0[m == 0] == 0).all()
    assert abs(r0.sum()) <= 1e-10 * max(ra0.sum(), 1.0)              # the residuals of a Cox model sum to zero


def test_degenerate_problems():
    X, time, event, m = _problem(40, 3, 3)
    beta = np.array([0.3, -0.2, 0.1])
    for mm, ee in ((np.zeros(40, int), event), (m, np.zeros(40, bool))):       # no rows; no events
        ev = REF.evaluate(X, time, ee, mm, 0.2, 0.25, beta)
        assert ev["loss"] == 0.0 and (ev["r"] == 0).all() and np.allclose(ev["grad"], 0.2 * 0.75 * beta, rtol=0, atol=1e-15)


@pytest.mark.parametrize("alpha", [0.0, 0.5])
def test_gradient_against_central_differences(alpha):
    X, time, event, m = _problem(120, 7, 11)
    beta = np.random.default_rng(5).normal(0, 0.4, 7)
    lam = 0.05
    ev = REF.evaluate(X, time, event, m, lam, alpha, beta)
    h = 1e-5
    for j in range(7):
        d = np.zeros(7); d[j] = h
        fd = (REF.evaluate(X, time, event, m, lam, alpha, beta + d)["f"] - REF.evaluate(X, time, event, m, lam, alpha, beta - d)["f"]) / (2 * h)
        assert abs(fd - ev["grad"][j]) <= 1e-8 * max(1.0, abs(fd)), (j, fd, ev["grad"][j])      # O(h^2) truncation + 2^-53 |f| / h


def test_ridge_fixed_point_against_lbfgs():
    """alpha = 0: the replica's fixed point against scipy's L-BFGS-B on the same objective, within the strong-convexity bound
    (rho_replica + rho_scipy) / (lambda (1 - alpha))"""
    from scipy.optimize import minimize
    X, time, event, m = _problem(150, 12, 21, heavy_ties=False)
    lam, alpha = 0.08, 0.0
    rep = REF.solve(X, time, event, m, lam, alpha)
    assert rep["status"] == 1
    fun = lambda b: (lambda ev: (ev["f"], ev["grad"]))(REF.evaluate(X, time, event, m, lam, alpha, b))
    sp = minimize(fun, np.zeros(12), jac=True, method="L-BFGS-B", options=dict(gtol=1e-10, ftol=1e-16, maxiter=5000))
    rho_sp = REF.kkt(sp.x, fun(sp.x)[1], 0.0)
    bound = (rep["kkt"] + rho_sp) / (lam * (1.0 - alpha))
    print("ridge: rho replica %.3e, rho scipy %.3e, bound %.3e, max |d beta| %.3e" % (rep["kkt"], rho_sp, bound, np.abs(rep["beta"] - sp.x).max()))
    assert np.abs(rep["beta"] - sp.x).max() <= bound


@pytest.mark.parametrize("alpha", [0.5, 1.0])
def test_lambda_max_gives_zero_and_just_below_does_not(alpha):
    from multimodal_survival_prediction_amd.gene_select import score_coefficients
    X, time, event, m = _problem(100, 9, 31)
    rows = np.repeat(np.arange(100), m)                              # the screen's view of the problem: a row repeated is a tie
    order, a, _, _ = score_coefficients(time, event, rows)
    U = a @ X[rows][order]
    assert np.allclose(U, -REF.evaluate(X, time, event, m, 0.0, 0.0, np.zeros(9))["grad"] * m.sum(), rtol=1e-12, atol=1e-12)
    lmax = float(CX.lambda_max_from_score(U, None, m.sum(), alpha))
    at = REF.solve(X, time, event, m, lmax, alpha)
    assert at["status"] == 1 and (at["beta"] == 0).all() and at["iters"] == 0
    below = REF.solve(X, time, event, m, 0.99 * lmax, alpha)
    assert below["status"] == 1 and (below["beta"] != 0).any()
    path = CX.log_path(np.array([lmax]), 6, 0.05)[0]
    assert path[0] == lmax and np.isclose(path[-1], 0.05 * lmax) and (np.diff(np.log(path)) < 0).all()


def test_nested_problems_never_count_a_validation_patient():
    cohort = CASES.make_cohort(90, 8, seed=3)
    folds = data.kfold_indices(90, 3, seed=42)
    rr, mults, plan = CX.nested_problems(cohort, folds, inner=3, seed=5)
    N = 90
    elig = set(rr.rows.tolist())
    assert (np.diff(rr.time) <= 0).all() and rr.glast[-1] and not (set(range(N)) - elig) & elig
    assert elig == {i for i in range(N) if cohort["has_survival"][i] and cohort["mask"][i, 1] != 0}
    for f, (tr, va) in enumerate(folds):
        vpos = rr.positions(va, N)
        assert (mults[f][:, vpos[vpos >= 0]] == 0).all()              # an outer validation patient: in no problem of the fold
        got = set(rr.rows[mults[f, 3] > 0].tolist())
        assert got == set(tr.tolist()) & elig and mults[f].max() == 1
        seen = []
        for j in range(3):
            ipos = rr.positions(plan[f]["inner_val"][j], N)
            assert (ipos >= 0).all() and (mults[f, j, ipos] == 0).all()     # an inner validation patient: not in the fit scored on it
            assert set(rr.rows[mults[f, j] > 0].tolist()) == got - set(plan[f]["inner_val"][j].tolist())
            seen += plan[f]["inner_val"][j].tolist()
        assert sorted(seen) == sorted(got)                           # the inner folds partition the training patients
    again = CX.nested_problems(cohort, folds, inner=3, seed=5)[1]
    other = CX.nested_problems(cohort, folds, inner=3, seed=6)[1]
    assert (again == mults).all() and (other != mults).any()


def test_coefficient_file_round_trip(tmp_path):
    coef = np.zeros(20)
    coef[[2, 7, 19]] = [0.1234567890123456, -3.5e-7, 2.0]
    res = dict(fold=1, lambda_=0.0123, lambda_index=4, coef=coef)
    p = str(tmp_path / "fold_2_coefficients.json")
    CX.save_coefficients(p, res, 0.5, gene_names=["g%d" % i for i in range(100)], columns=np.arange(20) * 3)
    back, d = CX.load_coefficients(p)
    assert (back == coef).all() and d["genes"] == ["g6", "g21", "g57"] and d["column"] == [6, 21, 57] and d["index"] == [2, 7, 19]
    assert d["lambda_"] == 0.0123 and d["alpha"] == 0.5 and d["fold"] == 1 and d["lambda_index"] == 4
    CX.save_coefficients(p, res, 1.0)
    back, d = CX.load_coefficients(p)
    assert (back == coef).all() and "genes" not in d and d["column"] == d["index"]


def test_pair_cindex_rule():
    h = np.array([3.0, 2.0, 2.0, 0.5])
    t = np.array([1.0, 2.0, 3.0, 4.0])
    assert CX.pair_cindex(h, [1, 1, 0, 0], t) == (3 + 1.5) / 5
    assert np.isnan(CX.pair_cindex(h, [0, 0, 0, 0], t))


@pytest.mark.parametrize("N,G", CASES.FIT_SIZES)
def test_replica_converges_on_the_gpu_tests_problems_and_its_kkt_floor(N, G):
    """The measurement `tol` rests on: every problem of the GPU fit test converges in the replica within max_iter at tol, and the floor
    the replica's KKT residual reaches on the hardest of them (the smallest lambda of a path) is printed"""
    c = CASES.fit_case(N, G)
    ref = CASES.fit_reference(N, G)
    its = np.array([r["iters"] for r in ref])
    print("N=%d G=%d: replica iterations max %d (alpha 0: %d, 0.5: %d, 1: %d)" % (
        N, G, its.max(), its[c["alpha"] == 0].max(), its[c["alpha"] == 0.5].max(), its[c["alpha"] == 1].max()))
    assert all(r["status"] == 1 and r["kkt"] <= CX.TOL for r in ref)
    floors = []
    for a in CASES.ALPHAS:
        p = [q for q in range(len(c["lam"])) if c["alpha"][q] == a][CASES.N_LAMBDA - 1]        # first multiplicity vector, smallest lambda
        fl = REF.solve(c["X"], c["rr"].time, c["rr"].event, c["mult"][p], c["lam"][p], a, beta0=ref[p]["beta"], max_iter=1500, floor=True)
        floors.append(fl["kkt_floor"])
        print("  alpha %.1f lambda %.3e: KKT floor %.2e" % (a, c["lam"][p], fl["kkt_floor"]))
    assert max(floors) <= 1e-7                                       # else tol must become 10 x the floor
