"""Elastic-net Cox regression on the GPU (csrc/coxnet.hip, ops.coxnet_*, coxnet.py, scripts/training/cox_baseline.py):
  1. one evaluation (eta, r, loss, gradient) against the float64 reference (tests/coxnet_ref.py) at the tile edges;
  2. bit identity of a problem's results whatever shares its launch;  3. rows outside the list are not read;
  4. fits against the replica of the solver;  5. standardize;  6. nested_cv against the reference through the same problems;
  7. the entry point, final_comparison.py's row.
Shapes are the kernels' edges (16-wide tiles, 64-wide strips, 256-row scan chunks), not the workload."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import coxnet_cases as CASES
import coxnet_ref as REF
from gpu_util import DEV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10          # x the sum of absolute terms of each quantity: <= 1100 fp64 terms at 2^-53 each ~ 1e-13, two decades and more for the order

# ---- 1. one evaluation ------------------------------------------------------------------------------------------------------------
NROWS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257, 1000]
GS = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 130]
PS = [1, 2, 15, 16, 17, 33]
N, LD = 1100, 136
KINDS = ("plain", "zero", "event_free", "single", "big", "plain")
# every row count with G and P cycling, every G, every P; the kinds of the problems rotate with the call
CALLS = ([(n, GS[(3 * i + 1) % len(GS)], PS[i % len(PS)]) for i, n in enumerate(NROWS)] + [(65, G, 17) for G in GS] + [(63, 17, P) for P in PS]
         + [(1000, 130, 33), (257, 65, 16)])


@pytest.fixture(scope="module")
def eval_data():
    rng = np.random.default_rng(11)
    x = rng.normal(0.0, 1.0, (N, LD)).astype(np.float32)
    x[:, 0] = np.abs(x[:, 0])                                     # the "big" problem's gene: eta in [0, 600]
    time = rng.integers(1, 60, N).astype(np.float64)              # heavy ties
    event = rng.random(N) < 0.55
    return dict(x=x, x_dev=torch.from_numpy(x).to(DEV), time=time, event=event)


def _eval_call(d, n, G, P, salt):
    """The problems of one call: a row list of n of the N patients, P problems of rotating kinds."""
    from multimodal_survival_prediction_amd import coxnet as CX
    rng = np.random.default_rng(1000 * n + 10 * G + P + salt)
    rows = rng.permutation(N)[:n]
    rows = rows[np.argsort(-d["time"][rows], kind="stable")]
    t, e = d["time"][rows], d["event"][rows]
    rr = CX.RiskRows(rows.astype(np.int64), t, e, np.concatenate([t[1:] != t[:-1], [True]]) if n else np.zeros(0, bool))
    mult = rng.integers(0, 4, (P, n)).astype(np.int32)
    beta = rng.normal(0.0, 0.3, (P, G))
    kinds = [KINDS[(p + salt) % len(KINDS)] for p in range(P)]
    for p, k in enumerate(kinds):
        if k == "zero":
            mult[p] = 0
        elif k == "event_free":
            mult[p] *= ~e
        elif k == "single" and n:
            mult[p] = 0
            mult[p, rng.integers(0, n)] = 2
        elif k == "big" and n:
            beta[p] = 0.0
            beta[p, 0] = 600.0 / float(d["x"][rows, 0].max())
    lam, alpha = rng.uniform(0.0, 0.3, P), rng.choice([0.0, 0.3, 1.0], P)
    scale = rng.uniform(0.5, 2.0, (P, G)) if salt % 2 else None
    if scale is not None:
        scale[[k == "big" for k in kinds], 0] = 1.0                # (eta = x_0 beta_0 / scale_0 stays in [0, 600])
    return rr, mult, beta, lam, alpha, scale, kinds


@pytest.mark.parametrize("i", range(len(CALLS)))
def test_evaluation_against_the_float64_reference(eval_data, i):
    from multimodal_survival_prediction_amd import ops
    d = eval_data
    n, G, P = CALLS[i]
    rr, mult, beta, lam, alpha, scale, kinds = _eval_call(d, n, G, P, i)
    got = ops.coxnet_eval(d["x_dev"][:, :G], rr.rows, rr.event, rr.glast, mult, lam, alpha, beta, scale=scale)   # ld = 136 > G
    assert got["eta"].shape == got["r"].shape == (P, n) and got["grad"].shape == (P, G)
    for k in ("eta", "r", "grad", "loss", "f", "obj", "kkt"):
        assert np.isfinite(got[k]).all(), k
    Xl = d["x"][rr.rows, :G].astype(np.float64)
    worst = dict(eta=0.0, r=0.0, loss=0.0, grad=0.0)
    for p in range(P):
        ref = REF.evaluate(Xl if scale is None else Xl / scale[p], rr.time, rr.event, mult[p], lam[p], alpha[p], beta[p])
        for k in ("eta", "r", "loss", "grad"):
            err, bound = np.abs(got[k][p] - ref[k]), np.asarray(ref[k + "_abs"])
            worst[k] = max(worst[k], float(np.max(err / (bound + 1e-300), initial=0.0)))
            assert (err <= TOL * bound + 1e-300).all(), (p, kinds[p], k, float(np.max(err)), float(np.max(bound, initial=0.0)))
        assert (got["r"][p][mult[p] == 0] == 0).all()               # selected, not multiplied
        assert got["n"][p] == mult[p].sum()
        if kinds[p] in ("zero", "event_free") or n == 0:
            assert got["loss"][p] == 0.0 and (got["r"][p] == 0).all()
            assert np.array_equal(got["grad"][p], lam[p] * (1.0 - alpha[p]) * beta[p])
        if kinds[p] == "big" and n:
            assert np.abs(got["eta"][p]).max() >= 599.0
    print("n %d G %d P %d: worst error / term bound" % (n, G, P), worst)


def test_calls_cover_the_lists():
    assert {c[0] for c in CALLS} >= set(NROWS) and {c[1] for c in CALLS} >= set(GS) and {c[2] for c in CALLS} >= set(PS)
    seen = set()
    for i, (n, G, P) in enumerate(CALLS):
        seen |= {KINDS[(p + i) % len(KINDS)] for p in range(P)} if n else set()
    assert seen == set(KINDS)


def test_wrapper_validates_what_the_launch_cannot(eval_data):
    from multimodal_survival_prediction_amd import ops
    x = eval_data["x_dev"]
    ok = dict(row=[3, 2, 1], event=[1, 0, 1], glast=[1, 1, 1], mult=[[1, 1, 1]], lam=[0.1], alpha=[0.5], beta=np.zeros((1, LD)))
    ops.coxnet_eval(x, **ok)
    for bad in (dict(row=[3, 2, N]), dict(row=[3, -1, 1]), dict(mult=[[1, -1, 1]]), dict(mult=[[1, 0.5, 1]]), dict(lam=[-0.1]),
                dict(lam=[float("nan")]), dict(alpha=[1.5]), dict(alpha=[-0.1]), dict(scale=np.zeros((1, LD))), dict(glast=[1, 1, 0]),
                dict(scale=-np.ones((1, LD))), dict(mult=[[1, 1]]), dict(beta=np.zeros((1, LD - 1))), dict(event=[1, 0])):
        with pytest.raises(ValueError):
            ops.coxnet_eval(x, **dict(ok, **bad))
    for kw in (dict(tol=0.0), dict(max_iter=0)):
        with pytest.raises(ValueError):
            ops.coxnet_fit(x, ok["row"], ok["event"], ok["glast"], ok["mult"], ok["lam"], ok["alpha"], **kw)
    none = ops.coxnet_eval(x, [], [], [], np.zeros((2, 0)), [0.1, 0.2], [0.0, 1.0], np.ones((2, LD)))      # an empty row list
    assert none["eta"].shape == (2, 0) and (none["loss"] == 0).all() and np.array_equal(none["grad"][0], 0.1 * np.ones(LD))
    fit0 = ops.coxnet_fit(x, [], [], [], np.zeros((2, 0)), [0.1, 0.2], [0.0, 1.0])
    assert (fit0["status"] == 1).all() and (fit0["beta"] == 0).all() and (fit0["iters"] == 0).all()


# ---- 2. / 3. bit identity -----------------------------------------------------------------------------------------------------------
def _rounds(x_dev, rr, mult, lam, alpha, rounds):
    """`rounds` lock-step rounds from beta = 0 (the first evaluates the start) -> eta, grad, beta, trial, iters, step, status"""
    import ctypes
    from multimodal_survival_prediction_amd import _lib, ops
    p, t = ops.coxnet_plan(x_dev, rr.rows, rr.event, rr.glast, mult, lam, alpha, tol=1e-12)     # (nothing freezes within the rounds)
    _lib.check(_lib.load_library().mms_coxnet_iterate(ctypes.byref(p), rounds, ops.stream()), "mms_coxnet_iterate")
    P, G, n = t["P"], t["G"], t["n"]
    o = {k: t[k][:P * G].reshape(P, G).cpu().numpy() for k in ("grad", "beta", "trial")}
    o.update(eta=t["E"][:P * n].reshape(P, n).cpu().numpy(), iters=t["iters"][:P].cpu().numpy(), step=t["step"][:P].cpu().numpy(),
             status=t["status"][:P].cpu().numpy())
    return o


KEYS = ("eta", "grad", "beta", "trial", "iters", "step", "status")


@pytest.mark.parametrize("N_,G", CASES.FIT_SIZES)
def test_bit_identity(N_, G):
    """the same call twice; a problem alone and at the first, a middle and the last position among 33 others: == after 40 iterations"""
    c = CASES.fit_case(N_, G)
    x_dev = torch.from_numpy(c["cohort"]["rnaseq"]).to(DEV)[:, :G]
    sub = np.arange(0, 72, 2)[:34]                                  # 34 problems of all alphas and multiplicity vectors
    run = lambda idx: _rounds(x_dev, c["rr"], c["mult"][idx], c["lam"][idx], c["alpha"][idx], 41)
    a, b = run(sub), run(sub)
    assert all(np.array_equal(a[k], b[k]) for k in KEYS)
    moving = ~((c["lam"][sub] >= c["lmax"][sub]) & (c["alpha"][sub] > 0))       # (beta = 0 is optimal at lambda_max: frozen at once)
    assert (a["iters"][moving] == 40).all() and (a["step"][moving] != 1.0).all() and (a["iters"][~moving] == 0).all()
    for tp in (4, 7):                                               # alpha = 0.5 and alpha = 1, mid-path
        target = sub[tp]
        assert c["alpha"][target] > 0 and c["lam"][target] < c["lmax"][target]
        alone = run(np.array([target]))
        others = np.delete(sub, tp)
        for pos in (0, 16, 33):
            idx = np.concatenate([others[:pos], [target], others[pos:]])
            got = run(idx)
            for k in KEYS:
                assert np.array_equal(got[k][pos], alone[k][0]) and np.array_equal(got[k][pos], a[k][tp]), (target, pos, k)


def test_rows_outside_the_list_are_not_read():
    """NaN in every ineligible patient's row changes no bit of an evaluation or of 40 iterations"""
    from multimodal_survival_prediction_amd import ops
    c = CASES.fit_case(120, 40)
    rr, G = c["rr"], c["G"]
    x = c["cohort"]["rnaseq"].copy()
    out = np.ones(len(x), bool)
    out[rr.rows] = False
    assert out.sum() >= 10
    xp = x.copy()
    xp[out] = np.nan
    idx = np.arange(0, 72, 5)
    res = []
    for xx in (x, xp):
        xd = torch.from_numpy(xx).to(DEV)[:, :G]
        ev = ops.coxnet_eval(xd, rr.rows, rr.event, rr.glast, c["mult"][idx], c["lam"][idx], c["alpha"][idx], np.full((len(idx), G), 0.05))
        res.append((ev, _rounds(xd, rr, c["mult"][idx], c["lam"][idx], c["alpha"][idx], 41)))
    for k in ("eta", "r", "grad", "loss", "f", "obj", "kkt"):
        assert np.isfinite(res[1][0][k]).all() and np.array_equal(res[0][0][k], res[1][0][k]), k
    for k in KEYS:
        assert np.isfinite(res[1][1][k]).all() and np.array_equal(res[0][1][k], res[1][1][k]), k


# ---- 4. fits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_,G", CASES.FIT_SIZES)
def test_fits_against_the_replica(N_, G):
    from multimodal_survival_prediction_amd import coxnet as CX, ops
    c = CASES.fit_case(N_, G)
    ref = CASES.fit_reference(N_, G)
    assert all(r["status"] == 1 for r in ref)                       # the inputs let the replica itself converge (also tests/test_cpu_coxnet.py)
    rr = c["rr"]
    x_dev = torch.from_numpy(c["cohort"]["rnaseq"]).to(DEV)[:, :G]
    fit = ops.coxnet_fit(x_dev, rr.rows, rr.event, rr.glast, c["mult"], c["lam"], c["alpha"], tol=CX.TOL, max_iter=CX.MAX_ITER)
    assert (fit["status"] == 1).all(), np.nonzero(fit["status"] != 1)
    worst = dict(kkt=0.0, obj=-np.inf, beta=0.0)
    for p, r in enumerate(ref):
        lam, al = c["lam"][p], c["alpha"][p]
        at = REF.evaluate(c["X"], rr.time, rr.event, c["mult"][p], lam, al, fit["beta"][p])
        assert at["kkt"] <= CX.TOL + TOL * at["grad_abs"].max(), (p, at["kkt"])
        assert fit["obj"][p] <= r["obj"] + 1e-9 * max(1.0, abs(r["obj"])), (p, fit["obj"][p] - r["obj"])
        assert abs(fit["obj"][p] - at["obj"]) <= TOL * (at["loss_abs"] / at["n"] + abs(at["obj"])), p
        worst["kkt"], worst["obj"] = max(worst["kkt"], at["kkt"]), max(worst["obj"], fit["obj"][p] - r["obj"])
        if al < 1:
            bound = (at["kkt"] + r["kkt"]) / (lam * (1.0 - al))     # strong convexity
            diff = np.abs(fit["beta"][p] - r["beta"]).max()
            worst["beta"] = max(worst["beta"], diff / bound if bound > 0 else 0.0)
            assert diff <= bound, (p, diff, bound)
        elif lam >= c["lmax"][p]:
            assert (fit["beta"][p] == 0).all() and fit["iters"][p] == 0
    print("N %d G %d: worst reference KKT %.3e, worst obj - replica obj %.3e, worst |d beta| / bound %.3e, iterations max %d (replica %d)" % (
        N_, G, worst["kkt"], worst["obj"], worst["beta"], fit["iters"].max(), max(r["iters"] for r in ref)))
    short = ops.coxnet_fit(x_dev, rr.rows, rr.event, rr.glast, c["mult"], c["lam"], c["alpha"], tol=CX.TOL, max_iter=3, check_every=2)
    need = np.array([r["iters"] > 3 for r in ref])
    assert need.sum() > 30 and (short["status"][need] == 2).all() and (short["iters"][need] == 3).all()
    assert (short["status"][~need] == 1).all()
    assert all(ops.COXNET_STATUS[int(s)] == "not converged" for s in short["status"][need])


# ---- 5. standardize -----------------------------------------------------------------------------------------------------------------
def test_standardize_makes_the_fit_scale_free():
    """a gene multiplied by 10 (exactly: its values are multiples of 2^-10): predict unchanged to 1e-9, its coefficient x 0.1"""
    from multimodal_survival_prediction_amd import coxnet as CX
    c = CASES.fit_case(120, 40)
    cohort, rr, G = dict(c["cohort"]), c["rr"], c["G"]
    x = cohort["rnaseq"][:, :G].copy()
    x[:, 1] = np.round(x[:, 1] * 1024.0) / 1024.0
    x[:, 7] = 2.5                                                  # a constant gene: scale 1, coefficient 0
    x10 = x.copy()
    x10[:, 1] *= np.float32(10.0)
    assert np.array_equal(x10[:, 1].astype(np.float64), x[:, 1].astype(np.float64) * 10.0)
    mults = c["mult"][[0, 18 * 3]]                                  # a fold and the bootstrap resample
    xd, xd10 = torch.from_numpy(x).to(DEV), torch.from_numpy(x10).to(DEV)
    lams, _ = CX.lambda_path(xd, cohort, rr, mults, 0.5, 4, 0.1, scale=CX.problem_scales(xd, rr, mults)[0])
    a = CX.cox_path(xd, cohort, mults, lams, 0.5, rr=rr)
    b = CX.cox_path(xd10, cohort, mults, lams, 0.5, rr=rr)
    assert a.converged().all() and b.converged().all() and a.coef.shape == (2, 4, G)
    assert (a.coef[:, 0] == 0).all() and (a.coef[:, -1, 1] != 0).all()      # lambda_max: beta = 0; gene 1 is in the model at the path's end
    assert (a.coef[:, :, 7] == 0).all() and a.scale[0, 7] == 1.0
    pa, pb = a.predict(xd, rr.rows), b.predict(xd10, rr.rows)
    assert pa.shape == (2, 4, len(rr)) and np.abs(pa - pb).max() <= 1e-9
    assert np.abs(b.coef[:, :, 1] - 0.1 * a.coef[:, :, 1]).max() <= 1e-9 * np.abs(a.coef[:, :, 1]).max()
    keep = np.arange(G) != 1
    assert np.abs(b.coef[:, :, keep] - a.coef[:, :, keep]).max() <= 1e-9
    assert np.abs(pa[0, 3] - x[rr.rows].astype(np.float64) @ a.coef[0, 3]).max() <= 1e-10 * (np.abs(x[rr.rows]).astype(np.float64) @ np.abs(a.coef[0, 3])).max()


# ---- 6. nested cross-validation -----------------------------------------------------------------------------------------------------
PLANTED = 5


@pytest.fixture(scope="module")
def nested_case():
    from multimodal_survival_prediction_amd import data
    cohort = CASES.make_cohort(240, 40, seed=77, ties=False)
    return dict(cpu=cohort, dev=_to_dev(cohort), folds=data.kfold_indices(240, 3, seed=42), ref_backend=REF.Backend())


def _to_dev(cohort):
    return {k: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in cohort.items()}


@pytest.mark.parametrize("criterion", ["cindex", "pl"])
def test_nested_cv_equals_the_reference_run(nested_case, criterion):
    from multimodal_survival_prediction_amd import coxnet as CX
    c = nested_case
    kw = dict(alpha=0.5, n_lambda=8, inner=3, criterion=criterion, seed=3)
    got = CX.nested_cv(c["dev"], c["folds"], **kw)
    ref = CX.nested_cv(c["cpu"], c["folds"], backend=c["ref_backend"], x=c["cpu"]["rnaseq"], **kw)
    for f, (g, r) in enumerate(zip(got, ref)):
        s = np.sort(r["curve"])[::-1]
        print("fold", f, criterion, "reference: winner", r["lambda_index"], "inner-criterion gap to the runner-up:", s[0] - s[1],
              "outer C", r["c_index"], "GPU", g["c_index"])
        assert s[0] - s[1] > 1e-6
        assert g["lambda_index"] == r["lambda_index"] and g["c_index"] == r["c_index"]
        assert np.allclose(g["lambdas"], r["lambdas"], rtol=1e-10, atol=0) and g["status"] == 1
        if criterion == "pl":                                       # (a C-index moves by 1 / pairs when two scores swap: only the winner is pinned)
            assert np.allclose(g["curve"], r["curve"], rtol=0, atol=1e-6 * max(1.0, np.abs(r["curve"]).max()))
        assert g["n_train"] + g["n_val"] == len(CX.risk_rows(c["cpu"]))


@pytest.mark.parametrize("criterion", ["cindex", "pl"])
def test_nested_cv_finds_a_planted_gene(nested_case, criterion):
    """a gene that orders the times: non-zero in every fold's chosen fit, outer C-index > 0.8"""
    from multimodal_survival_prediction_amd import coxnet as CX
    cohort = _to_dev(CASES.make_cohort(240, 40, seed=77, planted=PLANTED, ties=False))
    for g in CX.nested_cv(cohort, nested_case["folds"], alpha=0.5, n_lambda=8, inner=3, criterion=criterion, seed=3):
        assert g["status"] == 1 and g["coef"][PLANTED] != 0 and g["c_index"] > 0.8, (g["fold"], g["coef"][PLANTED], g["c_index"])


# ---- 7. the entry point -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("select", [0, 16])
def test_entry_point(tmp_path, select):
    from multimodal_survival_prediction_amd import coxnet as CX, data, gene_select
    env = dict(os.environ, MMS_PATIENTS="60", MMS_FOLDS="2", MMS_COX_NLAMBDA="6", MMS_COX_INNER="2", PYTHONPATH=ROOT)
    env.pop("MMS_SELECT_GENES", None)
    if select:
        env["MMS_SELECT_GENES"] = str(select)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "training", "cox_baseline.py")], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "results" / "cox_baseline"
    cv = json.load(open(out / "cv_results.json"))
    assert {"model", "n_folds", "num_epochs", "c_index_mean", "c_index_std", "fold_results", "hyperparameters"} <= set(cv)
    assert cv["model"] == "Cox elastic net" and cv["n_folds"] == 2 and cv["num_epochs"] == 0 and len(cv["fold_results"]) == 2
    hp = cv["hyperparameters"]
    assert hp["alpha"] == 0.5 and hp["n_lambda"] == 6 and hp["inner_folds"] == 2 and hp["criterion"] == "cindex"
    assert (hp.get("select_genes") == 16) if select else ("select_genes" not in hp)
    cohort = data.make_cohort(n=60, dims=(32, 32, 32), seed=427, complete=True)
    x = cohort["rnaseq"].to(DEV)
    folds = data.kfold_indices(60, 2, seed=42)
    for k, fr in enumerate(cv["fold_results"], 1):
        assert {"fold", "best_c_index", "best_epoch", "train_size", "val_size"} <= set(fr) and fr["best_epoch"] == 0 and fr["fold"] == k
        assert fr["train_size"] + fr["val_size"] == 60 and 0.0 <= fr["best_c_index"] <= 1.0 and fr["converged"]
        coef, d = CX.load_coefficients(str(out / f"fold_{k}_coefficients.json"))
        assert d["lambda_"] == fr["lambda"] and len(coef) == (select or 5005) and len(d["coef"]) == fr["nonzero"]
        import pandas as pd
        df = pd.read_csv(out / f"fold_{k}_predictions.csv")
        assert list(df.columns) == ["patient_id", "survival_time", "event", "risk_score"] and len(df) == fr["val_size"]
        rows = np.array([int(s.split("-")[1]) for s in df["patient_id"]])
        assert np.array_equal(rows, gene_select.eligible_rows(cohort, folds[k - 1][1]))
        full = np.zeros(5005)
        full[np.asarray(d["column"], dtype=np.int64)] = d["coef"]   # the file's coefficients on the cohort's full matrix
        eta = CX.predict(x, full[None, :], rows)[0]
        assert np.abs(eta - df["risk_score"].to_numpy()).max() <= 1e-10 * max(1.0, np.abs(eta).max())
        assert CX.pair_cindex(eta, df["event"].to_numpy(), df["survival_time"].to_numpy()) == pytest.approx(fr["best_c_index"], abs=1e-12)
    sys.path.insert(0, os.path.join(ROOT, "scripts", "training"))
    try:
        fc = importlib.import_module("final_comparison")
    finally:
        sys.path.pop(0)
    got = fc.collect(str(tmp_path))
    assert list(got) == ["Cox elastic net"] and got["Cox elastic net"]["mean"] == pytest.approx(cv["c_index_mean"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "training", "final_comparison.py")], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Cox elastic net (+)" in r.stdout and "nested cross-validation" in r.stdout, r.stdout + r.stderr
