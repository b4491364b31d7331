"""mms_cox_newton, multivariable.cox_fit / analyse and evaluate_model.py --adjust on the MI355X against the slow numpy reference
(tests/cox_newton_ref.py).

Shapes: n in {2, 3, 63, 64, 65, 257} and 600 (both sides of a wave and of the 256-thread stride that stages a row), p in {1, 2, 5, 15, 16},
ldx > p and ldw > n, S in {1, 3} with the masks 0b1, 0b10101, bit 15 alone and all bits set, R in {1, 70} (and 4 at n = 600).
Cohorts: REF.cohort (integer times 1..11, ties shared by events and censorings, about 60 % events, x rounded to two decimals, column 0
binary, a planted signal).  Weight rows: all ones, bootstrap draws, a row that draws nobody from the latest times, a row that draws
one patient 2^k <= n times (_rows says why a power of two).

Bounds.  A converged fit ends with a Newton step <= tol on both sides, so both points are within tol of the optimum:
|beta_gpu - beta_ref| <= 2 tol, and the reference's Newton step AT the GPU's beta is <= 2 tol.  loglik, loglik0 and info are compared
with the reference evaluated at the GPU's beta, within REL of the sum of the absolute terms.  se is compared with numpy's
sqrt(diag(inv(info_gpu))) within 8 p 2^-52 kappa(I) relative.  status and iters must EQUAL the reference's wherever every decision of
the reference (convergence, pivot, acceptance, beta bound) had a factor-10 margin; the seeds were chosen on the CPU, with the reference
alone, so that at most 5 % of a case's checked rows lack that margin (asserted)."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
from scipy import stats

pytestmark = pytest.mark.gpu

import cox_newton_ref as REF
from gpu_util import DEV
from multimodal_survival_prediction_amd import multivariable as MV
from multimodal_survival_prediction_amd import ops
from multimodal_survival_prediction_amd.bootstrap import bootstrap_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
MARGIN = 10.0
E2E_SEED = 0           # chosen on the CPU with the reference alone (e2e_reference: every decision with margin, no two scores too close)


def _rows(t, n, R, seed):
    """all ones, a row without the latest times, one patient many times, a second all-ones row, the rest bootstrap draws.  The one
    patient is drawn 2^k <= min(n, 127) times (int8 multiplicities end at 127): every sum of that row is then an exact scaling of one
    term, its information is exactly zero on both sides, and the singular decision does not hang on rounding."""
    w = bootstrap_weights(n, R, seed)
    w[0] = 1
    if R >= 4:
        w[1] = np.where(t <= np.median(t), 2, 0)
        w[2] = 0
        w[2, n // 2] = 1 << int(np.log2(min(n, 127)))
        w[3] = 1
    return w


def _launch(x, t, e, w, masks, info=True, **kw):
    """sorts the patients, pads both pitches (ldx = p + 3, ldw = n + 5) with values a stray read would show, launches"""
    order, glast = MV.launch_order(t)
    n, p = x.shape
    xd = torch.full((n, p + 3), 777.0, dtype=torch.float64, device=DEV)
    xd[:, :p] = torch.from_numpy(np.ascontiguousarray(x[order])).to(DEV)
    wd = torch.full((len(w), n + 5), 99, dtype=torch.int8, device=DEV)
    wd[:, :n] = torch.from_numpy(np.ascontiguousarray(w[:, order])).to(DEV)
    out = ops.cox_newton(xd[:, :p], t[order], e[order], glast, wd[:, :n], masks, info=info, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_fit(got, r, s, x, t, e, w, mask, ref, tol=TOL):
    """one problem of a launch against the reference's fit `ref` of the same problem -> False when the reference's decisions lack margin
    (then only what does not depend on them is checked)"""
    p = x.shape[1]
    cols = REF.mask_columns(mask, p)
    off = [a for a in range(p) if a not in cols]
    beta, se, info = got["beta"][r, s], got["se"][r, s], got["info"][r, s]
    assert np.isfinite(beta).all() and (beta[off] == 0.0).all() and np.isnan(se[off]).all(), (r, s)
    assert not np.signbit(beta[off]).any()
    at = REF.evaluate(x, t, e, w, beta, cols)                          # the reference AT the GPU's beta
    zero = REF.evaluate(x, t, e, w, np.zeros(p), cols)
    assert abs(got["loglik"][r, s] - at["l"]) <= REF.REL * at["abs_l"], (r, s, got["loglik"][r, s], at["l"])
    assert abs(got["loglik0"][r, s] - zero["l"]) <= REF.REL * zero["abs_l"], (r, s)
    assert (np.abs(info - at["I"]) <= REF.REL * at["abs_I"]).all(), (r, s, np.abs(info - at["I"]).max())
    assert (info == info.T).all()
    if ref["margin"] < MARGIN:
        return False
    assert got["status"][r, s] == ref["status"] and got["iters"][r, s] == ref["iters"], (r, s, got["status"][r, s], ref["status"], got["iters"][r, s], ref["iters"])
    if ref["status"] == 1:
        assert np.abs(beta - ref["beta"]).max() <= 2 * tol, (r, s, np.abs(beta - ref["beta"]).max())
        step, _, _ = REF.newton_step(at["I"], at["g"], cols)
        assert np.abs(step).max() <= 2 * tol, (r, s)
        sub = info[np.ix_(cols, cols)]
        kappa = np.linalg.cond(sub)
        want = np.sqrt(np.diag(np.linalg.inv(sub)))
        assert (np.abs(se[cols] - want) <= 8 * p * 2.0 ** -52 * kappa * want).all(), (r, s, kappa)
    else:
        assert np.isnan(se).all()
        if ref["status"] in (3, 6) and ref["iters"] == 0:
            assert (beta == 0).all() and got["loglik"][r, s] == got["loglik0"][r, s]
    return True


# (n, p, masks, R, seed): the seeds are the first from 0 (n = 600: from 60) at which reference_case reports at most 5 % without margin
CASES = [(2, 1, [0b1], 1, 1), (3, 2, [0b1, 0b10, 0b11], 1, 0), (63, 5, [0b1, 0b10101, 0b11111], 70, 35), (64, 2, [0b11], 70, 8),
         (65, 5, [0b11111], 1, 1), (257, 16, [1 << 15, 0xffff, 0b10101], 70, 18), (257, 15, [0x7fff], 1, 1),
         (600, 16, [0xffff, 0b10101, 1 << 15], 4, 109)]


def reference_case(n, p, masks, R, seed):
    """the reference's side of a case, from the reference alone (also how the seeds were chosen, on the CPU) -> (x, t, e, w, checked
    rows, fits[r][s], share of the checked problems without margin)"""
    x, t, e = REF.cohort(n, p, seed)
    w = _rows(t, n, R, seed + 2)
    rows = list(range(R)) if R < 8 else [0, 1, 2, 3, 4, 20, 36, 53, 69]
    fits = {r: [REF.fit(x, t, e, w[r], REF.mask_columns(m, p), tol=TOL) for m in masks] for r in rows}
    weak = sum(f["margin"] < MARGIN for fs in fits.values() for f in fs)
    return x, t, e, w, rows, fits, weak / (len(rows) * len(masks))


@pytest.mark.parametrize("n,p,masks,R,seed", CASES)
def test_launch_matches_reference(n, p, masks, R, seed):
    x, t, e, w, rows, fits, weak = reference_case(n, p, masks, R, seed)
    assert weak <= 0.05
    got = _launch(x, t, e, w, masks)
    S = len(masks)
    assert got["beta"].shape == (R, S, p) and got["info"].shape == (R, S, p, p) and got["status"].shape == (R, S)
    assert set(np.unique(got["status"])) <= {1, 2, 3, 4, 5, 6} and (got["iters"] >= 0).all() and (got["iters"] <= 30).all()
    for r in rows:
        for s, m in enumerate(masks):
            _check_fit(got, r, s, x, t, e, w[r], m, fits[r][s])
    if n >= 63:
        for s, m in enumerate(masks):                                  # the cohort is well behaved: the point fit converges, kappa is moderate
            cols = REF.mask_columns(m, p)
            assert got["status"][0, s] == 1 and np.linalg.cond(got["info"][0, s][np.ix_(cols, cols)]) <= 1e4
        lit = REF.fit(*REF.resampled(x, t, e, w[rows[-1]]), None, REF.mask_columns(masks[-1], p), tol=TOL)   # a row = the literal resample
        if lit["status"] == 1 and lit["margin"] >= MARGIN:
            assert np.abs(got["beta"][rows[-1], -1] - lit["beta"]).max() <= 2 * TOL
    if R >= 4:
        for k in got:                                                  # a replicate identical to the all-ones row: the same bits
            assert got[k][3].tobytes() == got[k][0].tobytes(), k


def test_status_cases():
    """no events: 6; a column constant in the subset: 3 (and the subset without it converges); one patient n times and n = 2 with a
    separating x: what the reference says"""
    x, t, e = REF.cohort(65, 3, 2)                                     # (the first seed from 0 at which every fit below has margin)
    w = _rows(t, 65, 4, 1)
    got = _launch(x, t, np.zeros(65, np.int64), w, [0b111, 0b1])
    assert (got["status"] == 6).all() and (got["beta"] == 0).all() and (got["loglik"] == 0).all() and (got["iters"] == 0).all()
    assert np.isnan(got["se"]).all() and (got["info"] == 0).all()
    const = x.copy(); const[:, 1] = 0.5
    masks = [0b111, 0b101, 0b10]
    got = _launch(const, t, e, w, masks)
    for r in range(4):
        fits = [REF.fit(const, t, e, w[r], REF.mask_columns(m, 3), tol=TOL) for m in masks]
        assert all(f["margin"] >= MARGIN for f in fits)
        assert (fits[0]["status"] == 3 and fits[2]["status"] == 3) if r != 2 else fits[0]["status"] in (3, 6)      # (row 2: the one patient)
        for s, m in enumerate(masks):
            assert _check_fit(got, r, s, const, t, e, w[r], m, fits[s])
    assert (got["status"][[0, 1, 3], 1] == 1).all() and got["status"][2, 1] in (3, 6)
    sx, st, se_ = np.array([[0.0], [1.0]]), np.array([2.0, 1.0]), np.array([1, 1])
    for kw in (dict(beta_max=0.1), dict(beta_max=1000.0, max_iter=2)):
        ref = REF.fit(sx, st, se_, tol=TOL, **kw)
        assert ref["status"] in (2, 4) and ref["margin"] >= MARGIN
        got = _launch(sx, st, se_, np.ones((1, 2), np.int8), [1], **kw)
        assert _check_fit(got, 0, 0, sx, st, se_, np.ones(2, np.int64), 1, ref)
        assert got["status"][0, 0] == ref["status"]


def test_bit_identity():
    """Q = 210 = 70 rows x 3 masks: the first, a middle and the last problem again alone (Q = 1), and everything again without info"""
    n, p, masks = 65, 5, [0b1, 0b10101, 0b11111]
    x, t, e = REF.cohort(n, p, 2)
    w = _rows(t, n, 70, 5)
    many = _launch(x, t, e, w, masks)
    bare = _launch(x, t, e, w, masks, info=False)
    assert "info" not in bare
    for k in bare:
        assert bare[k].tobytes() == many[k].tobytes(), k
    for r, s in ((0, 0), (33, 1), (69, 2), (2, 2)):
        one = _launch(x, t, e, w[r:r + 1], masks[s:s + 1])
        for k in one:
            assert one[k][0, 0].tobytes() == many[k][r, s].tobytes(), (r, s, k)


def test_host_refusals():
    x, t, e = REF.cohort(12, 3, 3)                                     # 12 patients on 11 times: a tie is certain
    order, glast = MV.launch_order(t)
    xs, ts, es, ok = np.ascontiguousarray(x[order]), t[order], e[order], np.ones((2, 12), np.int8)
    out = ops.cox_newton(xs, ts, es, glast, np.zeros((0, 12), np.int8), [0b111])
    assert out["beta"].shape == (0, 1, 3) and out["status"].shape == (0, 1)
    out = ops.cox_newton(xs, ts, es, glast, ok, np.zeros(0, np.int64))
    assert out["beta"].shape == (2, 0, 3)
    k = int(np.nonzero(glast == 0)[0][0])
    split = glast.copy(); split[k] = 1
    merged = glast.copy(); merged[int(np.nonzero(glast[:-1])[0][0])] = 0
    nan = xs.copy(); nan[5, 1] = np.nan
    inf = xs.copy(); inf[0, 0] = np.inf
    for kw in (dict(time=ts[::-1].copy()), dict(glast=split), dict(glast=merged), dict(w=-ok), dict(x=nan), dict(x=inf), dict(cmask=[0b1000]),
               dict(cmask=[0b111, 0]), dict(event=es * 2), dict(w=ok[:, :11]), dict(x=xs[:11])):
        args = dict(x=xs, time=ts, event=es, glast=glast, w=ok, cmask=[0b111])
        args.update(kw)
        with pytest.raises(ValueError):
            ops.cox_newton(**args)
    for kw in (dict(tol=0.0), dict(tol=0.01), dict(max_iter=0), dict(beta_max=0.0)):      # the library's own refusals, before any launch
        with pytest.raises(Exception, match="bad argument"):
            ops.cox_newton(xs, ts, es, glast, ok, [0b111], **kw)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _e2e_cohort(seed, n=65):
    rng = np.random.default_rng(seed)
    age, ct = rng.normal(62.0, 9.0, n).round(0), rng.normal(size=n).round(2)
    rna = (0.5 * ct + rng.normal(size=n)).round(2)
    t = np.ceil(rng.exponential(400.0, n) * np.exp(-(0.04 * (age - 62.0) + 0.6 * ct + 0.3 * rna)) / 10.0) * 10.0     # ties
    e = (rng.random(n) < 0.7).astype(np.int64)
    return dict(age=age, ct=ct, rna=rna), t, e


def e2e_reference(seed, R=200, alpha=0.05):
    """The reference's side of the end-to-end test, from the reference alone (also how E2E_SEED was chosen, on the CPU).  weak = the fits
    with a decision without margin; gap = the smallest distance between two patients' distinct X beta over the point fits (the apparent
    C-index is a rank statistic: it is equal exactly when no two scores are within the coefficients' error of each other).  A
    quantile moves by no more than its replicates do, so the interval ends need no such condition."""
    columns, t, e = _e2e_cohort(seed)
    names, base, add = ["age", "ct", "rna"], ["age"], ["ct", "rna"]
    d = MV.design(columns)
    models = MV.model_subsets(base, add)
    w = bootstrap_weights(len(t), R, seed)
    rows = np.concatenate([np.ones((1, len(t)), np.int64), w.astype(np.int64)])
    fits = [[REF.fit(d.X, t, e, r, [names.index(k) for k in m[1]], tol=TOL, evaluate=REF.evaluate_cumsum) for m in models] for r in rows]
    pick = lambda k: np.array([[f[k] for f in row] for row in fits])
    raw = {k: pick(k) for k in ("beta", "se", "loglik", "loglik0", "iters", "status")}
    # a status can differ only through a pivot, acceptance or bound decision, or through max_iter (a flipped convergence decision is
    # one iteration more or less: two below max_iter it cannot reach it)
    weak = int(sum(min(f["margins"]["pivot"], f["margins"]["acceptance"], f["margins"]["bound"]) < MARGIN or f["iters"] > 28 for row in fits for f in row))
    abs_l = [REF.evaluate(d.X, t, e, None, f["beta"], [names.index(k) for k in m[1]])["abs_l"] for m, f in zip(models, fits[0])]
    gap = min(np.diff(np.unique(d.X @ f["beta"])).min() for f in fits[0])
    return dict(w=w, raw=raw, weak=weak, abs_l=abs_l, gap=gap, xmax=np.abs(d.X).sum(1).max(), res=MV.analyse_statistics(raw, d.X, t, e, names, models, base, add, alpha, d.scale),
                models=models)


def test_analyse_end_to_end():
    """n = 65, base = age, add = a CT score and a correlated RNA-seq score (6 models), R = 200 on the reference's own weights.  A status
    can differ from the reference's only through a pivot, acceptance or bound decision or through max_iter (a flipped convergence
    decision costs one iteration), so the condition on the inputs is margin in those (e2e_reference's `weak`).  Then: the point
    estimates and every interval end within 2 tol (hazard ratios: 4 tol relative -- exp of a coefficient that is within 2 tol), the
    likelihood-ratio statistics within 4 REL of the sums of absolute terms of the two log-likelihoods, the p-values inside the bracket
    that leaves, n_degenerate and the status counts equal"""
    R = 200
    want = e2e_reference(E2E_SEED, R)
    assert want["weak"] == 0                                           # a condition on the inputs: every status must then be equal
    assert want["gap"] > 2 * 2 * TOL * want["xmax"]                    # ... and the patients' ranks by X beta
    columns, t, e = _e2e_cohort(E2E_SEED)
    res = MV.analyse(columns, t, e, ["age"], ["ct", "rna"], R=R, seed=E2E_SEED, tol=TOL)
    ref = want["res"]
    assert res["n_degenerate"] == ref["n_degenerate"] and res["status_counts"] == ref["status_counts"] and res["replicates"] == R
    assert res["n_dropped"] == 0 and res["patients"] == 65 and [m["model"] for m in res["models"]] == [m[0] for m in want["models"]]
    near = lambda a, b, tol: abs(a - b) <= tol or (np.isnan(a) and np.isnan(b))
    for m, mr in zip(res["models"], ref["models"]):
        assert m["status"] == mr["status"] == 1 and abs(m["iters"] - mr["iters"]) <= 1 and m["columns"] == mr["columns"]
        assert near(m["c_index"], mr["c_index"], 0.0)                  # (the gap condition above: the ranks agree)
        for k, c in m["coefficients"].items():
            cr = mr["coefficients"][k]
            for key in ("beta", "beta_boot_low", "beta_boot_high"):
                assert near(c[key], cr[key], 2 * TOL), (m["model"], k, key)
            for key in ("hr", "hr_boot_low", "hr_boot_high", "hr_low", "hr_high"):
                assert near(c[key], cr[key], 4 * TOL * cr[key] + 1e-7 * cr[key] * (key in ("hr_low", "hr_high"))), (m["model"], k, key)
            assert near(c["se"], cr["se"], 1e-7 * cr["se"])            # (se at two points 2 tol apart; the launch test bounds it sharply)
            assert c["hr_boot_low"] < c["hr"] < c["hr_boot_high"]
    index = {m[1]: s for s, m in enumerate(want["models"])}
    for k, full in (("ct", ("age", "ct")), ("rna", ("age", "rna")), ("all", ("age", "ct", "rna"))):
        tolc = 2 * 4 * REF.REL * (want["abs_l"][index[full]] + want["abs_l"][index[("age",)]])
        got, exp = res["lr_tests"][k], ref["lr_tests"][k]
        assert abs(got["chi2"] - exp["chi2"]) <= tolc and got["df"] == exp["df"]
        assert stats.chi2.sf(exp["chi2"] + tolc, exp["df"]) * (1 - 1e-12) <= got["p"] <= stats.chi2.sf(max(exp["chi2"] - tolc, 0), exp["df"]) * (1 + 1e-12)
    # the draw contract: the seed alone gives bootstrap_weights' rows, explicit weights give the same numbers
    again = MV.analyse(columns, t, e, ["age"], ["ct", "rna"], weights=want["w"], tol=TOL)
    assert json.dumps(again["models"], sort_keys=True) == json.dumps(res["models"], sort_keys=True)
    # cox_fit: the same point fits, one subset at a time or together
    d = MV.design(columns)
    fits = MV.cox_fit(d.X, t, e, subsets=[[0], [0, 1], [0, 1, 2]])
    assert fits[2]["beta"].tobytes() == np.array([res["models"][-1]["coefficients"][k]["beta"] for k in ("age", "ct", "rna")]).tobytes()
    assert fits[0]["loglik"] == res["models"][0]["loglik"] and fits[1]["aic"] == res["models"][3]["aic"]
    twice = MV.cox_fit(d.X, t, e, weights=np.full(65, 2))
    assert twice[0]["status"] == 1 and np.abs(twice[0]["beta"] - fits[2]["beta"]).max() <= 2 * TOL        # every patient twice: the same optimum
    assert twice[0]["se"] == pytest.approx(fits[2]["se"] / np.sqrt(2.0), rel=1e-6)


# ---- command line -------------------------------------------------------------------------------------------------------------------
def _load():
    spec = importlib.util.spec_from_file_location("evaluate_model", os.path.join(ROOT, "scripts", "analysis", "evaluate_model.py"))
    em = importlib.util.module_from_spec(spec); spec.loader.exec_module(em)
    return em


def test_evaluate_model_adjust(tmp_path):
    """a synthetic predictions file with a planted age effect and a planted score effect: --adjust adds exactly "multivariable" and
    multivariable.csv, the adjusted hazard ratio of the score has intervals that exclude 1, and without --adjust nothing changes"""
    import pandas as pd
    em = _load()
    rng = np.random.default_rng(3)
    n = 120
    age, score, other = rng.normal(60.0, 10.0, n).round(0), rng.normal(size=n).round(3), rng.normal(size=n).round(3)
    t = np.ceil(rng.exponential(500.0, n) * np.exp(-(0.05 * (age - 60.0) + 0.8 * score)))
    ids = [f"P{i:03d}" for i in range(n)]
    df = pd.DataFrame(dict(patient_id=ids, survival_time=t, event=(rng.random(n) < 0.75).astype(int), risk_score=score))
    cov = pd.DataFrame(dict(patient_id=ids[::-1] + ["EXTRA"], age=np.append(age[::-1], 50.0), site=["a"] * (n + 1)))
    cov.loc[5, "age"] = np.nan
    cov.to_csv(tmp_path / "cov.csv", index=False)
    pd.DataFrame(dict(patient_id=ids, risk_score=other)).to_csv(tmp_path / "noise.csv", index=False)
    s0 = em.evaluate(df, str(tmp_path / "a"), plots=False, bootstrap=100, seed=1)
    s1 = em.evaluate(df, str(tmp_path / "b"), plots=False, bootstrap=100, seed=1, adjust=str(tmp_path / "cov.csv"))
    assert set(s1) - set(s0) == {"multivariable"} and {k: v for k, v in s1.items() if k != "multivariable"} == s0
    assert os.path.exists(tmp_path / "b" / "multivariable.csv") and not os.path.exists(tmp_path / "a" / "multivariable.csv")
    assert json.load(open(tmp_path / "b" / "evaluation_summary.json"))["multivariable"]["lr_tests"] == s1["multivariable"]["lr_tests"]
    mv = s1["multivariable"]
    assert mv["base"] == ["age"] and mv["add"] == ["risk_score"] and mv["n_dropped"] == 1 and mv["patients"] == n - 1 and mv["replicates"] == 100
    assert [m["model"] for m in mv["models"]] == ["base", "risk_score", "base+risk_score"]
    c = mv["models"][-1]["coefficients"]["risk_score"]
    assert c["hr_low"] > 1 and c["hr_boot_low"] > 1 and c["p"] < 1e-3 and mv["lr_tests"]["risk_score"]["p"] < 1e-3
    assert mv["models"][-1]["coefficients"]["age"]["hr_low"] > 1 and mv["models"][-1]["coefficients"]["age"]["hr_per_unit"] == pytest.approx(
        np.exp(mv["models"][-1]["coefficients"]["age"]["beta"] / mv["scale"][0]))
    table = pd.read_csv(tmp_path / "b" / "multivariable.csv")
    assert list(table.columns[:4]) == ["model", "covariate", "beta", "se"] and len(table) == 4 and "hr_boot_low" in table.columns
    # a second score joins under its file's stem; point estimates alone without --bootstrap
    s2 = em.evaluate(df, str(tmp_path / "c"), plots=False, adjust=str(tmp_path / "cov.csv"), compare=[str(tmp_path / "noise.csv")])
    mv2 = s2["multivariable"]
    assert mv2["add"] == ["risk_score", "noise"] and len(mv2["models"]) == 6 and mv2["replicates"] == 0 and set(mv2["lr_tests"]) == {"risk_score", "noise", "all"}
    assert mv2["lr_tests"]["noise"]["p"] > 0.01 and "hr_boot_low" not in mv2["models"][-1]["coefficients"]["noise"]
    pd.DataFrame(dict(patient_id=ids[1:], risk_score=other[1:])).to_csv(tmp_path / "short.csv", index=False)
    with pytest.raises(ValueError, match="patient sets differ"):
        em.evaluate(df, str(tmp_path / "d"), plots=False, adjust=str(tmp_path / "cov.csv"), compare=[str(tmp_path / "short.csv")])


def test_evaluate_model_predict_bare_adjust(tmp_path, monkeypatch):
    """--predict ... --adjust (bare) on the tiny synthetic cohort writes covariates.csv for the predicted patients (age = clinical x 100)
    and adds exactly "multivariable"; without --adjust the summary and the predictions are what they were"""
    import pandas as pd
    from oracle import models as OM
    em = _load()
    monkeypatch.setenv("MMS_PATIENTS", "45")
    torch.manual_seed(5)
    torch.save(OM.RNASeqSurvivalModel(input_dim=5005).state_dict(), tmp_path / "fold_2_best.pth")
    base = ["--predict", str(tmp_path / "fold_2_best.pth"), "--model", "rnaseq", "--fold", "2", "--no-plots"]
    s0 = em.main(base + ["--predictions", str(tmp_path / "a" / "pred.csv"), "--outdir", str(tmp_path / "a")])
    s1 = em.main(base + ["--predictions", str(tmp_path / "b" / "pred.csv"), "--outdir", str(tmp_path / "b"), "--adjust"])
    assert set(s1) - set(s0) == {"multivariable"} and {k: v for k, v in s1.items() if k != "multivariable"} == s0
    assert open(tmp_path / "a" / "pred.csv", "rb").read() == open(tmp_path / "b" / "pred.csv", "rb").read()
    assert os.path.exists(tmp_path / "b" / "covariates.csv") and not os.path.exists(tmp_path / "a" / "covariates.csv")
    pred, cov = pd.read_csv(tmp_path / "b" / "pred.csv"), pd.read_csv(tmp_path / "b" / "covariates.csv")
    assert list(cov.columns) == ["patient_id", "age"] and list(cov["patient_id"]) == list(pred["patient_id"])
    mv = s1["multivariable"]
    assert mv["base"] == ["age"] and mv["add"] == ["risk_score"] and mv["patients"] + mv["n_dropped"] == len(pred) and mv["replicates"] == 0
    assert [m["model"] for m in mv["models"]] == ["base", "risk_score", "base+risk_score"]
    assert all(m["status"] in (1, 2, 3, 4, 5, 6) and np.isfinite(m["loglik"]) for m in mv["models"])
    assert len(pd.read_csv(tmp_path / "b" / "multivariable.csv")) == 4
