"""mms_td_metrics and absolute_risk.prediction_error on the MI355X against the slow numpy reference (tests/td_metrics_ref.py): exact
integer outputs, the product limits within one rounding per factor and per multiply, the weighted sums within the project's fp64
criterion, the NaN / zero conventions, independence of a replicate's bits from the rest of the launch, and intervals / paired p-values
equal to the reference's on the same weights.

Shapes: n in {2, 3, 63, 64, 65, 257} and 600 (the 256 threads stage a row in several strides; the whole row stays in LDS up to
MMS_TD_MAX_N, there is no tile to get past); H in {1, 2, 31, 32, 33, 63, 64} (both sides of the two-models-per-wave switch at 32);
M in {1, 3, 9} (9: past the four waves of a block with one model per wave, and an odd model left over with two per wave); R in {1, 70}
(and 4 at n = 600).
Labels: integer times 1..11 with 60 % events (events and censorings share times), risks rounded to one decimal; an all-censored and a
censoring-free cohort.  Horizons (H >= 3): one before the first time, one exactly on a tied time, one past the last time.  Weight rows:
all ones, bootstrap draws, a row that draws nobody from the latest times, a row that draws one patient n times."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import td_metrics_ref as REF
from gpu_util import DEV
from multimodal_survival_prediction_amd import absolute_risk as AR
from multimodal_survival_prediction_amd import ops
from multimodal_survival_prediction_amd.bootstrap import bootstrap_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E_SEED = 0           # chosen on the CPU with the reference alone: no degenerate replicate, no comparison within tolerance (asserted below)
# Derived quantities (AUC = num / (wcase wctrl), BS_null, IPA, the integrals and their quantiles) are quotients and products of at most
# three sums that each carry REL relative error, of values in [0, 1]: 4 REL covers them (and 4 REL per unit of |IPA|).
DERIVED = 4 * REF.REL


def _cohort(n, M, H, kind, seed):
    rng = np.random.default_rng([seed, n, M, H])
    t = rng.integers(1, 12, n).astype(np.float64)
    e = (rng.random(n) < 0.6).astype(np.int64)
    if kind == "allcens":
        e[:] = 0
    if kind == "nocens":
        e[:] = 1
    risk = rng.normal(size=(M, n)).round(1)
    if H == 1:
        tau = np.array([6.0])
    elif H == 2:
        tau = np.array([0.5, 12.0])
    else:
        tau = np.unique(np.concatenate([[0.5, 3.0, 12.0], np.linspace(0.8, 11.6, H - 3)]))
    assert len(tau) == H and (np.diff(tau) > 0).all()
    surv = rng.random((M, n, H))
    return t, e, risk, surv, tau


def _rows(t, n, R, seed):
    """all ones, a row without the latest times, one patient n times, the rest bootstrap draws"""
    w = bootstrap_weights(n, R, seed)
    w[0] = 1
    if R >= 3:
        w[1] = np.where(t <= np.median(t), 2, 0)
        w[2] = 0
        w[2, n // 2] = min(n, 127)                                     # (int8 multiplicities end at 127)
    return w


def _launch(t, e, risk, surv, tau, w):
    order, trank, es, hcut, rord = AR.metric_inputs(risk, t, e, tau)
    out = ops.td_metrics(trank, es, hcut, rord, np.ascontiguousarray(surv[:, order, :]), np.ascontiguousarray(w[:, order]))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_row(got, r, ref):
    assert np.array_equal(got["wctrl"][r], ref["wctrl"])                                           # integer-valued: exact
    for k in ("G", "km"):                                                                          # one rounding per factor and per multiply on each side
        assert (np.abs(got[k][r] - ref[k]) <= 2 * ref["nfac"] * REF.EPS * np.abs(ref[k])).all(), (k, r)
    for k in ("wcase", "brier", "auc_num"):
        assert (np.abs(got[k][r] - ref[k]) <= REF.REL * ref["abs_" + k]).all(), (k, r, np.abs(got[k][r] - ref[k]).max())
    nocase, noctrl = ref["wcase"] == 0, ref["wctrl"] == 0
    assert (got["wcase"][r][nocase] == 0).all() and (got["auc_num"][r][:, nocase | noctrl] == 0).all()
    assert np.isfinite(got["brier"][r]).all() and np.isfinite(got["wcase"][r]).all() and np.isfinite(got["G"][r]).all()
    assert (got["G"][r][~noctrl] > 0).all()                                                       # a drawn control: G(tau) > 0


CASES = [(2, 1, 1, "ties", 1), (3, 2, 3, "ties", 1), (63, 31, 9, "ties", 70), (64, 32, 3, "ties", 70), (65, 33, 9, "ties", 70),
         (257, 63, 3, "ties", 70), (64, 64, 1, "allcens", 70), (65, 32, 9, "nocens", 70), (600, 64, 9, "ties", 4), (257, 2, 1, "ties", 1)]


@pytest.mark.parametrize("n,H,M,kind,R", CASES)
def test_launch_matches_reference(n, H, M, kind, R):
    t, e, risk, surv, tau = _cohort(n, M, H, kind, 1)
    w = _rows(t, n, R, 3)
    got = _launch(t, e, risk, surv, tau, w)
    assert got["brier"].shape == (R, M, H) and got["G"].shape == (R, H)
    rows = range(R) if R < 8 else (0, 1, 2, 3, 36, 69)
    for r in rows:
        ref = (REF.metrics if n <= 3 else REF.metrics_vec)(t, e, risk, surv, tau, w[r])
        _check_row(got, r, ref)
        if r == 3:                                                                                 # a bootstrap row = the reference on the literally resampled arrays
            lit = REF.metrics_vec(*REF.resampled(t, e, risk, surv, w[r]), tau)
            _check_row(got, r, lit)
    ones = REF.metrics_vec(t, e, risk, surv, tau)                                                  # the all-ones row = the unweighted reference
    _check_row(got, 0, ones)
    if H >= 2:
        assert (got["G"][:, 0] == 1.0).all() and (got["km"][:, 0] == 1.0).all() and (got["wcase"][:, 0] == 0).all()      # before the first time
        want = ((1 - surv[:, :, 0]) ** 2 * w[0][None, :]).sum(1) / w[0].sum()
        assert np.abs(got["brier"][0, :, 0] - want).max() <= REF.REL * want.max()
        assert (got["wctrl"][:, -1] == 0).all() and (got["auc_num"][:, :, -1] == 0).all()          # past the last time: no control
    if kind == "allcens":
        assert (got["wcase"] == 0).all() and (got["km"] == 1.0).all() and (got["auc_num"] == 0).all()
    if kind == "nocens":
        assert (got["G"] == 1.0).all()
    # the host's conventions on these raw outputs: AUC is NaN exactly where a factor of its denominator is 0
    raw = {k: np.concatenate([v[:1], v]) for k, v in got.items()}                                  # (row 0 doubles as the point estimate)
    res = AR.prediction_error_statistics(dict(raw, wsum=np.concatenate([w[:1], w]).sum(1, dtype=np.int64)), tau)
    auc = res.auc.boot                                                                             # [M, H, R]
    assert np.array_equal(np.isnan(auc), np.broadcast_to(((got["wcase"] * got["wctrl"]) == 0).T[None], auc.shape))
    assert ((auc[~np.isnan(auc)] >= 0) & (auc[~np.isnan(auc)] <= 1 + DERIVED)).all()


@pytest.mark.parametrize("H", [32, 33])
def test_bit_identity_alone_and_among_70(H):
    """R = 70, M = 9; every seventh row again in a launch of its own, with all nine models and with the first model alone"""
    n, M = 65, 9
    t, e, risk, surv, tau = _cohort(n, M, H, "ties", 2)
    w = _rows(t, n, 70, 5)
    many = _launch(t, e, risk, surv, tau, w)
    for r in range(0, 70, 7):
        one = _launch(t, e, risk, surv, tau, w[r:r + 1])
        for k in one:
            assert one[k][0].tobytes() == many[k][r].tobytes(), (r, k)
        first = _launch(t, e, risk[:1], surv[:1], tau, w[r:r + 1])
        for k in ("G", "km", "wcase", "wctrl"):
            assert first[k][0].tobytes() == many[k][r].tobytes(), (r, k)
        for k in ("brier", "auc_num"):
            assert first[k][0, 0].tobytes() == many[k][r, 0].tobytes(), (r, k)


def test_no_replicates_and_host_checks():
    t, e, risk, surv, tau = _cohort(12, 2, 3, "ties", 3)                # 12 patients on 11 times: a tie is certain
    order, trank, es, hcut, rord = AR.metric_inputs(risk, t, e, tau)
    sv, ok = np.ascontiguousarray(surv[:, order, :]), np.ones((2, 12), np.int8)
    out = ops.td_metrics(trank, es, hcut, rord, sv, np.zeros((0, 12), np.int8))
    assert out["G"].shape == (0, 3) and out["brier"].shape == (0, 2, 3)
    twice = rord.copy(); twice[0, 1] = twice[0, 0]
    unflagged = rord.copy(); unflagged[1, -1] &= ~1
    split = hcut.copy(); split[1] = int(np.nonzero(np.diff(trank) == 0)[0][0]) + 1
    late_event = es.copy(); k = int(np.nonzero(np.diff(trank) == 0)[0][0]); late_event[k], late_event[k + 1] = 0, 1
    zero = ok.copy(); zero[1] = 0
    for kw in (dict(rord=twice), dict(rord=unflagged), dict(hcut=split), dict(hcut=hcut[::-1].copy()), dict(event=late_event),
               dict(trank=trank * 2), dict(w=zero), dict(w=-ok), dict(surv=np.where(sv > 0.9, np.nan, sv)), dict(surv=sv[:, :, :2])):
        args = dict(trank=trank, event=es, hcut=hcut, rord=rord, surv=sv, w=ok)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.td_metrics(**args)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _e2e_cohort(seed, n=65, H=8):
    rng = np.random.default_rng(seed)
    t = (rng.exponential(400.0, n)).round(-1) + 10                    # ties
    e = (rng.random(n) < 0.67).astype(np.int64)
    risk = np.stack([rng.normal(size=n), -np.log(t) + rng.normal(size=n) * 1.5, (-np.log(t) + rng.normal(size=n)).round(1)])
    tau = AR.default_horizons(t, e, H)
    fit = rng.random(n) < 0.5                                        # any fit set will do: the baseline only has to give probabilities
    surv = np.stack([AR.breslow_baseline(r[fit], t[fit], e[fit]).survival(r, tau) for r in risk])
    return t, e, risk, surv, tau


def _ends(x, alpha):
    """-> (low, high, clear): numpy's linear-interpolation quantiles of x [R] and the smallest gap between a replicate that defines
    one of them and its outer neighbour"""
    s = np.sort(x)
    gaps = []
    for q in (alpha / 2, 1 - alpha / 2):
        pos = q * (len(s) - 1)
        lo, hi = int(np.floor(pos)), int(np.ceil(pos))
        gaps += [s[lo] - s[lo - 1] if lo > 0 else np.inf, s[hi + 1] - s[hi] if hi + 1 < len(s) else np.inf]
    return np.quantile(x, alpha / 2), np.quantile(x, 1 - alpha / 2), min(gaps)


def e2e_reference(seed, R=200, alpha=0.05):
    """The reference's side of the end-to-end test, from the reference alone (also how E2E_SEED was chosen, on the CPU) -> dict with
    the point estimates, the intervals and p-values of IBS / iAUC, n_degenerate and `near`: the number of comparisons that a
    tolerance-sized error could flip (replicate differences within tolerance of 0, replicates within tolerance of a quantile's
    defining neighbour)."""
    t, e, risk, surv, tau = _e2e_cohort(seed)
    n, M = len(t), len(risk)
    w = np.concatenate([np.ones((1, n), np.int8), bootstrap_weights(n, R, seed)])
    rows = [REF.metrics_vec(t, e, risk, surv, tau, r) for r in w]
    der = [REF.derived(m) for m in rows]
    brier, auc = np.stack([m["brier"] for m in rows]), np.stack([d[0] for d in der])               # [1 + R, M, H]
    null, ipa = np.stack([d[1] for d in der]), np.stack([d[2] for d in der])
    ibs, iauc = REF.trapezoid_mean(brier, tau), REF.trapezoid_mean(auc, tau)                       # [1 + R, M]
    out = dict(w=w[1:], brier=brier[0], auc=auc[0], null=null[0], ipa=ipa[0], ibs=ibs[0], iauc=iauc[0],
               n_degenerate=int(np.isnan(auc[1:]).any(axis=(1, 2)).sum()), near=0, ci={}, p={}, delta_ci={})
    if out["n_degenerate"]:
        return out
    for name, x in (("ibs", ibs[1:]), ("iauc", iauc[1:])):
        tol = DERIVED * np.abs(x).max()
        for a in range(M):
            lo, hi, clear = _ends(x[:, a], alpha)
            out["ci"][name, a] = (lo, hi, x[:, a].std(ddof=1))
            out["near"] += int(clear <= 2 * tol)
            for b in range(M):
                d = x[:, a] - x[:, b]
                lo, hi, clear = _ends(d, alpha)
                out["delta_ci"][name, a, b] = (lo, hi)
                out["p"][name, a, b] = min(1.0, 2.0 * min((np.count_nonzero(d <= 0) + 1) / (R + 1), (np.count_nonzero(d >= 0) + 1) / (R + 1)))
                if a != b:
                    out["near"] += int((np.abs(d) <= 2 * tol).sum()) + int(clear <= 4 * tol)
    return out


def test_prediction_error_end_to_end():
    """n = 65, M = 3 (noise, a weak signal, a rounded score with risk ties), H = 8, R = 200 on the reference's own weights"""
    R = 200
    want = e2e_reference(E2E_SEED, R)
    assert want["n_degenerate"] == 0 and want["near"] == 0             # a condition on the inputs: every p-value must then be equal exactly
    t, e, risk, surv, tau = _e2e_cohort(E2E_SEED)
    res = AR.prediction_error(surv, risk, t, e, tau, R=R, seed=E2E_SEED)
    assert res.n_degenerate == 0 and res.replicates == R and res.brier.value.shape == (3, 8)
    close = lambda a, b: (np.abs(np.asarray(a) - np.asarray(b)) <= DERIVED * np.maximum(1.0, np.abs(np.asarray(b)))).all()
    assert close(res.brier.value, want["brier"]) and close(res.auc.value, want["auc"]) and close(res.brier_null.value, want["null"])
    assert close(res.ipa.value, want["ipa"]) and close(res.ibs.value, want["ibs"]) and close(res.iauc.value, want["iauc"])
    for name, est, diff in (("ibs", res.ibs, res.ibs_diff), ("iauc", res.iauc, res.iauc_diff)):
        for a in range(3):
            lo, hi, se = want["ci"][name, a]
            assert close(est.low[a], lo) and close(est.high[a], hi) and close(est.se[a], se)
            for b in range(3):
                assert diff.p_value[a, b] == want["p"][name, a, b], (name, a, b)
                assert close(diff.low[a, b], want["delta_ci"][name, a, b][0]) and close(diff.high[a, b], want["delta_ci"][name, a, b][1])
    assert (res.brier.low <= res.brier.high).all() and (res.auc.low <= res.auc.high).all()
    # the draw contract: the seed alone gives bootstrap_weights' rows, explicit weights give the same numbers
    again = AR.prediction_error(surv, risk, t, e, tau, weights=want["w"])
    assert again.ibs.boot.tobytes() == res.ibs.boot.tobytes() and again.iauc.boot.tobytes() == res.iauc.boot.tobytes()
    single = AR.prediction_error(surv[1], risk[1], t, e, tau, R=0)
    assert single.ibs.value[0].tobytes() == res.ibs.value[1].tobytes() and single.replicates == 0 and np.isnan(single.ibs.low).all()


# ---- command line -------------------------------------------------------------------------------------------------------------------
def _load():
    spec = importlib.util.spec_from_file_location("evaluate_model", os.path.join(ROOT, "scripts", "analysis", "evaluate_model.py"))
    em = importlib.util.module_from_spec(spec); spec.loader.exec_module(em)
    return em


def test_evaluate_model_horizons(tmp_path, monkeypatch):
    """--predict ... --horizons 4 --bootstrap 50 on the tiny synthetic cohort writes the four files and adds exactly "prediction_error";
    without --horizons the summary and the CSV bytes are what they were"""
    import pandas as pd
    from oracle import models as OM
    em = _load()
    monkeypatch.setenv("MMS_PATIENTS", "30")
    torch.manual_seed(5)
    torch.save(OM.RNASeqSurvivalModel(input_dim=5005).state_dict(), tmp_path / "fold_2_best.pth")
    base = ["--predict", str(tmp_path / "fold_2_best.pth"), "--model", "rnaseq", "--fold", "2", "--bootstrap", "50", "--no-plots"]
    s0 = em.main(base + ["--predictions", str(tmp_path / "a" / "pred.csv"), "--outdir", str(tmp_path / "a")])
    s1 = em.main(base + ["--predictions", str(tmp_path / "b" / "pred.csv"), "--outdir", str(tmp_path / "b"), "--horizons", "4"])
    assert set(s1) - set(s0) == {"prediction_error"} and {k: v for k, v in s1.items() if k != "prediction_error"} == s0
    assert open(tmp_path / "a" / "pred.csv", "rb").read() == open(tmp_path / "b" / "pred.csv", "rb").read()
    assert open(tmp_path / "a" / "kaplan_meier_table.csv", "rb").read() == open(tmp_path / "b" / "kaplan_meier_table.csv", "rb").read()
    for f in ("survival_curves.csv", "prediction_error.csv", "calibration.csv", "train_predictions.csv"):
        assert os.path.exists(tmp_path / "b" / f) and not os.path.exists(tmp_path / "a" / f), f
    pe = s1["prediction_error"]
    assert len(pe["horizons"]) == 4 and pe["replicates"] == 50 and pe["seed"] == 0 and 0 <= pe["ibs"] <= 1
    pred, curves = pd.read_csv(tmp_path / "b" / "pred.csv"), pd.read_csv(tmp_path / "b" / "survival_curves.csv")
    assert list(curves.columns[:4]) == ["patient_id", "survival_time", "event", "risk_score"] and len(curves.columns) == 8
    assert list(curves["patient_id"]) == list(pred["patient_id"])
    S = curves.iloc[:, 4:].to_numpy()
    assert ((S >= 0) & (S <= 1)).all() and (np.diff(S, axis=1) <= 0).all()
    table = pd.read_csv(tmp_path / "b" / "prediction_error.csv")
    assert list(table.columns[:5]) == ["horizon", "brier", "brier_null", "ipa", "auc"] and len(table) == 4 and "brier_low" in table.columns
    train = pd.read_csv(tmp_path / "b" / "train_predictions.csv")
    assert list(train.columns) == list(pred.columns) and len(train) + len(pred) == 30 and not set(train["patient_id"]) & set(pred["patient_id"])
    assert pd.read_csv(tmp_path / "b" / "calibration.csv")["patients"].sum() == len(pred)
