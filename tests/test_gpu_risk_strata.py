"""mms_logrank_scan and risk_strata.stratify on the MI355X against the slow numpy reference (tests/logrank_scan_ref.py): exact group
counts, U and V within the project's fp64 criterion, the chi2 / max / argmax contract bit for bit, independence of a problem's bits from
the rest of the launch, and permutation p-values equal to the reference's on the same permutations.

Shapes: n in {2, 3, 63, 64, 65, 257} and 600 (past one LDS stage of 512 positions); C in {0, 1, 63, 64, 65, 130} mixed in one launch,
plus 300 (past one chunk of 256 cuts per workgroup); Q in {1, 70}.  Every cut list of two or more cuts starts with the cut below every
rank and ends with the cut above every rank: one group is empty there, V = 0 and chi2 = 0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import stats

pytestmark = pytest.mark.gpu

import logrank_scan_ref as REF
from gpu_util import DEV
from multimodal_survival_prediction_amd import ops
from multimodal_survival_prediction_amd import risk_strata as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 63, 64, 65, 130)
STRATIFY_SEED = 0          # chosen on the CPU: the reference shows no replicate within tolerance of an observed statistic (asserted below)


def _labels(kind, n, seed):
    rng = np.random.default_rng([seed, n])
    t = rng.integers(1, 12, n).astype(np.float64)                    # heavy ties: events and censorings share times
    e = (rng.random(n) < 0.6).astype(np.int64)
    if kind == "lonely":                                             # the latest time has one patient: n_u = 1 at the first position
        t[n // 2], e[n // 2] = 20.0, 1
    if kind == "noevent":
        e[:] = 0
    return t, e


def _problem(n, C, rng):
    """a rank vector with ties (patient order) and C ascending cuts over it, the two one-group cuts included"""
    rank = np.unique(rng.integers(0, max(2, n // 2), n), return_inverse=True)[1].reshape(-1).astype(np.int32)
    k = int(rank.max()) + 1
    cuts = np.sort(rng.integers(0, k + 1, C)).astype(np.int32)
    if C >= 2:
        cuts[0], cuts[-1] = 0, k
    return rank, cuts


def _launch(t, e, ranks, cutlists, at=None, tables=True):
    """ranks in patient order -> the launch's outputs as host arrays"""
    order, _, h, c, pflag = RS.logrank_coefficients(t, e)
    coff = np.concatenate([[0], np.cumsum([len(x) for x in cutlists])])
    cut = np.concatenate(cutlists) if len(cutlists) else np.zeros(0, np.int32)
    out = ops.logrank_scan(torch.from_numpy(np.ascontiguousarray(np.stack(ranks)[:, order])).to(DEV), pflag, np.stack([h, c], 1), coff, cut,
                           at=at, tables=tables)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_problem(got, q, ref, C, at, n):
    """the checks of one problem against its reference table"""
    U, V = got["U"][q, :C], got["V"][q, :C]
    assert np.array_equal(got["n_high"][q, :C], ref["n_high"]) and np.array_equal(got["d_high"][q, :C], ref["d_high"])          # exact counts
    assert (np.abs(U - ref["U"]) <= REF.REL * ref["absU"]).all(), np.abs(U - ref["U"]).max()
    assert (np.abs(V - ref["V"]) <= REF.REL * ref["absV"]).all(), np.abs(V - ref["V"]).max()
    chi2 = RS.chi2_of(U, V)
    assert np.isfinite(chi2).all() and (chi2[V <= 0] == 0).all()
    one_group = (ref["n_high"] == 0) | (ref["n_high"] == n)
    assert (V[one_group] == 0).all() and (chi2[one_group] == 0).all()
    if C == 0:
        assert got["chi2_max"][q] == 0.0 and got["arg_max"][q] == -1 and got["chi2_at"][q] == 0.0
        return
    assert got["chi2_at"][q].tobytes() == chi2[at].tobytes()
    assert got["chi2_max"][q].tobytes() == chi2.max().tobytes()
    assert got["arg_max"][q] == int(np.argmax(chi2))                 # the first index attaining the maximum
    tol = REF.chi2_tolerance(ref)
    j, jr = int(got["arg_max"][q]), int(np.argmax(ref["chi2"]))
    assert abs(ref["chi2"][j] - ref["chi2"][jr]) <= tol[j] + tol[jr]
    assert (np.abs(chi2 - ref["chi2"]) <= tol).all()


@pytest.mark.parametrize("n,kind,extra", [(2, "ties", ()), (3, "ties", ()), (63, "ties", ()), (64, "ties", ()), (65, "lonely", ()),
                                          (64, "noevent", ()), (257, "ties", (300,)), (257, "lonely", ()), (600, "ties", (300,))])
def test_scan_matches_reference(n, kind, extra):
    t, e = _labels(kind, n, 1)
    rng = np.random.default_rng([7, n])
    probs = [_problem(n, C, rng) for C in SIZES + tuple(extra)]
    at = np.array([len(c) // 2 if len(c) else -1 for _, c in probs])
    got = _launch(t, e, [r for r, _ in probs], [c for _, c in probs], at=at)
    for q, (rank, cuts) in enumerate(probs):
        _check_problem(got, q, REF.scan(t, e, rank, cuts), len(cuts), at[q], n)
    if kind == "noevent":
        assert not got["U"].any() and not got["V"].any() and not got["chi2_max"].any() and not got["d_high"].any()


def test_bit_identity_alone_and_among_70():
    """Q = 70 with mixed cut counts; every seventh problem again in a launch of its own, with and without the tables"""
    n = 65
    t, e = _labels("ties", n, 2)
    rng = np.random.default_rng(70)
    probs = [_problem(n, SIZES[q % len(SIZES)], rng) for q in range(70)]
    at = np.array([len(c) - 1 for _, c in probs])
    many = _launch(t, e, [r for r, _ in probs], [c for _, c in probs], at=at)
    ref0 = REF.scan(t, e, *probs[5])
    _check_problem(many, 5, ref0, len(probs[5][1]), at[5], n)
    for q in range(0, 70, 7):
        rank, cuts = probs[q]
        C = len(cuts)
        for tables in (True, False):
            one = _launch(t, e, [rank], [cuts], at=at[q:q + 1], tables=tables)
            for k in ("chi2_max", "arg_max", "chi2_at") + (("U", "V", "n_high", "d_high") if tables else ()):
                a, b = (one[k][0, :C], many[k][q, :C]) if one[k].ndim == 2 else (one[k][0], many[k][q])
                assert a.tobytes() == b.tobytes(), (q, k, tables)


def test_no_problems_and_host_checks():
    t, e = _labels("ties", 8, 3)
    order, _, h, c, pflag = RS.logrank_coefficients(t, e)
    coef = np.stack([h, c], 1)
    out = ops.logrank_scan(torch.zeros(0, 8, dtype=torch.int32, device=DEV), pflag, coef, [0], [], tables=True)
    assert out["chi2_max"].shape == (0,) and out["U"].shape == (0, 0)
    rank = torch.zeros(2, 8, dtype=torch.int32, device=DEV)
    for kw in (dict(coff=[0, 2, 3], cut=[2, 1, 1]),                  # a set that is not ascending
               dict(coff=[0, 2, 1], cut=[1, 2]),                     # offsets that go back
               dict(coff=[0, 1, 2], cut=[1, 1], cset=[0, 2]),        # a set that does not exist
               dict(coff=[0, 1, 2], cut=[1, 1], at=[0, 1]),          # a designated cut outside its set
               dict(coff=[0, 1], cut=[1])):                          # one set for two problems and no map
        with pytest.raises(ValueError):
            ops.logrank_scan(rank, pflag, coef, **kw)
    with pytest.raises(ValueError):
        ops.logrank_scan(rank, pflag ^ 2, coef, [0, 1, 2], [1, 1])   # flags that contradict the coefficients
    # ascending is checked per set: the second set may start below the first one's end
    ops.logrank_scan(rank, pflag, coef, [0, 2, 4], [1, 2, 0, 1])


def _cohort(n, seed):
    rng = np.random.default_rng(seed)
    t = rng.exponential(400.0, n)
    e = (rng.random(n) < 0.67).astype(np.int64)
    risk = np.stack([rng.normal(size=n), -np.log(t) + rng.normal(size=n) * 1.5, (rng.normal(size=n)).round(1)])
    return t, e, risk


def test_stratify_matches_reference_statistics():
    """M = 3 (noise, a weak signal, a rounded score with ties), n = 120, R = 200, on the SAME permutations as the reference"""
    n, R = 120, 200
    t, e, risk = _cohort(n, STRATIFY_SEED)
    perms = RS.draw_permutations(n, R, STRATIFY_SEED)
    want = REF.stratify(risk, t, e, perms, 0.1)
    assert [w["near"] for w in want] == [0, 0, 0]                    # no comparison is left out: every p-value must be equal exactly
    res = RS.stratify(risk, t, e, permutations=perms, min_prop=0.1)
    assert res.replicates == R and len(res.models) == 3
    for m, w in zip(res.models, want):
        assert np.array_equal(m.threshold, w["thresholds"]) and m.median_index == w["median_index"]
        assert np.array_equal(m.n_high, w["obs"]["n_high"]) and np.array_equal(m.d_high, w["obs"]["d_high"])
        assert (np.abs(m.U - w["obs"]["U"]) <= REF.REL * w["obs"]["absU"]).all() and (np.abs(m.V - w["obs"]["V"]) <= REF.REL * w["obs"]["absV"]).all()
        tol = REF.chi2_tolerance(w["obs"])
        assert (np.abs(m.chi2 - w["obs"]["chi2"]) <= tol).all()
        assert m.p_adjusted == w["p_adjusted"] and m.median_p_permutation == w["p_median"]
        assert m.p_adjusted >= RS.permutation_p(np.array(m.best_chi2), m.chi2_median_perm)      # a maximum is >= the value at one cut
        assert m.best_chi2 == m.chi2[m.best_index] == m.chi2.max() and m.median_chi2 == m.chi2[m.median_index]
        assert m.median_p_asymptotic == pytest.approx(float(stats.chi2.sf(m.median_chi2, 1)))
    # the draw contract: seed alone gives the permutations of draw_permutations
    a = RS.stratify(risk[1], t, e, R=50, seed=4)
    b = RS.stratify(risk[1], t, e, permutations=RS.draw_permutations(n, 50, 4))
    assert np.array_equal(a.models[0].chi2_max_perm, b.models[0].chi2_max_perm) and a.models[0].p_adjusted == b.models[0].p_adjusted


def test_identity_replicate_is_the_observed_statistic():
    """the p-values' >= relies on it: the identity among the permutations gives the observed chi2_max and median chi2 bit for bit (the
    replicates run in another launch, without the tables, among other problems)"""
    n = 65
    t, e = _labels("ties", n, 4)
    rng = np.random.default_rng(12)
    risk = np.stack([rng.normal(size=n), rng.normal(size=n).round(1)])
    perms = RS.draw_permutations(n, 7, 3)
    perms[4] = np.arange(n)
    res = RS.stratify(risk, t, e, permutations=perms, min_prop=0.1)
    for m in res.models:
        assert m.chi2_max_perm[4].tobytes() == np.float64(m.best_chi2).tobytes()
        assert m.chi2_median_perm[4].tobytes() == np.float64(m.median_chi2).tobytes()
        assert m.p_adjusted >= 2 / 8 and m.median_p_permutation >= 2 / 8             # the identity counts: >=, not >


def test_planted_signal():
    n, R = 120, 200
    rng = np.random.default_rng(5)
    t = rng.exponential(400.0, n)
    e = (rng.random(n) < 0.67).astype(np.int64)
    res = RS.stratify(-t + rng.normal(size=n), t, e, R=R, seed=1)
    m = res.models[0]
    assert m.p_adjusted == 1 / (R + 1) and m.median_p_permutation == 1 / (R + 1)
    assert m.median_hazard_ratio[1] > 1.0                            # the high-risk group dies faster: the interval excludes 1


def _write_predictions(path, seed, n=90):
    import pandas as pd
    rng = np.random.default_rng(seed)
    t = rng.exponential(400.0, n).round(0) + 1
    e = (rng.random(n) < 0.67).astype(int)
    pd.DataFrame({"patient_id": [f"P{i:03d}" for i in range(n)], "survival_time": t, "event": e,
                  "risk_score": -np.log(t) + rng.normal(size=n) * (1.0 + seed)}).to_csv(path, index=False)
    return t, e


def _run(script, args, cwd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "analysis", script)] + args, cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_evaluate_model_stratify(tmp_path):
    import pandas as pd
    _write_predictions(tmp_path / "pred.csv", 0)
    _run("evaluate_model.py", ["--predictions", str(tmp_path / "pred.csv"), "--outdir", str(tmp_path / "with"), "--stratify", "200", "--no-plots"],
         tmp_path)
    s = json.load(open(tmp_path / "with" / "evaluation_summary.json"))
    rs = s["risk_stratification"]
    assert rs["replicates"] == 200 and rs["seed"] == 0 and rs["min_prop"] == 0.1
    assert set(rs["median"]) >= {"threshold", "n_high", "chi2", "p_asymptotic", "p_permutation", "hazard_ratio", "low", "high"}
    assert set(rs["best"]) >= {"threshold", "n_high", "chi2", "p_unadjusted", "p_adjusted", "hazard_ratio", "low", "high"}
    assert set(rs["km"]) == {"Low Risk", "High Risk"}
    assert rs["median"]["chi2"] == pytest.approx(s["logrank"]["chi2"], rel=1e-9)         # the same median split as the old four lines
    assert rs["median"]["n_high"] == s["risk_groups"]["high_risk"]
    assert 1 / 201 <= rs["best"]["p_adjusted"] <= 1
    cs = pd.read_csv(tmp_path / "with" / "cutpoint_scan.csv")
    assert list(cs.columns) == ["threshold", "n_high", "d_high", "U", "V", "chi2", "p_unadjusted", "median_split", "best"]
    assert len(cs) == rs["n_cuts"] and cs["median_split"].sum() == 1 and cs["best"].sum() == 1
    assert cs["chi2"].max() == pytest.approx(rs["best"]["chi2"], rel=1e-12) and (cs["n_high"] >= 9).all() and (cs["n_high"] <= 81).all()
    _run("evaluate_model.py", ["--predictions", str(tmp_path / "pred.csv"), "--outdir", str(tmp_path / "without"), "--no-plots"], tmp_path)
    s0 = json.load(open(tmp_path / "without" / "evaluation_summary.json"))
    assert "risk_stratification" not in s0 and not os.path.exists(tmp_path / "without" / "cutpoint_scan.csv")
    assert {k: v for k, v in s.items() if k != "risk_stratification"} == s0


def test_generate_km_curves_scores_the_best_fold(tmp_path, monkeypatch):
    """--model: the fold with the largest best_c_index of cv_results.json, scored through evaluate_model's --predict path (in process)"""
    import importlib.util
    import pandas as pd
    from multimodal_survival_prediction_amd import data
    from oracle import models as OM
    spec = importlib.util.spec_from_file_location("generate_km_curves", os.path.join(ROOT, "scripts", "analysis", "generate_km_curves.py"))
    gk = importlib.util.module_from_spec(spec); spec.loader.exec_module(gk)
    monkeypatch.setenv("MMS_PATIENTS", "30")
    torch.manual_seed(5)
    os.makedirs(tmp_path / "models" / "rnaseq"); os.makedirs(tmp_path / "results" / "rnaseq")
    torch.save(OM.RNASeqSurvivalModel(input_dim=5005).state_dict(), tmp_path / "models" / "rnaseq" / "fold_2_best.pth")
    json.dump({"fold_results": [{"fold": 1, "best_c_index": 0.61}, {"fold": 2, "best_c_index": 0.7}, {"fold": 3, "best_c_index": 0.7}],
               "hyperparameters": {"n_folds": 3}}, open(tmp_path / "results" / "rnaseq" / "cv_results.json", "w"))
    s = gk.main(["--model", "rnaseq", "--results-dir", str(tmp_path / "results"), "--models-dir", str(tmp_path / "models"),
                 "--outdir", str(tmp_path / "km"), "--stratify", "50", "--no-plots"])
    _, val = data.kfold_indices(30, 3, seed=42)[1]
    m = s["models"]["rnaseq"]
    assert m["source"]["fold"] == 2 and m["patients"] == len(val) == len(pd.read_csv(tmp_path / "km" / "rnaseq_predictions.csv"))
    assert m["km"]["Low Risk"]["patients"] + m["km"]["High Risk"]["patients"] == len(val) and os.path.exists(tmp_path / "km" / "rnaseq_km.csv")


def test_generate_km_curves(tmp_path):
    import pandas as pd
    _write_predictions(tmp_path / "a.csv", 0)
    _write_predictions(tmp_path / "b.csv", 0)
    df = pd.read_csv(tmp_path / "b.csv")
    df["risk_score"] = np.random.default_rng(9).normal(size=len(df))                      # the same patients, a score without signal
    df.to_csv(tmp_path / "b.csv", index=False)
    out = _run("generate_km_curves.py", ["--predictions", f"a={tmp_path / 'a.csv'}", f"b={tmp_path / 'b.csv'}", "--stratify", "200", "--no-plots"],
               tmp_path)
    d = tmp_path / "results" / "km_curves"
    s = json.load(open(d / "km_summary.json"))
    assert list(s["models"]) == ["a", "b"] and s["replicates"] == 200 and "a:" in out and "b:" in out
    assert s["models"]["a"]["best"]["p_adjusted"] < s["models"]["b"]["best"]["p_adjusted"]
    for k in ("a", "b"):
        km = pd.read_csv(d / f"{k}_km.csv")
        assert list(km.columns) == ["group", "time", "survival", "at_risk", "events", "variance", "low", "high"]
        assert set(km["group"]) == {"Low Risk", "High Risk"} and ((km["low"] <= km["survival"]) & (km["survival"] <= km["high"])).all()
        assert s["models"][k]["km"]["Low Risk"]["patients"] + s["models"][k]["km"]["High Risk"]["patients"] == 90
