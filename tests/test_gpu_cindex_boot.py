"""GPU: mms_cindex_boot (weighted / bootstrap Harrell-C pair counts on the int8 matrix cores) against the numpy bilinear form of
tests/cindex_boot_ref.py.  The counts are integers: every comparison is equality.  Risks, times and weights are asymmetric, so a wrong
operand lane map (rows for columns, a transposed pair matrix) cannot cancel; sizes sit on both sides of the 16-replicate MFMA tile, the
64-patient K step, the 64-column workgroup and the 4-model launch."""
import importlib.util
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

import cindex_boot_ref as REF
from gpu_util import DEV
from multimodal_survival_prediction_amd import bootstrap as B
from multimodal_survival_prediction_amd import survival_stats as SS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from multimodal_survival_prediction_amd import ops as o
    return o


def _dev(a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _gpu(ops, c, w, rule=0, strata=None, order=None):
    """the kernel's counts of cohort c under weights w [R, n] -> int64 numpy [M + 1, R]; order: a permutation applied to every per-patient array"""
    o = np.arange(c["risk"].shape[1]) if order is None else order
    out = ops.cindex_boot(_dev(B.dense_ranks(c["risk"])[:, o]), _dev(B.dense_ranks(c["time"])[o]), _dev(c["event"][o]),
                          _dev(np.asarray(w)[:, o], torch.int8), stratum=None if strata is None else _dev(strata[o]), pair_rule=rule)
    assert out.dtype == torch.int64 and tuple(out.shape) == (c["risk"].shape[0] + 1, len(w))
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 63, 64, 65, 130, 257])
def test_tile_edges(ops, n):
    c = REF.make_cohort(n, 2, seed=n)
    for R in (1, 15, 16, 17, 70):
        w = B.bootstrap_weights(n, R, seed=1000 * n + R)
        for rule in (0, 1):
            want = REF.weighted_counts(c["risk"], c["time"], c["event"], w, None, rule)
            assert np.array_equal(_gpu(ops, c, w, rule), want), (n, R, rule)


@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_model_counts(ops, M):
    c = REF.make_cohort(65, M, seed=M)
    w = B.bootstrap_weights(65, 33, seed=M)
    for rule in (0, 1):
        want = REF.weighted_counts(c["risk"], c["time"], c["event"], w, None, rule)
        assert want[:-1].min() != want[:-1].max()
        assert np.array_equal(_gpu(ops, c, w, rule), want), (M, rule)


def test_arbitrary_weights(ops):
    """Any multiplicities 0..127, whole zero rows included: the kernel is a weighted count, not only a bootstrap."""
    n, R = 130, 21
    c = REF.make_cohort(n, 3, seed=7)
    rng = np.random.default_rng(7)
    w = rng.integers(0, 128, size=(R, n)).astype(np.int8)
    w[rng.random((R, n)) < 0.3] = 0
    w[0, :5] = 127
    w[[3, 20]] = 0
    want = REF.weighted_counts(c["risk"], c["time"], c["event"], w, None, 1)
    got = _gpu(ops, c, w, 1)
    assert np.array_equal(got, want) and (got[:, [3, 20]] == 0).all() and got[-1].max() > 127 * 127


def test_input_order_does_not_matter(ops):
    n = 257
    c = REF.make_cohort(n, 2, seed=11, n_strata=2)
    w = B.bootstrap_weights(n, 40, seed=11, strata=c["strata"])
    by_time = np.argsort(c["time"], kind="stable")
    shuffled = np.random.default_rng(11).permutation(n)
    for rule in (0, 1):
        want = REF.weighted_counts(c["risk"], c["time"], c["event"], w, c["strata"], rule)
        for order in (None, by_time, by_time[::-1].copy(), shuffled):
            assert np.array_equal(_gpu(ops, c, w, rule, c["strata"], order), want)


def test_strata(ops):
    n, R = 130, 24
    c = REF.make_cohort(n, 2, seed=3, n_strata=3)
    s = c["strata"]
    w = B.bootstrap_weights(n, R, seed=3, strata=s)
    for rule in (0, 1):
        want = REF.weighted_counts(c["risk"], c["time"], c["event"], w, s, rule)
        got = _gpu(ops, c, w, rule, s)
        assert np.array_equal(got, want)
        assert not np.array_equal(got, _gpu(ops, c, w, rule))              # the strata do remove pairs
        parts = 0
        for u in range(3):
            m = s == u
            sub = dict(risk=c["risk"][:, m], time=c["time"][m], event=c["event"][m])
            parts = parts + _gpu(ops, sub, w[:, m], rule)
        assert np.array_equal(got, parts)


def test_point_estimates(ops):
    """All-ones weights: rule 0 is ops.cindex_counts, rule 1 is survival_stats.concordance_index."""
    for n in (37, 348):
        c = REF.make_cohort(n, 1, seed=n)
        ones = np.ones((1, n), np.int8)
        k0 = _gpu(ops, c, ones, 0)[:, 0]
        old = ops.cindex_counts(_dev(c["risk"][0], torch.float32), _dev(c["time"], torch.float32), _dev(c["event"], torch.float32)).cpu().tolist()
        assert k0.tolist() == [2 * old[0] + old[1], old[2]] and old[2] > 0
        k1 = _gpu(ops, c, ones, 1)[:, 0]
        assert k1[0] / (2.0 * k1[1]) == SS.concordance_index(c["time"], -c["risk"][0], c["event"]) and k1[1] > k0[1]


def test_all_censored_is_degenerate_not_an_error(ops):
    n, R = 65, 17
    c = REF.make_cohort(n, 2, seed=5)
    c["event"][:] = 0
    assert (_gpu(ops, c, B.bootstrap_weights(n, R, seed=5), 1) == 0).all()
    res = B.cindex_bootstrap(c["risk"], c["time"], c["event"], R=R, seed=5)
    assert res.n_degenerate == R and np.isnan(res.c).all() and np.isnan(res.ci_low).all() and np.isnan(res.p_value).all()


def test_config4_validation_fold(ops):
    """n = 1639 (config 4's validation fold), R = 256, M = 2 against the float64-matmul form (exact: every sum is far below 2^53)."""
    n, R = 1639, 256
    c = REF.make_cohort(n, 2, seed=4, n_times=400, n_risks=300)
    w = B.bootstrap_weights(n, R, seed=4)
    want = REF.weighted_counts(c["risk"], c["time"], c["event"], w, None, 1, float_matmul=True)
    assert np.array_equal(_gpu(ops, c, w, 1), want)
    assert np.array_equal(_gpu(ops, c, w, 1, order=np.argsort(c["time"], kind="stable")), want)


def test_cindex_bootstrap_end_to_end():
    n, R, alpha = 130, 100, 0.1
    c = REF.make_cohort(n, 3, seed=21, n_strata=2)
    res = B.cindex_bootstrap(torch.from_numpy(c["risk"]), c["time"], c["event"], R=R, seed=8, strata=c["strata"], alpha=alpha)
    w = np.concatenate([np.ones((1, n), np.int8), B.bootstrap_weights(n, R, 8, c["strata"])])
    k = REF.weighted_counts(c["risk"], c["time"], c["event"], w, c["strata"], 1)
    assert np.array_equal(res.counts, k) and res.n_degenerate == 0
    cb = k[:3].astype(np.float64) / (2.0 * k[3].astype(np.float64))
    assert np.array_equal(res.c, cb[:, 0]) and np.array_equal(res.c_boot, cb[:, 1:])
    boot = cb[:, 1:]
    assert np.abs(res.ci_low - np.quantile(boot, alpha / 2, axis=1)).max() <= 1e-12
    assert np.abs(res.ci_high - np.quantile(boot, 1 - alpha / 2, axis=1)).max() <= 1e-12
    assert np.abs(res.se - boot.std(axis=1, ddof=1)).max() <= 1e-12
    for a in range(3):
        for b in range(3):
            d = boot[a] - boot[b]
            p = min(1.0, 2 * min(((d <= 0).sum() + 1) / (R + 1), ((d >= 0).sum() + 1) / (R + 1)))
            assert abs(res.p_value[a, b] - p) <= 1e-12 and abs(res.delta[a, b] - (cb[a, 0] - cb[b, 0])) <= 1e-12
            assert abs(res.delta_ci_low[a, b] - np.quantile(d, alpha / 2)) <= 1e-12
            assert abs(res.delta_ci_high[a, b] - np.quantile(d, 1 - alpha / 2)) <= 1e-12
    assert (res.ci_low <= res.c).all() and (res.c <= res.ci_high).all()
    again = B.cindex_bootstrap(c["risk"], c["time"], c["event"], R=R, seed=8, strata=c["strata"], alpha=alpha)
    assert np.array_equal(again.counts, res.counts) and np.array_equal(again.c_boot, res.c_boot) and np.array_equal(again.p_value, res.p_value)
    # a single risk vector, caller's weights, float64 / bfloat16 inputs, the strict rule
    one = B.cindex_bootstrap(torch.from_numpy(c["risk"][0]).bfloat16(), c["time"].astype(np.float64), c["event"], weights=w[1:], pair_rule="harrell")
    hb = torch.from_numpy(c["risk"][:1]).bfloat16().float().numpy()
    assert np.array_equal(one.counts, REF.weighted_counts(hb, c["time"], c["event"], w, None, 0))


def _evaluate_model():
    spec = importlib.util.spec_from_file_location("evaluate_model", os.path.join(ROOT, "scripts", "analysis", "evaluate_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_evaluate_model_bootstrap_options(tmp_path):
    n = 90
    rng = np.random.default_rng(2)
    t = np.round(rng.exponential(500, n)) + 1
    base = -np.log(t) + rng.normal(0, 0.8, n)
    folds = {f"risk_fold_{k + 1}": base + rng.normal(0, 0.5, n) for k in range(3)}
    df = pd.DataFrame(dict(patient_id=[f"P{i:03d}" for i in range(n)], survival_time=t, event=(rng.random(n) < 0.6).astype(int),
                           risk_score=np.mean(list(folds.values()), axis=0), **folds))
    csv = str(tmp_path / "pred.csv")
    df.to_csv(csv, index=False)
    ev = _evaluate_model()
    plain = ev.main(["--predictions", csv, "--outdir", str(tmp_path / "plain"), "--no-plots"])
    assert set(plain) == {"test_patients", "deaths", "censored", "c_index", "median_survival_time", "median_risk_score", "risk_groups", "logrank",
                          "group_statistics"}
    other = df[["patient_id", "survival_time", "event"]].assign(risk_score=rng.normal(0, 1, n)).sample(frac=1, random_state=0)
    ocsv = str(tmp_path / "other.csv")
    other.to_csv(ocsv, index=False)
    s = ev.main(["--predictions", csv, "--outdir", str(tmp_path / "boot"), "--bootstrap", "200", "--seed", "3", "--no-plots", "--compare", ocsv])
    saved = json.load(open(tmp_path / "boot" / "evaluation_summary.json"))
    assert set(saved) == set(plain) | {"c_index_bootstrap"} and saved["c_index"] == plain["c_index"]
    b = saved["c_index_bootstrap"]
    assert set(b) == {"replicates", "seed", "alpha", "low", "high", "se", "n_degenerate", "members", "compare"}
    assert b["replicates"] == 200 and b["seed"] == 3 and b["alpha"] == 0.05 and b["n_degenerate"] == 0 and b["se"] > 0
    assert b["low"] <= saved["c_index"] <= b["high"] and b["low"] < b["high"]
    assert list(b["members"]) == ["risk_fold_1", "risk_fold_2", "risk_fold_3"]
    for k, m in b["members"].items():
        assert m["c_index"] == SS.concordance_index(df["survival_time"], -df[k], df["event"])
        assert abs(m["delta"] - (saved["c_index"] - m["c_index"])) <= 1e-12 and m["low"] <= m["high"] and 0 < m["p_value"] <= 1
    cmp = b["compare"][ocsv]                           # the other file is in another row order: joined on patient_id
    assert cmp["c_index"] == SS.concordance_index(df["survival_time"], -other.set_index("patient_id").loc[df["patient_id"], "risk_score"], df["event"])
    assert cmp["low"] > 0 and cmp["p_value"] < 0.05 and s["c_index_bootstrap"] == b          # noise against a real signal
    other.iloc[1:].to_csv(ocsv, index=False)
    with pytest.raises(ValueError, match="patient sets differ"):
        ev.main(["--predictions", csv, "--outdir", str(tmp_path / "bad"), "--bootstrap", "50", "--no-plots", "--compare", ocsv])
    with pytest.raises(SystemExit):
        ev.main(["--predictions", csv, "--outdir", str(tmp_path / "bad"), "--no-plots", "--compare", ocsv])
