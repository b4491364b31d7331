"""The numpy reference of the multivariable Cox fit (tests/cox_newton_ref.py) against a textbook table, its two evaluation forms and its
literal-resample form against each other, and the host side of multivariable (design, the nested models, the statistics layer fed with
the reference's outputs) against direct numpy / scipy expressions.  No GPU."""
import numpy as np
import pytest
from scipy import stats

import cox_newton_ref as REF
from multimodal_survival_prediction_amd import multivariable as MV
from multimodal_survival_prediction_amd.bootstrap import bootstrap_weights
from test_cpu_survival_stats import E_6MP, E_PLA, T_6MP, T_PLA


def test_freireich_breslow():
    """Kleinbaum & Klein, Survival Analysis, ch. 3 (model 1, placebo = 1; their package's default ties are Breslow's): coefficient
    1.509, standard error 0.410, -2 ln L = 172.759, hence l = -86.380; the null model's l = -93.985 and LR = 15.21"""
    t, e = np.array(T_6MP + T_PLA, dtype=np.float64), np.array(E_6MP + E_PLA)
    x = np.array([0.0] * 21 + [1.0] * 21)[:, None]
    f = REF.fit(x, t, e)
    assert f["status"] == 1 and f["iters"] <= 6 and f["margin"] >= 10
    assert f["beta"][0] == pytest.approx(1.5092, abs=5e-5) and f["se"][0] == pytest.approx(0.4096, abs=5e-5)
    assert f["loglik"] == pytest.approx(-86.380, abs=5e-4) and f["loglik0"] == pytest.approx(-93.985, abs=5e-4)
    assert 2 * (f["loglik"] - f["loglik0"]) == pytest.approx(15.21, abs=5e-3)
    assert MV.lr_test(f["loglik"], f["loglik0"], 1)["p"] == pytest.approx(stats.chi2.sf(2 * (f["loglik"] - f["loglik0"]), 1))
    fast = REF.fit(x, t, e, evaluate=REF.evaluate_cumsum)
    assert fast["status"] == 1 and fast["iters"] == f["iters"] and abs(fast["beta"][0] - f["beta"][0]) <= 2e-9


@pytest.mark.parametrize("n,p,cols", [(63, 5, [0, 2, 4]), (65, 3, [0, 1, 2]), (40, 2, [1])])
def test_evaluation_forms_and_literal_resample(n, p, cols):
    x, t, e = REF.cohort(n, p, 4)
    w = bootstrap_weights(n, 3, 7)[2]
    beta = np.zeros(p)
    beta[cols] = np.linspace(-0.4, 0.6, len(cols))
    a, b = REF.evaluate(x, t, e, w, beta, cols), REF.evaluate_cumsum(x, t, e, w, beta, cols)
    lit = REF.evaluate(*REF.resampled(x, t, e, w), None, beta, cols)
    for other in (b, lit):
        assert abs(a["l"] - other["l"]) <= REF.REL * a["abs_l"] and a["d"] == other["d"]
        assert (np.abs(a["g"] - other["g"]) <= REF.REL * a["abs_g"]).all() and (np.abs(a["I"] - other["I"]) <= REF.REL * a["abs_I"]).all()
    off = [k for k in range(p) if k not in cols]
    assert (a["g"][off] == 0).all() and (a["I"][off] == 0).all() and (a["I"][:, off] == 0).all()
    # the gradient is the derivative of l, the information that of -g (central differences)
    for k in cols:
        h = np.zeros(p); h[k] = 1e-5
        up, dn = REF.evaluate(x, t, e, w, beta + h, cols), REF.evaluate(x, t, e, w, beta - h, cols)
        assert (up["l"] - dn["l"]) / 2e-5 == pytest.approx(a["g"][k], abs=1e-6 * max(1.0, a["abs_g"][k]))
        assert (-(up["g"] - dn["g"]) / 2e-5)[cols] == pytest.approx(a["I"][k][cols], abs=1e-6 * max(1.0, a["abs_I"].max()))
    fw, fl = REF.fit(x, t, e, w, cols), REF.fit(*REF.resampled(x, t, e, w), None, cols)
    assert fw["status"] == fl["status"] == 1 and fw["iters"] == fl["iters"] and np.abs(fw["beta"] - fl["beta"]).max() <= 2e-9
    assert np.isnan(fw["se"][off]).all() and (fw["beta"][off] == 0).all()
    sub = np.ix_(cols, cols)
    assert fw["se"][cols] == pytest.approx(np.sqrt(np.diag(np.linalg.inv(fw["info"][sub]))), rel=1e-10)
    assert np.linalg.cond(fw["info"][sub]) <= 1e4


def test_reference_statuses():
    x, t, e = REF.cohort(30, 2, 1)
    assert REF.fit(x, t, np.zeros(30))["status"] == 6
    const = x.copy(); const[:, 1] = 0.5
    assert REF.fit(const, t, e)["status"] == 3 and REF.fit(const, t, e, cols=[0])["status"] == 1
    one = np.zeros(30, np.int64); one[int(np.nonzero(e)[0][0])] = 30
    assert REF.fit(x, t, e, one)["status"] == 3                       # one patient 30 times: every column is constant
    sep = dict(x=np.array([[0.0], [1.0]]), time=[2.0, 1.0], event=[1, 1])
    assert REF.fit(**sep, beta_max=0.1)["status"] == 4 and REF.fit(**sep, beta_max=1000.0, max_iter=2)["status"] == 2
    assert REF.fit(**sep, beta_max=0.1)["margin"] >= 10 and REF.fit(**sep, beta_max=1000.0, max_iter=2)["margin"] >= 10


def test_design():
    rng = np.random.default_rng(0)
    age, sex, score = rng.normal(60, 10, 20), rng.integers(0, 2, 20).astype(float), rng.normal(size=20)
    age[3], score[7] = np.nan, np.nan
    d = MV.design(dict(age=age, sex=sex, score=score))
    keep = np.ones(20, bool); keep[[3, 7]] = False
    assert d.n_dropped == 2 and np.array_equal(d.keep, keep) and d.names == ["age", "sex", "score"] and d.X.shape == (18, 3)
    assert np.array_equal(d.X[:, 1], sex[keep]) and d.scale[1] == 1 and d.center[1] == 0           # an indicator is left as it is
    assert d.X[:, 0] == pytest.approx((age[keep] - age[keep].mean()) / age[keep].std(ddof=1)) and d.scale[0] == pytest.approx(age[keep].std(ddof=1))
    assert abs(d.X[:, 2].mean()) <= 1e-12 and d.X[:, 2].std(ddof=1) == pytest.approx(1.0)
    raw = MV.design(dict(age=age, sex=sex), standardize=False)
    assert np.array_equal(raw.X[:, 0], age[~np.isnan(age)]) and raw.n_dropped == 1
    with pytest.raises(ValueError):
        MV.design(dict(age=age, flat=np.full(20, 2.0)))
    with pytest.raises(ValueError):
        MV.design(dict(age=np.where(np.arange(20) == 5, np.inf, age)))
    with pytest.raises(ValueError):
        MV.design({})


def test_nested_models_and_masks():
    m = MV.model_subsets(["age"], ["ct", "rna"])
    assert m == [("base", ("age",)), ("ct", ("ct",)), ("rna", ("rna",)), ("base+ct", ("age", "ct")), ("base+rna", ("age", "rna")),
                 ("base+all", ("age", "ct", "rna"))]
    assert MV.model_subsets(["age"], ["ct"]) == [("base", ("age",)), ("ct", ("ct",)), ("base+ct", ("age", "ct"))]        # base+all merged
    assert MV.model_subsets([], ["ct"]) == [("ct", ("ct",))]
    for bad in ((["age"], []), (["age"], ["age"]), (["a", "a"], ["b"])):
        with pytest.raises(ValueError):
            MV.model_subsets(*bad)
    assert MV.subset_masks([[0], [0, 2, 4], [15]], 16).tolist() == [1, 0b10101, 1 << 15]
    for bad in ([[]], [[0, 0]], [[3]], [[-1]], [[0], [0]]):
        with pytest.raises(ValueError):
            MV.subset_masks(bad, 3)
    order, glast = MV.launch_order([3.0, 5.0, 3.0, 1.0])
    assert order.tolist() == [1, 0, 2, 3] and glast.tolist() == [1, 0, 1, 1]


def _reference_raw(X, t, e, w, models, names, **kw):
    """the launch's outputs, from the reference: rows = the all-ones row, then w's"""
    col = {k: a for a, k in enumerate(names)}
    rows = np.concatenate([np.ones((1, len(t)), np.int64), w.astype(np.int64)])
    fits = [[REF.fit(X, t, e, r, [col[k] for k in m[1]], evaluate=REF.evaluate_cumsum, **kw) for m in models] for r in rows]
    pick = lambda k: np.array([[f[k] for f in row] for row in fits])
    return {k: pick(k) for k in ("beta", "se", "loglik", "loglik0", "iters", "status")}


def test_statistics_layer_on_reference_outputs():
    """analyse_statistics fed with the reference's fits: Wald table, quantiles over the non-degenerate replicates, n_degenerate, the status
    counts and the likelihood-ratio tests are the direct numpy / scipy expressions"""
    n, R, alpha = 40, 60, 0.1
    x, t, e = REF.cohort(n, 3, 11)
    names, base, add = ["age", "ct", "rna"], ["age"], ["ct", "rna"]
    d = MV.design(dict(zip(names, x.T)))
    models = MV.model_subsets(base, add)
    w = bootstrap_weights(n, R, 5)
    w[4] = 0; w[4, int(np.nonzero(e == 0)[0][0])] = 40                 # a replicate without events: status 6 in every model
    raw = _reference_raw(d.X, t, e, w, models, names)
    res = MV.analyse_statistics(raw, d.X, t, e, names, models, base, add, alpha, d.scale)
    ok = (raw["status"][1:] == 1).all(1)
    assert res["n_degenerate"] == int((~ok).sum()) >= 1 and res["replicates"] == R and res["patients"] == n and res["events"] == int(e.sum())
    assert sum(res["status_counts"].values()) == R * len(models) and res["status_counts"][6] >= len(models)
    assert [m["model"] for m in res["models"]] == [m[0] for m in models]
    q = stats.norm.ppf(1 - alpha / 2)
    for s, (label, cols) in enumerate(models):
        m = res["models"][s]
        assert m["loglik"] == raw["loglik"][0, s] and m["status"] == 1 and m["aic"] == 2 * len(cols) - 2 * raw["loglik"][0, s]
        for k in cols:
            a, c = names.index(k), m["coefficients"][k]
            b, se = raw["beta"][0, s, a], raw["se"][0, s, a]
            assert c["beta"] == b and c["se"] == se and c["z"] == pytest.approx(b / se) and c["p"] == pytest.approx(2 * stats.norm.sf(abs(b / se)))
            assert c["hr"] == pytest.approx(np.exp(b)) and c["hr_low"] == pytest.approx(np.exp(b - q * se)) and c["hr_high"] == pytest.approx(np.exp(b + q * se))
            assert c["hr_per_unit"] == pytest.approx(np.exp(b / d.scale[a]))
            boot = raw["beta"][1:, s, a][ok]
            assert c["beta_boot_low"] == np.quantile(boot, alpha / 2) and c["beta_boot_high"] == np.quantile(boot, 1 - alpha / 2)
            assert c["hr_boot_low"] == np.quantile(np.exp(boot), alpha / 2) and c["hr_boot_high"] == np.quantile(np.exp(boot), 1 - alpha / 2)
            assert c["beta_boot_se"] == pytest.approx(boot.std(ddof=1))
        from multimodal_survival_prediction_amd.survival_stats import concordance_index
        assert m["c_index"] == pytest.approx(concordance_index(t, -(d.X @ raw["beta"][0, s]), e))
    ll = {m[1]: raw["loglik"][0, s] for s, m in enumerate(models)}
    for k in add:
        chi2 = 2 * (ll[("age", k)] - ll[("age",)])
        assert res["lr_tests"][k] == dict(chi2=pytest.approx(chi2), df=1, p=pytest.approx(stats.chi2.sf(chi2, 1)))
    chi2 = 2 * (ll[("age", "ct", "rna")] - ll[("age",)])
    assert res["lr_tests"]["all"] == dict(chi2=pytest.approx(chi2), df=2, p=pytest.approx(stats.chi2.sf(chi2, 2)))
    # without a base model the tests are against the null model; without replicates there are no bootstrap entries
    only = MV.model_subsets([], ["ct"])
    raw0 = {k: v[:1, 1:2] for k, v in raw.items()}
    res0 = MV.analyse_statistics(raw0, d.X, t, e, names, only, [], ["ct"])
    assert res0["lr_tests"]["ct"]["chi2"] == pytest.approx(2 * (raw["loglik"][0, 1] - raw["loglik0"][0, 1])) and res0["replicates"] == 0
    assert "beta_boot_low" not in res0["models"][0]["coefficients"]["ct"] and res0["n_degenerate"] == 0
    # all replicates degenerate: NaN intervals
    bad = dict(raw, status=np.where(np.arange(R + 1)[:, None] > 0, 2, raw["status"]))
    resb = MV.analyse_statistics(bad, d.X, t, e, names, models, base, add, alpha)
    assert resb["n_degenerate"] == R and np.isnan(resb["models"][0]["coefficients"]["age"]["beta_boot_low"])
