"""risk_strata's host side: the coefficient builder, the cut enumeration, the permutation draw contract, the statistics layer and the
Kaplan-Meier bands (no GPU; the scan itself is tests/test_gpu_risk_strata.py)."""
import math

import numpy as np
import pytest
from scipy import stats

import logrank_scan_ref as REF
from multimodal_survival_prediction_amd import risk_strata as RS
from multimodal_survival_prediction_amd import survival_stats as SS

T_6MP = [6, 6, 6, 6, 7, 9, 10, 10, 11, 13, 16, 17, 19, 20, 22, 23, 25, 32, 32, 34, 35]
E_6MP = [1, 1, 1, 0, 1, 0, 1, 0, 0, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0]
T_PLA = [1, 1, 2, 2, 3, 4, 4, 5, 5, 8, 8, 8, 8, 11, 11, 12, 12, 15, 17, 22, 23]
E_PLA = [1] * 21


def _tied_cohort(seed, n):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 12, n).astype(float), (rng.random(n) < 0.6).astype(int), rng.normal(size=n).round(1)


def test_freireich_arm_as_risk():
    """placebo = the high-risk arm: two distinct risk values, so one cut -- the median split -- and the textbook chi2 16.79"""
    t, e = np.array(T_6MP + T_PLA, float), np.array(E_6MP + E_PLA)
    risk = np.array([0.0] * 21 + [1.0] * 21)
    cs = RS.admissible_cuts(risk, 0.1)
    assert cs.cut.tolist() == [1] and cs.threshold.tolist() == [0.0] and cs.median_index == 0
    order, a, h, c, pflag = RS.logrank_coefficients(t, e)
    U, V = RS.prefix_statistic(cs.rank[order] >= cs.cut[0], a, c)
    assert U * U / V == pytest.approx(16.79, abs=0.01)
    want = SS.logrank_test(T_PLA, T_6MP, E_PLA, E_6MP)[0]
    assert U * U / V == pytest.approx(want, rel=1e-12)
    ref = REF.scan(t, e, cs.rank, cs.cut)
    assert ref["chi2"][0] == pytest.approx(want, rel=1e-12) and ref["n_high"][0] == 21 and ref["d_high"][0] == 21


def test_reference_is_logrank_test_and_prefix_form_agrees():
    """the slow reference IS survival_stats.logrank_test's arithmetic, and the kernel's formulation equals it on heavy ties"""
    for seed in range(20):
        t, e, risk = _tied_cohort(seed, 40 + seed)
        if seed % 2:
            t[seed], e[seed] = 30.0, 1                           # the latest time has one patient and it is an event: n_u = 1
        cs = RS.admissible_cuts(risk, 0.0)
        ref = REF.scan(t, e, cs.rank, cs.cut)
        order, a, h, c, pflag = RS.logrank_coefficients(t, e)
        for k, cut in enumerate(cs.cut):
            hi = cs.rank >= cut
            chi2 = SS.logrank_test(t[hi], t[~hi], e[hi], e[~hi])[0] if hi.any() and (~hi).any() else 0.0
            assert ref["chi2"][k] == pytest.approx(chi2, rel=1e-12, abs=1e-13)
            U, V = RS.prefix_statistic(hi[order], a, c)
            assert abs(U - ref["U"][k]) <= 1e-12 * ref["absU"][k] and abs(V - ref["V"][k]) <= 1e-12 * max(ref["absV"][k], 1e-300)


def test_coefficients_against_their_definition():
    t = np.array([5, 3, 5, 1, 3, 3, 9, 1, 7.0])
    e = np.array([1, 0, 1, 1, 1, 1, 0, 0, 1])
    order, a, h, c, pflag = RS.logrank_coefficients(t, e)
    ts, es = t[order], e[order]
    assert (np.diff(ts) <= 0).all() and sorted(order.tolist()) == list(range(9))
    n = len(t)
    for i in range(n):
        u = ts[i]
        last = i == n - 1 or ts[i + 1] != u
        nu, du = (t >= u).sum(), ((t == u) & (e == 1)).sum()
        want_h = du / nu if last and du > 0 else 0.0
        want_c = du * (nu - du) / (nu * nu * (nu - 1)) if last and du > 0 and nu >= 2 else 0.0
        assert h[i] == pytest.approx(want_h, rel=1e-15) and c[i] == pytest.approx(want_c, rel=1e-15)
        want_a = es[i] - sum(((t == w) & (e == 1)).sum() / (t >= w).sum() for w in np.unique(t) if w <= u)
        assert a[i] == pytest.approx(want_a, abs=1e-14)
        assert pflag[i] == int(es[i]) | (2 if (want_h or want_c) else 0)
        if last:
            assert i + 1 == nu                                   # at a tie group's last position the positions so far are the risk set
    # the earliest position alone at risk (n_u = 1): logrank_test skips n < 2 -- no variance term, and O - E cancels (h = 1 against e = 1)
    o2, a2, h2, c2, f2 = RS.logrank_coefficients([9.0, 4.0, 4.0], [1, 1, 0])
    assert h2.tolist() == [1.0, 0.0, 1 / 3] and c2 == pytest.approx([0.0, 0.0, 1 / 9]) and f2.tolist() == [3, 1, 2]
    assert a2 == pytest.approx([1 - 1 - 1 / 3, 1 - 1 / 3, -1 / 3])
    # no events: nothing anywhere
    o3, a3, h3, c3, f3 = RS.logrank_coefficients([3.0, 2.0, 1.0], [0, 0, 0])
    assert not a3.any() and not h3.any() and not c3.any() and not f3.any()


def test_cut_enumeration():
    rng = np.random.default_rng(3)
    for n, min_prop in ((40, 0.1), (41, 0.25), (17, 0.0), (30, 0.5)):
        risk = rng.normal(size=n).round(1)                       # ties in the risk
        cs = RS.admissible_cuts(risk, min_prop)
        m = math.ceil(min_prop * n - 1e-9)
        assert RS.min_group(n, min_prop) == m
        assert (np.diff(cs.cut) > 0).all() and len(cs.cut) == len(cs.threshold)
        med_high = SS.risk_groups(risk) == "High Risk"
        for k, (cut, thr) in enumerate(zip(cs.cut, cs.threshold)):
            hi = cs.rank >= cut
            assert np.array_equal(hi, risk > thr)                # the > convention; equal risks are never split
            assert thr in risk
            if k != cs.median_index:
                assert hi.sum() >= m and (~hi).sum() >= m
        assert np.array_equal(cs.rank >= cs.cut[cs.median_index], med_high)
        # every admissible split is there: try each distinct value
        want = {v for v in np.unique(risk)[:-1] if (risk > v).sum() >= m and (risk <= v).sum() >= m}
        assert want <= set(cs.threshold.tolist()) and len(cs.threshold) <= len(want) + 1
        thr_ref, im_ref = REF.thresholds(risk, min_prop)
        assert np.array_equal(thr_ref, cs.threshold) and im_ref == cs.median_index
    # 0.1 * 120 is 12, not 13
    assert RS.min_group(120, 0.1) == 12 and RS.min_group(121, 0.1) == 13 and RS.min_group(10, 0.0) == 0
    # more than half of the patients at the largest value: the median split has an empty high group and is still listed
    cs = RS.admissible_cuts([1.0, 2.0, 2.0, 2.0], 0.25)
    assert not (cs.rank >= cs.cut[cs.median_index]).any() and (SS.risk_groups([1.0, 2.0, 2.0, 2.0]) == "Low Risk").all()
    # a constant risk: one cut, everybody low
    cs = RS.admissible_cuts([0.5] * 6, 0.1)
    assert len(cs.cut) == 1 and not (cs.rank >= cs.cut[0]).any()


def test_permutation_draw_contract():
    rng = np.random.default_rng(11)
    want = np.stack([rng.permutation(9) for _ in range(5)])
    assert np.array_equal(RS.draw_permutations(9, 5, 11), want)
    assert np.array_equal(RS.draw_permutations(9, 3, 11), want[:3])          # a prefix: replicates are drawn in order
    assert RS.draw_permutations(9, 0, 0).shape == (0, 9)
    assert not np.array_equal(RS.draw_permutations(9, 5, 12), want)
    with pytest.raises(ValueError):
        RS.draw_permutations(0, 5, 0)


def test_statistics_layer():
    """hand-made chi2 tables: chi2[r][c] of R = 4 replicates and C = 3 cuts of one model"""
    obs = np.array([1.0, 5.0, 5.0])
    rep = np.array([[0.5, 6.0, 0.1], [5.0, 0.2, 0.3], [0.1, 0.2, 0.3], [1.0, 4.9, 5.0]])
    assert RS.first_argmax(obs) == 1 and RS.first_argmax(np.zeros(0)) == -1          # the smallest index wins
    mx = rep.max(1)
    p_adj, p_med = RS.strata_statistics(np.array([obs.max()]), np.array([obs[0]]), mx[None, :], rep[None, :, 0])
    assert p_adj[0] == (1 + 3) / 5                               # 6.0, 5.0 (>= counts equality), 5.0
    assert p_med[0] == (1 + 2) / 5                               # 5.0 and 1.0 (equality again)
    # the observed maximum referred to ANY single cut's replicates cannot beat the adjusted p: a replicate's maximum is >= its value
    # at that cut.  (This includes the best cut's own permutation p -- the number cut-point shopping would report.)
    for c in range(3):
        assert p_adj[0] >= RS.permutation_p(np.array(obs.max()), rep[:, c])
    assert RS.permutation_p(np.array(7.0), rep[:, 0]) == 1 / 5   # never below 1 / (R + 1)
    assert RS.permutation_p(np.array(1.0), np.zeros(0)) == 1.0   # R = 0
    # assemble: table statistics, argmax by the launch's index, hazard ratios
    cs = RS.CutSet(rank=np.zeros(4, np.int32), cut=np.array([1, 2, 3], np.int32), threshold=np.array([0.1, 0.2, 0.3]), median_index=0)
    tab = dict(U=np.array([[1.0, -2.0, 3.0]]), V=np.array([[1.0, 0.8, 0.0]]), n_high=np.array([[3, 2, 1]]), d_high=np.array([[2, 1, 1]]))
    res = RS.assemble([cs], tab, np.array([5.0]), np.array([1]), np.array([1.0]), mx[None, :], rep[None, :, 0], n=4, alpha=0.05)
    m = res.models[0]
    assert m.chi2.tolist() == [1.0, 5.0, 0.0] and m.best_index == 1 and m.best_threshold == 0.2 and m.p_adjusted == 0.8
    assert m.p_unadjusted[1] == pytest.approx(stats.chi2.sf(5.0, 1)) and m.p_unadjusted[2] == 1.0
    z = stats.norm.ppf(0.975)
    assert m.best_hazard_ratio == pytest.approx((math.exp(-2.5), math.exp(-2.5 - z / math.sqrt(0.8)), math.exp(-2.5 + z / math.sqrt(0.8))))
    assert m.median_hazard_ratio[0] == pytest.approx(math.e) and m.median_p_asymptotic == pytest.approx(stats.chi2.sf(1.0, 1))
    assert all(math.isnan(x) for x in RS.peto_hazard_ratio(1.0, 0.0))
    s = res.summary()
    assert s["replicates"] == 4 and s["models"][0]["best"]["p_adjusted"] == 0.8 and s["models"][0]["median"]["n_high"] == 3


def test_generate_km_curves_picks_the_best_fold():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("generate_km_curves", os.path.join(root, "scripts", "analysis", "generate_km_curves.py"))
    gk = importlib.util.module_from_spec(spec); spec.loader.exec_module(gk)
    folds = [{"fold": 1, "best_c_index": 0.61}, {"fold": 2, "best_c_index": 0.7}, {"fold": 3, "best_c_index": 0.7}]
    assert gk.best_fold({"fold_results": folds, "hyperparameters": {"n_folds": 5}}) == (2, 0.7, 5)       # the first of two equal folds
    assert gk.best_fold({"fold_results": folds[:1], "n_folds": 3}) == (1, 0.61, 3) and gk.best_fold({"fold_results": folds})[2] == 3
    with pytest.raises(SystemExit):
        gk.main([])                                              # neither --model nor --predictions


def test_km_bands_hand_computed():
    """times 1, 2 (censored), 3, 4 of four patients: S = 3/4, 3/4, 3/8, 0; Greenwood sums 1/12, 1/12, 1/12 + 1/2"""
    cur = RS.km_curve([1, 2, 3, 4], [1, 0, 1, 1], alpha=0.05, group="g")
    assert cur.time.tolist() == [0, 1, 2, 3, 4] and cur.survival.tolist() == [1.0, 0.75, 0.75, 0.375, 0.0]
    s2 = [0.0, 1 / 12, 1 / 12, 1 / 12 + 1 / 2]
    for k in range(4):
        assert cur.variance[k] == pytest.approx(cur.survival[k] ** 2 * s2[k])
    assert cur.variance[4] == float("inf")
    z = stats.norm.ppf(0.975)
    for k in (1, 2, 3):
        S = cur.survival[k]
        th = z * math.sqrt(s2[k]) / math.log(S)                 # negative
        assert cur.low[k] == pytest.approx(S ** math.exp(-th)) and cur.high[k] == pytest.approx(S ** math.exp(th))
        assert 0 < cur.low[k] < S < cur.high[k] < 1
    assert (cur.low[0], cur.high[0], cur.low[4], cur.high[4]) == (1.0, 1.0, 0.0, 0.0)
    # S = 0.75: log-log band with se(log(-log S)) = sqrt(1/12) / |log 0.75|  ->  [0.1279, 0.9605] (hand-computed)
    assert cur.low[1] == pytest.approx(0.1279, abs=5e-4) and cur.high[1] == pytest.approx(0.9605, abs=5e-4)
    assert cur.median == 3.0 and cur.median_low == 1.0 and cur.median_high == 4.0
    rows = cur.rows()
    assert rows[1]["group"] == "g" and rows[1]["at_risk"] == 4 and rows[1]["events"] == 1
    lo, hi = RS.km_groups([1, 2, 3, 4, 5, 6], [1, 1, 1, 0, 0, 1], [True, True, True, False, False, False])
    assert lo.group == "Low Risk" and hi.group == "High Risk" and hi.median == 2.0 and lo.median == 6.0
    assert len(RS.km_groups([1, 2], [1, 1], [False, False])) == 1
