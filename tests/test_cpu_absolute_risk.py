"""absolute_risk's host side and the reference the GPU tests lean on (no GPU; the launch itself is tests/test_gpu_absolute_risk.py):
the Breslow baseline against a hand-computed example, the reference (tests/td_metrics_ref.py) against the uncensored closed forms and
against literal resampling, the horizon / integral rules, the calibration table, the statistics layer on hand-made raw outputs, and the
host input preparation -- checked by walking the prepared tables the way the kernel does, in plain Python."""
import math

import numpy as np
import pytest
from scipy import stats

import td_metrics_ref as REF
from multimodal_survival_prediction_amd import absolute_risk as AR
from multimodal_survival_prediction_amd.bootstrap import bootstrap_weights


def _tied_cohort(seed, n, M=2, H=5):
    """heavy ties: integer times 1..11, 60 % events, risks rounded to one decimal; horizons before the first time, on tied times, past the last"""
    rng = np.random.default_rng(seed)
    t, e = rng.integers(1, 12, n).astype(float), (rng.random(n) < 0.6).astype(int)
    risk = rng.normal(size=(M, n)).round(1)
    tau = np.array([0.5, 3.0, 6.5, 9.0, 11.0, 12.0])[:H] if H <= 6 else np.linspace(0.5, 12.0, H)
    surv = rng.random((M, n, len(tau)))
    return t, e, risk, surv, tau


# ---- Breslow ------------------------------------------------------------------------------------------------------------------------
T6, E6 = np.array([2.0, 3.0, 3.0, 5.0, 6.0, 8.0]), np.array([1, 1, 1, 0, 1, 0])
ETA6 = np.log(np.array([1.0, 2.0, 1.0, 2.0, 1.0, 1.0]))


def test_breslow_by_hand():
    """e^eta = 1 2 1 2 1 1.  t = 2: one event, risk set everybody, 8 -> 1/8.  t = 3: TWO events (a tie), risk set 2 + 1 + 2 + 1 + 1 = 7
    -> 2/7.  t = 6: one event, risk set 1 + 1 -> 1/2.  The censorings at 5 and 8 add no step."""
    b = AR.breslow_baseline(ETA6, T6, E6)
    assert b.time.tolist() == [2.0, 3.0, 6.0]
    want = np.array([1 / 8, 1 / 8 + 2 / 7, 1 / 8 + 2 / 7 + 1 / 2])
    assert b.H0 == pytest.approx(want, rel=1e-14)
    assert b.cumulative_hazard([1.9, 2.0, 2.5, 3.0, 5.9, 6.0, 100.0]) == pytest.approx([0, want[0], want[0], want[1], want[1], want[2], want[2]], rel=1e-14)
    s = b.survival(np.log([2.0, 1.0]), [3.0, 7.0])
    assert s.shape == (2, 2)
    assert s == pytest.approx(np.exp(-np.outer([2.0, 1.0], [want[1], want[2]])), rel=1e-14)


def test_breslow_survival_is_monotone_and_shift_invariant():
    rng = np.random.default_rng(0)
    n = 50
    t, e, eta = rng.exponential(300, n).round(-1) + 10, rng.random(n) < 0.6, rng.normal(size=n)
    b = AR.breslow_baseline(eta, t, e)
    grid = np.linspace(1, t.max() + 50, 40)
    s = b.survival(eta, grid)
    assert s.shape == (n, 40) and (np.diff(s, axis=1) <= 0).all() and (s <= 1).all() and (s >= 0).all()
    assert (np.diff(s[np.argsort(eta)], axis=0) <= 0).all()                    # a higher risk never survives better
    assert (np.diff(b.H0) > 0).all()
    # a constant added to eta in the fit set AND in the prediction changes nothing (the baseline absorbs it)
    for c in (3.5, -700.0, 700.0):
        b2 = AR.breslow_baseline(eta + c, t, e)
        assert b2.survival(eta + c, grid) == pytest.approx(s, rel=1e-9, abs=1e-300)
    assert AR.breslow_baseline(eta, t, np.zeros(n)).survival(eta, grid).min() == 1.0        # no event: no hazard
    with pytest.raises(ValueError):
        AR.breslow_baseline(eta, t[:-1], e)


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def test_reference_without_censoring():
    """no censoring: G = 1, BS(tau) is the plain mean of ([t > tau] - S)^2 and the AUC is the Mann-Whitney statistic of cases against controls"""
    t, _, risk, surv, tau = _tied_cohort(1, 30)
    e = np.ones(30, int)
    for fn in (REF.metrics, REF.metrics_vec):
        m = fn(t, e, risk, surv, tau)
        assert (m["G"] == 1.0).all()
        auc, _, _ = REF.derived(m)
        for h, x in enumerate(tau):
            alive = (t > x).astype(float)
            assert m["brier"][:, h] == pytest.approx(((alive[None, :] - surv[:, :, h]) ** 2).mean(1), rel=1e-13)
            assert m["km"][h] == pytest.approx(alive.mean(), rel=1e-13)
            n1, n0 = int((t <= x).sum()), int((t > x).sum())
            if n1 == 0 or n0 == 0:
                assert np.isnan(auc[:, h]).all()
                continue
            for k in range(len(risk)):
                ranks = stats.rankdata(np.concatenate([risk[k][t <= x], risk[k][t > x]]))
                u = ranks[:n1].sum() - n1 * (n1 + 1) / 2                       # the cases' Mann-Whitney U: midranks count a tie 1/2
                assert auc[k, h] == pytest.approx(u / (n1 * n0), rel=1e-13)
    assert np.isnan(auc[:, 0]).all() and np.isnan(auc[:, -1]).all()            # a horizon without a case, one without a control


def test_reference_loop_and_array_forms_agree():
    t, e, risk, surv, tau = _tied_cohort(2, 40)
    w = bootstrap_weights(40, 3, 5)
    for row in [None] + list(w):
        a, b = REF.metrics(t, e, risk, surv, tau, row), REF.metrics_vec(t, e, risk, surv, tau, row)
        for k in ("G", "km", "wctrl", "nfac"):
            assert np.array_equal(a[k], b[k]), k
        for k in ("wcase", "brier", "auc_num"):
            assert np.abs(a[k] - b[k]).max() <= 1e-13 * max(1.0, np.abs(a[k]).max()), k


def test_weighted_equals_resampled():
    """multiplicities w on the original arrays = unit weights on the literally resampled arrays"""
    n = 40
    t, e, risk, surv, tau = _tied_cohort(3, n)
    rows = list(bootstrap_weights(n, 6, 11))
    lone = np.zeros(n, np.int8); lone[7] = n                                   # one patient drawn n times
    early = np.where(t <= 8, 2, 0).astype(np.int8)                             # nobody from the latest times
    for w in rows + [lone, early]:
        a = REF.metrics(t, e, risk, surv, tau, w)
        b = REF.metrics(*REF.resampled(t, e, risk, surv, w), tau)
        assert a["W"] == b["W"] and np.array_equal(a["wctrl"], b["wctrl"])
        for k in ("G", "km", "wcase", "brier", "auc_num"):
            assert np.abs(a[k] - b[k]).max() <= 1e-12 * max(1.0, np.abs(b[k]).max()), k
        assert np.isfinite(a["wcase"]).all() and np.isfinite(a["brier"]).all()


def test_reference_edge_horizons():
    t, e, risk, surv, tau = _tied_cohort(4, 25)
    m = REF.metrics(t, e, risk, surv, tau)
    assert m["wcase"][0] == 0 and m["wctrl"][0] == 25 and m["G"][0] == 1.0 and m["km"][0] == 1.0
    assert m["brier"][:, 0] == pytest.approx(((1 - surv[:, :, 0]) ** 2).mean(1), rel=1e-14)          # before the first time: sum w (1 - S)^2 / sum w
    assert m["wctrl"][-1] == 0 and (m["auc_num"][:, -1] == 0).all()
    none = REF.metrics(t, np.zeros(25, int), risk, surv, tau)                                     # all censored: no case anywhere
    assert (none["wcase"] == 0).all() and (none["km"] == 1.0).all() and (none["auc_num"] == 0).all()


# ---- rules --------------------------------------------------------------------------------------------------------------------------
def test_default_and_explicit_horizons():
    rng = np.random.default_rng(5)
    t, e = rng.exponential(400, 80), rng.random(80) < 0.6
    h = AR.default_horizons(t, e)
    lo, hi = np.quantile(t[e], [0.1, 0.9])
    assert len(h) == 16 and h[0] == lo and h[-1] == pytest.approx(hi, rel=1e-15) and np.diff(h) == pytest.approx((hi - lo) / 15, rel=1e-9)
    assert len(AR.default_horizons(t, e, H=1)) == 1 and len(AR.default_horizons(t, e, H=64)) == 64
    with pytest.raises(ValueError):
        AR.default_horizons(t, np.zeros(80))
    for bad in ([], [1.0, 1.0], [2.0, 1.0], [0.0, 1.0], [-1.0], [1.0, float("nan")], [1.0, float("inf")]):
        with pytest.raises(ValueError):
            AR.check_horizons(bad)
    assert AR.check_horizons([1, 2.5]).tolist() == [1.0, 2.5]


def test_trapezoid_rules():
    x = np.array([1.0, 2.0, 4.0])
    y = np.array([[0.2, 0.4, 0.1], [0.5, float("nan"), 0.5]])
    got = AR._trapezoid_mean(y, x)
    assert got[0] == pytest.approx((0.3 * 1 + 0.25 * 2) / 3, rel=1e-15) and np.isnan(got[1])
    assert got[0] == pytest.approx(REF.trapezoid_mean(y, x)[0], rel=1e-15)
    assert AR._trapezoid_mean(y[:, :1], x[:1]).tolist() == [0.2, 0.5]           # H = 1: the value itself


def test_calibration_table():
    rng = np.random.default_rng(6)
    n = 53
    t, e = rng.exponential(300, n), rng.random(n) < 0.7
    s = rng.random(n)
    rows = AR.calibration_table(s, t, e, 200.0, groups=5)
    assert [r["group"] for r in rows] == [1, 2, 3, 4, 5] and [r["patients"] for r in rows] == [11, 11, 11, 10, 10]
    pred = [r["predicted"] for r in rows]
    assert pred == sorted(pred) and sum(r["patients"] * r["predicted"] for r in rows) == pytest.approx((1 - s).sum(), rel=1e-12)
    from multimodal_survival_prediction_amd import survival_stats as SS
    idx = np.argsort(1 - s, kind="stable")[:11]
    times, surv, _, _ = SS.kaplan_meier(t[idx], e[idx])
    assert rows[0]["observed"] == pytest.approx(1 - surv[np.searchsorted(times, 200.0, side="right") - 1], rel=1e-12)
    assert all(0 <= r["low"] <= r["observed"] <= r["high"] <= 1 for r in rows)
    with pytest.raises(ValueError):
        AR.calibration_table(s, t, e, 200.0, groups=0)


def _raw(brier, auc_num, wcase, wctrl, G, km, wsum):
    return dict(brier=np.array(brier, float), auc_num=np.array(auc_num, float), wcase=np.array(wcase, float), wctrl=np.array(wctrl, float),
                G=np.array(G, float), km=np.array(km, float), wsum=np.array(wsum, float))


def test_statistics_layer_by_hand():
    """M = 2, H = 2, rows: the point estimate, three replicates, and one replicate without a control at the second horizon"""
    tau = [1.0, 3.0]
    raw = _raw(brier=[[[0.20, 0.30], [0.10, 0.20]], [[0.22, 0.30], [0.12, 0.18]], [[0.18, 0.34], [0.10, 0.26]], [[0.20, 0.26], [0.06, 0.22]],
                      [[0.90, 0.90], [0.90, 0.90]]],
               auc_num=[[[6.0, 8.0], [3.0, 4.0]], [[6.0, 6.0], [3.0, 6.0]], [[4.0, 8.0], [4.0, 4.0]], [[8.0, 8.0], [2.0, 2.0]], [[1.0, 0.0], [1.0, 0.0]]],
               wcase=[[2.0, 4.0]] * 5, wctrl=[[4.0, 2.0]] * 4 + [[4.0, 0.0]], G=[[1.0, 0.5]] * 5, km=[[0.8, 0.5]] * 5, wsum=[10.0] * 5)
    r = AR.prediction_error_statistics(raw, tau, alpha=0.5, seed=3)
    assert r.n_degenerate == 1 and r.replicates == 4 and r.seed == 3 and r.alpha == 0.5
    assert r.brier.value.tolist() == [[0.20, 0.30], [0.10, 0.20]] and r.auc.value.tolist() == [[0.75, 1.0], [0.375, 0.5]]
    assert r.ibs.value == pytest.approx([0.25, 0.15], rel=1e-15) and r.iauc.value == pytest.approx([0.875, 0.4375], rel=1e-15)
    null = np.array([(2 * 0.64 + 4 * 0.04 / 1.0) / 10, (4 * 0.25 + 2 * 0.25 / 0.5) / 10])
    assert r.brier_null.value == pytest.approx(null, rel=1e-15)
    assert r.ipa.value == pytest.approx(1 - np.array([[0.20, 0.30], [0.10, 0.20]]) / null, rel=1e-15)
    assert np.isnan(r.auc.boot[:, 1, 3]).all() and np.isnan(r.iauc.boot[:, 3]).all()              # the degenerate replicate
    ibs = np.array([[0.26, 0.26, 0.23], [0.15, 0.18, 0.14]])                                      # of the three that count
    assert r.ibs.boot[:, :3] == pytest.approx(ibs, rel=1e-15)
    assert r.ibs.low == pytest.approx(np.quantile(ibs, 0.25, axis=1), rel=1e-15) and r.ibs.high == pytest.approx(np.quantile(ibs, 0.75, axis=1), rel=1e-15)
    assert r.ibs.se == pytest.approx(ibs.std(axis=1, ddof=1), rel=1e-15)
    assert r.brier.high[1, 1] == pytest.approx(np.quantile([0.18, 0.26, 0.22], 0.75), rel=1e-15)   # 0.90 of the degenerate row is left out
    d = ibs[0] - ibs[1]
    assert r.ibs_diff.delta[0, 1] == pytest.approx(0.10, rel=1e-14) and r.ibs_diff.low[0, 1] == pytest.approx(np.quantile(d, 0.25), rel=1e-14)
    assert r.ibs_diff.p_value[0, 1] == min(1.0, 2 * min((0 + 1) / 4, (3 + 1) / 4)) and r.ibs_diff.p_value[1, 0] == 0.5
    assert r.ibs_diff.p_value[0, 0] == 1.0                                                       # d = 0 counts on both sides
    iauc = np.array([[(0.75 + 0.75) / 2, (0.5 + 1.0) / 2, (1.0 + 1.0) / 2], [(0.375 + 0.75) / 2, (0.5 + 0.5) / 2, (0.25 + 0.25) / 2]])
    assert r.iauc.boot[:, :3] == pytest.approx(iauc, rel=1e-15) and r.iauc_diff.delta[0, 1] == pytest.approx(0.4375, rel=1e-15)
    # every replicate degenerate: NaN intervals, the point estimates stay
    raw["wctrl"][1:] = [4.0, 0.0]
    r = AR.prediction_error_statistics(raw, tau)
    assert r.n_degenerate == 4 and np.isnan(r.ibs.low).all() and np.isnan(r.iauc_diff.p_value).all() and r.ibs.value == pytest.approx([0.25, 0.15])
    # H = 1: the integrals are the values
    one = {k: (v[..., :1] if v.ndim > 1 else v) for k, v in raw.items()}
    r1 = AR.prediction_error_statistics(one, tau[:1])
    assert r1.ibs.value.tolist() == r1.brier.value[:, 0].tolist() and r1.iauc.value.tolist() == [0.75, 0.375] and r1.n_degenerate == 0


# ---- host input preparation ---------------------------------------------------------------------------------------------------------
def _walk(trank, event, hcut, rord, surv, w):
    """The kernel's formulation in plain Python on the PREPARED tables (time-ascending positions, risk orders with tie flags): one
    pass in time order with running integer sums for the product limits, one pass in risk order per (model, horizon) that commits
    case_group * (below + group_controls / 2) at the end of each group of equal risks."""
    n, H, M = len(trank), len(hcut), len(rord)
    W = int(w.sum())
    g, km, before, run, d = 1.0, 1.0, 0, 0, 0
    gminus, G, KM = np.zeros(n), np.ones(H), np.ones(H)
    for i in range(n):
        gminus[i] = g
        run += int(w[i]); d += int(w[i]) if event[i] else 0
        if i == n - 1 or trank[i + 1] != trank[i]:
            sa, nu, sb = W - before, W - before - d, W - run
            if sa > 0:
                km *= float(nu) / float(sa)
            if nu > 0:
                g *= float(sb) / float(nu)
            G[hcut == i + 1], KM[hcut == i + 1] = g, km
            before, d = run, 0
    cw = np.array([float(w[i]) / gminus[i] if event[i] and w[i] else 0.0 for i in range(n)])
    out = dict(G=G, km=KM, wcase=np.array([cw[:c].sum() for c in hcut]), wctrl=np.array([float(w[c:].sum()) for c in hcut]),
               brier=np.zeros((M, H)), auc_num=np.zeros((M, H)))
    for m in range(M):
        for h in range(H):
            bc = bk = num = gcase = 0.0
            below = gctrl = 0
            for q in rord[m]:
                p, S = q >> 1, surv[m, q >> 1, h]
                cc, wk = (cw[p], 0) if p < hcut[h] else (0.0, int(w[p]))
                bc += cc * S * S; bk += wk * (1 - S) ** 2; gcase += cc; gctrl += wk
                if q & 1:
                    num += gcase * (below + 0.5 * gctrl); below += gctrl; gcase, gctrl = 0.0, 0
            out["brier"][m, h] = (bc + (bk / G[h] if below > 0 else 0.0)) / W
            out["auc_num"][m, h] = num
    return out


def test_metric_inputs():
    n = 41
    t, e, risk, surv, tau = _tied_cohort(7, n, M=3, H=6)
    order, trank, es, hcut, rord = AR.metric_inputs(risk, t, e, tau)
    assert sorted(order.tolist()) == list(range(n))
    ts = t[order]
    assert (np.diff(ts) >= 0).all() and np.array_equal(es, e[order])
    same = np.diff(ts) == 0
    assert not (same & (np.diff(es) > 0)).any()                                # events before censorings inside a time group
    assert trank[0] == 0 and np.array_equal(np.diff(trank), (~same).astype(int))
    assert hcut.tolist() == [int((t <= x).sum()) for x in tau] and hcut[0] == 0 and hcut[-1] == n
    for m in range(3):
        pos, flag = rord[m] >> 1, rord[m] & 1
        assert sorted(pos.tolist()) == list(range(n))
        r = risk[m][order][pos]
        assert (np.diff(r) >= 0).all() and flag[-1] == 1 and np.array_equal(flag[:-1], (np.diff(r) != 0).astype(int))
    assert trank.dtype == np.int32 and hcut.dtype == np.int32 and rord.dtype == np.int32 and es.dtype == np.int32


def test_prepared_tables_walked_like_the_kernel_give_the_reference():
    n = 41
    t, e, risk, surv, tau = _tied_cohort(8, n, M=3, H=6)
    order, trank, es, hcut, rord = AR.metric_inputs(risk, t, e, tau)
    lone = np.zeros(n, np.int8); lone[3] = n
    for w in [np.ones(n, np.int8)] + list(bootstrap_weights(n, 4, 2)) + [lone, np.where(t <= 7, 1, 0).astype(np.int8)]:
        got = _walk(trank, es, hcut, rord, surv[:, order, :], w[order])
        ref = REF.metrics(t, e, risk, surv, tau, w)
        assert np.array_equal(got["wctrl"], ref["wctrl"])
        assert got["G"].tobytes() == ref["G"].tobytes() and got["km"].tobytes() == ref["km"].tobytes()       # the same factors in the same order
        for k in ("wcase", "brier", "auc_num"):
            assert (np.abs(got[k] - ref[k]) <= REF.REL * ref["abs_" + k]).all(), k
