"""The shared host layer of the evaluation modules (risk_sets.py; replicate rows and their summaries in bootstrap.py) on hand-sized
inputs: no GPU, no launch."""
import ast
import os

import numpy as np
import pytest

from multimodal_survival_prediction_amd import bootstrap as B
from multimodal_survival_prediction_amd import gene_select as GS
from multimodal_survival_prediction_amd import risk_sets as RK
from multimodal_survival_prediction_amd import risk_strata as RS

PKG = os.path.dirname(os.path.abspath(RK.__file__))
EVALUATION_MODULES = ("bootstrap", "gene_select", "risk_strata", "absolute_risk", "multivariable", "coxnet")

LABELS = {                                      # name -> (time, event)
    "empty": ([], []),
    "one": ([2.0], [1]),
    "all-equal": ([3.0, 3.0, 3.0, 3.0], [1, 0, 1, 1]),
    "ties-at-both-ends": ([5.0, 5.0, 3.0, 1.0, 1.0], [1, 0, 1, 1, 0]),
    "unsorted": ([1.0, 5.0, 3.0, 5.0, 1.0, 2.0], [0, 1, 0, 1, 1, 1]),
}


def _brute(t, e):
    """per patient: #{j: t_j >= t_i}, #{j: t_j = t_i, e_j}, and sum over the distinct times u <= t_i of d_u / n_u"""
    t, e = np.asarray(t, dtype=np.float64), np.asarray(e) != 0
    n_at = np.array([np.count_nonzero(t >= u) for u in t], dtype=np.float64)
    d_at = np.array([np.count_nonzero(e & (t == u)) for u in t], dtype=np.float64)
    b = np.array([sum(np.count_nonzero(e & (t == u)) / np.count_nonzero(t >= u) for u in np.unique(t) if u <= ti) for ti in t], dtype=np.float64)
    return n_at, d_at, b


@pytest.mark.parametrize("name", list(LABELS))
def test_descending_groups(name):
    t = np.asarray(LABELS[name][0], dtype=np.float64)
    order, first, gid, last, glast = RK.descending_groups(t)
    n = len(t)
    assert order.tolist() == sorted(range(n), key=lambda i: -t[i])                          # (sorted is stable)
    ts = t[order]
    assert first.tolist() == [i == 0 or ts[i] != ts[i - 1] for i in range(n)]
    assert glast.tolist() == [i == n - 1 or ts[i] != ts[i + 1] for i in range(n)]
    assert last.tolist() == [i for i in range(n) if glast[i]] and len(last) == len(np.unique(t))
    assert gid.tolist() == [int(np.count_nonzero(np.unique(t) > v)) for v in ts]
    assert first.dtype == glast.dtype == bool and len(first) == len(gid) == len(glast) == n


@pytest.mark.parametrize("name", list(LABELS))
def test_risk_set_table_against_brute_force_counts(name):
    t, e = (np.asarray(v, dtype=np.float64) for v in LABELS[name])
    T = RK.risk_set_table(t, e)
    n_at, d_at, b = _brute(t, e)
    assert np.array_equal(T.e, e[T.order]) and T.e.dtype == np.float64
    assert np.array_equal(T.n_u[T.gid], n_at[T.order]) and np.array_equal(T.d_u[T.gid], d_at[T.order])
    assert np.array_equal(T.h_u, T.d_u / T.n_u) and T.b == pytest.approx(b[T.order], rel=1e-15, abs=0)      # (<= 4 terms, summed in another order)
    assert T.last.tolist() == [int(v) - 1 for v in T.n_u]                                    # a group ends where its risk set ends


def test_risk_set_table_rows_with_repeats():
    t, e = np.array([5.0, 5.0, 3.0, 1.0, 1.0]), np.array([1, 0, 1, 1, 0])
    rows = np.array([4, 2, 2, 0, 3, 2, 1])                                                   # patient 2 three times: a tie group of its own
    T = RK.risk_set_table(t, e, rows)
    n_at, d_at, b = _brute(t[rows], e[rows])
    assert rows[T.order].tolist() == [0, 1, 2, 2, 2, 4, 3]                                   # stable: equal times keep the order of `rows`
    assert np.array_equal(T.n_u[T.gid], n_at[T.order]) and np.array_equal(T.d_u[T.gid], d_at[T.order])
    assert T.b == pytest.approx(b[T.order], rel=1e-15, abs=0)
    empty = RK.risk_set_table(t, e, [])
    assert all(len(v) == 0 for v in empty)


@pytest.mark.parametrize("name", list(LABELS))
def test_both_analyses_share_one_table(name):
    t, e = LABELS[name]
    lo, la, h, c, pflag = RS.logrank_coefficients(t, e)
    so, sa, sb, sq = GS.score_coefficients(t, e)
    assert np.array_equal(lo, so) and la.tobytes() == sa.tobytes()                           # bit for bit
    T = RK.risk_set_table(t, e)
    assert np.array_equal(h[T.last], T.h_u) and np.count_nonzero(h) == np.count_nonzero(T.h_u) and sb.tobytes() == T.b.tobytes()
    assert pflag.dtype == np.int32 and len(pflag) == len(c) == len(sq) == len(t)


def test_score_chi2_is_both_modules_statistic():
    assert GS.score_statistic is RK.score_chi2 and RS.chi2_of is RK.score_chi2
    assert RK.score_chi2([3.0, 2.0, 1.0], [2.0, 0.0, -1.0]).tolist() == [4.5, 0.0, 0.0]


def test_run_flags_and_to_numpy():
    first, last = RK.run_flags([1, 1, 2, 3, 3, 3])
    assert first.tolist() == [True, False, True, True, False, False] and last.tolist() == [False, True, True, False, False, True]
    assert [len(v) for v in RK.run_flags([])] == [0, 0] and [v.tolist() for v in RK.run_flags([7])] == [[True], [True]]
    import torch
    x = torch.tensor([0.5, float("nan")], dtype=torch.bfloat16)
    assert RK.to_numpy(x).dtype == np.float32 and np.isnan(RK.to_numpy(x)[1])                # unnamed: nothing is checked
    with pytest.raises(ValueError, match="risk contains NaN"):
        RK.to_numpy(x, "risk")
    risk, t, e = RK.risk_matrix(np.float32([0.1, 0.2]), [1, 2], [0, 1])
    assert risk.shape == (1, 2) and risk.dtype == np.float32 and t.shape == e.shape == (2,)
    for bad in ((np.zeros((2, 3)), [1, 2], [0, 1]), (np.zeros(2), [1, 2], [0]), (np.zeros(0), [], []), (np.zeros((2, 2, 2)), [1, 2], [0, 1])):
        with pytest.raises(ValueError):
            RK.risk_matrix(*bad)


# ---- bootstrap.py: the replicate rows and their summaries ---------------------------------------------------------------------------
@pytest.mark.parametrize("strata", [None, [0, 1, 0, 1, 1, 0, 1]])
def test_replicate_rows(strata):
    n, R, seed = 7, 3, 11
    w = B.replicate_rows(n, R, seed, strata)
    assert w.dtype == np.int8 and w.shape == (1 + R, n) and (w[0] == 1).all()
    assert np.array_equal(w[1:], B.bootstrap_weights(n, R, seed, strata))
    one = B.replicate_rows(n, 0, seed, strata)
    assert one.shape == (1, n) and one.dtype == np.int8 and (one == 1).all()
    own = B.replicate_rows(n, R, seed, strata, weights=np.arange(14.0).reshape(2, 7))           # integral floats are multiplicities
    assert own.dtype == np.int8 and own[1:].tolist() == np.arange(14).reshape(2, 7).tolist() and (own[0] == 1).all()
    assert B.replicate_rows(n, R, seed, strata, weights=np.zeros((0, n))).shape == (1, n)


@pytest.mark.parametrize("bad", [-1, 128, 1.5, "width", "1-D"])
def test_replicate_rows_reject_bad_weights(bad):
    w = np.ones((2, 7))
    if bad == "width":
        w = np.ones((2, 6))
    elif bad == "1-D":
        w = np.ones(7)
    else:
        w[1, 3] = bad
    with pytest.raises(ValueError):
        B.replicate_rows(7, 2, 0, weights=w)
    with pytest.raises(ValueError):
        B.multiplicity_rows(w, 7)


def _direct(rows, alpha):
    """the statistics of [K, R'] replicate values by direct numpy calls, row by row (the se of <= 5 values: sums of <= 5 terms in
    whatever order agree to a few units of float64's last place, hence the caller's 1e-15)"""
    lo = [np.quantile(r, alpha / 2) if len(r) else np.nan for r in rows]
    hi = [np.quantile(r, 1 - alpha / 2) if len(r) else np.nan for r in rows]
    se = [np.std(r, ddof=1) if len(r) > 1 else np.nan for r in rows]
    return np.array(lo), np.array(hi), np.array(se)


@pytest.mark.parametrize("Rp", [0, 1, 5])
def test_estimate_and_paired_against_direct_quantiles(Rp):
    rng = np.random.default_rng(Rp)
    M, R, alpha = 2, 6, 0.2
    all_ = rng.normal(size=(M, 1 + R))
    ok = np.zeros(R, bool)
    ok[rng.permutation(R)[:Rp]] = True
    est = B.estimate(all_, ok, alpha)
    lo, hi, se = _direct(all_[:, 1:][:, ok], alpha)
    assert np.array_equal(est.value, all_[:, 0]) and np.array_equal(est.boot, all_[:, 1:])
    assert np.array_equal(est.low, lo, equal_nan=True) and np.array_equal(est.high, hi, equal_nan=True)
    assert est.se == pytest.approx(se, rel=1e-15, abs=0, nan_ok=True) and np.isnan(est.se).all() == (Rp < 2) and np.isnan(est.low).all() == (Rp < 1)
    pr = B.paired(est, ok, alpha)
    assert np.array_equal(pr.delta, all_[:, :1] - all_[None, :, 0])
    d = all_[0, 1:][ok] - all_[1, 1:][ok]
    if Rp == 0:
        assert all(np.isnan(v).all() for v in (pr.low, pr.high, pr.p_value))
    else:
        assert pr.low[0, 1] == np.quantile(d, alpha / 2) and pr.high[0, 1] == np.quantile(d, 1 - alpha / 2)
        assert pr.low[1, 0] == np.quantile(-d, alpha / 2) and pr.p_value[0, 0] == 1.0
        want = min(1.0, 2.0 * min((np.count_nonzero(d <= 0) + 1) / (Rp + 1), (np.count_nonzero(d >= 0) + 1) / (Rp + 1)))
        assert pr.p_value[0, 1] == pr.p_value[1, 0] == want
    cube = B.estimate(np.stack([all_, 2.0 * all_]), ok, alpha)                               # leading axes are carried along
    assert cube.low.shape == (2, M) and np.array_equal(cube.low[0], est.low, equal_nan=True)


def test_bootstrap_statistics_is_estimate_and_paired():
    # M = 2, R = 5, replicate 3 degenerate (no comparable pair)
    counts = np.array([[12, 14, 20, 0, 8, 16], [10, 14, 30, 0, 4, 10], [10, 10, 20, 0, 8, 10]], dtype=np.int64)
    r = B.bootstrap_statistics(counts, alpha=0.2)
    with np.errstate(divide="ignore", invalid="ignore"):
        c_all = np.where(counts[2] > 0, counts[:2] / (2.0 * counts[2]), np.nan)
    ok = counts[2, 1:] > 0
    est = B.estimate(c_all, ok, 0.2)
    pr = B.paired(est, ok, 0.2)
    assert r.n_degenerate == 1 and r.replicates == 5
    for got, want in ((r.c, est.value), (r.c_boot, est.boot), (r.ci_low, est.low), (r.ci_high, est.high), (r.se, est.se), (r.delta, pr.delta),
                      (r.delta_ci_low, pr.low), (r.delta_ci_high, pr.high), (r.p_value, pr.p_value)):
        assert got.tobytes() == want.tobytes()
    assert not np.isnan(r.se).any() and not np.isnan(r.p_value).any()


def test_no_evaluation_module_imports_a_siblings_private_name():
    for mod in EVALUATION_MODULES + ("risk_sets",):
        with open(os.path.join(PKG, mod + ".py")) as f:
            tree = ast.parse(f.read())
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level == 1 and node.module:
                private = [a.name for a in node.names if a.name.startswith("_")]
                assert not private, "%s.py imports %s from .%s" % (mod, private, node.module)
