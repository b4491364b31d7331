"""CPU: the bilinear identity behind mms_cindex_boot (pair counts on literally resampled arrays == w'Sw / w'Pw), the draw contract of
bootstrap_indices / bootstrap_weights, and the statistics layer (percentile CI, p-value, degenerate replicates) on hand-made counts."""
import numpy as np
import pytest

import cindex_boot_ref as REF
from multimodal_survival_prediction_amd import bootstrap as B
from multimodal_survival_prediction_amd import survival_stats as SS


@pytest.mark.parametrize("n", [2, 37, 130])
@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("n_strata", [0, 3])
def test_literal_counts_equal_weighted_counts(n, rule, n_strata):
    c = REF.make_cohort(n, 2, seed=100 + n, n_strata=min(n_strata, n))
    R = 6
    idx = B.bootstrap_indices(n, R, seed=n, strata=c["strata"])
    w = B.bootstrap_weights(n, R, seed=n, strata=c["strata"])
    assert np.array_equal(w, np.stack([np.bincount(r, minlength=n) for r in idx]))
    lit = REF.literal_counts(c["risk"], c["time"], c["event"], idx, c["strata"], rule)
    wtd = REF.weighted_counts(c["risk"], c["time"], c["event"], w, c["strata"], rule)
    assert lit.dtype == np.int64 and np.array_equal(lit, wtd)
    assert np.array_equal(wtd, REF.weighted_counts(c["risk"], c["time"], c["event"], w, c["strata"], rule, float_matmul=True))
    if n > 2:
        assert lit[-1].max() > 0                      # the case is not vacuous
    # ranks replace the values without changing a count
    assert np.array_equal(wtd, REF.weighted_counts(B.dense_ranks(c["risk"]), B.dense_ranks(c["time"]), c["event"], w, c["strata"], rule))


@pytest.mark.parametrize("n", [37, 130])
def test_lifelines_rule_with_unit_weights_is_concordance_index(n):
    c = REF.make_cohort(n, 1, seed=n)
    k = REF.weighted_counts(c["risk"], c["time"], c["event"], np.ones((1, n), np.int8), None, 1)
    assert k[0, 0] / (2.0 * k[1, 0]) == pytest.approx(SS.concordance_index(c["time"], -c["risk"][0], c["event"]), abs=1e-15)
    k0 = REF.weighted_counts(c["risk"], c["time"], c["event"], np.ones((1, n), np.int8), None, 0)
    assert k0[1, 0] < k[1, 0]                         # tied times with mixed events exist: the two rules differ here


def test_draw_contract():
    n, R = 50, 7
    strata = np.array([2, 0, 1] * 16 + [2, 2])
    a, b = B.bootstrap_indices(n, R, 5, strata), B.bootstrap_indices(n, R, 5, strata)
    assert a.dtype == np.int64 and a.shape == (R, n) and np.array_equal(a, b)
    assert not np.array_equal(a, B.bootstrap_indices(n, R, 6, strata))
    # the documented order: replicate by replicate, strata ascending, one rng.integers(0, n_s, n_s) per stratum
    rng = np.random.default_rng(5)
    for r in range(R):
        row = np.concatenate([np.nonzero(strata == s)[0][rng.integers(0, (strata == s).sum(), size=(strata == s).sum())] for s in (0, 1, 2)])
        assert np.array_equal(a[r], row)
    w = B.bootstrap_weights(n, R, 5, strata)
    assert w.dtype == np.int8 and w.shape == (R, n)
    for s in (0, 1, 2):
        assert (w[:, strata == s].sum(1) == (strata == s).sum()).all()
    assert (B.bootstrap_weights(n, R, 5).sum(1) == n).all()
    u = np.random.default_rng(9)
    assert np.array_equal(B.bootstrap_indices(4, 2, 9), np.stack([u.integers(0, 4, size=4), u.integers(0, 4, size=4)]))


def test_multiplicity_above_127_raises(monkeypatch):
    """No seed makes one patient come up 128 times, so the generator is replaced by one whose draws all hit position 0."""
    class Fixed:
        def integers(self, lo, hi, size):
            return np.zeros(size, dtype=np.int64)
    monkeypatch.setattr(np.random, "default_rng", lambda seed: Fixed())
    assert B.bootstrap_weights(127, 1, 0).tolist() == [[127] + [0] * 126]
    with pytest.raises(OverflowError):
        B.bootstrap_weights(128, 1, 0)


def test_dense_ranks_keep_the_callers_ties():
    x = np.array([0.1, 0.1 + 1e-9, 0.1, -3.0], dtype=np.float64)
    assert B.dense_ranks(x).tolist() == [1, 2, 1, 0]
    assert B.dense_ranks(x.astype(np.float32)).tolist() == [1, 1, 1, 0]     # at float32 they ARE ties
    assert B.dense_ranks(np.stack([x, -x])).tolist() == [[1, 2, 1, 0], [1, 0, 1, 2]] and B.dense_ranks(x).dtype == np.int32


def _counts(num, den):
    return np.array(list(num) + [den], dtype=np.int64)


def test_statistics_on_hand_made_counts():
    # 2 models, 5 replicates (column 0 = point estimate); replicate 3 is degenerate
    den = [10, 10, 20, 0, 8, 10]
    a = [12, 14, 20, 0, 8, 16]
    b = [10, 14, 30, 0, 4, 10]
    r = B.bootstrap_statistics(_counts([a, b], den), alpha=0.2)
    ca, cb = np.array([0.7, 0.5, 0.5, 0.8]), np.array([0.7, 0.75, 0.25, 0.5])
    assert r.c.tolist() == [0.6, 0.5] and r.n_degenerate == 1 and r.replicates == 5
    assert np.isnan(r.c_boot[:, 2]).all() and np.array_equal(r.c_boot[:, [0, 1, 3, 4]], np.stack([ca, cb]))
    assert r.ci_low.tolist() == [np.quantile(ca, 0.1), np.quantile(cb, 0.1)] and r.ci_high.tolist() == [np.quantile(ca, 0.9), np.quantile(cb, 0.9)]
    assert r.se.tolist() == [ca.std(ddof=1), cb.std(ddof=1)]
    d = ca - cb                                        # [0, -.25, .25, .3]: 2 values <= 0, 3 values >= 0, R' = 4
    assert r.delta[0, 1] == 0.6 - 0.5 and r.delta[1, 0] == 0.5 - 0.6 and r.delta[0, 0] == 0
    assert r.delta_ci_low[0, 1] == np.quantile(d, 0.1) and r.delta_ci_high[0, 1] == np.quantile(d, 0.9)
    assert r.p_value[0, 1] == min(1.0, 2 * min(3 / 5, 4 / 5)) == 1.0 and r.p_value[0, 0] == 1.0
    # a clear difference: every replicate favours model a -> p = 2 * (0 + 1) / (R' + 1)
    r2 = B.bootstrap_statistics(_counts([[18, 18, 16, 18, 20], [10, 10, 10, 12, 8]], [10] * 5))
    assert r2.p_value[0, 1] == r2.p_value[1, 0] == 2 * 1 / 5 and r2.delta_ci_low[0, 1] > 0 and r2.n_degenerate == 0


def test_statistics_all_degenerate_is_nan_not_an_error():
    r = B.bootstrap_statistics(np.zeros((3, 6), dtype=np.int64))
    assert r.n_degenerate == 5
    for v in (r.c, r.c_boot, r.se, r.ci_low, r.ci_high, r.delta, r.delta_ci_low, r.delta_ci_high, r.p_value):
        assert np.isnan(v).all()
    one = B.bootstrap_statistics(_counts([[4, 0, 2]], [4, 0, 2]))      # a single good replicate: quantiles exist, the spread does not
    assert one.ci_low[0] == one.ci_high[0] == 0.5 and np.isnan(one.se[0]) and one.n_degenerate == 1


def test_argument_errors_come_before_the_gpu():
    with pytest.raises(ValueError):
        B.cindex_bootstrap(np.array([0.1, np.nan]), np.array([1.0, 2.0]), np.array([1, 0]), R=2)
    with pytest.raises(ValueError):
        B.cindex_bootstrap(np.array([0.1, 0.2]), np.array([1.0, 2.0]), np.array([1, 0]), R=2, pair_rule="other")
    with pytest.raises(ValueError):
        B.cindex_bootstrap(np.zeros((2, 3)), np.array([1.0, 2.0]), np.array([1, 0]), R=2)
