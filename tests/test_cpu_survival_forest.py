"""The numpy replica of the random survival forest (tests/rsf_ref.py) against independent code, and the host side of
survival_forest.py (hash, bootstrap draws, mortality weights) against the replica.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rsf_ref as REF

from multimodal_survival_prediction_amd import survival_forest as SF
from multimodal_survival_prediction_amd import survival_stats as SS


def cohort(n, p, seed, n_times=None):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, p)).astype(np.float32)
    time = rng.integers(1, n_times + 1, n).astype(np.float64) if n_times else np.round(rng.exponential(10.0, n), 1) + 1.0
    ev = rng.random(n) < 0.65
    order, gid = REF.positions(time)
    return X[order], time[order], ev[order].astype(np.int64), gid


def test_hash_and_draws_match_the_package():
    xs = np.array([0, 1, 2, 0xFFFFFFFF, 0x9E3779B9, 123456789], dtype=np.uint64)
    assert [int(v) for v in SF.hash_u32(xs.copy())] == [REF.h32(int(v)) for v in xs]
    # the mixer is csrc/common.h's (the dropout replica states it independently)
    import dropout_ref as DR
    assert [REF.h32(int(v)) for v in xs] == [DR.hash_u32_int(int(v)) for v in xs]
    for seed, tid, m in ((0, 0, 17), (7, 41, 100), (2 ** 31 + 5, 3000, 1)):
        assert np.array_equal(SF.bootstrap_draws(seed, tid, m), REF.draws(seed, tid, m))
        assert int(SF.tree_key(seed, tid)) == REF.tree_key(seed, tid)


def test_bootstrap_mults():
    folds = [(np.array([0, 2, 4, 6, 8, 9]), np.array([1, 3, 5, 7])), (np.array([1, 3, 5, 7, 9]), np.array([0, 2, 4, 6, 8]))]
    m = SF.bootstrap_mults(folds, 10, 4, seed=3)
    assert m.dtype == np.uint8 and m.shape == (8, 10)
    assert np.array_equal(m, REF.bootstrap_mults([f[0] for f in folds], 10, 4, 3))
    assert (m[:4].sum(1) == 6).all() and (m[4:].sum(1) == 5).all()
    assert (m[:4][:, folds[0][1]] == 0).all() and (m[4:][:, folds[1][1]] == 0).all()          # validation rows are never drawn
    assert not np.array_equal(m[0], m[1])
    assert np.array_equal(SF.bootstrap_mults([f[0] for f in folds], 10, 4, seed=3), m)          # plain training arrays


@pytest.mark.parametrize("seed", range(6))
def test_statistic_equals_logrank_test_on_repeated_patients(seed):
    """random splits of random nodes: U^2 / V == survival_stats.logrank_test with every patient repeated mult times, to 1e-10"""
    rng = np.random.default_rng(100 + seed)
    X, time, ev, gid = cohort(60, 5, seed, n_times=9 if seed % 2 else None)
    mult = rng.integers(0, 4, 60)
    member = (mult > 0) & (rng.random(60) < 0.8)
    c = REF.candidates(X, ev, gid, mult, member, s=seed, tid=seed, seed=1, mtry=4, nsplit=3, min_leaf=1)
    idx = np.nonzero(member)[0]
    seen = 0
    for i in range(12):
        left = X[idx, c["feat"][i]] <= c["thr"][i]
        U, V, nL, dL, K, mag = REF.logrank_uv(mult[idx], ev[idx], gid[idx], left)               # the loop form against the array form
        assert (nL, dL, K) == (c["n_left"][i], c["d_left"][i], c["K"][i])
        assert U == pytest.approx(c["U"][i], rel=1e-12, abs=1e-12) and V == pytest.approx(c["V"][i], rel=1e-12)
        rep = lambda a, m: np.repeat(a[m], mult[m])
        a, b = idx[left], idx[~left]
        chi2, _ = SS.logrank_test(rep(time, a), rep(time, b), rep(ev, a), rep(ev, b))
        assert c["chi2"][i] == pytest.approx(chi2, rel=1e-10, abs=1e-300)
        seen += chi2 > 0
    assert seen >= 3


def test_single_member_at_risk_adds_nothing():
    """Y = 1 at the latest time: logrank_test skips the time, the contract's terms are 0 there"""
    time = np.array([9.0, 5.0, 5.0, 3.0, 2.0]); ev = np.array([1, 1, 0, 1, 1]); gid = np.array([0, 1, 1, 2, 3]); w = np.ones(5, np.int64)
    for left in (np.array([1, 0, 1, 0, 1], bool), np.array([0, 1, 0, 1, 0], bool)):
        U, V, _, _, K, _ = REF.logrank_uv(w, ev, gid, left)
        chi2, _ = SS.logrank_test(time[left], time[~left], ev[left], ev[~left])
        assert K == 4 and U * U / V == pytest.approx(chi2, rel=1e-12)


@pytest.fixture(scope="module")
def grown():
    X, time, ev, gid = cohort(120, 12, 5)
    folds = [np.arange(0, 120, 2), np.arange(1, 120, 2)]
    mults = REF.bootstrap_mults(folds, 120, 3, seed=9)
    masks = np.zeros((2, 120), bool); masks[0, folds[0]] = True; masks[1, folds[1]] = True
    hz = np.quantile(time[ev != 0], [0.25, 0.5, 0.75])
    trees, morts, Hs = REF.forest(X, time, ev, gid, mults, np.arange(6), 9, 4, 5, 4, 4, masks, np.repeat([0, 1], 3), hz)
    return X, time, ev, gid, mults, masks, hz, trees, morts, Hs


def test_heap_leaf_and_count_invariants(grown):
    X, time, ev, gid, mults, masks, hz, trees, morts, Hs = grown
    for t, m in zip(trees, mults):
        assert t["n_node"][0] == m.sum() and t["d_node"][0] == (m * ev).sum()
        split = np.nonzero(t["feat"] >= 0)[0]
        assert len(split) >= 2
        for s in split:
            assert t["n_node"][2 * s + 1] + t["n_node"][2 * s + 2] == t["n_node"][s]
            assert t["d_node"][2 * s + 1] + t["d_node"][2 * s + 2] == t["d_node"][s]
            assert min(t["n_node"][2 * s + 1], t["n_node"][2 * s + 2]) >= 4 and t["stat"][s] > 0
            assert s == 0 or t["feat"][(s - 1) // 2] >= 0
        leaves = [s for s in range(len(t["feat"])) if t["feat"][s] < 0 and t["n_node"][s] > 0]
        assert sum(t["n_node"][s] for s in leaves) == m.sum()
        assert all(t["n_node"][s] >= 4 for s in leaves)                                          # no leaf below min_leaf
        for s in leaves:
            assert m[t["node"] == s].sum() == t["n_node"][s]
        assert set(np.unique(t["node"][m > 0])) == set(leaves) and (t["node"][m == 0] == -1).all()
        assert int(np.log2(max(leaves) + 1)) <= 4                                                # max_depth


def test_leaf_hazard_is_nelson_aalen_of_the_risk_table(grown):
    X, time, ev, gid, mults, masks, hz, trees, morts, Hs = grown
    for i, (t, m) in enumerate(zip(trees, mults)):
        tj = np.unique(time[masks[i // 3] & (ev != 0)])
        for s in np.nonzero((t["feat"] < 0) & (t["n_node"] > 0))[0]:
            mem = t["node"] == s
            tt, ee = np.repeat(time[mem], m[mem]), np.repeat(ev[mem], m[mem])
            times, _, at_risk, deaths = SS.kaplan_meier(tt, ee)
            cum = np.cumsum(deaths[1:] / at_risk[1:])
            H = lambda u: cum[np.searchsorted(times[1:], u, side="right") - 1] if u >= times[1] else 0.0
            assert Hs[i][s] == pytest.approx([H(u) for u in hz], rel=1e-12, abs=1e-300)
            assert morts[i][s] == pytest.approx(sum(H(u) for u in tj), rel=1e-12, abs=1e-300)


def test_mortality_weights_reproduce_the_sum_over_event_times(grown):
    X, time, ev, gid, mults, masks, hz, trees, morts, Hs = grown
    W = SF.mortality_weights(time, ev, masks)
    t, m = trees[4], mults[4]
    for s in np.nonzero((t["feat"] < 0) & (t["n_node"] > 0))[0]:
        us, inc = REF.leaf_hazard(time, ev, m, t["node"] == s)
        pos = [int(np.nonzero(time == u)[0][0]) for u in us]
        assert float((inc * W[1][pos]).sum()) == pytest.approx(morts[4][s], rel=1e-12, abs=1e-300)


def test_prediction_masks(grown):
    X, time, ev, gid, mults, masks, hz, trees, morts, Hs = grown
    mo, H, cnt = REF.predict(trees, morts, Hs, X)
    assert (cnt == 6).all() and np.isfinite(mo).all()
    use = np.zeros((6, 120), bool); use[:3, 1::2] = True                                         # fold 0's trees on fold 0's validation rows
    mo2, H2, cnt2 = REF.predict(trees, morts, Hs, X, use)
    assert np.isnan(mo2[0::2]).all() and (cnt2[1::2] == 3).all() and np.isnan(H2[0]).all()
    # an in-bag training row lands in the leaf the grower left it in
    for t, m in zip(trees, mults):
        for r in np.nonzero(m > 0)[0][:10]:
            assert REF.drop(t, X[r]) == t["node"][r]


def test_a_value_equal_to_the_threshold_goes_left():
    t = dict(feat=np.array([0, -1, -1]), thr=np.array([1.5, 0, 0], np.float32))
    assert REF.drop(t, np.array([1.5], np.float32)) == 1 and REF.drop(t, np.array([np.nextafter(np.float32(1.5), np.float32(2))])) == 2


def test_fit_refuses_bad_arguments_before_touching_the_gpu():
    with pytest.raises(TypeError):
        SF.fit(np.zeros((4, 2), np.float32), np.ones(4), np.ones(4), np.ones((1, 4)))
    with pytest.raises(ValueError):
        SF.bootstrap_mults([np.zeros(0, np.int64)], 4, 1)
    with pytest.raises(ValueError):
        SF.bootstrap_mults([np.zeros(300, np.int64)], 4, 1)                                      # one row drawn 300 times


def test_the_gpu_cases_are_unambiguous_in_the_replica():
    """What test_gpu_survival_forest.py relies on, checked here without a GPU: no node of the whole-tree and cross-validation cases has a
    rival within the rounding bound of its winner, no two mortalities that a C-index compares are close enough to flip, and the planted
    gene has the largest summed chi2 in every fold."""
    import rsf_cases as CASES
    c = CASES.trees_case()
    m = [x for t in c["trees"] for x in t["margins"]]
    assert len(m) >= 60 and all(gap > bnd for gap, bnd in m) and max(bnd for _, bnd in m) < 1e-10
    assert max(int(np.nonzero(t["feat"] >= 0)[0].max()) for t in c["trees"]) >= 15              # splits at the last level
    cv = CASES.cv_case()
    assert all(gap > bnd for mm in cv["margins"] for gap, bnd in mm)
    for fr in cv["folds_ref"]:
        for mo, lv in ((fr["val_mort"], fr["leaves_val"]), (fr["oob_mort"], fr["leaves_oob"])):
            gap, same = CASES.flip_gap(mo, lv)
            assert gap > 1e-9 and same
        assert int(np.argmax(fr["chi2"])) == CASES.PLANTED and 0.0 < fr["c_index"] < 1.0
        assert fr["c_index"] == SS.concordance_index(cv["time"][fr["val_rows"]], -fr["val_mort"], cv["ev"][fr["val_rows"]])
