"""Gradient-boosted Cox trees on the CPU: the numpy replica (tests/gbm_ref.py) against closed forms, the host logic of boosting.py
(hash thresholds, binning, nested_cv's selection and tie rules), the baseline script's files and the comparison tool's row."""
import importlib
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

import gbm_cases as CASES
import gbm_ref as REF
from multimodal_survival_prediction_amd import boosting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    sys.path.insert(0, os.path.join(ROOT, "scripts", "training"))
    try:
        return importlib.import_module(name)
    finally:
        sys.path.pop(0)


# ---- the replica against closed forms --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "one"])
def test_gradient_is_the_derivative_of_the_replicas_log_likelihood(name):
    """d loglik / d F_i = mult_i g_i by a central difference.  With pi = mult e^F / S in (0, 1) the third derivative of log S in F_i is
    pi (1 - pi) (1 - 2 pi), at most 0.0963 in magnitude, so the truncation error is at most step^2 / 6 * 0.0963 * (all weighted events);
    each of the two evaluations carries the rounding bound of the log-likelihood, divided by 2 step."""
    c = CASES.case(name)
    order, gid = REF.positions(c["time"])
    ev, w = c["event"][order], c["mults"][0][order]
    rng = np.random.default_rng(3)
    F = rng.normal(size=c["n"]) * 0.7
    gr = REF.gradient(F, w, ev, gid)
    assert gr["loglik"] == pytest.approx(REF.loglik(F, w, ev, gid), rel=1e-13)
    step = 1e-4
    tol = step * step / 6 * 0.0963 * float((w * ev).sum()) + 2 * REF.bound_loglik(gr, c["n"]) / (2 * step)
    assert tol < 1e-5
    worst = 0.0
    for i in rng.permutation(c["n"])[:25]:
        up, dn = F.copy(), F.copy()
        up[i] += step; dn[i] -= step
        fd = (REF.loglik(up, w, ev, gid) - REF.loglik(dn, w, ev, gid)) / (up[i] - dn[i])
        worst = max(worst, abs(fd - w[i] * gr["g"][i]))
        assert abs(fd - w[i] * gr["g"][i]) <= tol, (i, fd, w[i] * gr["g"][i], tol)
    print("worst finite-difference error %.3e, tolerance %.3e" % (worst, tol))
    assert (gr["h"] >= -1e-15).all() and (gr["g"][w == 0] == 0).all()


def test_one_stump_on_six_patients_by_hand():
    """Six patients, distinct times 6..1, all events, F = 0: S at the k-th longest time is k, Lambda_i = sum_{k >= i} 1 / k, so
    g = 1 - Lambda = (-1.45, -0.45, 0.05, 0.3833.., 0.6333.., 0.8333..) from the longest time down and h = Lambda - sum 1 / k^2.  One gene
    that is 0 for the three longest times and 1 for the others, B = 2: the only cut sends the three longest left, G_L = -1.85 = -G_R."""
    time, ev, w = np.array([6.0, 5, 4, 3, 2, 1]), np.ones(6, np.int64), np.ones(6, np.int64)
    order, gid = REF.positions(time)
    assert list(order) == [0, 1, 2, 3, 4, 5]
    gr = REF.gradient(np.zeros(6), w, ev, gid)
    lam = [sum(Fraction(1, k) for k in range(i + 1, 7)) for i in range(6)]
    q2 = [sum(Fraction(1, k * k) for k in range(i + 1, 7)) for i in range(6)]
    assert np.allclose(gr["g"], [-1.45, -0.45, 0.05, 1 - 37 / 60, 1 - 11 / 30, 1 - 1 / 6], rtol=0, atol=1e-14)
    assert np.allclose(gr["h"], [float(a - b) for a, b in zip(lam, q2)], rtol=0, atol=1e-14)
    assert gr["loglik"] == pytest.approx(-np.log(720.0), rel=1e-14)          # -sum log k
    qg, qh = REF.quantise(gr["g"], gr["h"])
    want_g = [round((1 - a) * 2 ** 32) for a in lam]
    want_h = [round((a - b) * 2 ** 32) for a, b in zip(lam, q2)]
    assert np.abs(qg - np.array(want_g)).max() <= 1 and np.abs(qh - np.array(want_h)).max() <= 1
    xb = np.array([[0, 0, 0, 1, 1, 1]], np.uint8)
    edges = np.array([[0.5]], np.float32)
    t = REF.grow(xb, edges, qg, qh, w, 2, 1, 1, 1.0, 0.0, 0.1, np.ones(1, bool), 3)
    assert t["feat"][0] == 0 and t["bin"][0] == 0 and t["thr"][0] == np.float32(0.5) and list(t["n_node"]) == [6, 3, 3]
    assert abs(int(t["G"][1]) + round(1.85 * 2 ** 32)) <= 3 and t["G"][1] + t["G"][2] == t["G"][0] == qg.sum() and abs(int(t["G"][0])) <= 6
    GL, HL, GR, HR = (float(t[k][s]) / 2 ** 32 for k, s in (("G", 1), ("H", 1), ("G", 2), ("H", 2)))
    G0, H0 = float(t["G"][0]) / 2 ** 32, float(t["H"][0]) / 2 ** 32
    assert t["gain"][0] == GL * GL / (HL + 1.0) + GR * GR / (HR + 1.0) - G0 * G0 / (H0 + 1.0)
    assert t["gain"][0] == pytest.approx(1.85 ** 2 / (float(lam[0] + lam[1] + lam[2] - q2[0] - q2[1] - q2[2]) + 1)
                                         + 1.85 ** 2 / (float(lam[3] + lam[4] + lam[5] - q2[3] - q2[4] - q2[5]) + 1), rel=1e-8)
    assert t["value"][1] == 0.1 * (GL / (HL + 1.0)) and t["value"][2] == 0.1 * (GR / (HR + 1.0)) and t["value"][0] == 0.0
    assert list(t["node"]) == [1, 1, 1, 2, 2, 2] and t["value"][1] < 0 < t["value"][2]      # the short survivors' risk goes up


@pytest.mark.parametrize("name", sorted(CASES.SHAPES))
def test_the_replicas_cases(name):
    """What the cases are for, asserted on the replica: the training log-likelihood does not decrease over the rounds (nu <= 0.1,
    subsample = 1), the problem without events grows single leaves of value 0, the blocking min_leaf grows none, the low colsample admits
    no gene in some round and some gene in another, and NO node needs the near-tie excuse (the committed seed was chosen for that)."""
    c, r = CASES.case(name), CASES.replica_cached(name)
    assert sum(x["excused"] for x in r) == 0
    for q, x in enumerate(r):
        if c["prm"]["subsample"][q] == 1.0 and c["prm"]["learning_rate"][q] <= 0.1:
            assert (np.diff(x["loglik"]) >= 0).all(), (q, x["loglik"])
    assert any((t["feat"] >= 0).any() for x in r for t in x["trees"])
    if c["P"] > 1:
        assert all((t["feat"] < 0).all() and (t["value"] == 0).all() and t["G"][0] == 0 for t in r[1]["trees"]) and (r[1]["F"] == 0).all()
        assert all((t["feat"] < 0).all() for t in r[2]["trees"]) and any(t["value"][0] != 0 for t in r[2]["trees"])
        assert 0 < r[3]["empty_rounds"] < c["rounds"]
    if name == "deep":
        assert max(int(np.nonzero(t["feat"] >= 0)[0].max()) for t in r[0]["trees"]) >= 31      # a split on the deepest level


def test_pair_counts_are_the_concordance_index():
    from multimodal_survival_prediction_amd.survival_stats import concordance_index
    c = CASES.case("tiny")
    order, gid = REF.positions(c["time"])
    F = np.round(np.random.default_rng(0).normal(size=c["n"]), 1)
    mask = c["masks"][0][order]
    c2, cm = REF.pair_counts(F, c["event"][order], gid, mask)
    assert c2 / (2.0 * cm) == pytest.approx(concordance_index(c["time"][order][mask], -F[mask], c["event"][order][mask]), abs=1e-15)


# ---- host logic of the package -------------------------------------------------------------------------------------------------------
def test_hash_thresholds_at_the_ends():
    assert int(boosting.rate_threshold(1.0)) == 0xFFFFFFFF and int(boosting.rate_threshold(0.0)) == 0 and int(boosting.rate_threshold(0.5)) == 2 ** 31
    assert REF.threshold(1.0) == 0xFFFFFFFF and REF.threshold(0.0) == 0
    with pytest.raises(ValueError):
        boosting.rate_threshold(1.5)
    rowid = np.arange(500)
    for pid, m in ((0, 0), (7, 3), (123456, 299)):
        assert REF.rows_in(11, pid, m, rowid, 0xFFFFFFFF).all() and REF.genes_in(11, pid, m, 500, 0xFFFFFFFF).all()
        hm = REF.round_key(11, pid, m)
        zero = np.array([REF.h32(((int(r) + 1) * 0x9E3779B9 + hm) & REF.M32) == 0 for r in rowid])
        assert (REF.rows_in(11, pid, m, rowid, 0) == zero).all() and not REF.genes_in(11, pid, m, 500, 0).any()
        for thr in (0, 2 ** 31, 0x30000000, 0xFFFFFFFF):
            assert (boosting.row_sample(11, pid, m, 500, thr) == REF.rows_in(11, pid, m, rowid, thr)).all()
            assert (boosting.gene_sample(11, pid, m, 500, thr) == REF.genes_in(11, pid, m, 500, thr)).all()
    half = REF.rows_in(11, 5, 2, np.arange(4000), 2 ** 31).mean()
    assert 0.46 < half < 0.54 and (REF.rows_in(11, 5, 2, rowid, 2 ** 31) != REF.rows_in(11, 5, 3, rowid, 2 ** 31)).any()


def test_binning_is_searchsorted_and_cuts_are_raw_thresholds():
    import torch
    c = CASES.case("bins64")
    x = torch.from_numpy(c["X"])
    for B in (4, 32, 64):
        edges = boosting.quantile_edges(x, B)
        xb = boosting.bin_matrix(x, edges).numpy()
        e = edges.numpy()
        assert e.shape == (c["p"], B - 1) and (np.diff(e, axis=1) >= 0).all() and xb.dtype == np.uint8 and xb.max() <= B - 1
        assert (xb == CASES.bins_of(c["X"], e)).all()
        for f in (0, 1, 5):
            for b in range(B - 1):
                assert ((xb[f] <= b) == (c["X"][:, f] <= e[f, b])).all()
        assert len(np.unique(xb[0])) == 1 and len(np.unique(xb[1])) == 2          # the constant gene, the two-valued gene: empty bins
        assert np.allclose(e, CASES.edges_of(c["X"], B), rtol=1e-6, atol=1e-7)


def test_select_rounds_and_its_tie_rules():
    c = np.full((2, 3, 5), 0.5)
    assert boosting.select_rounds(c)[:2] == (0, 1)                              # all equal: the fewest rounds, the first grid point
    c[1, :, 3] = 0.7
    assert boosting.select_rounds(c)[:2] == (1, 4)
    c[0, :, 3] = 0.7
    assert boosting.select_rounds(c)[:2] == (0, 4)                              # same rounds: the earlier grid point
    c[1, :, 1] = 0.7
    assert boosting.select_rounds(c)[:2] == (1, 2)                              # fewer rounds beat the earlier grid point
    c[0, 0, 0], c[0, 1, 0], c[0, 2, 0] = 0.9, 0.6, np.nan                       # the mean is over the scored folds: 0.75
    g, r, mean = boosting.select_rounds(c)
    assert (g, r) == (0, 1) and mean[0, 0] == pytest.approx(0.75) and mean.shape == (2, 5)
    c[:] = np.nan
    assert boosting.select_rounds(c)[:2] == (0, 1)
    assert boosting.default_grid((0.1, 0.3), (1, 2, 3))[4] == dict(learning_rate=0.3, max_depth=2)


def _fake_results(N, folds, G, J, M, p, rng):
    grid = boosting.default_grid((0.1, 0.3), (2,))[:G]
    out = []
    for f, (tr, va) in enumerate(folds):
        inner = rng.uniform(0.4, 0.8, (G, J, M))
        g, r, mean = boosting.select_rounds(inner)
        counts = np.zeros(p, np.int64); counts[[3, 7, 11]] = [2, 5, 1]
        gain = np.zeros(p); gain[[3, 7, 11]] = [0.5, 2.5, 0.1]
        out.append(dict(fold=f, grid_index=g, grid_point=grid[g], grid=grid, rounds=r, c_index=0.6 + 0.01 * f, inner=inner, inner_mean=mean,
                        outer_curve=rng.uniform(0.4, 0.8, (G, M)), val_rows=np.asarray(va), val_F=rng.normal(size=len(va)),
                        train_rows=np.asarray(tr), train_F=rng.normal(size=len(tr)), importance=(counts, gain), n_train=len(tr), n_val=len(va)))
    return out


def test_baseline_script_writes_the_schema(tmp_path):
    import pandas as pd
    gb = _script("gbm_baseline")
    rng = np.random.default_rng(0)
    N, G, J, M, p = 60, 2, 3, 6, 20
    label = np.stack([rng.integers(1, 30, N).astype(np.float64), (rng.random(N) < 0.7).astype(np.float64)], 1)
    perm = rng.permutation(N)
    folds = [(np.sort(np.concatenate([perm[:k * 20], perm[(k + 1) * 20:]])), np.sort(perm[k * 20:(k + 1) * 20])) for k in range(3)]
    res = _fake_results(N, folds, G, J, M, p, rng)
    hz = [5.0, 10.0, 20.0]
    cv = gb.write_outputs(res, label, folds, hz, str(tmp_path / "out"), hyper={"rounds": M}, seconds=1.5)
    assert cv == json.load(open(tmp_path / "out" / "cv_results.json"))
    assert {"model", "n_folds", "num_epochs", "c_index_mean", "c_index_std", "fold_results", "hyperparameters"} <= set(cv)
    assert cv["model"] == "Gradient-boosted Cox trees" and cv["n_folds"] == 3 and cv["num_epochs"] == M and cv["hyperparameters"]["horizons"] == hz
    for k, fr in enumerate(cv["fold_results"], 1):
        r = res[k - 1]
        assert {"fold", "best_c_index", "best_epoch", "train_size", "val_size"} <= set(fr) and fr["best_epoch"] == r["rounds"] and fr["fold"] == k
        df = pd.read_csv(tmp_path / "out" / f"fold_{k}_predictions.csv")
        assert list(df.columns) == ["patient_id", "survival_time", "event", "risk_score"] and len(df) == 20
        assert [int(s.split("-")[1]) for s in df["patient_id"]] == list(folds[k - 1][1]) and np.allclose(df["risk_score"], r["val_F"])
        cu = pd.read_csv(tmp_path / "out" / f"fold_{k}_survival_curves.csv")
        S = cu[[c for c in cu.columns if c.startswith("S_")]].to_numpy()
        assert list(cu.columns) == list(df.columns) + [f"S_{float(h)!r}" for h in hz] and ((S > 0) & (S <= 1)).all() and (np.diff(S, axis=1) <= 0).all()
        im = pd.read_csv(tmp_path / "out" / f"fold_{k}_importance.csv")
        assert list(im.columns) == ["index", "column", "gene", "splits", "gain_sum"] and list(im["index"]) == [7, 3, 11] and list(im["splits"]) == [5, 2, 1]
        cur = pd.read_csv(tmp_path / "out" / f"fold_{k}_curves.csv")
        assert len(cur) == G * M and cur["chosen"].sum() == 1 and list(cur.columns[:4]) == ["grid_index", "learning_rate", "max_depth", "rounds"]
        row = cur[cur["chosen"] == 1].iloc[0]
        assert (row["grid_index"], row["rounds"]) == (r["grid_index"], r["rounds"]) and row["inner_mean"] == pytest.approx(cur["inner_mean"].max())
        assert np.allclose(cur[[f"inner_{j + 1}" for j in range(J)]].mean(1), cur["inner_mean"])


def test_final_comparison_row_and_unchanged_output_without_it(tmp_path, capsys):
    fc = _script("final_comparison")
    assert fc.RESULTS_FILES["Gradient-boosted Cox trees"] == "results/gbm_baseline/cv_results.json" and "Gradient-boosted Cox trees" in fc.NESTED
    assert fc.NESTED[:2] == ("Cox elastic net", "Random survival forest") and "(+) nested cross-validation" in fc.NESTED_NOTE

    def put(rel, vals):
        os.makedirs(tmp_path / os.path.dirname(rel), exist_ok=True)
        json.dump({"fold_results": [{"best_c_index": v, "val_size": 10} for v in vals], "c_index_mean": float(np.mean(vals)),
                   "c_index_std": float(np.std(vals))}, open(tmp_path / rel, "w"))
    put("results/cox_baseline/cv_results.json", [0.6, 0.62, 0.61])
    put("results/rnaseq_only/cv_results.json", [0.7, 0.66, 0.71])
    fc.main(str(tmp_path))
    before = capsys.readouterr().out
    assert "  " + fc.NESTED_NOTE + "\n" in before and "boosted" not in before
    put("results/gbm_baseline/cv_results.json", [0.64, 0.63, 0.66])
    fc.main(str(tmp_path))
    after = capsys.readouterr().out
    assert "Gradient-boosted Cox trees (+)" in after and fc.NESTED_NOTE + fc.GBM_CLAUSE in after and "Cox elastic net (+)" in after
