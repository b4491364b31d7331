"""Gradient-boosted Cox trees on the GPU against the numpy replica (tests/gbm_ref.py), stage by stage on the device's own inputs:
  1. the quantised gradients of every round against the replica's on the F rebuilt from the device's own trees, within 1 + 2^32 bound;
  2. from the device's own qg / qh: the prefixed histograms of every level and every table of every node with ==;
  3. F, the pair counts and predict with ==, the log-likelihood within its bound;
  4. placement independence: alone, first among 24, last among 24, byte-equal; both histogram forms give the same bits;
  5. nested_cv, the entry point and the comparison tool's row.
Shapes (tests/gbm_cases.py): n = 67 and 300 (past one 256-position chunk), p = 5 and 70 (three tiles of 32 genes, the last with 6),
B = 4, 32, 64, D = 1, 2, 3 and one D = 6 case, M = 4 rounds, P = 1 and 24."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gbm_cases as CASES
import gbm_ref as REF
from multimodal_survival_prediction_amd import boosting

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = ("feat", "bin", "thr", "n_node", "G", "H", "gain", "value")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fit_case(c, problems=None, **kw):
    q = np.arange(c["P"]) if problems is None else np.asarray(problems)
    prm = {k: v[q] for k, v in c["prm"].items()}
    return boosting.fit(dev(c["X"]), c["time"], c["event"], c["mults"][q], rounds=c["rounds"], bins=c["B"], seed=c["seed"],
                        eval_masks=c["masks"][q], problem_ids=c["ids"][q], **prm, **kw)


@pytest.mark.parametrize("name", sorted(CASES.SHAPES))
def test_every_stage_against_the_replica(name):
    c = CASES.case(name)
    b = fit_case(c, trace=True)
    n, p, B, P, M, nn = c["n"], c["p"], c["B"], c["P"], c["rounds"], c["nn"]
    edges = b.edges.cpu().numpy()
    order, gid = REF.positions(c["time"])
    assert (b.trace["order"] == order).all() and edges.shape == (p, B - 1)
    xb = CASES.bins_of(c["X"][order], edges)
    ev = c["event"][order]
    tab = {k: b.tables[k].cpu().numpy() for k in TABLES}
    qg_d, qh_d = b.trace["qg"].cpu().numpy(), b.trace["qh"].cpu().numpy()                 # [M, P, n]
    lev = [[{k: v.cpu().numpy() for k, v in lv.items()} for lv in rnd] for rnd in b.trace["levels"]]
    F_dev = b.F.cpu().numpy()[:, order]
    at = [0, 1, M - 1, M]
    pred = b.predict(dev(c["X"]), rounds=at)                                            # [P, K, n] rows of X
    assert tab["feat"].shape == (P, M, nn) and len(lev[0]) == int(c["prm"]["max_depth"].max())
    worst_q = worst_ll = 0.0
    excused = splits = 0
    for q in range(P):
        prm = {k: c["prm"][k][q] for k in c["prm"]}
        mult, mask, pid = c["mults"][q][order], c["masks"][q][order], int(c["ids"][q])
        F = np.zeros(n)
        after = [F.copy()]
        for m in range(M):
            # 1. the gradient on the F rebuilt from the device's own trees
            gr = REF.gradient(F, mult, ev, gid)
            qg, qh = REF.quantise(gr["g"], gr["h"])
            bg, bh = REF.bound_q(gr, n)
            rg, rh = np.abs(qg_d[m, q] - qg) / (1.0 + REF.QSCALE * bg), np.abs(qh_d[m, q] - qh) / (1.0 + REF.QSCALE * bh)
            worst_q = max(worst_q, rg.max(), rh.max())
            assert rg.max() <= 1.0 and rh.max() <= 1.0, (q, m, rg.max(), rh.max())
            assert (qg_d[m, q][mult == 0] == 0).all() and (qh_d[m, q] >= 0).all()
            bl = REF.bound_loglik(gr, n)
            worst_ll = max(worst_ll, abs(b.curve["loglik"][q, m] - gr["loglik"]) / bl)
            assert abs(b.curve["loglik"][q, m] - gr["loglik"]) <= bl, (q, m)
            # 2. the tree from the device's own quantised gradients: everything with ==
            wt = np.where(REF.rows_in(c["seed"], pid, m, order, REF.threshold(prm["subsample"])), mult, 0)
            adm = REF.genes_in(c["seed"], pid, m, p, REF.threshold(prm["colsample"]))
            t = REF.grow(xb, edges, qg_d[m, q], qh_d[m, q], wt, B, int(prm["max_depth"]), int(prm["min_leaf"]), float(prm["l2"]),
                         float(prm["min_gain"]), float(prm["learning_rate"]), adm, nn)
            excused += len(t["excused"]); splits += int((t["feat"] >= 0).sum())
            for level in range(len(lev[m])):
                for k in ("n", "G", "H"):
                    want = t["levels"][level][k] if level < len(t["levels"]) else 0
                    assert (lev[m][level][k][q] == want).all(), (q, m, level, k)
            for k in TABLES:
                assert (tab[k][q, m] == t[k]).all(), (q, m, k, tab[k][q, m], t[k])
            # 3. F and the pair counts
            F = F + t["value"][t["node"]]
            after.append(F.copy())
            c2, cm = REF.pair_counts(F, ev, gid, mask)
            assert (b.curve["conc2"][q, m], b.curve["comparable"][q, m]) == (c2, cm), (q, m)
        gr = REF.gradient(F, mult, ev, gid)
        assert abs(b.curve["loglik"][q, M] - gr["loglik"]) <= REF.bound_loglik(gr, n)
        assert (F_dev[q] == F).all()
        for k, a in enumerate(at):
            assert (pred[q, k][order] == after[a]).all(), (q, a)
    assert (b.predict(dev(c["X"])) == b.F.cpu().numpy()).all() and (pred[:, 0] == 0).all()
    print("%s: worst |dq| / (1 + 2^32 bound) %.3f, worst log-likelihood error / bound %.3f, %d splits, %d excused" % (name, worst_q, worst_ll, splits, excused))
    assert excused == 0 and splits > 0
    cnt, gain = b.importance()
    assert cnt.sum() == (tab["feat"] >= 0).sum() and gain.sum() == pytest.approx(tab["gain"][tab["feat"] >= 0].sum())


def test_placement_independence_and_histogram_forms():
    """problem 7 of the wide case (depth 3, subsample 0.7, colsample 0.5) alone, first among 24 and last among 24: byte-equal tables and
    F; and the private-histogram form gives the bits of the members form for all 24"""
    c = CASES.case("wide")
    q = 7
    assert c["prm"]["max_depth"][q] == 3 and c["prm"]["subsample"][q] < 1 and c["prm"]["colsample"][q] < 1
    others = [i for i in range(c["P"]) if i != q]
    alone, first, last = fit_case(c, [q]), fit_case(c, [q] + others), fit_case(c, others + [q])
    for k in TABLES:
        assert alone.tables[k].cpu().numpy()[0].tobytes() == first.tables[k].cpu().numpy()[0].tobytes() == last.tables[k].cpu().numpy()[-1].tobytes(), k
    assert alone.F.cpu().numpy()[0].tobytes() == first.F.cpu().numpy()[0].tobytes() == last.F.cpu().numpy()[-1].tobytes()
    assert alone.curve["conc2"][0].tobytes() == first.curve["conc2"][0].tobytes() == last.curve["conc2"][-1].tobytes()
    assert alone.curve["loglik"][0].tobytes() == first.curve["loglik"][0].tobytes() == last.curve["loglik"][-1].tobytes()
    assert (alone.tables["feat"] >= 0).sum() > 4
    members, private, default = fit_case(c, form=1), fit_case(c, form=2), fit_case(c)
    for k in TABLES:
        assert members.tables[k].cpu().numpy().tobytes() == private.tables[k].cpu().numpy().tobytes() == default.tables[k].cpu().numpy().tobytes(), k
    assert members.F.cpu().numpy().tobytes() == private.F.cpu().numpy().tobytes()


def test_save_load_and_host_checks(tmp_path):
    c = CASES.case("tiny")
    b = fit_case(c)
    b.save(str(tmp_path / "b.npz"))
    z = boosting.load(str(tmp_path / "b"))
    x = dev(c["X"])
    assert (z.predict(x, rounds=[1, 4]) == b.predict(x, rounds=[1, 4])).all() and z.hyper["max_depth"][0] == 1 and int(z.hyper["bins"]) == 4
    assert (z.curve["loglik"] == b.curve["loglik"]).all()
    with pytest.raises(ValueError):
        b.predict(x, rounds=[3, 1])
    with pytest.raises(ValueError):
        b.predict(x[:, :1].contiguous())
    with pytest.raises(ValueError):
        boosting.fit(x, c["time"], c["event"], c["mults"], rounds=2, max_depth=7)
    with pytest.raises(ValueError):
        boosting.fit(x, c["time"], c["event"], c["mults"] + 300, rounds=2)
    empty = boosting.fit(x, c["time"], c["event"], np.zeros((0, c["n"]), np.int64), rounds=2)
    assert empty.n_problems == 0 and empty.predict(x).shape == (0, c["n"])


def test_nested_cv_reads_per_fold_gene_matrices():
    """MMS_SELECT_GENES leaves one matrix per fold in the cohort: every outer fold's problems are their own fit on that fold's genes and
    keep their ids, so fold f equals fold f of a run over that matrix alone -- bytes, choice and all"""
    from multimodal_survival_prediction_amd import data
    N, p = 90, 30
    X, t, e = CASES.make_data(N, p, 21)
    folds = data.kfold_indices(N, 3, seed=42)
    cols = [np.sort(np.random.default_rng(f).permutation(p)[:12]) for f in range(3)]
    base = dict(label=torch.from_numpy(np.stack([t, e.astype(np.float64)], 1)), has_survival=torch.ones(N, dtype=torch.bool), n=N)
    kw = dict(inner=3, rounds=6, grid=boosting.default_grid((0.1, 0.3), (1, 2)), seed=5, min_leaf=5, subsample=0.8, bins=16)
    got = boosting.nested_cv(dict(base, rnaseq=dev(X), rnaseq_folds=[dev(X[:, k]) for k in cols]), folds, **kw)
    for f in range(3):
        one = boosting.nested_cv(dict(base, rnaseq=dev(X[:, cols[f]])), folds, **kw)[f]
        assert got[f]["val_F"].tobytes() == one["val_F"].tobytes() and got[f]["inner"].tobytes() == one["inner"].tobytes()
        assert (got[f]["grid_index"], got[f]["rounds"], got[f]["c_index"]) == (one["grid_index"], one["rounds"], one["c_index"])
        assert len(got[f]["importance"][0]) == 12 and got[f]["importance"][0].sum() > 0 and got[f]["inner"].shape == (4, 3, 6)


def test_nested_cv_entry_point_and_comparison_row(tmp_path):
    import pandas as pd
    from multimodal_survival_prediction_amd import data
    env = dict(os.environ, MMS_PATIENTS="120", MMS_FOLDS="3", MMS_GBM_ROUNDS="12", MMS_GBM_INNER="3", MMS_GBM_LR="0.1,0.3", MMS_GBM_DEPTH="1,2",
               PYTHONPATH=ROOT)
    for k in ("MMS_SELECT_GENES", "MMS_GBM_MIN_LEAF", "MMS_GBM_L2", "MMS_GBM_SUBSAMPLE", "MMS_GBM_COLSAMPLE", "MMS_GBM_BINS", "MMS_GBM_SEED"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "training", "gbm_baseline.py")], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "results" / "gbm_baseline"
    cv = json.load(open(out / "cv_results.json"))
    assert cv["model"] == "Gradient-boosted Cox trees" and cv["n_folds"] == 3 and cv["num_epochs"] == 12 and len(cv["fold_results"]) == 3
    hp = cv["hyperparameters"]
    assert (hp["rounds"], hp["learning_rate"], hp["max_depth"], hp["min_leaf"], hp["bins"], hp["inner_folds"]) == (12, [0.1, 0.3], [1, 2], 10, 32, 3)
    folds = data.kfold_indices(120, 3, seed=42)
    from multimodal_survival_prediction_amd.survival_stats import concordance_index
    for k, fr in enumerate(cv["fold_results"], 1):
        assert fr["train_size"] + fr["val_size"] == 120 and 0.0 <= fr["best_c_index"] <= 1.0 and 1 <= fr["best_epoch"] <= 12
        df = pd.read_csv(out / f"fold_{k}_predictions.csv")
        assert list(df.columns) == ["patient_id", "survival_time", "event", "risk_score"] and len(df) == fr["val_size"]
        assert sorted(int(s.split("-")[1]) for s in df["patient_id"]) == sorted(int(i) for i in folds[k - 1][1])
        assert concordance_index(df["survival_time"], -df["risk_score"], df["event"]) == pytest.approx(fr["best_c_index"], abs=1e-12)
        cu = pd.read_csv(out / f"fold_{k}_survival_curves.csv")
        S = cu[[c for c in cu.columns if c.startswith("S_")]].to_numpy()
        assert S.shape[1] == len(hp["horizons"]) and ((S > 0) & (S <= 1)).all() and (np.diff(S, axis=1) <= 0).all()
        im = pd.read_csv(out / f"fold_{k}_importance.csv")
        assert list(im.columns) == ["index", "column", "gene", "splits", "gain_sum"] and len(im) == fr["genes_split_on"]
        # the chosen round count is that of the recorded inner curves: best mean, then the fewest rounds, then the earliest grid point
        cur = pd.read_csv(out / f"fold_{k}_curves.csv")
        assert len(cur) == 4 * 12 and np.allclose(cur[["inner_1", "inner_2", "inner_3"]].mean(1), cur["inner_mean"], rtol=1e-12)
        best = cur[cur["inner_mean"] == cur["inner_mean"].max()].sort_values(["rounds", "grid_index"]).iloc[0]
        assert (int(best["grid_index"]), int(best["rounds"])) == (fr["grid_index"], fr["best_epoch"]) and int(best["chosen"]) == 1 and cur["chosen"].sum() == 1
        assert cur["outer"].between(0, 1).all()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "training", "final_comparison.py")], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Gradient-boosted Cox trees (+)" in r.stdout and "(+) nested cross-validation" in r.stdout, r.stdout + r.stderr
