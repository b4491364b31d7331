"""Random survival forest on the MI355X (csrc/rsf.hip, ops.rsf_*, survival_forest.py, scripts/training/rsf_baseline.py) against the numpy
replica (tests/rsf_ref.py; cases and their references: tests/rsf_cases.py):
  1. the candidate tables of level 0;  2. whole trees, node by node from the GPU's own membership;  3. a tree's bytes do not depend on
  what shares its launches;  4. leaves and masked prediction;  5. cross_validate;  6. the entry point and the comparison tools.

U and V are compared within rsf_ref.bound_uv, which states its derivation (the replica forms the textbook terms, the kernel the fused
ones: a few unit roundoffs per term of the sum's magnitude); counts are compared with ==.
Shapes are the kernel's edges, not the workload: n = 67 (one partial scan chunk) and 300 (past one chunk of 256 positions), C = 5 and
300 (past one chunk of 256 lanes), members not a multiple of the walk's unroll of 4."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rsf_cases as CASES
import rsf_ref as REF
from gpu_util import DEV
from multimodal_survival_prediction_amd import survival_forest as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(forest):
    return {k: getattr(forest, k).cpu().numpy() for k in ("feat", "thr", "stat", "n_node", "d_node", "mort", "H", "node")}


def close(got, ref, rel):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.array_equal(np.isnan(got), np.isnan(ref)) and bool((np.abs(got - ref)[~np.isnan(ref)] <= rel * np.abs(ref)[~np.isnan(ref)]).all())


# ---- 1. candidate tables, level 0 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,mtry,nsplit", [("base", 67, 1, 5), ("base", 67, 30, 10), ("lonely", 67, 30, 10), ("noevent", 67, 1, 5),
                                                 ("constant", 67, 1, 5), ("base", 300, 30, 10)])
def test_level0_candidate_tables(kind, n, mtry, nsplit):
    X, t, e, mults = CASES.level0_case(kind, n)
    ids = [0, 5, 11]
    forest, cand = SF.fit(dev(X), t, e, mults, mtry=mtry, nsplit=nsplit, min_leaf=5, max_depth=3, seed=9, tree_ids=ids, candidates_level=0)
    cand, tab = {k: v.cpu().numpy() for k, v in cand.items()}, host(forest)
    Xp, tp, ep, gid, mp, order = CASES.in_positions(X, t, e, mults)
    if kind == "lonely":
        assert (tp[0] > tp[1]) and ep[0] == 1                                         # Y = 1 at the first tie group
    for i, tid in enumerate(ids):
        c = REF.candidates(Xp, ep, gid, mp[i], mp[i] > 0, 0, tid, 9, mtry, nsplit, 5)
        assert cand["U"].shape == (3, 1, mtry * nsplit)
        assert np.array_equal(cand["n_left"][i, 0], c["n_left"]) and np.array_equal(cand["d_left"][i, 0], c["d_left"])
        bu, bv = REF.bound_uv(c["K"], c["mag"], c["V"])
        du, dv = np.abs(cand["U"][i, 0] - c["U"]), np.abs(cand["V"][i, 0] - c["V"])
        print(kind, n, mtry * nsplit, "tree", tid, "max |dU| / bound", float(np.max(du / np.maximum(bu, 1e-300))), "max |dV| / bound",
              float(np.max(dv / np.maximum(bv, 1e-300))))
        assert (du <= bu).all() and (dv <= bv).all()
        assert tab["n_node"][i, 0] == c["n"] and tab["d_node"][i, 0] == c["d"]
        if kind in ("noevent", "constant"):
            assert c["best"] == -1 and tab["feat"][i, 0] == -1 and tab["stat"][i, 0] == 0.0          # no admissible candidate with chi2 > 0: a leaf
            if kind == "noevent":
                assert not cand["U"][i, 0].any() and not cand["V"][i, 0].any()
            else:
                assert (cand["n_left"][i, 0] == c["n"]).all()
        else:
            gap, bnd = REF.node_margin(c)
            assert c["best"] >= 0 and gap > bnd                                       # the replica's own margin first
            b = c["best"]
            assert tab["feat"][i, 0] == c["feat"][b] and tab["thr"][i, 0] == c["thr"][b]
            assert abs(tab["stat"][i, 0] - c["chi2"][b]) <= REF.chi2_rel_bound(c, b) * c["chi2"][b]
            assert tab["n_node"][i, 1] == c["n_left"][b] and tab["d_node"][i, 2] == c["d"] - c["d_left"][b]


# ---- 2. whole trees ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grown():
    c = CASES.trees_case()
    forest = SF.fit(dev(c["X"]), c["time"], c["ev"], c["mults"], horizons=c["hz"], train_sets=(c["masks"], c["wset"]), **c["kw"])
    return c, forest, host(forest)


def test_whole_trees_node_by_node(grown):
    c, forest, g = grown
    kw = c["kw"]
    node_gpu = g["node"][:, c["order"]]                                               # per position
    nodes = threshold_members = 0
    for i in range(len(c["mults"])):
        m = c["mp"][i]
        node = np.where(m > 0, 0, -1)
        assert g["n_node"][i, 0] == m.sum() and g["d_node"][i, 0] == (m * c["ep"]).sum()
        for s in range((1 << kw["max_depth"]) - 1):
            if s > 0 and g["feat"][i, (s - 1) // 2] < 0:
                assert g["feat"][i, s] == -1 and g["n_node"][i, s] == 0                 # absent
                continue
            member = node == s
            assert g["n_node"][i, s] == m[member].sum() and g["d_node"][i, s] == (m * c["ep"])[member].sum()
            if g["n_node"][i, s] < 2 * kw["min_leaf"]:
                assert g["feat"][i, s] == -1
                continue
            r = REF.candidates(c["Xp"], c["ep"], c["gid"], m, member, s, i, kw["seed"], kw["mtry"], kw["nsplit"], kw["min_leaf"])
            if r["best"] < 0:
                assert g["feat"][i, s] == -1
                continue
            gap, bnd = REF.node_margin(r)
            assert gap > bnd, (i, s, gap, bnd)                                          # zero ambiguous nodes: the seed was chosen for it
            b = r["best"]
            assert g["feat"][i, s] == r["feat"][b] and g["thr"][i, s] == r["thr"][b], (i, s)
            assert abs(g["stat"][i, s] - r["chi2"][b]) <= REF.chi2_rel_bound(r, b) * r["chi2"][b]
            f, thr = int(r["feat"][b]), r["thr"][b]
            at = member & (c["Xp"][:, f] == thr)
            assert at.any()                                                             # the member that lent the threshold ...
            node = np.where(member, 2 * s + 1 + (c["Xp"][:, f] > thr), node)
            assert (node[at] == 2 * s + 1).all()                                        # ... goes left
            threshold_members += int(at.sum())
            nodes += 1
        assert np.array_equal(node_gpu[i][m > 0], node[m > 0])                          # the routing left every patient where the replica does
        assert (g["n_node"][i][g["feat"][i] >= 0] >= 2 * kw["min_leaf"]).all()
        assert np.array_equal(g["feat"][i], c["trees"][i]["feat"])                      # and the replica alone grows the same tree
    assert nodes >= 60 and threshold_members >= nodes
    assert (g["feat"][:, 15:31] >= 0).any()                                             # splits down to the last level


# ---- 3. lock-step independence -------------------------------------------------------------------------------------------------------
def test_a_tree_does_not_depend_on_what_shares_its_launches(grown):
    c, forest, g = grown
    n = len(c["time"])
    others = REF.bootstrap_mults([np.arange(0, 150, 2), np.arange(20, 150), np.arange(0, 90)], n, 8, seed=77)[:23]
    masks = np.concatenate([c["masks"], np.ones((1, n), bool)])
    X = dev(c["X"])
    for k, at in ((2, 13), (5, 0)):
        alone = host(SF.fit(X, c["time"], c["ev"], c["mults"][k:k + 1], horizons=c["hz"], train_sets=(c["masks"], c["wset"][k:k + 1]),
                            tree_ids=[k], **c["kw"]))
        mults = np.concatenate([others[:at], c["mults"][k:k + 1], others[at:]])
        wset = np.concatenate([np.arange(at) % 3, c["wset"][k:k + 1], 2 - np.arange(23 - at) % 3])
        ids = np.concatenate([100 + np.arange(at), [k], 200 + np.arange(23 - at)])
        among = host(SF.fit(X, c["time"], c["ev"], mults, horizons=c["hz"], train_sets=(masks, wset), tree_ids=ids, **c["kw"]))
        assert len(mults) == 24
        for name in alone:
            assert alone[name][0].tobytes() == among[name][at].tobytes() == g[name][k].tobytes(), (k, name)
        assert any(among["feat"][j].tobytes() != among["feat"][at].tobytes() for j in range(24) if j != at)


# ---- 4. leaves and prediction --------------------------------------------------------------------------------------------------------
def test_leaves_against_the_replica(grown):
    c, forest, g = grown
    leaves = 0
    for i, t in enumerate(c["trees"]):
        assert np.array_equal(g["feat"][i], t["feat"])
        leaf = (t["feat"] < 0) & (t["n_node"] > 0)
        leaves += int(leaf.sum())
        assert close(g["mort"][i][leaf], c["morts"][i][leaf], 1e-12) and close(g["H"][i][leaf], c["Hs"][i][leaf], 1e-12)
        assert not g["mort"][i][~leaf].any() and not g["H"][i][~leaf].any()
        assert (c["morts"][i][leaf] > 0).any()
    assert leaves >= 7 * 8


def test_prediction_masks_against_the_replica(grown):
    c, forest, g = grown
    n, T = len(c["time"]), len(c["mults"])
    rng = np.random.default_rng(1)
    Xall = np.concatenate([c["X"], rng.normal(size=(5, c["X"].shape[1])).astype(np.float32)])          # 5 rows that are not in training
    R = len(Xall)
    oob = np.zeros((T, R), bool)
    oob[:, :n] = (c["mults"] == 0) & c["masks"][c["wset"]]
    fold = np.zeros((T, R), bool)
    fold[:4] = np.concatenate([~c["masks"][0], np.ones(5, bool)])                                         # set 0's trees x rows outside set 0
    for name, use in (("all", None), ("oob", oob), ("fold", fold)):
        got = forest.predict(dev(Xall), use=use)
        mo, H, cnt = REF.predict(c["trees"], c["morts"], c["Hs"], Xall, use)
        assert np.array_equal(got["count"], cnt), name
        assert close(got["mortality"], mo, 1e-12) and close(got["hazard"], H, 1e-12), name
        assert close(got["survival"], np.exp(-H), 1e-12), name
        if name == "all":
            assert (cnt == T).all()
        if name == "oob":                                                                                 # rows no tree admits: NaN, counted
            assert (cnt[n:] == 0).all() and np.isnan(got["mortality"][n:]).all() and np.isnan(got["survival"][n:]).all()
            assert (cnt[140:150] == 0).all() and (cnt[:140] > 0).any() and int((cnt == 0).sum()) == int(np.isnan(got["mortality"]).sum())
        if name == "fold":
            assert (cnt[:110] == 0).all() and (cnt[110:] == 4).all()
    assert forest.predict(dev(Xall[:0]))["mortality"].shape == (0,)
    with pytest.raises(ValueError):
        forest.predict(dev(Xall[:, :8]))                                                                  # the forest splits on later genes


def test_importance_and_save_load(grown, tmp_path):
    c, forest, g = grown
    cnt, chi = forest.importance()
    ref_c, ref_x = np.zeros(40, np.int64), np.zeros(40)
    for i in range(7):
        for s in np.nonzero(g["feat"][i] >= 0)[0]:
            ref_c[g["feat"][i, s]] += 1; ref_x[g["feat"][i, s]] += g["stat"][i, s]
    assert np.array_equal(cnt, ref_c) and np.allclose(chi, ref_x, rtol=1e-12) and cnt.sum() == (g["feat"] >= 0).sum()
    forest.save(str(tmp_path / "f.npz"))
    back = SF.load(str(tmp_path / "f.npz"), DEV)
    assert back.hyper == forest.hyper and back.p == 40 and np.array_equal(back.horizons, forest.horizons)
    a, b = forest.predict(dev(c["X"][:20])), back.predict(dev(c["X"][:20]))
    assert a["mortality"].tobytes() == b["mortality"].tobytes() and a["survival"].tobytes() == b["survival"].tobytes()


# ---- 5. cross_validate ---------------------------------------------------------------------------------------------------------------
def test_cross_validate_against_the_replica():
    c = CASES.cv_case()
    for mm in c["margins"]:
        for gap, bnd in mm:
            assert gap > bnd                                                            # the replica's trees are unambiguous
    for fr in c["folds_ref"]:
        for mo, lv in ((fr["val_mort"], fr["leaves_val"]), (fr["oob_mort"], fr["leaves_oob"])):
            gap, same = CASES.flip_gap(mo, lv)
            assert gap > 1e-9 and same                                                  # no pair of mortalities close enough to flip
    N = len(c["time"])
    cohort = dict(rnaseq=dev(c["X"]), label=torch.from_numpy(np.stack([c["time"], c["ev"].astype(np.float64)], 1)),
                  has_survival=torch.ones(N, dtype=torch.bool), n=N)
    res = SF.cross_validate(cohort, c["folds"], n_trees=c["T"], horizons=c["hz"], **c["kw"])
    assert len(res) == 3
    for r, fr in zip(res, c["folds_ref"]):
        assert np.array_equal(r["val_rows"], fr["val_rows"]) and r["oob_missing"] == fr["oob_missing"]
        assert close(r["val_mortality"], fr["val_mort"], 1e-12) and close(r["val_survival"], np.exp(-fr["val_H"]), 1e-12)
        print("fold", r["fold"], "C", r["c_index"], fr["c_index"], "OOB C", r["oob_c_index"], fr["oob_c_index"])
        assert r["c_index"] == fr["c_index"] and r["oob_c_index"] == fr["oob_c_index"]
        assert np.array_equal(r["importance"][0], fr["counts"]) and np.allclose(r["importance"][1], fr["chi2"], rtol=1e-10)
        # measured on the CPU (tests/rsf_cases.py, CV_SEED): the planted gene has the replica's largest summed chi2 in every fold
        assert int(np.argmax(fr["chi2"])) == CASES.PLANTED


def test_cross_validate_reads_per_fold_gene_matrices():
    """MMS_SELECT_GENES leaves one matrix per fold in the cohort: every fold's trees read their own, and keep their forest-wide hash streams"""
    c = CASES.cv_case()
    N = len(c["time"])
    cols = [np.sort(np.random.default_rng(f).permutation(30)[:12]) for f in range(3)]
    base = dict(label=torch.from_numpy(np.stack([c["time"], c["ev"].astype(np.float64)], 1)), has_survival=torch.ones(N, dtype=torch.bool), n=N)
    per_fold = dict(base, rnaseq=dev(c["X"]), rnaseq_folds=[dev(c["X"][:, k]) for k in cols])
    got = SF.cross_validate(per_fold, c["folds"], n_trees=c["T"], horizons=c["hz"], **c["kw"])
    for f in range(3):
        one = SF.cross_validate(dict(base, rnaseq=dev(c["X"][:, cols[f]])), c["folds"], n_trees=c["T"], horizons=c["hz"], **c["kw"])[f]
        assert got[f]["val_mortality"].tobytes() == one["val_mortality"].tobytes() and got[f]["c_index"] == one["c_index"]
        assert got[f]["oob_c_index"] == one["oob_c_index"] and len(got[f]["importance"][0]) == 12


# ---- 6. the entry point --------------------------------------------------------------------------------------------------------------
def test_rsf_baseline_entry_point(tmp_path):
    import pandas as pd
    from multimodal_survival_prediction_amd import data
    env = dict(os.environ, MMS_PATIENTS="90", MMS_FOLDS="3", MMS_RSF_TREES="20", PYTHONPATH=ROOT)
    for k in ("MMS_SELECT_GENES", "MMS_RSF_MTRY", "MMS_RSF_NSPLIT", "MMS_RSF_MIN_LEAF", "MMS_RSF_DEPTH", "MMS_RSF_SEED"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "training", "rsf_baseline.py")], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "results" / "rsf_baseline"
    cv = json.load(open(out / "cv_results.json"))
    assert {"model", "n_folds", "num_epochs", "c_index_mean", "c_index_std", "fold_results", "hyperparameters"} <= set(cv)
    assert cv["model"] == "Random survival forest" and cv["n_folds"] == 3 and cv["num_epochs"] == 0 and len(cv["fold_results"]) == 3
    hp = cv["hyperparameters"]
    assert (hp["n_trees"], hp["mtry"], hp["nsplit"], hp["min_leaf"], hp["max_depth"], hp["seed"]) == (20, 71, 10, 15, 10, 0)
    hz = hp["horizons"]
    assert len(hz) == 3 and "select_genes" not in hp
    folds = data.kfold_indices(90, 3, seed=42)
    for k, fr in enumerate(cv["fold_results"], 1):
        assert {"fold", "best_c_index", "best_epoch", "train_size", "val_size", "oob_c_index"} <= set(fr) and fr["best_epoch"] == 0 and fr["fold"] == k
        assert fr["train_size"] + fr["val_size"] == 90 and 0.0 <= fr["best_c_index"] <= 1.0 and 0.0 <= fr["oob_c_index"] <= 1.0
        df = pd.read_csv(out / f"fold_{k}_predictions.csv")
        assert list(df.columns) == ["patient_id", "survival_time", "event", "risk_score"] and len(df) == fr["val_size"]
        assert sorted(int(s.split("-")[1]) for s in df["patient_id"]) == sorted(int(i) for i in folds[k - 1][1])
        assert np.isfinite(df["risk_score"]).all() and df["risk_score"].nunique() > 3
        from multimodal_survival_prediction_amd.survival_stats import concordance_index
        assert concordance_index(df["survival_time"], -df["risk_score"], df["event"]) == pytest.approx(fr["best_c_index"], abs=1e-12)
        cu = pd.read_csv(out / f"fold_{k}_survival_curves.csv")
        assert list(cu.columns) == ["patient_id", "survival_time", "event", "risk_score"] + [f"S_{float(h)!r}" for h in hz]
        S = cu[[c for c in cu.columns if c.startswith("S_")]].to_numpy()
        assert list(cu["patient_id"]) == list(df["patient_id"]) and ((S > 0) & (S <= 1)).all() and (np.diff(S, axis=1) <= 0).all()
        im = pd.read_csv(out / f"fold_{k}_importance.csv")
        assert list(im.columns) == ["index", "column", "gene", "splits", "chi2_sum"] and len(im) == fr["genes_split_on"] > 0
        assert (im["splits"] > 0).all() and (np.diff(im["chi2_sum"]) <= 0).all() and (im["index"] == im["column"]).all() and im["index"].max() < 5005
    sys.path.insert(0, os.path.join(ROOT, "scripts", "training"))
    try:
        fc = importlib.import_module("final_comparison")
    finally:
        sys.path.pop(0)
    got = fc.collect(str(tmp_path))
    assert list(got) == ["Random survival forest"] and got["Random survival forest"]["mean"] == pytest.approx(cv["c_index_mean"])
    assert "Random survival forest" in fc.NESTED
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "training", "final_comparison.py")], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Random survival forest (+)" in r.stdout, r.stdout + r.stderr
    # another model's predictions of fold 1's patients, compared with the forest's by evaluate_model.py: C-index and curves
    df = pd.read_csv(out / "fold_1_predictions.csv")
    df["risk_score"] = np.random.default_rng(0).normal(size=len(df)) - 0.01 * df["survival_time"]
    df.to_csv(tmp_path / "other.csv", index=False)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "analysis", "evaluate_model.py"), "--predictions", "other.csv", "--outdir",
                        "eval", "--no-plots", "--bootstrap", "50", "--compare", str(out / "fold_1_predictions.csv"), "--horizons",
                        ",".join(repr(float(h)) for h in hz), "--baseline", "other.csv", "--compare-curves", str(out / "fold_1_survival_curves.csv")],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    s = json.load(open(tmp_path / "eval" / "evaluation_summary.json"))
    assert str(out / "fold_1_predictions.csv") in json.dumps(s["c_index_bootstrap"])
    cmp_ = s["prediction_error"]["compare"][str(out / "fold_1_survival_curves.csv")]
    assert 0.0 <= cmp_["ibs"] <= 1.0 and np.isfinite(cmp_["ibs_difference"]["delta"])
