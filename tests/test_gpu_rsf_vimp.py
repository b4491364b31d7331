"""Permutation importance of the survival forest on the MI355X (csrc/rsf.hip: mms_rsf_vimp; ops.rsf_vimp; Forest.vimp; cross_validate(vimp);
scripts/training/rsf_baseline.py) against the numpy replica tests/rsf_vimp_ref.py.

The forests are grown on the device and the DEVICE's tables, base mortalities M0 and tree counts go to the replica, so every comparison
is ==: the delta sums D byte for byte (one sequential float64 sum in a stated order), M = M0 + D / cnt byte for byte (IEEE division), the
pair counts as integers -- also against a plain numpy count over the kernel's own M.
  1. D, M and the counts;  2. edge shapes;  3. a problem does not depend on what shares its launch;  4. cross_validate;  5. the entry point.
Shapes are the kernel's edges: n = 67 (a partial stride of 256 rows) and 300 (past one), times and events tied, rows no tree admits."""
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
import rsf_vimp_ref as VREF
from gpu_util import DEV
from multimodal_survival_prediction_amd import gene_select, ops
from multimodal_survival_prediction_amd import survival_forest as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tables(forest):
    return {k: getattr(forest, k).cpu().numpy() for k in ("feat", "thr", "mort")}


def base(forest, xd, use, sets):
    """M0 and cnt of every set as the device computes them: mms_rsf_predict over the set's trees and the mask"""
    F = int(np.max(sets)) + 1
    got = [forest.predict(xd, use=(use & (np.asarray(sets) == f)[:, None]).astype(np.uint8)) for f in range(F)]
    return np.stack([g["mortality"] for g in got]), np.stack([g["count"] for g in got])


def reference(forest, X, time, ev, use, sets, R, xd=None):
    xd = dev(X) if xd is None else xd
    M0, cnt = base(forest, xd, use, sets)
    t = tables(forest)
    ref = VREF.vimp(X, time, ev, t["feat"], t["thr"], t["mort"], use, sets, M0, cnt, forest.hyper["seed"], forest.tree_id, R, p=forest.p)
    return ref, M0, cnt


def check(out, ref, time, ev, cnt):
    """the launch against the replica, == everywhere; -> the number of rows whose D is not zero"""
    probs = ref["problems"]
    assert [(int(f), int(g)) for f, g in zip(out["problems"]["set"], out["problems"]["gene"])] == [(f, g) for f, g, _ in probs]
    off = out["problems"]["off"]
    assert [[int(v) for v in out["problems"]["tree"][off[q]:off[q + 1]]] for q in range(len(probs))] == [tr for _, _, tr in probs]
    assert np.array_equal(out["conc2"], ref["conc2"]) and np.array_equal(out["comparable"], ref["comparable"])
    assert out["conc2"].dtype == np.int64 and out["comparable"].dtype == np.int64
    R = ref["conc2"].shape[1]
    for q, (f, g, _) in enumerate(probs):
        rows = cnt[f] > 0
        for r in range(R):
            assert out["D"][q, r].tobytes() == ref["D"][q, r].tobytes(), (q, r)
            assert out["M"][q, r][rows].tobytes() == ref["M"][q, r][rows].tobytes(), (q, r)
            assert np.isnan(out["M"][q, r][~rows]).all() and not out["D"][q, r][~rows].any()
            assert (int(out["conc2"][q, r]), int(out["comparable"][q, r])) == VREF.pair_counts(time, ev, out["M"][q, r], rows)
    assert np.array_equal(out["base_conc2"], ref["base_conc2"]) and np.array_equal(out["base_comparable"], ref["base_comparable"])
    assert out["c_base"].tobytes() == ref["c_base"].tobytes()
    assert out["vimp"].tobytes() == ref["vimp"].tobytes() and out["vimp_reps"].tobytes() == ref["vimp_reps"].tobytes()
    assert np.array_equal(out["n_rows"], (cnt > 0).sum(1))
    return int((ref["D"] != 0).sum())


# ---- 1. D bit for bit ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grown():
    c = CASES.trees_case()
    forest = SF.fit(dev(c["X"]), c["time"], c["ev"], c["mults"], horizons=c["hz"], train_sets=(c["masks"], c["wset"]), **c["kw"])
    use = (c["mults"] == 0) & c["masks"][c["wset"]]
    return c, forest, use


def test_seven_trees_bit_for_bit(grown):
    c, forest, use = grown
    ref, M0, cnt = reference(forest, c["X"], c["time"], c["ev"], use, c["wset"], 2)
    out = forest.vimp(dev(c["X"]), c["time"], c["ev"], use, sets=c["wset"], nperm=2, return_delta=True)
    assert out["D"].shape == (len(ref["problems"]), 2, 150) and len(ref["problems"]) >= 20
    assert check(out, ref, c["time"], c["ev"], cnt) > 100
    assert (cnt[:, 140:] == 0).all() and (cnt == 0).any(1).all()                       # rows outside both problems
    assert any(len(tr) > 1 for _, _, tr in ref["problems"])                            # a sum of more than one tree
    assert (out["conc2"] != out["base_conc2"][out["problems"]["set"]][:, None]).any()


@pytest.fixture(scope="module")
def cv_forest():
    """cv_case()'s 3 x 20 trees grown on the device the way cross_validate grows them: it hands the launches the eligible patients in
    coxnet.risk_rows' order, stable time-descending, so X / time / ev of the returned case are in that order (row = time position)"""
    c = CASES.cv_case()
    N, T, kw, order = len(c["time"]), c["T"], c["kw"], c["order"]
    inv = np.empty(N, np.int64); inv[order] = np.arange(N)
    trains = [inv[np.asarray(tr)] for tr, _ in c["folds"]]
    mults = SF.bootstrap_mults(trains, N, T, kw["seed"])
    masks = np.zeros((3, N), bool)
    for f, tr in enumerate(trains):
        masks[f, tr] = True
    sets = np.repeat(np.arange(3), T)
    c = dict(c, X=c["X"][order], time=c["time"][order], ev=c["ev"][order])
    forest = SF.fit(dev(c["X"]), c["time"], c["ev"], mults, horizons=c["hz"], train_sets=(masks, sets), tree_ids=np.arange(3 * T), **kw)
    return c, forest, (mults == 0) & masks[sets], sets


def test_cv_forest_bit_for_bit(cv_forest):
    c, forest, use, sets = cv_forest
    ref, M0, cnt = reference(forest, c["X"], c["time"], c["ev"], use, sets, 2)
    out = forest.vimp(dev(c["X"]), c["time"], c["ev"], use, sets=sets, nperm=2, return_delta=True)
    assert check(out, ref, c["time"], c["ev"], cnt) > 500 and len(ref["problems"]) >= 45


# ---- 2. edge shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [67, 300])
def test_edge_masks_ties_and_pitch(n):
    X, t, e, _ = CASES.level0_case("base", n)
    rng = np.random.default_rng(n)
    mults = rng.integers(0, 3, (6, n))
    xw = torch.zeros(n, X.shape[1] + 3, dtype=torch.float32, device=DEV)
    xw[:, :X.shape[1]] = dev(X)
    xd = xw[:, :X.shape[1]]                                                             # ldx > p
    forest = SF.fit(dev(X), t, e, mults, mtry=12, nsplit=5, min_leaf=4, max_depth=3, seed=9, tree_ids=[0, 5, 11, 12, 40, 41])
    use = mults == 0
    use[4] = False                                                                      # a tree admitting no row
    use[5] = False; use[5, n // 3] = True                                               # ... and one admitting one row
    sets = np.array([0, 0, 0, 1, 1, 1])
    ref, M0, cnt = reference(forest, X, t, e, use, sets, 2, xd)
    assert (cnt == 0).any(1).all() and (cnt[0] > 1).any() and len(np.unique(t)) <= 8 and n > len(np.unique(t))
    assert not xd.is_contiguous() and xd.stride(0) == X.shape[1] + 3
    out = forest.vimp(xd, t, e, use, sets=sets, nperm=2, return_delta=True)
    assert check(out, ref, t, e, cnt) > n // 4
    plain = forest.vimp(dev(X), t, e, use, sets=sets, nperm=2, return_delta=True)
    assert all(np.asarray(out[k]).tobytes() == np.asarray(plain[k]).tobytes() for k in ("D", "M", "conc2", "comparable", "vimp"))
    feat = tables(forest)["feat"]
    assert (feat[:, 3:7] >= 0).any() and (feat[:, 7:] < 0).all()                        # splits at the deepest level the depth allows


def handmade():
    """Three trees of 7 nodes over 5 genes, written by hand: tree 0 splits on gene 1 at the root AND at node 1 (twice along one path) and
    on gene 2 at node 2; tree 1 carries gene 4 in its LAST level (nodes 3..6), where the walk has stopped (2 s + 2 >= nn) and must not read
    it or step to a child; tree 2 is a stump."""
    feat = np.full((3, 7), -1, np.int32)
    thr = np.zeros((3, 7), np.float32)
    feat[0, :3], thr[0, :3] = [1, 1, 2], [0.3, -0.4, 0.1]
    feat[1, :3], thr[1, :3] = [3, 2, 0], [0.0, 0.5, -0.2]
    feat[1, 3:7], thr[1, 3:7] = 4, 0.0
    mort = np.zeros((3, 7))
    mort[0, 3:7] = [0.25, 1.5, 3.0, 0.125]
    mort[1, 3:7] = [2.0, 0.75, 0.5, 4.0]
    mort[2, 0] = 1.0
    z = lambda dt: torch.zeros(3, 7, dtype=dt, device=DEV)
    return SF.Forest(dev(feat), dev(thr), z(torch.float64), z(torch.int32), z(torch.int32), dev(mort), torch.zeros(3, 7, 0, dtype=torch.float64,
                     device=DEV), np.zeros(0), 5, dict(seed=21), np.array([4, 2, 9]))


def test_handmade_forest_stop_rule_and_a_gene_twice_on_a_path():
    forest = handmade()
    n = 83
    rng = np.random.default_rng(5)
    X = np.round(rng.normal(size=(n, 5)), 1).astype(np.float32)
    t, e = CASES.labels("base", n, 1)
    use = rng.random((3, n)) < 0.7
    ref, M0, cnt = reference(forest, X, t, e, use, [0, 0, 0], 3)
    out = forest.vimp(dev(X), t, e, use, nperm=3, return_delta=True)
    check(out, ref, t, e, cnt)
    genes = [g for _, g, _ in ref["problems"]]
    assert genes == [0, 1, 2, 3, 4] and ref["problems"][2][2] == [0, 1]
    assert all(out["D"][0, r].any() for r in range(3))          # gene 0 stands only at tree 1's deepest splitting node: its children end the walk
    q4 = genes.index(4)
    assert not out["D"][q4].any() and (out["conc2"][q4] == out["base_conc2"][0]).all() and (out["vimp"][0, 4] == 0.0)     # never read
    # gene 1: both nodes read the donor's value, so D is one of the four leaf differences of tree 0 -- among them a row whose own value
    # goes right at the root while the donor's goes left at both nodes (a walk substituting at the root alone could not get there)
    don = ref["donor"][0, 0]
    far = use[0] & (X[:, 1] > np.float32(0.3)) & (X[don, 1] <= np.float32(-0.4))
    assert far.any() and (cnt[0][far] > 0).all()
    for i in np.nonzero(far)[0]:
        own = 5 if X[i, 2] <= np.float32(0.1) else 6
        assert out["D"][1, 0, i] == 0.25 - [3.0, 0.125][own - 5]


def test_pitched_mask_and_donor_views(cv_forest):
    """ops.rsf_vimp reads use / donor through one row pitch above n: the same bytes as from contiguous tables"""
    c, forest, use, sets = cv_forest
    a = launch_args(forest, c["X"], c["time"], c["ev"], use, sets, 2)
    n, T = use.shape[1], use.shape[0]
    uw = torch.full((T, n + 5), 1, dtype=torch.uint8, device=DEV)                       # the padding admits: reading it would show
    dw = torch.full((2, T, n + 5), n - 1, dtype=torch.int32, device=DEV)
    uw[:, :n], dw[:, :, :n] = a["use"], a["donor"]
    pitched = dict(a, use=uw[:, :n], donor=dw[:, :, :n])
    assert not pitched["use"].is_contiguous()
    got, want = launch(pitched), launch(a)
    assert all(got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes() for k in ("conc2", "comparable", "D", "M"))
    with pytest.raises(ValueError):
        launch(dict(a, donor=a["donor"] + n))                                           # donors past the last row
    with pytest.raises(ValueError):
        launch(dict(a, ptree=a["ptree"] + T))
    with pytest.raises(ValueError):
        launch(dict(a, pset=a["pset"] + 3))
    with pytest.raises(ValueError):
        launch(dict(a, x=a["x"][:, :8].contiguous()))                                   # the forest splits on later genes


def test_stumps_launch_nothing_and_no_comparable_pair_raises(grown):
    c, forest, use = grown
    X, t, e, mults = CASES.level0_case("base", 67)
    stumps = SF.fit(dev(X), t, e, mults, mtry=6, nsplit=5, min_leaf=5, max_depth=0, seed=1)
    assert int((stumps.feat >= 0).sum()) == 0
    out = stumps.vimp(dev(X), t, e, mults == 0, nperm=2, return_delta=True)
    assert out["vimp"].shape == (1, 37) and not out["vimp"].any() and not out["vimp_reps"].any() and out["conc2"].shape == (0, 2)
    assert out["D"].shape == (0, 2, 67) and len(out["problems"]["set"]) == 0 and 0.0 <= out["c_base"][0] <= 1.0
    with pytest.raises(ValueError):
        stumps.vimp(dev(X), t, np.zeros(67, np.int64), mults == 0)                      # no event: no comparable pair (no launch)
    with pytest.raises(ValueError):
        forest.vimp(dev(c["X"]), c["time"], np.zeros(150, np.int64), use, sets=c["wset"])      # ... and through the launch
    with pytest.raises(ValueError):
        forest.vimp(dev(c["X"]), c["time"], c["ev"], use & (c["wset"] == 0)[:, None], sets=c["wset"])      # set 1 admits no row


# ---- 3. launch sharing -----------------------------------------------------------------------------------------------------------------
def launch_args(forest, X, time, ev, use, sets, R):
    """what Forest.vimp hands to ops.rsf_vimp, put together here from the replica's tables"""
    xd = dev(X)
    M0, cnt = base(forest, xd, use, sets)
    order, gid = REF.positions(time)
    tg = np.empty(len(time), np.int32); tg[order] = gid
    probs = VREF.problem_table(tables(forest)["feat"], sets)
    off = np.concatenate([[0], np.cumsum([len(tr) for _, _, tr in probs])]).astype(np.int32)
    use_d = dev(use.astype(np.uint8))
    return dict(x=xd, feat=forest.feat, thr=forest.thr, mort=forest.mort, use=use_d,
                donor=SF.permutation_donors(forest.hyper["seed"], forest.tree_id, use_d, R), M0=dev(M0), cnt=dev(cnt.astype(np.int32)),
                event=dev(np.asarray(ev).astype(np.int32)), tgroup=dev(tg), pset=np.array([f for f, _, _ in probs], np.int32),
                pgene=np.array([g for _, g, _ in probs], np.int32), poff=off,
                ptree=np.array([t for _, _, tr in probs for t in tr], np.int32))


def launch(a):
    return ops.rsf_vimp(a["x"], a["feat"], a["thr"], a["mort"], a["use"], a["donor"], a["M0"], a["cnt"], a["event"], a["tgroup"], a["pset"],
                        a["pgene"], a["poff"], a["ptree"], delta=True)


def test_a_problem_does_not_depend_on_what_shares_its_launch(cv_forest):
    c, forest, use, sets = cv_forest
    a = launch_args(forest, c["X"], c["time"], c["ev"], use, sets, 3)
    every = {k: v.cpu().numpy() for k, v in launch(a).items()}
    P = len(a["pset"])
    assert every["D"].shape == (P, 3, 90) and P >= 45
    first = {k: v.cpu().numpy() for k, v in launch(dict(a, donor=a["donor"][:1].contiguous())).items()}      # R = 1: the first repeat of R = 3
    for k in every:
        assert first[k][:, 0].tobytes() == every[k][:, 0].tobytes(), k
    assert any(every["D"][:, 0].tobytes() != every["D"][:, r].tobytes() for r in (1, 2))
    for q in (0, P // 2, P - 1):
        lo, hi = a["poff"][q], a["poff"][q + 1]
        alone = launch(dict(a, pset=a["pset"][q:q + 1], pgene=a["pgene"][q:q + 1], poff=np.array([0, hi - lo], np.int32), ptree=a["ptree"][lo:hi]))
        for k in every:
            assert alone[k].cpu().numpy()[0].tobytes() == every[k][q].tobytes(), (q, k)


# ---- 4. cross_validate -----------------------------------------------------------------------------------------------------------------
def cohort_of(c, X=None, **more):
    N = len(c["time"])
    return dict(rnaseq=dev(c["X"] if X is None else X), label=torch.from_numpy(np.stack([c["time"], c["ev"].astype(np.float64)], 1)),
                has_survival=torch.ones(N, dtype=torch.bool), n=N, **more)


def test_cross_validate_vimp_against_the_replica(cv_forest):
    cp, grown_alone, use, sets = cv_forest                                              # the case in time positions ...
    c = CASES.cv_case()                                                                 # ... and in the cohort's order
    res = SF.cross_validate(cohort_of(c), c["folds"], n_trees=c["T"], horizons=c["hz"], vimp=2, **c["kw"])
    forest = res[0]["forest"]
    assert forest.feat.cpu().numpy().tobytes() == grown_alone.feat.cpu().numpy().tobytes()
    ref, M0, cnt = reference(forest, cp["X"], cp["time"], cp["ev"], use, sets, 2)
    unused = 0
    for f, r in enumerate(res):
        assert r["vimp"].shape == (30,) and r["vimp_reps"].shape == (2, 30) and r["vimp"].dtype == np.float64
        assert r["vimp"].tobytes() == ref["vimp"][f].tobytes() and r["vimp_reps"].tobytes() == ref["vimp_reps"][f].tobytes()
        assert int(np.argmax(r["vimp"])) == CASES.PLANTED and all(int(np.argmax(v)) == CASES.PLANTED for v in r["vimp_reps"])
        gone = r["importance"][0] == 0
        unused += int(gone.sum())
        assert (r["vimp"][gone] == 0.0).all() and (r["vimp_reps"][:, gone] == 0.0).all()
        assert ref["c_base"][f] == r["oob_c_index"]
        print("fold", f, "planted", r["vimp"][CASES.PLANTED], "runner-up", np.delete(r["vimp"], CASES.PLANTED).max())
    assert unused > 0
    plain = SF.cross_validate(cohort_of(c), c["folds"], n_trees=c["T"], horizons=c["hz"], vimp=0, **c["kw"])
    default = SF.cross_validate(cohort_of(c), c["folds"], n_trees=c["T"], horizons=c["hz"], **c["kw"])
    for r, q, d in zip(res, plain, default):
        assert set(q) == set(d) == set(r) - {"vimp", "vimp_reps"}
        for k in ("val_mortality", "c_index", "oob_c_index"):
            assert np.asarray(r[k]).tobytes() == np.asarray(q[k]).tobytes() == np.asarray(d[k]).tobytes(), k
        assert all(r["importance"][j].tobytes() == q["importance"][j].tobytes() for j in (0, 1))


def test_cross_validate_vimp_reads_per_fold_gene_matrices():
    c = CASES.cv_case()
    cols = [np.sort(np.random.default_rng(f).permutation(30)[:12]) for f in range(3)]
    cols = [np.union1d(k, [CASES.PLANTED]) for k in cols]
    per_fold = cohort_of(c, rnaseq_folds=[dev(c["X"][:, k]) for k in cols])
    assert gene_select.fold_matrix(per_fold, 1).shape[1] == len(cols[1])
    got = SF.cross_validate(per_fold, c["folds"], n_trees=c["T"], horizons=c["hz"], vimp=2, **c["kw"])
    for f in range(3):
        one = SF.cross_validate(cohort_of(c, c["X"][:, cols[f]]), c["folds"], n_trees=c["T"], horizons=c["hz"], vimp=2, **c["kw"])[f]
        assert got[f]["vimp"].shape == (len(cols[f]),) and got[f]["vimp"].any()
        assert got[f]["vimp"].tobytes() == one["vimp"].tobytes() and got[f]["vimp_reps"].tobytes() == one["vimp_reps"].tobytes()
        assert got[f]["val_mortality"].tobytes() == one["val_mortality"].tobytes()


# ---- 5. the entry point ----------------------------------------------------------------------------------------------------------------
def run_baseline(tmp, **more):
    env = dict(os.environ, MMS_PATIENTS="90", MMS_FOLDS="3", MMS_RSF_TREES="20", PYTHONPATH=ROOT)
    for k in ("MMS_SELECT_GENES", "MMS_RSF_MTRY", "MMS_RSF_NSPLIT", "MMS_RSF_MIN_LEAF", "MMS_RSF_DEPTH", "MMS_RSF_SEED", "MMS_RSF_VIMP"):
        env.pop(k, None)
    env.update(more)
    os.makedirs(tmp, exist_ok=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "training", "rsf_baseline.py")], cwd=tmp, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return tmp / "results" / "rsf_baseline"


def test_rsf_baseline_writes_vimp_files_only_when_asked(tmp_path):
    import pandas as pd
    out = run_baseline(tmp_path / "with", MMS_RSF_VIMP="2")
    cv = json.load(open(out / "cv_results.json"))
    assert cv["hyperparameters"]["vimp_repeats"] == 2
    for k in (1, 2, 3):
        vi, im = pd.read_csv(out / f"fold_{k}_vimp.csv"), pd.read_csv(out / f"fold_{k}_importance.csv")
        assert list(vi.columns) == ["index", "column", "gene", "splits", "chi2_sum", "vimp", "vimp_sd"]
        assert list(im.columns) == ["index", "column", "gene", "splits", "chi2_sum"]
        assert len(vi) == len(im) > 0 and (np.diff(vi["vimp"]) <= 0).all() and (vi["vimp_sd"] >= 0).all() and vi["vimp"].abs().max() > 0
        a, b = vi.sort_values("index").reset_index(drop=True), im.sort_values("index").reset_index(drop=True)
        assert list(a["index"]) == list(b["index"]) and list(a["splits"]) == list(b["splits"]) and list(a["gene"]) == list(b["gene"])
        assert np.array_equal(a["chi2_sum"].to_numpy(), b["chi2_sum"].to_numpy()) and np.isfinite(vi["vimp"]).all()
    plain = run_baseline(tmp_path / "without")
    cv0 = json.load(open(plain / "cv_results.json"))
    assert "vimp_repeats" not in cv0["hyperparameters"] and not [f for f in os.listdir(plain) if f.endswith("_vimp.csv")]
    assert sorted(os.listdir(plain)) == sorted(f for f in os.listdir(out) if not f.endswith("_vimp.csv"))
    assert {k: v for k, v in cv["hyperparameters"].items() if k != "vimp_repeats"} == cv0["hyperparameters"]
    assert [fr["best_c_index"] for fr in cv["fold_results"]] == [fr["best_c_index"] for fr in cv0["fold_results"]]
