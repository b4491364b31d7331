"""TreeSHAP without a GPU: the numpy replica of the contract (tests/tree_shap_ref.py) against an independent brute-force Shapley value,
its local accuracy on every case of the device tests, and the host-side pieces of multimodal_survival_prediction_amd.tree_shap."""
import numpy as np
import pytest

import tree_shap_cases as C
import tree_shap_ref as REF
from multimodal_survival_prediction_amd import tree_shap


@pytest.mark.parametrize("name", ["stump", "rootleaf", "repeat"])
def test_replica_equals_brute_force_on_the_small_cases(name):
    c = C.case(name)
    rows = slice(0, 12)
    for masked in (False, True):
        use = c["use"][:, rows] if masked else None
        phi, base = REF.shap(c["x"][rows], *C.tables(c), use)
        bphi, bbase = REF.shapley_bruteforce(c["x"][rows], *C.tables(c), use)
        assert np.abs(phi - bphi).max() <= 1e-13 and np.abs(base - bbase).max() <= 1e-13
        assert np.abs(phi).max() > 0


@pytest.mark.parametrize("seed", range(4))
def test_replica_equals_brute_force_on_random_trees(seed):
    c = C.random_small(seed)
    phi, base = REF.shap(c["x"], *C.tables(c))
    bphi, bbase = REF.shapley_bruteforce(c["x"], *C.tables(c))
    assert np.abs(phi - bphi).max() <= 1e-13 and np.abs(base - bbase).max() <= 1e-13
    assert np.abs(phi).max() > 0


@pytest.mark.parametrize("name", C.NAMES)
def test_replica_is_locally_accurate(name):
    """base + sum phi = the sum of the leaf values a row reaches, within the bound the device tests use; a row no tree admits gets 0"""
    c = C.case(name)
    tol = C.tolerance(name)
    for masked in (False, True):
        phi, base = C.reference(name, masked)
        want = REF.reached(c["x"], c["feat"], c["thr"], c["value"], c["goff"], c["use"] if masked else None)
        assert (np.abs(base + phi.sum(2) - want) <= tol[:, None]).all()
    assert (phi[:, 0] == 0).all() and (base[:, 0] == 0).all()        # masked: row 0 is admitted by no tree


def test_cases_hold_what_they_are_for():
    """x == thr occurs at a split node of every case with a split, `repeat` repeats a gene 4 times on a path, chain12 reaches depth 12
    with 12 distinct genes and with one, and the empty group of `groups` is empty"""
    for name in C.NAMES:
        c = C.case(name)
        t, s = np.nonzero(c["feat"] >= 0)
        assert any((c["x"][:, c["feat"][a, b]] == c["thr"][a, b]).any() for a, b in zip(t, s)), name
    paths = [p for _, p in REF.leaves(C.case("repeat")["feat"][1], C.case("repeat")["cover"][1])]
    assert max(len(p) for p in paths) == 4
    ch = C.case("chain12")
    deep = [max(REF.leaves(ch["feat"][t], ch["cover"][t]), key=lambda lp: len(lp[1]))[1] for t in range(2)]
    assert len(deep[0]) == 12 and len({e[1] for e in deep[0]}) == 12 and len(deep[1]) == 12 and len({e[1] for e in deep[1]}) == 1
    assert list(np.diff(C.case("groups")["goff"])) == [3, 0, 1, 5]


def test_slots_of_the_groups_case():
    c = C.case("groups")
    slot, genes = tree_shap.slots(c["feat"], c["goff"])
    assert len(genes) == 4 and len(genes[1]) == 0 and tree_shap.n_slots(genes) == max(len(g) for g in genes) >= 1
    assert slot.dtype == np.int32 and slot.shape == c["feat"].shape
    for g in range(4):
        a, b = c["goff"][g], c["goff"][g + 1]
        f = c["feat"][a:b]
        assert (np.diff(genes[g]) > 0).all() and set(genes[g]) == set(f[f >= 0])
        assert (genes[g][slot[a:b][f >= 0]] == f[f >= 0]).all() and (slot[a:b][f < 0] == 0).all()
    assert len(set(map(tuple, genes))) == 4                          # the groups' gene sets, and so their slots, differ
    assert tree_shap.n_slots([np.zeros(0, np.int64)]) == 1           # U >= 1 even when nothing splits
    with pytest.raises(ValueError):
        tree_shap.slots(c["feat"], [0, 3, 2, 9])


def test_cover_check_raises_when_children_do_not_sum():
    c = C.case("gbm6")
    tree_shap.check_tables(c["feat"], c["cover"])
    for delta, node in ((1, 1), (-1, 2)):
        cover = c["cover"].copy()
        cover[0, node] += delta
        with pytest.raises(ValueError):
            tree_shap.check_tables(c["feat"], cover)
    cover = c["cover"].copy()
    cover[0, 0] = cover[0, 2]; cover[0, 1] = 0                       # the children sum, but one is empty: z = 0 is not a split
    with pytest.raises(ValueError):
        tree_shap.check_tables(c["feat"], cover)
    tree_shap.check_tables(C.case("rootleaf")["feat"][:1], C.case("rootleaf")["cover"][:1])      # no split node: nothing to check


def test_pooled_score_leaves_out_patients_without_a_value(tmp_path):
    """a patient no tree admits (base NaN) is in no mean, whether or not the fold has a column: the denominator counts valued rows"""
    import pandas as pd
    nan = np.nan
    a = tree_shap.ShapValues([np.array([0, 2])], [np.array([[1.0, -3.0], [nan, nan], [2.0, 1.0]])], [np.array([0.5, nan, 0.25])])
    b = tree_shap.ShapValues([np.zeros(0, np.int64)], [np.zeros((3, 0))], [np.array([1.0, nan, nan])])      # a fold that never split
    folds = [tree_shap.write_fold(str(tmp_path), 1, a, ["p0", "p1", "p2"], columns=[4, 9, 7]),
             tree_shap.write_fold(str(tmp_path), 2, b, ["q0", "q1", "q2"])]
    assert list(folds[0][0]) == [4, 7] and np.array_equal(folds[0][2], a.base[0], equal_nan=True)
    score = tree_shap.write_pooled(str(tmp_path), folds, 10)
    want = np.zeros(10)
    want[4], want[7] = 3.0 / 3, 4.0 / 3                              # 2 valued patients of fold 1 + 1 of fold 2
    assert np.array_equal(score, want)
    df = pd.read_csv(tmp_path / "shap_importance.csv")
    assert list(df.columns) == ["gene", "score"] and list(df["gene"][:2]) == ["gene_0", "gene_1"] and np.array_equal(df["score"], want)
    im = pd.read_csv(tmp_path / "fold_1_shap_importance.csv")
    assert list(im["column"]) == [7, 4] and list(im["mean_abs_shap"]) == [2.0, 1.5] and list(im["mean_shap"]) == [-1.0, 1.5]


def test_shap_values_views():
    sv = tree_shap.ShapValues([np.array([1, 4])], [np.array([[0.5, -2.0], [np.nan, np.nan], [-1.5, 0.0]])], [np.array([1.0, np.nan, 2.0])])
    d = sv.dense(0, 6)
    assert d.shape == (3, 6) and d[0, 1] == 0.5 and d[0, 4] == -2.0 and d[0, 0] == 0 and np.isnan(d[1]).all()
    assert list(sv.mean_abs(0)) == [1.0, 1.0]
    assert sv.top(0, 0, 1) == [(4, -2.0)] and sv.top(0, 2, 5) == [(1, -1.5), (4, 0.0)]
