"""Permutation importance of the survival forest without a GPU: the donor tables and the problem table of the package (torch on the CPU)
against the numpy replica (tests/rsf_vimp_ref.py), and the replica alone on rsf_cases.cv_case()'s forest."""
import functools

import numpy as np
import torch

import rsf_cases as CASES
import rsf_ref as REF
import rsf_vimp_ref as VREF
from multimodal_survival_prediction_amd import survival_forest as SF


def _use(seed=0, T=6, n=41):
    rng = np.random.default_rng(seed)
    use = rng.random((T, n)) < 0.4
    use[1] = False                                                   # a tree admitting no row
    use[2] = False; use[2, 17] = True                                # ... and one admitting one
    return use


# ---- 1. donors ---------------------------------------------------------------------------------------------------------------------
def test_a_donor_table_permutes_the_admitted_rows_and_nothing_else():
    use = _use()
    ids = [0, 3, 4, 9, 60, 61]
    don = VREF.donor_table(7, ids, use, 3)
    n = use.shape[1]
    moved = 0
    for r in range(3):
        for t in range(len(ids)):
            a = np.nonzero(use[t])[0]
            assert np.array_equal(np.sort(don[r, t][a]), a)                          # a permutation of the admitted rows
            assert np.array_equal(don[r, t][~use[t]], np.arange(n)[~use[t]])          # the identity elsewhere
            moved += int((don[r, t] != np.arange(n)).sum())
    assert moved > 0.5 * 3 * use.sum()
    assert np.array_equal(don[:, 1], np.broadcast_to(np.arange(n), (3, n)))           # 0 admitted rows
    assert np.array_equal(don[:, 2], np.broadcast_to(np.arange(n), (3, n)))           # 1 admitted row
    assert not np.array_equal(don[0, 0], don[1, 0]) and not np.array_equal(don[1, 0], don[2, 0])      # changes with the repeat
    same_mask = np.stack([use[0], use[0]])
    two = VREF.donor_table(7, [0, 1], same_mask, 1)
    assert not np.array_equal(two[0, 0], two[0, 1])                                   # ... and with the tree id
    assert np.array_equal(two[0, 0], don[0, 0])
    assert not np.array_equal(VREF.donor_table(8, [0], use[:1], 1)[0, 0], don[0, 0])  # ... and with the seed


def test_donors_depend_on_the_mask_only():
    """the table is a function of (seed, id, repeat, mask): a non-admitted row's data is never read -- the signature takes none -- and the
    order among the admitted rows does not move when only rows outside the mask are dropped from or added to the matrix's tail"""
    use = _use()[0]
    a = VREF.donors(7, 0, 1, use)
    longer = np.concatenate([use, np.zeros(5, bool)])                 # five more rows the tree does not admit
    b = VREF.donors(7, 0, 1, longer)
    assert np.array_equal(b[:len(use)], a) and np.array_equal(b[len(use):], len(use) + np.arange(5))


# ---- 2. the package's table -----------------------------------------------------------------------------------------------------------
def test_permutation_donors_equals_the_replica():
    use = _use(3, T=9, n=300)
    ids = np.array([0, 1, 2, 500, 501, 2499, 7, 8, 65534])
    got = SF.permutation_donors(11, ids, use, 4)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == (4, 9, 300)
    assert np.array_equal(got, VREF.donor_table(11, ids, use, 4))
    t = SF.permutation_donors(11, ids, torch.from_numpy(use.astype(np.uint8)), 4)     # a tensor in, a tensor out
    assert torch.is_tensor(t) and t.dtype == torch.int32 and np.array_equal(t.numpy(), got)
    assert np.array_equal(SF.permutation_donors(2 ** 32 + 11, ids, use, 1), got[:1])  # the seed is taken mod 2^32


# ---- 3. the problem table ---------------------------------------------------------------------------------------------------------------
def _table(feat, sets=None, p=None):
    t = {k: v.numpy() for k, v in SF.problem_table(torch.from_numpy(np.asarray(feat, np.int32)), sets, p).items()}
    return [(int(t["set"][q]), int(t["gene"][q]), [int(v) for v in t["tree"][t["off"][q]:t["off"][q + 1]]]) for q in range(len(t["set"]))], t


def test_problem_table_equals_the_replica():
    feat = np.full((5, 7), -1)
    feat[0, [0, 1, 2]] = [4, 4, 2]                                    # tree 0 splits twice on gene 4
    feat[1, [0, 2]] = [2, 4]
    feat[3, [0, 1, 4]] = [0, 4, 0]                                    # tree 2 is a stump
    feat[4, 0] = 2
    for sets in (None, [0, 0, 1, 1, 0], [1, 0, 0, 0, 2]):
        got, raw = _table(feat, sets, 6)
        ref = VREF.problem_table(feat, sets)
        assert got == ref
        assert all(tr == sorted(set(tr)) for _, _, tr in got)         # ascending, no duplicates
        assert raw["off"][0] == 0 and raw["off"][-1] == len(raw["tree"]) and all(v.dtype == np.int32 for v in raw.values())
    assert _table(feat, None, 6)[0] == [(0, 0, [3]), (0, 2, [0, 1, 4]), (0, 4, [0, 1, 3])]
    got, raw = _table(np.full((4, 1), -1), None, 6)                   # stumps
    assert got == [] and list(raw["off"]) == [0] and len(raw["tree"]) == 0
    c = CASES.cv_case()
    feat = np.stack([t["feat"] for t in c["trees"]])
    assert _table(feat, np.repeat(np.arange(3), c["T"]), 30)[0] == VREF.problem_table(feat, np.repeat(np.arange(3), c["T"]))


# ---- 4. the replica alone on the cross-validation case ----------------------------------------------------------------------------------
VIMP_SEED = CASES.CV_SEED       # the forest's own seed (cross_validate passes it on): the planted gene ranks first with it (asserted below)


@functools.lru_cache(maxsize=None)
def cv_rows():
    """cv_case()'s forest with its rows in the order in which cross_validate hands them to the launch: coxnet.risk_rows lists the
    eligible patients (here: all) in stable time-descending order, so row i of the matrix is time position i -- the order the replica's
    trees live in already."""
    c = CASES.cv_case()
    N, K, T, kw = len(c["time"]), 3, c["T"], c["kw"]
    order = c["order"]
    inv = np.empty(N, np.int64); inv[order] = np.arange(N)
    Xp, tp, ep = c["X"][order], c["time"][order], c["ev"][order]
    trains = [inv[np.asarray(tr)] for tr, _ in c["folds"]]
    mults = REF.bootstrap_mults(trains, N, T, kw["seed"])
    masks = np.zeros((K, N), bool)
    for f, tr in enumerate(trains):
        masks[f, tr] = True
    sets = np.repeat(np.arange(K), T)
    morts = [REF.leaves(tp, ep, mults[i], c["trees"][i], masks[sets[i]], c["hz"])[0] for i in range(K * T)]
    Hs = [np.zeros((len(m), 0)) for m in morts]
    use = (mults == 0) & masks[sets]                                 # out of bag
    M0, cnt = np.zeros((K, N)), np.zeros((K, N), np.int64)
    for f in range(K):
        M0[f], _, cnt[f] = REF.predict(c["trees"], morts, Hs, Xp, use & (sets == f)[:, None])
    feat, thr = np.stack([t["feat"] for t in c["trees"]]), np.stack([t["thr"] for t in c["trees"]])
    return dict(X=Xp, time=tp, ev=ep, feat=feat, thr=thr, mort=np.stack(morts), use=use, sets=sets, M0=M0, cnt=cnt, ids=np.arange(K * T))


def test_the_replica_ranks_the_planted_gene_first_on_the_cv_case():
    v = cv_rows()
    R = 3
    out = VREF.vimp(v["X"], v["time"], v["ev"], v["feat"], v["thr"], v["mort"], v["use"], v["sets"], v["M0"], v["cnt"], VIMP_SEED, v["ids"], R)
    assert (out["comparable"] > 0).all() and (out["base_comparable"] > 0).all()
    unused_total = 0
    for f in range(3):
        used = np.zeros(30, bool)
        used[np.unique(v["feat"][v["sets"] == f][v["feat"][v["sets"] == f] >= 0])] = True
        assert used[CASES.PLANTED]
        unused_total += int((~used).sum())
        assert (out["vimp"][f][~used] == 0.0).all() and (out["vimp_reps"][f][:, ~used] == 0.0).all()      # exactly 0.0
        rest = np.delete(np.arange(30), CASES.PLANTED)
        for r in range(R):
            vr = out["vimp_reps"][f, r]
            print("fold", f, "repeat", r, "planted", vr[CASES.PLANTED], "runner-up", vr[rest].max())
            assert int(np.argmax(vr)) == CASES.PLANTED and vr[CASES.PLANTED] > vr[rest].max() > -1.0
        assert int(np.argmax(out["vimp"][f])) == CASES.PLANTED
        # the base count is the out-of-bag C-index cross_validate reports
        assert out["c_base"][f] == CASES.cv_case()["folds_ref"][f]["oob_c_index"]
    assert unused_total > 0
