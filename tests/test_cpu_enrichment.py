"""Gene-set enrichment, host side: the .gmt reader, the set index, the null residuals, the enrichment score by hand, the per-set
summaries on a hand-made matrix, the permutation-variance identity, and the numpy replica (tests/gsea_ref.py) finding a planted set."""
import itertools

import numpy as np
import pytest

import gsea_ref as REF
from multimodal_survival_prediction_amd import enrichment as E
from multimodal_survival_prediction_amd import gene_select


def test_gmt_round_trip_and_reports(tmp_path):
    sets = {"A": ["g1", "g2", "g3"], "B": ["g2", "zz", "g4", "yy"], "C": ["g5"]}
    E.write_gmt(tmp_path / "s.gmt", sets, descriptions={"A": "first"})
    back, desc = E.read_gmt(tmp_path / "s.gmt", descriptions=True)
    assert back == sets and list(back) == ["A", "B", "C"] and desc == {"A": "first", "B": "na", "C": "na"}
    (tmp_path / "dup.gmt").write_text("A\tna\tg1\tg2\tg1\t\tg3\n\nB\tna\tg2\n")
    assert E.read_gmt(tmp_path / "dup.gmt") == {"A": ["g1", "g2", "g3"], "B": ["g2"]}          # duplicates inside a set collapse
    (tmp_path / "twice.gmt").write_text("A\tna\tg1\nA\tna\tg2\n")
    with pytest.raises(ValueError, match="twice"):
        E.read_gmt(tmp_path / "twice.gmt")
    names = ["g%d" % j for j in range(1, 7)]                                              # columns g1 .. g6
    off, gene, kept, rep = E.index_sets(sets, names, min_size=2, max_size=3)
    assert kept == ["A", "B"] and off.tolist() == [0, 3, 5] and gene.tolist() == [0, 1, 2, 1, 3]
    assert rep["dropped"] == {"C": "too small (1 matched)"} and rep["unmatched"] == {"B": ["zz", "yy"]}
    off, gene, kept, rep = E.index_sets(sets, names, min_size=1, max_size=2)
    assert kept == ["B", "C"] and rep["dropped"] == {"A": "too large (3 matched)"}
    _, _, kept, rep = E.index_sets({"all": names}, names, min_size=1, max_size=500)       # k <= G - 1 whatever max_size says
    assert kept == [] and rep["dropped"] == {"all": "too large (6 matched)"}


def test_null_residuals_sum_to_zero_and_are_the_score_coefficients():
    rng = np.random.default_rng(5)
    time = np.round(rng.exponential(30.0, 90), 0) + 1                                      # a coarse grid: tie groups
    event = (rng.random(90) < 0.6).astype(int)
    rows = rng.permutation(90)[:61]
    m = E.null_residuals(time, event, rows)
    assert abs(m.sum()) <= 2e-14
    order, a, _, _ = gene_select.score_coefficients(time, event, rows)
    assert np.array_equal(m[order], a)
    assert np.allclose(m, REF.null_residuals(time, event, rows), rtol=0, atol=1e-13)
    assert np.array_equal(E.null_residuals(time, event), E.null_residuals(time, event, np.arange(90)))


Z6 = np.array([3.0, 2.0, 1.0, -1.0, -2.0, -3.0])


def test_es_by_hand():
    # members at positions 0 and 2; weight 1: NR = 4, run = .75 .5 .75 .5 .25 0 -> the FIRST of the two maxima
    assert REF.es_one(Z6, [0, 2], 1) == (0.75, 0)
    # weight 0: hits add 1/2, run = .5 .25 .75 .5 .25 0
    assert REF.es_one(Z6, [0, 2], 0) == (0.75, 2)
    # members at the bottom: four misses reach -1 at position 3
    es, peak = REF.es_one(Z6, [4, 5], 1)
    assert (es, peak) == (-1.0, 3) and REF.leading_edge(Z6, [4, 5], es, peak) == [4, 5]
    assert E.leading_edge(Z6, [5, 4], es, peak).tolist() == [4, 5]
    assert E.leading_edge(Z6, [2, 0], 0.75, 0).tolist() == [0] and REF.leading_edge(Z6, [0, 2], 0.75, 2) == [0, 2]
    # NR = 0: the members' weights are all |0| -> scored with weight 0; zeros (of either sign) rank by gene index
    z = np.array([1.0, 0.0, -0.0, 0.0, -0.0, -1.0])
    assert REF.ranking(z).tolist() == E.ranking(z).tolist() == [0, 1, 2, 3, 4, 5]
    assert REF.es_one(z, [1, 2], 1) == REF.es_one(z, [1, 2], 0) == (0.75, 2)
    # hi = -lo: H M M H M H with steps of 1/3 -> run = 1/3 0 -1/3 0 -1/3 0; the tie goes to the positive side, its first position
    es, peak, _, run, _ = REF.es_one(np.array([6.0, 5.0, 4.0, 3.0, 2.0, 1.0]), [0, 3, 5], 0, detail=True)
    assert run.max() == -run.min() == 1.0 / 3.0 and (es, peak) == (1.0 / 3.0, 0)
    # a negative score's peak is the first position of the minimum: M H M H M M... -> -1/4 at 0 and again at 2
    es, peak, gap, run, _ = REF.es_one(Z6, [1, 3], 0, detail=True)
    assert run.tolist() == [-0.25, 0.25, 0.0, 0.5, 0.25, 0.0] and (es, peak) == (0.5, 3)
    es, peak, gap, run, _ = REF.es_one(Z6, [2, 5], 0, detail=True)
    assert run.tolist() == [-0.25, -0.5, 0.0, -0.25, -0.5, 0.0] and (es, peak, gap) == (-0.5, 1, np.inf)
    # weighted sums round: there the gap says how far the runner-up position is
    assert REF.es_one(Z6, [0, 2], 1, detail=True)[2] == 0.0 and REF.es_one(Z6, [0, 1], 1, detail=True)[2] == 0.25


ES_HAND = np.array([[0.5, -0.5, 0.25],
                    [0.25, -0.25, -0.125],
                    [0.75, 0.375, -0.25],
                    [-0.5, -0.75, -0.375],
                    [0.5, -0.5, -0.5]])


@pytest.mark.parametrize("summarise", [E.summarise, REF.summarise], ids=["package", "replica"])
def test_summaries_by_hand(summarise):
    """set 0: nulls >= 0 are .25 .75 .5 (mean .5) -> NES 1, two of three reach .5 -> p 3/4; set 1 mirrors it; set 2 is positive with
    only negative nulls -> p = 1, NES nan, and it is left out of the observed pool.  Null NES: >= 0: .5 1.5 1 (set 0), 1 (set 1); < 0:
    -1 (set 0), -.5 -1.5 -1 (set 1), -.4 -.8 -1.2 -1.6 (set 2).  The per-replicate max |NES| are .5, 1.5, 1.5, 1.6."""
    s = summarise(ES_HAND)
    assert s["es"].tolist() == [0.5, -0.5, 0.25]
    assert s["p"].tolist() == [0.75, 0.75, 1.0]
    assert s["nes"][:2].tolist() == [1.0, -1.0] and np.isnan(s["nes"][2])
    assert s["fdr"][:2].tolist() == [0.75, 0.625] and np.isnan(s["fdr"][2])
    assert s["fwer"][:2].tolist() == [0.8, 0.8] and np.isnan(s["fwer"][2])


def test_package_and_replica_summaries_agree():
    rng = np.random.default_rng(11)
    es = rng.uniform(-0.6, 0.6, (40, 9))
    es[1:, 4] = -np.abs(es[1:, 4])
    es[0, 4] = 0.3
    a, b = E.summarise(es), REF.summarise(es)
    for k in ("es", "nes", "p", "fdr", "fwer"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_permutation_variance_identity():
    """over all 5! relabellings the standardised score has mean 0 and variance 1: s_g is the exact permutation variance"""
    time, event = np.array([5.0, 3.0, 3.0, 8.0, 1.0]), np.array([1, 1, 0, 0, 1])
    x = np.random.default_rng(2).normal(size=(5, 4)).astype(np.float32)
    m = REF.null_residuals(time, event)
    perm = np.array(list(itertools.permutations(range(5))))
    _, Z = REF.scores(x, np.arange(5), m, perm)
    assert np.abs(Z.mean(0)).max() <= 1e-12 and np.abs((Z * Z).mean(0) - 1.0).max() <= 1e-12


SANITY_SEED = 0


def test_replica_finds_the_planted_set():
    """n = 120, G = 300, five disjoint sets of 20; the hazard is exp(0.6 * the mean of set 0's genes), which share one latent factor
    (half of each gene's variance) so that the set carries signal at this n; R = 999 relabellings.  numpy default_rng(SANITY_SEED):
    set 0 came out at p = 0.0084 (NES 1.83), the other four between 0.24 and 0.96."""
    rng = np.random.default_rng(SANITY_SEED)
    n, G, R = 120, 300, 999
    x = rng.normal(size=(n, G))
    x[:, :20] = np.sqrt(0.5) * x[:, :20] + np.sqrt(0.5) * rng.normal(size=(n, 1))
    t = rng.exponential(1.0, n) / np.exp(0.6 * x[:, :20].mean(1))
    c = rng.exponential(2.5, n)
    time, event = np.minimum(t, c), (t <= c).astype(int)
    m = REF.null_residuals(time, event)
    perm = np.concatenate([np.arange(n)[None, :], np.stack([rng.permutation(n) for _ in range(R)])])
    _, Z = REF.scores(x, np.arange(n), m, perm)
    off, gene = np.arange(0, 101, 20), np.arange(100)
    es, _, _ = REF.es_all(Z, off, gene, 1)
    s = REF.summarise(es)
    print("planted-set p:", s["p"], "nes:", s["nes"])
    assert s["p"][0] <= 0.01 and s["es"][0] > 0
