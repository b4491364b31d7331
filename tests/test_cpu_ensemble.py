"""Host side of multimodal_survival_prediction_amd.ensemble: the rank combination on hand-made arrays, the constructor's refusals that
need no GPU, the lazy export.  No GPU."""
import numpy as np
import pytest
import torch


def test_midranks_with_ties_written_out_by_hand():
    from multimodal_survival_prediction_amd import ensemble as E
    # sorted: -1 (position 1), 0.5 0.5 (positions 2, 3 -> 2.5 each)
    assert E.midranks([0.5, -1.0, 0.5]).tolist() == [2.5, 1.0, 2.5]
    # 2 2 2 -> positions 1, 2, 3: all 2;   7 alone on top: 4
    assert E.midranks([2.0, 7.0, 2.0, 2.0]).tolist() == [2.0, 4.0, 2.0, 2.0]
    assert E.midranks([3.0]).tolist() == [1.0]
    # sorted: -2 (1), 0 0 (2, 3 -> 2.5), 1 (4), 5 5 5 (5, 6, 7 -> 6)
    assert E.midranks([5.0, 0.0, 1.0, 5.0, -2.0, 0.0, 5.0]).tolist() == [6.0, 2.5, 4.0, 6.0, 1.0, 2.5, 6.0]


def test_rank_combination_on_hand_made_arrays():
    from multimodal_survival_prediction_amd import ensemble as E
    h = np.array([[0.1, 0.3, 0.2, 0.3],          # ranks 1, 3.5, 2, 3.5
                  [10.0, -5.0, 10.0, 10.0],      # ranks 3, 1, 3, 3 (the scale of a member does not matter)
                  [0.0, 1.0, 2.0, 3.0]])         # ranks 1, 2, 3, 4
    want = np.array([(1 + 3 + 1) / 3, (3.5 + 1 + 2) / 3, (2 + 3 + 3) / 3, (3.5 + 3 + 4) / 3]) / 4
    got = E.combine_rank(h)
    assert got.shape == (4,) and np.allclose(got, want, rtol=0, atol=1e-15)
    # a per-member shift and positive scale leave the combination unchanged: the point of ranks for Cox log-hazards
    assert np.array_equal(E.combine_rank(h * np.array([[2.0], [0.5], [3.0]]) + np.array([[7.0], [-3.0], [0.25]])), got)
    assert np.array_equal(E.combine_rank(h[:1]), np.array([1, 3.5, 2, 3.5]) / 4)
    with pytest.raises(ValueError):
        E.combine_rank(np.zeros((3, 0)))
    with pytest.raises(ValueError):
        E.combine_rank(np.zeros(3))


def test_constructor_refusals_that_need_no_gpu():
    from multimodal_survival_prediction_amd import models
    from multimodal_survival_prediction_amd.ensemble import FoldEnsemble
    torch.manual_seed(0)
    mk = lambda: models.RNASeqSurvivalModel(input_dim=16).eval()
    with pytest.raises(ValueError, match="1..10 models"):
        FoldEnsemble([mk() for _ in range(11)])
    with pytest.raises(ValueError, match="1..10 models"):
        FoldEnsemble([])
    old = models.USE_MONAI
    models.USE_MONAI = False
    try:
        other = models.SimpleFusionModel(rna_dim=16).eval()
    finally:
        models.USE_MONAI = old
    with pytest.raises(ValueError, match="one class"):
        FoldEnsemble([mk(), other])
    tr = mk()
    tr.train()
    with pytest.raises(RuntimeError, match="model 1 is in train mode"):
        FoldEnsemble([mk(), tr])
    with pytest.raises(ValueError, match="1..10 models"):
        FoldEnsemble.from_checkpoints(["a.pth"] * 11, mk)


def test_ensemble_is_exported_lazily():
    import multimodal_survival_prediction_amd as pkg
    assert "ensemble" in pkg.__all__ and hasattr(pkg.ensemble, "FoldEnsemble") and hasattr(pkg.ensemble, "combine_rank")
    assert "attribution" in pkg.__all__ and hasattr(pkg.attribution, "saliency")
