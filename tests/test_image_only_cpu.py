"""CPU: the test-side restatement of ImageOnlyModel (tests/image_only_ref.py) against the reference-executed fixture
tests/golden/g8_image_only.npz (tests/golden/generate_image_only_golden.py), and the parameter surface of the HIP model class."""
import os

import numpy as np
import pytest
import torch

import image_only_ref as R

G8 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g8_image_only.npz")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def golden():
    return np.load(G8)


def build_ref():
    torch.manual_seed(83)
    return R.ImageOnlyModel()


def test_fixture_is_small_and_holds_both_cases():
    z = golden()
    assert os.path.getsize(G8) < 1 << 20
    assert z["a.ct"].shape == (8, 1, 16, 16, 8) and z["b.ct"].shape == (3, 1, 9, 10, 7)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_matches_reference_fixture(tag):
    z = golden()
    m = build_ref()
    assert [k for k, _ in m.named_parameters()] == list(z["param_names"]) and list(m.state_dict().keys()) == list(z["state_keys"])
    np.testing.assert_allclose([float(p.detach().double().sum()) for p in m.parameters()], z["init_sum"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose([float(p.detach().double().abs().sum()) for p in m.parameters()], z["init_abs"], rtol=1e-9)
    m.train()
    risk = m(torch.tensor(z[tag + ".ct"]))
    assert _rel(risk.detach(), z[tag + ".train_risk"]) <= 1e-6
    (torch.tensor(z[tag + ".coef"]) * risk).sum().backward()
    for k, p in m.named_parameters():
        assert _rel(p.grad, z[tag + ".grad." + k]) <= 1e-6, k
    for k, b in m.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(z[tag + ".buf." + k]) == 1
        else:
            assert _rel(b, z[tag + ".buf." + k]) <= 1e-6, k
    m.eval()
    with torch.no_grad():
        assert _rel(m(torch.tensor(z[tag + ".ct"])), z[tag + ".eval_risk"]) <= 1e-6


def test_restated_loop_rules():
    """a batch of one patient and a batch without an event: forward (running statistics move), loss 0, no step"""
    torch.manual_seed(0)
    m = build_ref()
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    ct = torch.rand(5, 1, 16, 16, 8)
    t = torch.tensor([5., 4., 3., 2., 1.])
    before = [p.detach().clone() for p in m.parameters()]
    mean, usable = R.train_epoch(m, [(ct[:1], t[:1], torch.ones(1)), (ct[1:], t[1:], torch.zeros(4))], opt)
    assert mean == 0 and usable == 0
    assert all(torch.equal(a, b) for a, b in zip(before, m.parameters()))
    assert int(m.encoder[1].num_batches_tracked) == 2
    mean, usable = R.train_epoch(m, [(ct, t, torch.tensor([1., 0., 1., 0., 1.]))], opt)
    assert mean > 0 and usable == 1 and not torch.equal(before[0], next(m.parameters()))
    h, e = torch.tensor([3., 2., 1., 0.]), torch.tensor([1., 1., 0., 1.])
    assert R.cindex(h, e, torch.tensor([1., 2., 3., 4.])) == 1.0 and R.cindex(-h, e, torch.tensor([1., 2., 3., 4.])) == 0.0


def test_hip_model_parameter_surface():
    """the HIP model class keeps the reference's names and creation order, whatever models.USE_MONAI says (no GPU needed to build it)"""
    import multimodal_survival_prediction_amd as pkg
    from multimodal_survival_prediction_amd import models as HM
    assert pkg.ImageOnlyModel is HM.ImageOnlyModel
    z = golden()
    old = HM.USE_MONAI
    try:
        for flag in (True, False):
            HM.USE_MONAI = flag
            torch.manual_seed(83)
            net = HM.ImageOnlyModel()
            ref = build_ref()
            assert list(net.state_dict().keys()) == list(z["state_keys"])
            for (k, a), (_, b) in zip(net.state_dict().items(), ref.state_dict().items()):
                assert a.shape == b.shape and torch.equal(a, b), k
    finally:
        HM.USE_MONAI = old


def test_head_program_and_widths():
    from multimodal_survival_prediction_amd import models as HM
    from multimodal_survival_prediction_amd.engine import fallback_widths, head_program
    net = HM.ImageOnlyModel()
    prog = head_program(net)
    assert prog["kind"] == "ImageOnlyModel" and prog["bufs"] == dict(feats=64, f1=32, hz=1) and prog["enc_width"] == 64
    assert [L.out_relu for L in prog["lins"]] == [True, False] and "rna" not in prog["bufs"] and "clin" not in prog["bufs"]
    assert fallback_widths(net.encoder) == (16, 32, 64)
    bad = torch.nn.Sequential(torch.nn.Conv3d(1, 24, 3, stride=2, padding=1), torch.nn.BatchNorm3d(24), torch.nn.ReLU(),
                              torch.nn.Conv3d(24, 32, 3, stride=2, padding=1), torch.nn.BatchNorm3d(32), torch.nn.ReLU(),
                              torch.nn.Conv3d(32, 64, 3, stride=2, padding=1), torch.nn.BatchNorm3d(64), torch.nn.ReLU())
    with pytest.raises(ValueError):
        fallback_widths(bad)
