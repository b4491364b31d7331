"""GPU parity of the input-gradient attribution path against the fp32 CPU oracle under torch autograd: mms_conv0_bwd_data alone, the
two encoders' input-gradient drivers, SurvivalEngine.attribute on whole models, and that the path leaves training untouched.
Criterion everywhere (SURVEY section 4's op-level 1e-4): max|d| <= 1e-4 max|ref| and relative L2 <= 1e-4.  With frozen statistics
BatchNorm is a per-channel affine map, so the train-mode ReLU-flip lottery of tests/test_gpu_densenet.py does not arise."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4


def check(got, ref, what):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    assert got.shape == ref.shape, what
    assert bool(torch.isfinite(got).all()), what + ": non-finite"
    mx = float((got - ref).abs().max() / ref.abs().max())
    l2 = float((got - ref).norm() / ref.norm())
    print("%s: max %.3e  L2 %.3e" % (what, mx, l2))
    assert mx <= TOL and l2 <= TOL, "%s: max-rel %.3e, rel-L2 %.3e > %g" % (what, mx, l2, TOL)


def _grads(net, args, diff, proj, dtype):
    leaves = [a.to(dtype).clone().requires_grad_() if i in diff else a.to(dtype) for i, a in enumerate(args)]
    out = net(*leaves)
    out = out[0] if isinstance(out, tuple) else out
    out = out.flatten(1) if out.dim() > 2 else out
    grads = torch.autograd.grad(out.sum() if proj is None else (out * proj.to(dtype)).sum(), [leaves[i] for i in diff])
    return out.detach(), grads


def conditioned_case(make, what, tries=8):
    """make(k) -> (oracle model in eval mode, args, indices of the differentiated args, projection or None): the first k whose REFERENCE
    is accurate -> (model, args, projection, output, gradients), all fp32.  Two correct fp32 implementations disagree on the sign of a ReLU input that
    sits within rounding of zero, and one such flip deep in DenseNet121 moves the whole input gradient by 1e-4..1e-2: the fp32 oracle
    against the same oracle in fp64 measured 6e-7 relative L2 on most seeds and 2e-4..3e-3 on roughly every third (which ones depends on
    the host's convolution code).  A case on which the fp32 oracle is within 1e-5 of its fp64 self has no ReLU input that close to
    zero, so on it the 1e-4 margin belongs to the kernels.  The search is over the reference alone; nothing of the code under test
    enters it."""
    for k in range(tries):
        ref, args, diff, proj = make(k)
        out, g32 = _grads(ref, args, diff, proj, torch.float32)
        _, g64 = _grads(copy.deepcopy(ref).double(), args, diff, proj, torch.float64)
        errs = [float((a.double() - b).norm() / b.norm()) for a, b in zip(g32, g64)]
        print("%s, case %d: fp32 oracle against fp64 oracle, relative L2 %s" % (what, k, ", ".join("%.2e" % e for e in errs)))
        if max(errs) <= 1e-5:
            return ref, args, proj, out, g32
    pytest.fail("%s: no case in %d on which the fp32 reference is within 1e-5 of the fp64 one" % (what, tries))


def randomize_bn(ref, x, seed):
    """Non-trivial running statistics (three train-mode forwards) and affine parameters: the defaults mean 0 / var 1 / gamma 1 would
    hide a wrong statistic or parameter pointer."""
    g = torch.Generator().manual_seed(seed)
    ref.train()
    with torch.no_grad():
        for _ in range(3):
            ref(*x) if isinstance(x, tuple) else ref(x)
        for m in ref.modules():
            if isinstance(m, (torch.nn.BatchNorm3d, torch.nn.BatchNorm1d)):
                m.weight.mul_(1 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.add_(0.1 * torch.randn(m.bias.shape, generator=g))
    ref.eval()


# ---- 1. the stem kernel alone ---------------------------------------------------------------------------------------------------------
def _conv0_case(B, dims, seed):
    from multimodal_survival_prediction_amd import ops
    g = torch.Generator().manual_seed(seed)
    out = tuple((d + 1) // 2 for d in dims)
    dbn = torch.randn(B, 64, *out, generator=g)
    dbn = dbn * (torch.rand(dbn.shape, generator=g) > 0.4)                 # as relu0's mask leaves it
    w = torch.randn(64, 1, 7, 7, 7, generator=g) * 0.05
    gamma = 1 + 0.2 * torch.randn(64, generator=g)
    beta = 0.1 * torch.randn(64, generator=g)
    rmean, rvar = 0.1 * torch.randn(64, generator=g), 0.5 + torch.rand(64, generator=g)
    a = gamma / torch.sqrt(rvar + 1e-5)
    want = torch.nn.grad.conv3d_input((B, 1) + tuple(dims), w, a.view(1, 64, 1, 1, 1) * dbn, stride=2, padding=3)
    dev = dict(dbn=dbn.permute(0, 2, 3, 4, 1).reshape(-1, 64).contiguous().to(DEV), w=w.reshape(64, 343).contiguous().to(DEV),
               gamma=gamma.to(DEV), beta=beta.to(DEV), rmean=rmean.to(DEV), rvar=rvar.to(DEV))
    dev["bn"] = ops.bnsrc(dev["gamma"], dev["beta"], dbn.numel() // 64, False, rmean=dev["rmean"], rvar=dev["rvar"])
    return dev, want, out


@pytest.mark.parametrize("B,dims", [(1, (8, 8, 8)), (3, (16, 12, 8)), (2, (32, 32, 16)), (2, (9, 13, 7))])
def test_conv0_bwd_data(B, dims):
    """8^3: every voxel within the padding's reach, all eight parity classes; 16x12x8: unequal extents; 32x32x16: several tiles per
    axis; 9x13x7: odd extents (mms_conv0_fwd takes them on its tile-GEMM form) and partial tiles."""
    from multimodal_survival_prediction_amd import ops
    dev, want, out = _conv0_case(B, dims, 11)
    dx = torch.full((B,) + tuple(dims), float("nan"), device=DEV)          # written, not accumulated
    ops.conv0_bwd_data(dev["dbn"], dev["bn"], dev["w"], dims, out, dx)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dx).all())
    check(dx, want[:, 0], "conv0_bwd_data %s" % (dims,))
    dx2 = torch.full_like(dx, float("nan"))
    ops.conv0_bwd_data(dev["dbn"], dev["bn"], dev["w"], dims, out, dx2)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2)                                            # no float atomics: bit-identical


def test_conv0_bwd_data_group():
    from multimodal_survival_prediction_amd import ops
    B, dims = 2, (16, 16, 8)
    cases = [_conv0_case(B, dims, s) for s in (21, 22)]
    singles, members = [], []
    for dev, want, out in cases:
        dx = torch.full((B,) + dims, float("nan"), device=DEV)
        ops.conv0_bwd_data(dev["dbn"], dev["bn"], dev["w"], dims, out, dx)
        singles.append(dx)
        members.append((dev["dbn"], dev["bn"], dev["w"], torch.full((B,) + dims, float("nan"), device=DEV)))
    ops.conv0_bwd_data(None, None, None, dims, cases[0][2], None, group=members)
    torch.cuda.synchronize()
    for (dev, want, out), one, m in zip(cases, singles, members):
        assert torch.equal(one, m[3])
        check(m[3], want[:, 0], "conv0_bwd_data_group member")


# ---- 2. DenseNet121 encoder ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,dims", [(2, (32, 32, 32)), (1, (64, 64, 32))])
def test_densenet_input_grad(B, dims):
    from oracle.densenet3d import DenseNet121 as OracleNet
    from multimodal_survival_prediction_amd.densenet import DenseNet121

    def make(k):
        torch.manual_seed(3 + k)
        ref = OracleNet()
        x = torch.randn(B, 1, *dims)
        randomize_bn(ref, torch.randn(B, 1, *dims), 4)
        return ref, (x,), (0,), torch.randn(B, 128)

    ref, (x,), wproj, feats, (want,) = conditioned_case(make, "densenet %s" % (dims,))
    net = DenseNet121()
    net.load_state_dict(ref.state_dict())
    net.to(DEV).eval()
    state0 = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        f0 = net(x.to(DEV)).clone()
    got_f, dx = net.input_grad(x.to(DEV), wproj.to(DEV))
    torch.cuda.synchronize()
    check(got_f, feats, "densenet eval features")
    check(dx, want, "densenet d/dx %s" % (dims,))
    # nothing but the workspace was written: parameters, buffers, .grad, and a second eval forward
    for k, v in net.state_dict().items():
        assert torch.equal(v, state0[k]), k
    assert all(p.grad is None for p in net.parameters())
    with torch.no_grad():
        assert torch.equal(net(x.to(DEV)), f0)
    _, dx2 = net.input_grad(x.to(DEV), wproj.to(DEV))
    assert torch.equal(dx, dx2)


# ---- 3. 3-conv encoders ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", [(32, 64, 128), (16, 32, 64)])
def test_fallback_input_grad(widths):
    from multimodal_survival_prediction_amd import attribution
    B, dims = 2, (16, 16, 8)

    def make(k):
        torch.manual_seed(5 + k)
        if widths == (32, 64, 128):
            from oracle.models import _fallback_encoder
            ref = _fallback_encoder(128)
        else:
            from image_only_ref import ImageOnlyModel
            ref = ImageOnlyModel().encoder
        x = torch.randn(B, 1, *dims)
        randomize_bn(ref, torch.randn(4, 1, *dims), 6)
        return ref, (x,), (0,), torch.randn(B, widths[2])

    ref, (x,), wproj, feats, (want,) = conditioned_case(make, "3-conv %s" % (widths,))
    enc = copy.deepcopy(ref).to(DEV).eval()
    got_f, dx = attribution.encoder_input_grad(enc, x.to(DEV), wproj.to(DEV))
    torch.cuda.synchronize()
    check(got_f, feats, "3-conv features")
    check(dx, want, "3-conv d/dx %s" % (widths,))
    for (k, a), (_, b) in zip(ref.state_dict().items(), enc.state_dict().items()):
        assert torch.equal(a, b.cpu()), k


# ---- 4. whole models ---------------------------------------------------------------------------------------------------------------------
def _oracle(kind, use_monai, rna_dim, seed):
    from oracle import models as OM
    torch.manual_seed(seed)
    if kind == "PartialModalityNet":
        return OM.PartialModalityNet(rna_dim=rna_dim, use_monai=use_monai)
    if kind == "SimpleFusionModel":
        return OM.SimpleFusionModel(rna_dim=rna_dim, use_monai=use_monai)
    if kind == "RNASeqSurvivalModel":
        return OM.RNASeqSurvivalModel(input_dim=rna_dim)
    from image_only_ref import ImageOnlyModel
    return ImageOnlyModel()


def _hip(kind, use_monai, rna_dim, ref=None):
    """the HIP model of that class (on the DenseNet121-3D or the 3-conv encoder) with the oracle's state, in eval mode"""
    from multimodal_survival_prediction_amd import models
    old = models.USE_MONAI
    models.USE_MONAI = use_monai
    try:
        torch.manual_seed(0)
        net = {"PartialModalityNet": lambda: models.PartialModalityNet(rna_dim=rna_dim), "SimpleFusionModel": lambda: models.SimpleFusionModel(rna_dim=rna_dim),
               "RNASeqSurvivalModel": lambda: models.RNASeqSurvivalModel(input_dim=rna_dim), "ImageOnlyModel": lambda: models.ImageOnlyModel()}[kind]()
    finally:
        models.USE_MONAI = old
    if ref is not None:
        net.load_state_dict(ref.state_dict())
    return net.to(DEV).eval()


def _inputs(B, dims, rna_dim, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 1, *dims, generator=g), torch.randn(B, rna_dim, generator=g), torch.randn(B, 1, generator=g)


@pytest.mark.parametrize("use_monai", [True, False])
def test_attribute_partial_modality(use_monai):
    B, dims, rd = 3, (32, 32, 32), 64
    mask = torch.tensor([[0., 1., 1.], [1., 0., 1.], [1., 1., 0.]])          # per row, one modality absent

    def make(k):
        ref = _oracle("PartialModalityNet", use_monai, rd, 7 + k)
        ct, rna, clin = _inputs(B, dims, rd, 8 + k)
        ct, rna = ct * mask[:, 0].view(B, 1, 1, 1, 1), rna * mask[:, 1:2]    # (as the dataset makes them)
        randomize_bn(ref, (torch.randn(4, 1, *dims), torch.randn(4, rd), torch.randn(4, 1), torch.ones(4, 3)), 9)
        return ref, (ct, rna, clin, mask), (0, 1, 2), None

    # per-row torch.autograd.grad(hazard[b], inputs): rows do not interact in eval mode, so the sum's gradient holds every row's
    ref, (ct, rna, clin, _), _, hz, (gct, grna, gclin) = conditioned_case(make, "PartialModalityNet")
    net = _hip("PartialModalityNet", use_monai, rd, ref)
    from multimodal_survival_prediction_amd.engine import engine_of
    eng = engine_of(net)
    r = eng.attribute(ct.to(DEV), rna.to(DEV), clin.to(DEV), mask=mask.to(DEV))
    torch.cuda.synchronize()
    check(r["hazard"], hz, "hazard")
    assert r["gate"].shape == (B, 3)
    assert r["ct"].shape == ct.shape and r["rna"].shape == rna.shape and r["clinical"].shape == clin.shape
    assert float(r["ct"][0].abs().max()) == 0.0 and float(r["rna"][1].abs().max()) == 0.0 and float(r["clinical"][2].abs().max()) == 0.0
    assert float(gct[0].abs().max()) == 0.0                                    # (the oracle agrees)
    check(r["ct"][1:], gct[1:], "d hazard / d ct")
    check(r["rna"][[0, 2]], grna[[0, 2]], "d hazard / d rna")
    check(r["clinical"][:2], gclin[:2], "d hazard / d clinical")
    assert all(p.grad is None for p in net.parameters())
    only = eng.attribute(ct.to(DEV), rna.to(DEV), clin.to(DEV), mask=mask.to(DEV), wrt=("rna",))
    assert only["ct"] is None and only["clinical"] is None and torch.equal(only["rna"], r["rna"])


def test_attribute_simple_fusion():
    B, dims, rd = 3, (32, 32, 32), 64

    def make(k):
        ref = _oracle("SimpleFusionModel", True, rd, 7 + k)
        ct, rna, _ = _inputs(B, dims, rd, 10 + k)
        randomize_bn(ref, (torch.randn(4, 1, *dims), torch.randn(4, rd)), 11)
        return ref, (ct, rna), (0, 1), None

    ref, (ct, rna), _, hz, (gct, grna) = conditioned_case(make, "SimpleFusionModel")
    net = _hip("SimpleFusionModel", True, rd, ref)
    from multimodal_survival_prediction_amd.engine import engine_of
    r = engine_of(net).attribute(ct.to(DEV), rna.to(DEV))
    check(r["hazard"], hz, "hazard")
    check(r["ct"], gct, "d hazard / d image")
    check(r["rna"], grna, "d hazard / d rnaseq")
    assert r["clinical"] is None and r["gate"] is None


def test_attribute_image_only():
    B, dims = 3, (32, 32, 32)

    def make(k):
        ref = _oracle("ImageOnlyModel", False, 0, 7 + k)
        ct, _, _ = _inputs(B, dims, 4, 12 + k)
        randomize_bn(ref, torch.randn(4, 1, *dims), 13)
        return ref, (ct,), (0,), None

    ref, (ct,), _, hz, (gct,) = conditioned_case(make, "ImageOnlyModel")
    net = _hip("ImageOnlyModel", False, 0, ref)
    from multimodal_survival_prediction_amd.engine import engine_of
    r = engine_of(net).attribute(ct.to(DEV))
    check(r["hazard"], hz, "hazard")
    check(r["ct"], gct, "d hazard / d ct")
    assert r["rna"] is None and r["clinical"] is None


def test_attribute_rnaseq_and_chunks_of_32():
    """RNASeqSurvivalModel: rna only.  40 rows = a 32-row and an 8-row call, bit for bit (rows are independent)."""
    rd = 64

    def make(k):
        ref = _oracle("RNASeqSurvivalModel", True, rd, 7 + k)
        rna = torch.randn(40, rd, generator=torch.Generator().manual_seed(14 + k))
        randomize_bn(ref, torch.randn(16, rd), 15)
        return ref, (rna,), (0,), None

    ref, (rna,), _, hz, (grna,) = conditioned_case(make, "RNASeqSurvivalModel")
    net = _hip("RNASeqSurvivalModel", True, rd, ref)
    from multimodal_survival_prediction_amd.engine import engine_of
    eng = engine_of(net)
    r = eng.attribute(None, rna.to(DEV))
    check(r["hazard"], hz, "hazard")
    check(r["rna"], grna, "d hazard / d rnaseq")
    assert r["ct"] is None and r["clinical"] is None and r["rna"].shape == (40, rd)
    a, b = eng.attribute(None, rna[:32].to(DEV)), eng.attribute(None, rna[32:].to(DEV))
    assert torch.equal(r["rna"], torch.cat([a["rna"], b["rna"]])) and torch.equal(r["hazard"], torch.cat([a["hazard"], b["hazard"]]))


def test_attribute_40_rows_on_the_3conv_encoder():
    B, dims, rd = 40, (16, 16, 8), 64
    net = _hip("PartialModalityNet", False, rd)
    ct, rna, clin = _inputs(B, dims, rd, 16)
    mask = torch.ones(B, 3)
    from multimodal_survival_prediction_amd.engine import engine_of
    eng = engine_of(net)
    d = lambda t: t.to(DEV)
    r = eng.attribute(d(ct), d(rna), d(clin), mask=d(mask))
    a = eng.attribute(d(ct[:32]), d(rna[:32]), d(clin[:32]), mask=d(mask[:32]))
    b = eng.attribute(d(ct[32:]), d(rna[32:]), d(clin[32:]), mask=d(mask[32:]))
    for k in ("hazard", "gate", "ct", "rna", "clinical"):
        assert torch.equal(r[k], torch.cat([a[k], b[k]])), k
    assert float(r["ct"].abs().max()) > 0


def test_attribute_refusals():
    from multimodal_survival_prediction_amd import models
    from multimodal_survival_prediction_amd.engine import engine_of
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    old = models.USE_MONAI
    models.USE_MONAI = False
    try:
        torch.manual_seed(0)
        net = models.RNASeqSurvivalModel(input_dim=32).to(DEV)
        moe = models.SimMLM_SurvivalNet(rna_dim=32).to(DEV).eval()
        folds = [models.ImageOnlyModel().to(DEV).eval() for _ in range(2)]
    finally:
        models.USE_MONAI = old
    net.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        engine_of(net).attribute(None, torch.randn(4, 32, device=DEV))
    with pytest.raises(RuntimeError, match="SimMLM_SurvivalNet is not supported"):
        engine_of(moe).attribute(torch.rand(2, 1, 16, 16, 8, device=DEV), torch.randn(2, 32, device=DEV), torch.randn(2, 1, device=DEV),
                                 mask=torch.ones(2, 3, device=DEV))
    with pytest.raises(RuntimeError, match="not implemented for fold groups"):
        FoldGroupEngine(folds).attribute(torch.rand(2, 1, 16, 16, 8, device=DEV))


# ---- 5. training is unchanged ----------------------------------------------------------------------------------------------------------
def test_training_is_unchanged_by_attribute():
    """train_step x 2, attribute, train_step == train_step x 3: MultiModalSurvivalNet on the 3-conv encoder at 8 x 8 x 8, B = 4.  At this
    size the path has no float atomics that meet (every weight-gradient element is flushed once: fb_conv_bwd_w's row split is 1 below 512
    rows; the heads' gradients are plain stores), only fp64 statistic atomics -- so two plain runs are compared first, and the run with
    attribute must sit within that run-to-run spread (x 4), with a floor of 1e-6 of the largest weight: a thousandth of what one Adam
    step at lr 1e-3 moves a weight, and far below what a disturbed gradient, statistic or optimiser word would cause."""
    from multimodal_survival_prediction_amd import models
    from multimodal_survival_prediction_amd.engine import SurvivalEngine
    B, dims, rd = 4, (8, 8, 8), 64
    ct, rna, clin = _inputs(B, dims, rd, 17)
    time, event = torch.tensor([5., 3., 8., 1.]), torch.tensor([1., 0., 1., 1.])
    d = lambda t: t.to(DEV)

    def run(with_attr):
        old = models.USE_MONAI
        models.USE_MONAI = False
        try:
            torch.manual_seed(18)
            net = models.MultiModalSurvivalNet(rna_dim=rd).to(DEV)
        finally:
            models.USE_MONAI = old
        eng = SurvivalEngine(net, lr=1e-3)
        step = lambda: eng.train_step(d(ct), d(rna), d(clin), time=d(time), event=d(event), use_graph=False)
        net.train(); step(); step()
        if with_attr:
            net.eval()
            r = eng.attribute(d(ct), d(rna), d(clin))
            assert float(r["ct"].abs().max()) > 0
            net.train()
        step()
        torch.cuda.synchronize()
        return eng.flat.clone(), eng.m.clone(), eng.v.clone(), [b.clone().double() for b in net.buffers()]

    r0, r1, ra = run(False), run(False), run(True)
    for i, what in enumerate(("weights", "adam m", "adam v")):
        spread, diff = float((r0[i] - r1[i]).abs().max()), float((r0[i] - ra[i]).abs().max())
        print("%s: run-to-run spread %.3e, with attribute %.3e" % (what, spread, diff))
        assert diff <= max(4 * spread, 1e-6 * float(r0[i].abs().max())), (what, diff, spread)
    for b0, b1, ba in zip(r0[3], r1[3], ra[3]):
        assert float((b0 - ba).abs().max()) <= max(4 * float((b0 - b1).abs().max()), 1e-6 * float(b0.abs().max()))


# ---- 6. entry point ----------------------------------------------------------------------------------------------------------------------
def test_evaluate_model_attribute_entry_point(tmp_path, monkeypatch):
    from multimodal_survival_prediction_amd import data
    from oracle import models as OM
    spec = importlib.util.spec_from_file_location("evaluate_model", os.path.join(ROOT, "scripts", "analysis", "evaluate_model.py"))
    em = importlib.util.module_from_spec(spec); spec.loader.exec_module(em)
    n = 12
    monkeypatch.setenv("MMS_PATIENTS", str(n))
    monkeypatch.chdir(tmp_path)
    cls, ctor, ckw, _, folds, _ = em.MODELS["final"]
    cohort = data.make_cohort(n=n, **ckw)
    torch.manual_seed(19)
    ref = OM.MultiModalSurvivalNet(rna_dim=cohort["rnaseq"].shape[1], use_monai=True)
    torch.save(ref.state_dict(), tmp_path / "fold_1_best.pth")
    em.main(["--predict", str(tmp_path / "fold_1_best.pth"), "--model", "final", "--fold", "1", "--predictions", str(tmp_path / "pred.csv"),
             "--outdir", str(tmp_path / "results"), "--no-plots", "--attribute", "--top", "7"])
    import pandas as pd
    df = pd.read_csv(tmp_path / "pred.csv")
    adir = tmp_path / "results" / "attribution"
    maps = sorted(p for p in os.listdir(adir) if p.endswith("_ct.npy"))
    assert len(maps) == len(df) and set(maps) == {"%s_ct.npy" % i for i in df["patient_id"]}
    vol = np.load(adir / maps[0])
    assert vol.shape == tuple(cohort["image"].shape[-3:]) and np.isfinite(vol).all() and np.abs(vol).max() > 0
    genes = pd.read_csv(adir / "gene_scores.csv")
    assert len(genes) == 7 and list(genes.columns) == ["gene", "mean_abs_grad"] and (np.diff(genes["mean_abs_grad"]) <= 0).all()
