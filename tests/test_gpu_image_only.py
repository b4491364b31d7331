"""ImageOnlyModel (the CT-only baseline) and the width-generic 3-conv encoder kernels under it.
  1. the fold-group conv ops at the new widths (Cin / Cout multiples of 16, half-filled last column tiles) against torch on the CPU, 1e-4
  2. argument checks of the ops and of the width-parametrised drivers (mms_fb3_*)
  3. the width drivers at (16, 32, 64): group path vs scalar single-model path vs fp64 torch
  4. the model against the reference-executed fixture tests/golden/g8_image_only.npz (SurvivalEngine, FoldGroupEngine of 1 and 2 members)
  5. the autograd contract of the nn.Module
  6. a group step against single steps
  7. train_epoch_image / validate_image and the lock-step style "image" against the restated loop (tests/image_only_ref.py) at lr = 0
  8. the entry point scripts/training/image_only_training.py end to end, final_comparison and evaluate_model on its output
  9. the fused tail (mms_img_tail_*_group) against torch, and the model on it against the fixture
Every test fails before this model existed: the class, the style, the entry points and the accepted widths were not there."""
import copy
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, rel_err, assert_close

import image_only_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G8 = os.path.join(ROOT, "tests", "golden", "g8_image_only.npz")
W3 = (16, 32, 64)


def _lib():
    from multimodal_survival_prediction_amd import _lib as L, ops
    return L.load_library(), L.structs(), ops


def _widths(w):
    return (ctypes.c_int * 3)(*w)


# ------------------------------------------------------------------------------------------------------------------
# 1. group ops at the new widths against torch on the CPU
# ------------------------------------------------------------------------------------------------------------------
_CASES = {}


def _cases(cin, cout, grid, ng):
    from test_gpu_fb_group import _op_case
    key = (cin, cout, grid)
    if key not in _CASES:      # the references are computed once and shared by the ng = 1 and ng = 3 runs
        _CASES[key] = [_op_case(cin, cout, grid, 2000 + 17 * g + cin) for g in range(3)]
    return _CASES[key][:ng]


@pytest.mark.parametrize("ng", [1, 3])
@pytest.mark.parametrize("grid", [(5, 6, 7), (8, 8, 4)])
@pytest.mark.parametrize("cin,cout", [(1, 16), (16, 32), (32, 64), (48, 80)])
def test_group_ops_match_torch_at_new_widths(cin, cout, grid, ng):
    """(48, 80): a half-filled last 32-wide tile in both column directions (Cout = 80 of the forward / weight gradient, Cin = 48 of the
    data gradient); (1, 16) and (16, 32): a single half-filled tile."""
    from test_gpu_fb_group import _conv_blocks
    lib, S, ops = _lib()
    cases = _cases(cin, cout, grid, ng)
    arr, dev = _conv_blocks(S, ops, cases, msplit=2)
    st = ops.stream()
    assert lib.mms_fb_conv_fwd_group(arr, ng, st) == 0
    assert lib.mms_fb_conv_bwd_w_group(arr, ng, st) == 0
    if cin > 1:
        assert lib.mms_fb_conv_bwd_x_group(arr, ng, st) == 0
    torch.cuda.synchronize()
    for g, (c, d) in enumerate(zip(cases, dev)):
        names = ["y", "osum", "osumsq", "dw", "dbias"] + (["dbn_in", "s1", "s2"] if cin > 1 else [])
        for k in names:
            e = rel_err(d[k].reshape(c[k].shape), c[k])
            print(f"  {cin}->{cout} {grid} ng={ng} member {g} {k}: {e:.2e}")
            assert e <= 1e-4, (g, k, e)


# ------------------------------------------------------------------------------------------------------------------
# 2. argument checks
# ------------------------------------------------------------------------------------------------------------------
def test_ops_and_width_drivers_reject_bad_arguments():
    from test_gpu_fb_group import _conv_blocks
    lib, S, ops = _lib()
    st = ops.stream()
    cases = _cases(16, 32, (8, 8, 4), 3)
    fns = (lib.mms_fb_conv_fwd_group, lib.mms_fb_conv_bwd_w_group, lib.mms_fb_conv_bwd_x_group)
    seen = []

    def fresh():
        arr, dev = _conv_blocks(S, ops, cases, msplit=1)
        seen.append(dev)
        return arr

    def untouched():
        torch.cuda.synchronize()
        for dev in seen:
            for d in dev:
                assert float((d["y"] - 7.0).abs().max()) == 0.0
                for k in ("osum", "osumsq", "dw", "dbias", "dbn_in", "s1", "s2"):
                    assert float(d[k].abs().max()) == 0.0, k

    for field, val in (("Cout", 8), ("Cin", 24), ("Cin", 144)):
        arr = fresh()
        for g in range(3):
            setattr(arr[g], field, val)
        for fn in fns:
            assert fn(arr, 3, st) == -1, (field, val)
    arr = fresh()
    arr[1].Cin = 32                                   # mismatched members
    for fn in fns:
        assert fn(arr, 3, st) == -1
    arr = fresh()
    arr[2].Cout = 16
    for fn in fns:
        assert fn(arr, 3, st) == -1
    untouched()
    # width drivers
    B, dims = 2, (8, 8, 4)
    n16, n32 = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.mms_fb3_workspace_bytes(_widths(W3), B, *dims, ctypes.byref(n16)) == 0
    assert lib.mms_fb3_workspace_bytes(_widths((32, 64, 128)), B, *dims, ctypes.byref(n32)) == 0 and n32.value != n16.value
    for bad in ((8, 32, 64), (16, 24, 64), (16, 32, 72), (16, 32, 144)):
        assert lib.mms_fb3_workspace_bytes(_widths(bad), B, *dims, ctypes.byref(n32)) == -1
    assert lib.mms_fb3_workspace_bytes(None, B, *dims, ctypes.byref(n16)) == -1
    ws = torch.zeros(n32.value, dtype=torch.uint8, device=DEV)
    x = torch.zeros(B, 1, *dims, device=DEV)
    out = torch.full((B, 64), 7.0, device=DEV)
    enc = _encoder(1).to(DEV)
    tab = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    ptab, btab = tab([p.detach() for p in enc.parameters()]), tab(list(enc.buffers()))
    grads = [torch.zeros_like(p) for p in enc.parameters()]
    gtab = tab(grads)
    nul12, nul9 = (ctypes.c_void_p * 12)(), (ctypes.c_void_p * 9)()
    fwd = lambda nbytes, w, pt=ptab, bt=btab, ldo=64: lib.mms_fb3_forward(ws.data_ptr(), nbytes, _widths(w) if w else None, B, *dims, x.data_ptr(), pt, bt,
                                                                         out.data_ptr(), ldo, 1, st)
    bwd = lambda nbytes, w, pt=ptab, gt=gtab: lib.mms_fb3_backward(ws.data_ptr(), nbytes, _widths(w) if w else None, B, *dims, x.data_ptr(), pt,
                                                                   out.data_ptr(), 64, gt, st)
    assert fwd(n32.value, W3) == -1 and bwd(n32.value, W3) == -1                  # a workspace sized for other widths
    assert lib.mms_fb3_init(ws.data_ptr(), n32.value, _widths(W3), B, *dims, btab, st) == -1
    assert fwd(n16.value, (16, 32, 72)) == -1 and fwd(n16.value, None) == -1       # widths
    assert fwd(n16.value, W3, pt=nul12) == -1 and fwd(n16.value, W3, pt=None) == -1      # null tables / entries
    assert bwd(n16.value, W3, gt=nul12) == -1 and bwd(n16.value, W3, gt=None) == -1
    assert lib.mms_fb3_init(ws.data_ptr(), n16.value, _widths(W3), B, *dims, nul9, st) == -1
    assert fwd(n16.value, W3, ldo=32) == -1                                         # out narrower than widths[2]
    n48 = ctypes.c_size_t(0)
    assert lib.mms_fb3_workspace_bytes(_widths((16, 48, 64)), B, *dims, ctypes.byref(n48)) == 0 and n48.value <= n32.value
    assert fwd(n48.value, (16, 48, 64)) == -1 and bwd(n48.value, (16, 48, 64)) == -1      # the scalar kernels: widths that divide 256
    P = lambda vals: (ctypes.c_void_p * len(vals))(*vals)
    gws, gx, gout = P([ws.data_ptr()] * 2), P([x.data_ptr()] * 2), P([out.data_ptr()] * 2)
    gp, gb, gg = P([ctypes.addressof(ptab)] * 2), P([ctypes.addressof(btab)] * 2), P([ctypes.addressof(gtab)] * 2)
    gfwd = lambda ng, nbytes, w, pt=gp: lib.mms_fb3_forward_group(ng, gws, nbytes, _widths(w) if w else None, B, *dims, gx, pt, gb, gout, 64, 1, st)
    gbwd = lambda ng, nbytes, w, gt=gg: lib.mms_fb3_backward_group(ng, gws, nbytes, _widths(w) if w else None, B, *dims, gx, gp, gout, 64, gt, st)
    assert gfwd(2, n32.value, W3) == -1 and gbwd(2, n32.value, W3) == -1
    assert gfwd(2, n16.value, (16, 40, 64)) == -1 and gfwd(2, n16.value, None) == -1
    assert gfwd(0, n16.value, W3) == -1 and gfwd(11, n16.value, W3) == -1
    assert gfwd(2, n16.value, W3, pt=P([ctypes.addressof(ptab), ctypes.addressof(nul12)])) == -1
    assert gfwd(2, n16.value, W3, pt=None) == -1 and gbwd(2, n16.value, W3, gt=None) == -1
    assert gbwd(2, n16.value, W3, gt=P([ctypes.addressof(gtab), ctypes.addressof(nul12)])) == -1
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0 and all(float(g.abs().max()) == 0.0 for g in grads)      # nothing was launched


# ------------------------------------------------------------------------------------------------------------------
# 3. width drivers: group path vs scalar path vs fp64 torch
# ------------------------------------------------------------------------------------------------------------------
def _encoder(seed, widths=W3):
    torch.manual_seed(seed)
    layers, ci = [], 1
    for co in widths:
        layers += [torch.nn.Conv3d(ci, co, 3, stride=2, padding=1), torch.nn.BatchNorm3d(co), torch.nn.ReLU()]
        ci = co
    enc = torch.nn.Sequential(*layers, torch.nn.AdaptiveAvgPool3d(1), torch.nn.Flatten())
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm3d):
                m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.1)
    return enc


class _Side:
    """Device state of one path (scalar or group) for the ng encoders: own parameters, buffers, gradients, workspaces."""

    def __init__(self, lib, ops, encs, B, dims, widths):
        self.enc = [copy.deepcopy(e).to(DEV) for e in encs]
        self.params = [[p.detach() for p in e.parameters()] for e in self.enc]
        self.bufs = [list(e.buffers()) for e in self.enc]
        self.grads = [[torch.zeros_like(p) for p in ps] for ps in self.params]
        tab = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        self.ptab, self.btab, self.gtab = [tab(p) for p in self.params], [tab(b) for b in self.bufs], [tab(g) for g in self.grads]
        n = ctypes.c_size_t(0)
        assert lib.mms_fb3_workspace_bytes(_widths(widths), B, *dims, ctypes.byref(n)) == 0
        self.nbytes = n.value
        self.ws = [torch.empty(n.value, dtype=torch.uint8, device=DEV) for _ in encs]
        for w, b in zip(self.ws, self.btab):
            assert lib.mms_fb3_init(w.data_ptr(), n.value, _widths(widths), B, *dims, b, ops.stream()) == 0
        self.out = [torch.zeros(B, widths[2], device=DEV) for _ in encs]

    def arrays(self):
        P = lambda vals: (ctypes.c_void_p * len(vals))(*vals)
        a = lambda tabs: P([ctypes.addressof(t) for t in tabs])
        return P([w.data_ptr() for w in self.ws]), a(self.ptab), a(self.btab), a(self.gtab), P([o.data_ptr() for o in self.out])


@pytest.mark.parametrize("B,dims", [(4, (16, 16, 8)), (3, (9, 10, 7))])
def test_width_drivers_match_scalar_path_and_fp64(B, dims):
    lib, S, ops = _lib()
    ng, C = 3, W3[2]
    st = ops.stream()
    wd = _widths(W3)
    encs = [_encoder(400 + g) for g in range(ng)]
    gen = torch.Generator().manual_seed(11)
    xs = [torch.rand(B, 1, *dims, generator=gen) for _ in range(ng)]
    douts = [torch.randn(B, C, generator=gen) for _ in range(ng)]
    xd, dd = [x.to(DEV) for x in xs], [d.to(DEV) for d in douts]
    sc, gr = _Side(lib, ops, encs, B, dims, W3), _Side(lib, ops, encs, B, dims, W3)
    P = lambda vals: (ctypes.c_void_p * len(vals))(*vals)
    ws, ptab, btab, gtab, out = gr.arrays()
    xp, dp = P([x.data_ptr() for x in xd]), P([d.data_ptr() for d in dd])
    nb = sc.nbytes
    for g in range(ng):
        assert lib.mms_fb3_forward(sc.ws[g].data_ptr(), nb, wd, B, *dims, xd[g].data_ptr(), sc.ptab[g], sc.btab[g], sc.out[g].data_ptr(), C, 1, st) == 0
        assert lib.mms_fb3_backward(sc.ws[g].data_ptr(), nb, wd, B, *dims, xd[g].data_ptr(), sc.ptab[g], dd[g].data_ptr(), C, sc.gtab[g], st) == 0
    assert lib.mms_fb3_forward_group(ng, ws, nb, wd, B, *dims, xp, ptab, btab, out, C, 1, st) == 0
    assert lib.mms_fb3_backward_group(ng, ws, nb, wd, B, *dims, xp, ptab, dp, C, gtab, st) == 0
    torch.cuda.synchronize()
    for g in range(ng):
        assert_close(gr.out[g], sc.out[g], 1e-4, f"train features {g}")
        e64 = copy.deepcopy(encs[g]).double().train()
        o64 = e64(xs[g].double())
        o64.backward(douts[g].double())
        assert_close(gr.out[g], o64.detach(), 1e-4, f"group train features vs fp64 {g}")
        assert_close(sc.out[g], o64.detach(), 1e-4, f"scalar train features vs fp64 {g}")
        for (k, a), b, c in zip(e64.named_buffers(), gr.bufs[g], sc.bufs[g]):
            if "num_batches" in k:
                assert int(a) == int(b) == int(c) == 1
            else:
                assert_close(b, a, 1e-4, f"group {k} {g}"); assert_close(c, a, 1e-4, f"scalar {k} {g}")
        # all 12 gradients: each path against fp64, per tensor, relative to the largest gradient of its kind (conv biases feed a
        # training-mode BatchNorm: exactly zero, rounding noise on the device)
        refs = [p.grad for p in e64.parameters()]
        for i, ((k, _), ref) in enumerate(zip(e64.named_parameters(), refs)):
            scale = float(ref.abs().max())
            for name, side in (("group", gr), ("scalar", sc)):
                got = side.grads[g][i].double().cpu()
                if k.endswith("bias") and k[0] in "036":
                    assert float(got.abs().max()) <= 1e-4 * max(float(refs[i - 1].abs().max()), 1e-30), (name, k)
                else:
                    e = float((got - ref).abs().max()) / scale
                    print(f"  {dims} member {g} {name} {k}: {e:.2e}")
                    assert e <= 1e-4, (name, k, e)
    for g in range(ng):
        assert lib.mms_fb3_forward(sc.ws[g].data_ptr(), nb, wd, B, *dims, xd[g].data_ptr(), sc.ptab[g], sc.btab[g], sc.out[g].data_ptr(), C, 0, st) == 0
    assert lib.mms_fb3_forward_group(ng, ws, nb, wd, B, *dims, xp, ptab, btab, out, C, 0, st) == 0
    torch.cuda.synchronize()
    for g in range(ng):
        e64 = copy.deepcopy(encs[g]).double().train()
        e64(xs[g].double())
        e64.eval()
        with torch.no_grad():
            o64 = e64(xs[g].double())
        assert_close(gr.out[g], sc.out[g], 1e-4, f"eval features {g}")
        assert_close(gr.out[g], o64, 1e-4, f"eval features vs fp64 {g}")
        assert int(gr.bufs[g][2]) == 1


# ------------------------------------------------------------------------------------------------------------------
# 4. the model against the reference-executed fixture
# ------------------------------------------------------------------------------------------------------------------
def _fixture_model():
    from multimodal_survival_prediction_amd import models as HM
    torch.manual_seed(83)
    return HM.ImageOnlyModel()


def _check_against_fixture(z, tag, model, eng, P):
    """after a train-mode forward and the backward of the fixture's linear functional on plan P"""
    assert_close(P.buf["hz"][:, 0], torch.tensor(z[tag + ".train_risk"]), 1e-4, "train risk")
    for k, b in model.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(z[tag + ".buf." + k]) == 1
        else:
            assert_close(b, torch.tensor(z[tag + ".buf." + k]), 1e-4, k)
    gv = {id(p): v for p, v in zip(eng.params, eng.gviews)}
    gmax = max(float(np.abs(z[tag + ".grad." + k]).max()) for k, _ in model.named_parameters())
    for k, p in model.named_parameters():
        ref = torch.tensor(z[tag + ".grad." + k])
        if float(ref.abs().max()) < 1e-5 * gmax:      # exactly-zero gradients (a conv bias feeding a training-mode BatchNorm): noise
            assert float(gv[id(p)].abs().max()) < 1e-4 * gmax, k
        else:
            assert_close(gv[id(p)].reshape(ref.shape), ref, 1e-4, k)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_model_matches_reference_fixture_single_engine(tag):
    from multimodal_survival_prediction_amd.engine import SurvivalEngine
    z = np.load(G8)
    model = _fixture_model().to(DEV).train()
    eng = SurvivalEngine(model, lr=0.0, weight_decay=0.0)
    ct = torch.tensor(z[tag + ".ct"]).to(DEV)
    P = eng.plan(ct.shape[0], tuple(ct.shape[-3:]))
    assert P.fallback and tuple(P.widths) == W3
    eng.load_batch(P, ct)
    eng.gflat.zero_()
    eng._forward(P, True)
    P.dbuf["hz"][:, 0].copy_(torch.tensor(z[tag + ".coef"]))
    eng._backward_from_dhz(P)
    torch.cuda.synchronize()
    _check_against_fixture(z, tag, model, eng, P)
    hz, gate = eng.forward_eval(ct)
    assert gate is None
    assert_close(hz, torch.tensor(z[tag + ".eval_risk"]), 1e-4, "eval risk")
    model.eval()
    with torch.no_grad():
        assert_close(model(ct), torch.tensor(z[tag + ".eval_risk"]), 1e-4, "eval risk through the module")


@pytest.mark.parametrize("n_members", [1, 2])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_model_matches_reference_fixture_fold_group(tag, n_members):
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    z = np.load(G8)
    ms = [_fixture_model().to(DEV).train() for _ in range(n_members)]
    ge = FoldGroupEngine(ms, fused_tail=False, lr=0.0, weight_decay=0.0)          # the pool launch + two mms_linear launches
    ct = torch.tensor(z[tag + ".ct"]).to(DEV)
    GP = ge.plan(ct.shape[0], tuple(ct.shape[-3:]))
    assert GP.fallback and tuple(GP.widths) == W3 and not GP.img_tail
    for e, P in zip(GP.eng, GP.Ps):
        e.load_batch(P, ct)
    ge._zero(GP)
    ge._forward(GP, True)
    for P in GP.Ps:
        P.dbuf["hz"][:, 0].copy_(torch.tensor(z[tag + ".coef"]))
    ge._backward_from_dhz(GP)
    torch.cuda.synchronize()
    for m, e, P in zip(ms, GP.eng, GP.Ps):
        _check_against_fixture(z, tag, m, e, P)
    for hz, gate in ge.forward_eval([dict(ct=ct)] * n_members, use_graph=False):
        assert gate is None
        assert_close(hz, torch.tensor(z[tag + ".eval_risk"]), 1e-4, "eval risk")


# ------------------------------------------------------------------------------------------------------------------
# 5. autograd contract
# ------------------------------------------------------------------------------------------------------------------
def test_autograd_contract_and_state_dict_interchange():
    import multimodal_survival_prediction_amd as pkg
    z = np.load(G8)
    torch.manual_seed(3)
    net = pkg.ImageOnlyModel().to(DEV)
    ct = torch.tensor(z["a.ct"]).to(DEV)
    net.train()
    r0 = net(ct)
    assert r0.shape == (8,) and r0.requires_grad
    r0.sum().backward()
    for k, p in net.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), k
    assert float(net.risk_head.weight.grad.abs().max()) > 0 and float(net.encoder[0].weight.grad.abs().max()) > 0
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    opt.step()
    r1 = net(ct)
    assert float((r1 - r0).detach().abs().max()) > 1e-4
    # one patient: legal in training mode (no BatchNorm1d in this model)
    assert net(ct[:1]).shape == (1,)
    with pytest.raises(RuntimeError):
        net(ct.cpu())
    # state_dict: the fixture's keys; loads into the restated class and back, same eval risks
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    assert list(sd.keys()) == list(z["state_keys"])
    ref = R.ImageOnlyModel()
    ref.load_state_dict(sd, strict=True)
    ref.eval(); net.eval()
    with torch.no_grad():
        want = ref(ct.cpu())
        assert_close(net(ct), want, 1e-4, "HIP -> restated class")
        torch.manual_seed(9)
        ref2 = R.ImageOnlyModel()
        for m in ref2.modules():
            if isinstance(m, torch.nn.BatchNorm3d):
                m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)
        net2 = pkg.ImageOnlyModel()
        net2.load_state_dict(ref2.state_dict(), strict=True)
        net2.to(DEV).eval(); ref2.eval()
        assert_close(net2(ct), ref2(ct.cpu()), 1e-4, "restated class -> HIP")


# ------------------------------------------------------------------------------------------------------------------
# 6. group step equals single steps (bounds of test_gpu_fb_group.test_fallback_group_step_equals_single_steps)
# ------------------------------------------------------------------------------------------------------------------
def _img_models(G):
    from multimodal_survival_prediction_amd import models as HM
    out = []
    for g in range(G):
        torch.manual_seed(100 + g)
        m = HM.ImageOnlyModel()
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, torch.nn.BatchNorm3d):
                    mod.weight.uniform_(0.5, 1.5); mod.bias.normal_(0, 0.1)
        out.append(m)
    return out


def test_group_step_equals_single_steps():
    from multimodal_survival_prediction_amd.engine import SurvivalEngine
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    from test_gpu_models import _batch
    G, B, dims = 3, 4, (16, 16, 8)
    base = _img_models(G)
    solo = [copy.deepcopy(m).to(DEV).train() for m in base]
    grp = [copy.deepcopy(m).to(DEV).train() for m in base]
    kw = dict(lr=1e-4, weight_decay=1e-4)
    se = [SurvivalEngine(m, **kw) for m in solo]
    ge = FoldGroupEngine(grp, **kw)
    for it in range(3):
        batches = []
        for g in range(G):
            ct, _, _, t, e, _ = _batch(B, dims, 8, 50 + 10 * it + g)
            if it == 1 and g == 1:
                e = torch.zeros_like(e)       # a batch without events
            batches.append(dict(ct=ct, time=t, event=e))
        for g in range(G):
            se[g].train_step(skip_if_unusable=True, use_graph=it > 0, **batches[g])
        ge.train_step(batches, skip_if_unusable=True, use_graph=it > 0)
        torch.cuda.synchronize()
        assert ge.plan(B, dims).fallback
        if it == 0:
            for g in range(G):
                a, b = se[g].gflat.double(), ge.engines[g].gflat.double()
                l2 = float(((a - b) ** 2).sum().sqrt() / (a ** 2).sum().sqrt())
                print(f"  ImageOnlyModel member {g}: first-step gradient L2 {l2:.2e}")
                assert l2 <= 1e-2, (g, l2)
    stats_s = [e.epoch_stats() for e in se]
    stats_g = ge.epoch_stats()
    for g in range(G):
        assert stats_g[g]["n_batches"] == 3 and stats_g[g]["n_usable"] == stats_s[g]["n_usable"] == (2 if g == 1 else 3)
        assert abs(stats_g[g]["sum_loss"] - stats_s[g]["sum_loss"]) <= 5e-2 * max(1.0, abs(stats_s[g]["sum_loss"])), (g, stats_g[g], stats_s[g])
        assert float(ge.engines[g].step_count) == float(se[g].step_count)
        tot = close = 0
        worst = 0.0
        for p, q in zip(solo[g].parameters(), grp[g].parameters()):
            d = (p.detach() - q.detach()).abs()
            tot += d.numel(); close += int((d <= 2e-5).sum()); worst = max(worst, float(d.max()))
        assert worst <= 6.5e-4, worst
        assert close / tot >= 0.9, close / tot
        for (k, b), (_, c) in zip(solo[g].named_buffers(), grp[g].named_buffers()):
            if "num_batches" in k:
                assert int(b) == int(c) == 3
            else:
                assert rel_err(c, b) <= 1e-2, k


# ------------------------------------------------------------------------------------------------------------------
# 7. epoch loops against the restated loop at lr = 0
# ------------------------------------------------------------------------------------------------------------------
def _epoch_cohort(dims, seed=5):
    """22 labelled patients with an image; patients 4..7 without an event (a whole batch of 4 in every fold's order below)."""
    rng = np.random.default_rng(seed)
    n = 22
    img = torch.tensor(rng.random((n, 1) + dims, dtype=np.float32))
    time = (rng.exponential(1000, n) + 1 + np.arange(n) * 1e-2).astype(np.float32)
    event = (rng.random(n) < 0.6).astype(np.float32)
    event[0] = event[8] = event[12] = event[16] = event[20] = 1
    event[4:8] = 0
    return dict(image=img.contiguous(), rnaseq=torch.zeros(n, 4), clinical=torch.zeros(n, 1), label=torch.tensor(np.stack([time, event], 1)),
                mask=torch.tensor(np.tile(np.array([[1, 0, 0]], np.float32), (n, 1))), has_survival=torch.ones(n, dtype=torch.bool), n=n, dims=dims)


_EPOCH = {}


def _epoch_reference():
    """Per fold: the restated loop on the CPU (computed once, shared by the sequential and the lock-step test)."""
    if not _EPOCH:
        dims, K, B = (16, 16, 8), 3, 4
        cpu = _epoch_cohort(dims)
        # fold f: 21 of the 22 patients: the five whole batches 0..3 | 4..7 (no event) | ... | 16..19 rotated by f, and a tail of ONE patient
        blocks = [np.arange(4 * b, 4 * b + 4) for b in range(5)]
        order = [np.concatenate(blocks[f:] + blocks[:f] + [np.array([20 + f % 2])]) for f in range(K)]
        base, refs = [], []
        for f in range(K):
            torch.manual_seed(20 + f)
            base.append(R.ImageOnlyModel())
            m = copy.deepcopy(base[f])
            bat = lambda idx: [(cpu["image"][idx[i:i + B]], cpu["label"][idx[i:i + B], 0], cpu["label"][idx[i:i + B], 1]) for i in range(0, len(idx), B)]
            assert len(bat(order[f])[-1][0]) == 1 and any(float(b[2].sum()) == 0 and len(b[2]) == 4 for b in bat(order[f]))
            mean, usable = R.train_epoch(m, bat(order[f]), None)
            vloss, c = R.validate(m, bat(np.arange(22)))
            refs.append(dict(mean=mean, usable=usable, vloss=vloss, c=c, model=m))
        _EPOCH.update(dims=dims, K=K, B=B, cpu=cpu, order=order, base=base, refs=refs)
    return _EPOCH


def _hip_model(state):
    from multimodal_survival_prediction_amd import models as HM
    m = HM.ImageOnlyModel()
    m.load_state_dict(state.state_dict())
    return m.to(DEV)


def _check_fold(E, f, tr, st, va, model):
    ref = E["refs"][f]
    assert abs(tr - ref["mean"]) <= 1e-4 * max(1.0, abs(ref["mean"])), (f, tr, ref["mean"])
    assert st["n_usable"] == ref["usable"] == 4 and st["n_batches"] == 6, (f, st, ref["usable"])
    for (k, x), (_, y) in zip(ref["model"].named_buffers(), model.named_buffers()):
        if "num_batches" in k:
            assert int(x) == int(y) == 6, (f, k)
        else:
            assert rel_err(y, x) <= 1e-4, (f, k)
    assert abs(va[0] - ref["vloss"]) <= 1e-4 * max(1.0, abs(ref["vloss"])), (f, va, ref["vloss"])
    assert va[1] == ref["c"], (f, va[1], ref["c"])


def test_epoch_and_validate_image_match_restated_loop():
    from multimodal_survival_prediction_amd import data, training as T
    E = _epoch_reference()
    cohort = data.cohort_to(E["cpu"], DEV)
    for f in range(E["K"]):
        m = _hip_model(E["base"][f])
        opt = T.FusedOptimizer(m, lr=0.0, weight_decay=1e-4)
        tr = T.train_epoch_image(m, data.BatchLoader(cohort, E["order"][f], E["B"], shuffle=False), opt, DEV)
        st = opt.engine.epoch_stats()
        va = T.validate_image(m, data.BatchLoader(cohort, np.arange(22), E["B"], shuffle=False), DEV)
        _check_fold(E, f, tr, st, va, m)


def test_lockstep_image_epoch_matches_restated_loop_and_sequential():
    """the style "image" of train_epoch_lockstep / validate_lockstep (3 folds as sub-groups on three streams): the same figures as the
    restated loop, hence as the sequential epochs of the test above; the tail of ONE patient forms its own group step"""
    from multimodal_survival_prediction_amd import data, training as T
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    E = _epoch_reference()
    cohort = data.cohort_to(E["cpu"], DEV)
    gm = [_hip_model(E["base"][f]) for f in range(E["K"])]
    ge = FoldGroupEngine(gm, lr=0.0, weight_decay=1e-4)
    loaders = [data.BatchLoader(cohort, E["order"][f], E["B"], shuffle=False) for f in range(E["K"])]
    tr = T.train_epoch_lockstep(ge, loaders, "image", concurrent=3)
    torch.cuda.synchronize()
    assert all(GP.fallback for GP in ge.plans.values()) and any(GP.B == 1 for GP in ge.plans.values())
    st = ge.epoch_stats()
    va = T.validate_lockstep(ge, [data.BatchLoader(cohort, np.arange(22), E["B"], shuffle=False) for _ in range(E["K"])], "image", DEV)
    for f in range(E["K"]):
        _check_fold(E, f, tr[f], st[f], va[f], gm[f])
    # lock-step against sequential, directly: the same folds one engine at a time
    for f in range(E["K"]):
        m = _hip_model(E["base"][f])
        opt = T.FusedOptimizer(m, lr=0.0, weight_decay=1e-4)
        tr_s = T.train_epoch_image(m, data.BatchLoader(cohort, E["order"][f], E["B"], shuffle=False), opt, DEV)
        st_s = opt.engine.epoch_stats()
        va_s = T.validate_image(m, data.BatchLoader(cohort, np.arange(22), E["B"], shuffle=False), DEV)
        assert abs(tr[f] - tr_s) <= 1e-4 * max(1.0, abs(tr_s)), (f, tr[f], tr_s)
        assert st[f]["n_usable"] == st_s["n_usable"] and st[f]["n_batches"] == st_s["n_batches"]
        assert abs(va[f][0] - va_s[0]) <= 1e-4 * max(1.0, abs(va_s[0])) and va[f][1] == va_s[1], (f, va[f], va_s)
        for (k, x), (_, y) in zip(m.named_buffers(), gm[f].named_buffers()):
            assert int(x) == int(y) if "num_batches" in k else rel_err(y, x) <= 1e-4, (f, k)
    # named batches (what the entry point's driver hands the group): one gather launch per step, same figures
    gm2 = [_hip_model(E["base"][f]) for f in range(E["K"])]
    ge2 = FoldGroupEngine(gm2, lr=0.0, weight_decay=1e-4)
    lazy = [data.BatchLoader(cohort, E["order"][f], E["B"], shuffle=False, lazy=True) for f in range(E["K"])]
    tr2 = T.train_epoch_lockstep(ge2, lazy, "image", concurrent=1)
    st2 = ge2.epoch_stats()
    for f in range(E["K"]):
        assert abs(tr2[f] - tr[f]) <= 1e-4 * max(1.0, abs(tr[f])) and st2[f]["n_usable"] == st[f]["n_usable"]
        for (k, x), (_, y) in zip(gm[f].named_buffers(), gm2[f].named_buffers()):
            assert int(x) == int(y) if "num_batches" in k else rel_err(y, x) <= 1e-4, (f, k)


def test_batch_and_width_rules_of_the_engines():
    """one patient trains unless the volume shrinks to a single voxel (torch's BatchNorm3d rule); widths a path cannot run are refused
    by that path with a reason, not by a bare error code from a driver"""
    from multimodal_survival_prediction_amd import models as HM
    from multimodal_survival_prediction_amd.engine import SurvivalEngine
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    eng = SurvivalEngine(HM.ImageOnlyModel().to(DEV).train())
    t, e = torch.ones(1), torch.ones(1)
    with pytest.raises(ValueError, match="single voxel"):
        eng.train_step(torch.rand(1, 1, 8, 8, 8), time=t, event=e)
    eng.train_step(torch.rand(1, 1, 16, 8, 8), time=t, event=e, use_graph=False)       # 2 voxels: legal, no step
    eng.train_step(torch.rand(2, 1, 8, 8, 8), time=torch.tensor([1., 2.]), event=torch.ones(2), use_graph=False)
    torch.cuda.synchronize()
    assert eng.epoch_stats()["n_batches"] == 2 and eng.epoch_stats()["n_usable"] == 1

    def with_widths(w):
        m = HM.ImageOnlyModel()
        layers, ci = [], 1
        for co in w:
            layers += [torch.nn.Conv3d(ci, co, 3, stride=2, padding=1), torch.nn.BatchNorm3d(co), torch.nn.ReLU()]
            ci = co
        m.encoder = torch.nn.Sequential(*layers, torch.nn.AdaptiveAvgPool3d(1))
        m.fc[0] = torch.nn.Linear(w[2], 32)
        return m.to(DEV).train()
    x = torch.rand(2, 1, 8, 8, 4, device=DEV)
    with pytest.raises(ValueError, match="divide 256"):          # 80: group kernels only
        with_widths((16, 80, 64))(x)
    ge = FoldGroupEngine([with_widths((16, 80, 64))])
    (hz, _), = ge.forward_eval([dict(ct=x)], use_graph=False)
    assert hz.shape == (2,) and bool(torch.isfinite(hz).all())
    with pytest.raises(ValueError, match="48 and 112"):
        FoldGroupEngine([with_widths((16, 48, 64))]).forward_eval([dict(ct=x)], use_graph=False)
    with pytest.raises(ValueError, match="multiples of 16"):
        with_widths((16, 24, 64))(x)


# ------------------------------------------------------------------------------------------------------------------
# 9. fused tail: BN3 + ReLU + pool -> Linear + ReLU -> Linear in one launch per pass
# ------------------------------------------------------------------------------------------------------------------
def _tail_case(B, V, C, seed, N1=32, N2=1):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *sh: torch.randn(*sh, generator=gen, dtype=torch.float64).float().double()
    y, dhz = r(B, V, C), r(B, N2)
    gamma, beta = (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5).float().double(), (r(C) * 0.3)
    w1, b1, w2, b2 = [t.requires_grad_(True) for t in (r(N1, C) / np.sqrt(C), r(N1) * 0.1, r(N2, N1) / np.sqrt(N1), r(N2) * 0.1)]
    rows = y.reshape(-1, C)
    mean = rows.mean(0)
    var = (rows * rows).mean(0) - mean * mean
    xh = (y - mean) / torch.sqrt(var + 1e-5)
    z = (gamma * xh + beta).requires_grad_(True)
    feats = torch.relu(z).mean(1)
    f1 = torch.relu(feats @ w1.T + b1)
    hz = f1 @ w2.T + b2
    (hz * dhz).sum().backward()
    gz = z.grad
    ref = dict(feats=feats.detach(), f1=f1.detach(), hz=hz.detach(), dw1=w1.grad, db1=b1.grad, dw2=w2.grad, db2=b2.grad, dbn=gz,
               s1=gz.reshape(-1, C).sum(0), s2=(gz * xh).reshape(-1, C).sum(0))
    f = lambda t: t.detach().float().contiguous().to(DEV)
    d = dict(y=f(y), gamma=f(gamma), beta=f(beta), w1=f(w1), b1=f(b1), w2=f(w2), b2=f(b2), dhz=f(dhz), sum=rows.sum(0).to(DEV),
             sumsq=(rows * rows).sum(0).to(DEV), feats=torch.zeros(B, C + 8, device=DEV), f1=torch.zeros(B, N1, device=DEV),
             hz=torch.zeros(B, N2, device=DEV), dw1=torch.zeros(N1, C, device=DEV), db1=torch.zeros(N1, device=DEV),
             dw2=torch.zeros(N2, N1, device=DEV), db2=torch.zeros(N2, device=DEV), dbn=torch.zeros(B, V, C, device=DEV),
             s1=torch.zeros(C, dtype=torch.float64, device=DEV), s2=torch.zeros(C, dtype=torch.float64, device=DEV))
    return d, ref


def _tail_blocks(S, ops, devs, B, V, C, N1=32, N2=1):
    pool, lf1, lf2, lb1, lb2 = [], [], [], [], []
    for d in devs:
        p = S["FbPoolP"]()
        p.y = d["y"].data_ptr(); p.C = C; p.V = V; p.B = B
        p.bn = ops.bnsrc(d["gamma"], d["beta"], B * V, True, sum=d["sum"], sumsq=d["sumsq"])
        p.out = d["feats"].data_ptr(); p.ldo = d["feats"].stride(0)
        p.dbn = d["dbn"].data_ptr(); p.s1 = d["s1"].data_ptr(); p.s2 = d["s2"].data_ptr()
        pool.append(p)
        pro = ops.inprolog()
        ptr = lambda t: t.data_ptr()
        lf1.append(S["LinearFwdP"](ptr(d["feats"]), d["feats"].stride(0), B, C, pro, ptr(d["w1"]), ptr(d["b1"]), N1, ptr(d["f1"]), N1, 1))
        lf2.append(S["LinearFwdP"](ptr(d["f1"]), N1, B, N1, pro, ptr(d["w2"]), ptr(d["b2"]), N2, ptr(d["hz"]), N2, 0))
        lb1.append(S["LinearBwdP"](None, N1, ptr(d["f1"]), N1, 1, ptr(d["feats"]), d["feats"].stride(0), B, C, pro, ptr(d["w1"]), N1,
                                   ptr(d["dw1"]), ptr(d["db1"]), None, 0, None, None))
        lb2.append(S["LinearBwdP"](ptr(d["dhz"]), N2, ptr(d["hz"]), N2, 0, ptr(d["f1"]), N1, B, N1, pro, ptr(d["w2"]), N2,
                                   ptr(d["dw2"]), ptr(d["db2"]), None, 0, None, None))
    arr = lambda name, xs: (S[name] * len(xs))(*xs)
    return arr("FbPoolP", pool), arr("LinearFwdP", lf1), arr("LinearFwdP", lf2), arr("LinearBwdP", lb1), arr("LinearBwdP", lb2)


@pytest.mark.parametrize("ng", [1, 3])
@pytest.mark.parametrize("B,V,C", [(4, 8, 64), (3, 6, 64)])
def test_fused_tail_matches_torch(B, V, C, ng):
    lib, S, ops = _lib()
    st = ops.stream()
    cases = [_tail_case(B, V, C, 700 + g) for g in range(ng)]          # different weights and inputs per member
    pool, lf1, lf2, lb1, lb2 = _tail_blocks(S, ops, [d for d, _ in cases], B, V, C)
    assert lib.mms_img_tail_fwd_group(pool, lf1, lf2, ng, st) == 0
    assert lib.mms_img_tail_bwd_group(pool, lb1, lb2, ng, st) == 0
    torch.cuda.synchronize()
    for g, (d, ref) in enumerate(cases):
        assert_close(d["feats"][:, :C], ref["feats"], 1e-4, f"feats {g}")
        assert float(d["feats"][:, C:].abs().max()) == 0.0
        for k in ("f1", "hz", "dw1", "db1", "dw2", "db2", "dbn", "s1", "s2"):
            e = rel_err(d[k].reshape(ref[k].shape), ref[k])
            print(f"  tail ({B}, {V}, {C}) ng={ng} member {g} {k}: {e:.2e}")
            assert e <= 1e-4, (g, k, e)
    # blocks that are not the chain: refused, nothing launched
    before = cases[0][0]["hz"].clone()
    lf2[0].x = cases[0][0]["feats"].data_ptr()                           # l2 does not read l1's output
    assert lib.mms_img_tail_fwd_group(pool, lf1, lf2, ng, st) == -1
    lb1[0].out_relu = 0
    assert lib.mms_img_tail_bwd_group(pool, lb1, lb2, ng, st) == -1
    assert lib.mms_img_tail_fwd_group(pool, lf1, None, ng, st) == -1 and lib.mms_img_tail_bwd_group(pool, None, lb2, ng, st) == -1
    assert lib.mms_img_tail_fwd_group(pool, lf1, lf2, 0, st) == -1 and lib.mms_img_tail_fwd_group(pool, lf1, lf2, 11, st) == -1
    torch.cuda.synchronize()
    assert torch.equal(before, cases[0][0]["hz"])


@pytest.mark.parametrize("n_members", [1, 2])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_fused_tail_model_matches_reference_fixture(tag, n_members):
    """the fold group with fused_tail=True (mms_img_forward_group / _backward_group) against the reference-executed fixture"""
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    z = np.load(G8)
    ms = [_fixture_model().to(DEV).train() for _ in range(n_members)]
    ge = FoldGroupEngine(ms, lr=0.0, weight_decay=0.0)          # fused_tail: the default
    ct = torch.tensor(z[tag + ".ct"]).to(DEV)
    GP = ge.plan(ct.shape[0], tuple(ct.shape[-3:]))
    assert GP.img_tail
    for e, P in zip(GP.eng, GP.Ps):
        e.load_batch(P, ct)
    ge._zero(GP)
    ge._forward(GP, True)
    for P in GP.Ps:
        P.dbuf["hz"][:, 0].copy_(torch.tensor(z[tag + ".coef"]))
    ge._backward_from_dhz(GP)
    torch.cuda.synchronize()
    for m, e, P in zip(ms, GP.eng, GP.Ps):
        _check_against_fixture(z, tag, m, e, P)
    for hz, _ in ge.forward_eval([dict(ct=ct)] * n_members):
        assert_close(hz, torch.tensor(z[tag + ".eval_risk"]), 1e-4, "eval risk")


# ------------------------------------------------------------------------------------------------------------------
# 8. entry point end to end
# ------------------------------------------------------------------------------------------------------------------
def test_image_only_entry_point_end_to_end(tmp_path, monkeypatch):
    env = dict(os.environ, MMS_PATIENTS="200", MMS_EPOCHS="2", MMS_FOLDS="3", MMS_BATCH_SIZE="4", MMS_VOLUME="16,16,8")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "training", "image_only_training.py")], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    res = json.load(open(tmp_path / "results" / "image_only" / "cv_results.json"))
    assert set(res) >= {"c_index_mean", "c_index_std", "fold_results"}
    folds = res["fold_results"]
    assert [f["fold"] for f in folds] == [1, 2, 3] and all(set(f) >= {"fold", "best_c_index"} and 0.0 <= f["best_c_index"] <= 1.0 for f in folds)
    assert abs(res["c_index_mean"] - np.mean([f["best_c_index"] for f in folds])) < 1e-12
    assert res["patients"] == sum(f["val_size"] for f in folds) >= 12
    # a checkpoint loads into the restated class
    ckpt = tmp_path / "models" / "image_only" / "fold_2_best.pth"
    sd = torch.load(ckpt, map_location="cpu")
    ref = R.ImageOnlyModel()
    ref.load_state_dict(sd, strict=True)
    # final_comparison lists the model
    sys.path.insert(0, os.path.join(ROOT, "scripts", "training"))
    try:
        import importlib
        fc = importlib.import_module("final_comparison")
    finally:
        sys.path.pop(0)
    got = fc.collect(str(tmp_path))
    assert "Image-Only" in got and len(got["Image-Only"]["fold_values"]) == 3
    # evaluate_model.py --model image_only --predict: the checkpoint's eval forward on the fold's held-out patients
    from test_gpu_evaluate import _load
    from multimodal_survival_prediction_amd import data
    em = _load()
    for k in ("MMS_PATIENTS", "MMS_FOLDS", "MMS_BATCH_SIZE", "MMS_VOLUME"):
        monkeypatch.setenv(k, env[k])
    s = em.main(["--predict", str(ckpt), "--model", "image_only", "--fold", "2", "--predictions", str(tmp_path / "pred.csv"),
                 "--outdir", str(tmp_path / "out"), "--no-plots"])
    import pandas as pd
    df = pd.read_csv(tmp_path / "pred.csv")
    assert len(df) == s["test_patients"] == folds[1]["val_size"]
    cohort = data.make_cohort(n=200, dims=(16, 16, 8), seed=608, complete=False)
    usable = np.nonzero(cohort["has_survival"].numpy() & (cohort["mask"].numpy()[:, 0] != 0))[0]
    _, val = data.kfold_indices(len(usable), 3, seed=42)[1]
    ref.eval()
    with torch.no_grad():
        want = ref(cohort["image"][torch.as_tensor(usable[val])]).numpy()
    assert np.abs(df["risk_score"].to_numpy() - want).max() <= 1e-4 * max(1.0, np.abs(want).max())
