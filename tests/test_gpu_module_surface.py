"""The torch-facing surface of an engine-owned DenseNet121 model (models.py's promise: parameters stay ordinary torch leaves).

Weight changes from outside the fused step -- load_state_dict, p.copy_(), p.mul_(), torch.optim.SGD / Adam -- must reach the derived
conv2 packs before the next launch (SurvivalEngine.sync_packs, engine._weights_token): the packs are compared bit for bit with the
stand-alone pack kernels on the current weights, the eval hazards and a training step with the CPU oracle / a fresh engine on the same
weights.  A write through p.data moves no version counter: only sync_packs(force=True) is pinned for it.

One workspace per (batch size, volume size): a backward whose forward is no longer the latest on its workspace raises, and so does a
second backward over the same forward (DESIGN.md "Weight changes and the module surface").

Shapes: the smallest with MFMA-fragment-pack layers (volume 32x32x32: dense blocks 2 and 3, layers 6..41); B = 2 in eval mode, B = 8 in
training mode (block 4 then normalises over 8 rows, the floor tests/test_gpu_densenet.py::test_transition_prepass_equals_fused_form
explains).  Every case first runs one forward through the engine, so that the packs exist and the stored token is current."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, assert_close, assert_conv2_packs_current, rel_err
from test_gpu_dead_backward import SPREAD, _spread
from test_gpu_densenet import _make, structured_volumes
from test_gpu_models import _grad_stats

DIMS, RNA = (32, 32, 32), 64
FRAG_COPY, FRAG_MUL, PLAIN_MUL = 7, 15, 57      # conv2 layers (0..57): two with a fragment pack (block 2), one without (block 4's last)
LR = 0.02                                      # conv2 weights have std 0.036 (kaiming), the hand-set gradients std 1: a step of O(1) of the weights
LAST = "ct_encoder.features.denseblock4.denselayer16.layers.conv2.weight"


def _no_dropout(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def _oracle(seed=None, state=None):
    from oracle import models as OM
    if seed is not None:
        torch.manual_seed(seed)
    m = _no_dropout(OM.MultiModalSurvivalNet(rna_dim=RNA, use_monai=True))
    if state is not None:
        m.load_state_dict({k: v.detach().cpu() for k, v in state.items()})
    return m


def _hip(state):
    from multimodal_survival_prediction_amd import models as HM
    net = _no_dropout(HM.MultiModalSurvivalNet(rna_dim=RNA))
    net.load_state_dict(state)
    return net.to(DEV)


def _inputs(B, seed=3):
    g = torch.Generator().manual_seed(seed)
    return structured_volumes(B, DIMS, seed), torch.randn(B, RNA, generator=g), torch.rand(B, 1, generator=g)


def _w2(model):
    """the 58 conv2 weights in layer order"""
    ws = [p for k, p in model.named_parameters() if k.endswith("layers.conv2.weight")]
    assert len(ws) == 58
    return ws


_BASE = {}


def _base():
    """Two random oracle models' weights, the eval inputs and the first model's oracle hazards: computed once, never changed."""
    if not _BASE:
        ref = _oracle(seed=5).eval()
        x = _inputs(2)
        with torch.no_grad():
            h0 = ref(*x)
        _BASE.update(sd0={k: v.clone() for k, v in ref.state_dict().items()}, sd1={k: v.clone() for k, v in _oracle(seed=77).state_dict().items()},
                     x=x, h0=h0)
    return _BASE


# ---- the changes (each takes the live HIP model) ------------------------------------------------------------------------------------------
def _ch_load(net):
    net.load_state_dict(_base()["sd1"])


def _ch_copy(net):
    w = _w2(net)[FRAG_COPY]
    new = torch.randn(w.shape, generator=torch.Generator().manual_seed(7)) * (3 * 0.036)
    with torch.no_grad():
        w.copy_(new.to(DEV))


def _ch_mul(net):
    ws = _w2(net)
    with torch.no_grad():
        ws[FRAG_MUL].mul_(-1.5)
        ws[PLAIN_MUL].mul_(-1.5)


def _ch_opt(make):
    def change(net):
        ws = _w2(net)
        g = torch.Generator().manual_seed(11)
        for w in ws:
            w.grad = torch.randn(w.shape, generator=g).to(DEV)
        make(ws).step()
        for w in ws:
            w.grad = None
    return change


CHANGES = {
    "load_state_dict": _ch_load,
    "copy_": _ch_copy,
    "mul_": _ch_mul,
    "sgd_step": _ch_opt(lambda ws: torch.optim.SGD(ws, lr=LR)),
    "adam_step_foreach": _ch_opt(lambda ws: torch.optim.Adam(ws, lr=LR, foreach=True)),
    "adam_step_single": _ch_opt(lambda ws: torch.optim.Adam(ws, lr=LR, foreach=False)),
}
KINDS = sorted(CHANGES)


def _live(B=2, use_graph=False, state=None):
    """A HIP model with a live engine: one eval forward done (twice through the graph with use_graph: captured, then replayed)."""
    from multimodal_survival_prediction_amd.engine import engine_of
    b = _base()
    net = _hip(b["sd0"] if state is None else state).eval()
    eng = engine_of(net)
    x = b["x"] if B == 2 else _inputs(B, seed=4)
    for _ in range(2 if use_graph else 1):
        hz, _g = eng.forward_eval(*[t.to(DEV) for t in x], use_graph=use_graph)
    hz = hz.clone()
    assert eng.w2["fragmask"] != 0
    assert (eng.w2["fragmask"] >> FRAG_COPY) & 1 and (eng.w2["fragmask"] >> FRAG_MUL) & 1 and not (eng.w2["fragmask"] >> PLAIN_MUL) & 1
    return net, eng, x, hz


def _eval(eng, x, use_graph=False):
    return eng.forward_eval(*[t.to(DEV) for t in x], use_graph=use_graph)[0].clone()


@pytest.mark.parametrize("kind", KINDS)
def test_packs_follow_weight_change(kind):
    """After the change and ONE forward_eval: every derived pack is the pack of the current weights, bit for bit."""
    net, eng, x, _ = _live()
    before = [w.detach().clone() for w in _w2(net)]
    CHANGES[kind](net)
    assert any(not torch.equal(a, w.detach()) for a, w in zip(before, _w2(net)))
    _eval(eng, x)
    assert_conv2_packs_current(eng)


@pytest.mark.parametrize("kind,use_graph", [(k, False) for k in KINDS] + [("mul_", True)])
def test_eval_hazards_follow_weight_change(kind, use_graph):
    """Eval hazards after the change against a fresh ORACLE model holding the HIP model's state_dict, at the project's 1e-4.  That this can
    fail is shown on the oracle alone: its hazards before and after the change differ by >= 1e-2 (100 x the tolerance) -- and still do when
    only the layers WITH a forward fragment pack keep their old weights, which is what an engine with stale packs computes (the other
    layers' forwards read the primary storage).  use_graph: the eval graph was captured and replayed before the change; the replay after
    it must see the new packs."""
    b = _base()
    net, eng, x, hz0 = _live(use_graph=use_graph)
    assert_close(hz0, b["h0"], 1e-4, "eval hazards before the change")
    CHANGES[kind](net)
    got = _eval(eng, x, use_graph)
    ref = _oracle(state=net.state_dict()).eval()
    with torch.no_grad():
        want = ref(*x)
        for i, (w, w_old) in enumerate(zip(_w2(ref), _w2(_oracle(state=b["sd0"])))):
            if (eng.w2["fragmask"] >> i) & 1:
                w.copy_(w_old)
        stale = ref(*x)
    moved, moved_stale = rel_err(want, b["h0"]), rel_err(want, stale)
    print(f"{kind}: oracle hazards moved by {moved:.2e} (vs old fragment-layer weights: {moved_stale:.2e}); HIP vs oracle {rel_err(got, want):.2e}")
    assert moved >= 1e-2 and moved_stale >= 1e-2, (moved, moved_stale)
    assert_close(got, want, 1e-4, f"eval hazards after {kind}")


def test_data_write_needs_force():
    """A write through p.data moves no version counter (tests/test_cpu_param_versions.py::test_data_write_is_invisible): what is pinned
    is that sync_packs(force=True) repairs the packs -- not that they are stale before it."""
    b = _base()
    net, eng, x, _ = _live()
    _w2(net)[FRAG_MUL].data.mul_(-1.5)
    eng.sync_packs(force=True)
    got = _eval(eng, x)
    assert_conv2_packs_current(eng)
    ref = _oracle(state=net.state_dict()).eval()
    with torch.no_grad():
        want = ref(*x)
    assert rel_err(want, b["h0"]) >= 1e-2
    assert_close(got, want, 1e-4, "eval hazards after a .data write and sync_packs(force=True)")


def _train_batch(B=8):
    g = torch.Generator().manual_seed(21)
    ct, rna, clin = _inputs(B, seed=4)
    return ct, rna, clin, torch.rand(B, generator=g) * 10 + 0.5, (torch.arange(B) % 3 != 1).float()


def _train_backward(net, batch):
    from multimodal_survival_prediction_amd import losses as HL
    ct, rna, clin, t, e = [v.to(DEV) for v in batch]
    net.train()
    hz = net(ct, rna, clin)
    HL.cox_loss(hz, e, t).backward()
    torch.cuda.synchronize()
    return hz


def _oracle_backward(state, batch):
    from oracle import losses as OL
    ref = _oracle(state=state).train()
    ct, rna, clin, t, e = batch
    OL.cox_loss(ref(ct, rna, clin), e, t).backward()
    return ref


def test_training_step_follows_weight_change():
    """load_state_dict on a live engine, then one training-mode forward + backward on the autograd path: every gradient tensor against a
    FRESH model and engine built from the same state_dict, at the spread of two runs of the same code (test_gpu_models.py::
    test_run_twice_spread, per tensor relative to its maximum, same small-tensor rule) -- the backward-data packs of all 58 layers are in
    it; and the last conv2 layer's weight gradient against the oracle at 2e-4 (as tests/test_gpu_w2pack.py::test_packed_model_surface)."""
    b, batch = _base(), _train_batch()
    net, eng, _, _ = _live(B=8)
    net.load_state_dict(b["sd1"])
    _train_backward(net, batch)
    fresh = _hip(b["sd1"])
    _train_backward(fresh, batch)
    worst = _spread([p.grad for p in net.parameters()], [p.grad.clone() for p in fresh.parameters()])
    print(f"training step after load_state_dict on a live engine vs a fresh engine: worst per-tensor gradient difference {worst:.2e}")
    assert worst <= SPREAD
    ref = _oracle_backward(b["sd1"], batch)
    assert_close(dict(net.named_parameters())[LAST].grad, dict(ref.named_parameters())[LAST].grad, 2e-4, "last conv2 weight gradient")


def test_group_member_follows_weight_change():
    """A fold group of two: load_state_dict on member 1 only.  Member 1 follows (oracle on its new weights, 1e-4); member 0's hazards are
    bit for bit what they were."""
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    b = _base()
    nets = [_hip(b["sd0"]).eval(), _hip(_oracle(seed=31).state_dict()).eval()]
    ge = FoldGroupEngine(nets)
    batches = [dict(ct=b["x"][0], rna=b["x"][1], clinical=b["x"][2]) for _ in range(2)]
    first = [hz.clone() for hz, _ in ge.forward_eval(batches)]
    for e in ge.engines:
        assert e.w2["fragmask"] != 0
    assert_close(first[0], b["h0"], 1e-4, "member 0 before")
    nets[1].load_state_dict(b["sd1"])
    second = [hz.clone() for hz, _ in ge.forward_eval(batches)]
    ref = _oracle(state=b["sd1"]).eval()
    with torch.no_grad():
        want = ref(*b["x"])
    assert rel_err(want, first[1].cpu()) >= 1e-2          # (the member's hazards had to move)
    assert_close(second[1], want, 1e-4, "member 1 after load_state_dict")
    assert torch.equal(second[0], first[0])
    for e in ge.engines:
        assert_conv2_packs_current(e)


# ---- one workspace per (batch size, volume size) ------------------------------------------------------------------------------------------
def test_backward_of_an_overwritten_forward_raises():
    """SurvivalEngine.plan keys a workspace by (batch size, volume size): training and eval forwards, with or without gradients, share it
    at equal shapes; another batch size has its own.  net(x1); net(x2): the backward through the first raises and touches nothing, the
    backward through the second is what it always was -- head gradients at 1e-4 and the last conv2 gradient at 2e-4 against the oracle.
    An eval-mode no_grad forward at the same shape between a training forward and its backward raises too; one at another batch size
    does not."""
    from multimodal_survival_prediction_amd import losses as HL
    b = _base()
    batch1, batch2 = _train_batch(), tuple(torch.flip(v, dims=[0]).contiguous() for v in _train_batch())
    net = _hip(b["sd0"]).train()
    d = lambda batch: [v.to(DEV) for v in batch]
    ct1, rna1, clin1, t1, e1 = d(batch1)
    ct2, rna2, clin2, t2, e2 = d(batch2)
    h1 = net(ct1, rna1, clin1)
    h2 = net(ct2, rna2, clin2)
    with pytest.raises(RuntimeError, match="another forward ran on this model's workspace"):
        HL.cox_loss(h1, e1, t1).backward()
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in net.parameters())
    HL.cox_loss(h2, e2, t2).backward()
    torch.cuda.synchronize()
    ref = _oracle_backward(b["sd0"], batch2)
    # (head gradients: the strict criterion and small-tensor rule of tests/test_gpu_models.py::test_model_parity_autograd_path)
    hmax = _grad_stats(ref, net)[3]
    assert hmax <= 1e-4, hmax
    assert_close(dict(net.named_parameters())[LAST].grad, dict(ref.named_parameters())[LAST].grad, 2e-4, "last conv2 weight gradient")
    # an eval-mode no_grad forward on the same plan
    h1 = net(ct1, rna1, clin1)
    net.eval()
    with torch.no_grad():
        net(ct2, rna2, clin2)
    net.train()
    with pytest.raises(RuntimeError, match="another forward ran on this model's workspace"):
        HL.cox_loss(h1, e1, t1).backward()
    # ... and on another plan (B = 2): the training forward's workspace is untouched
    h1 = net(ct1, rna1, clin1)
    net.eval()
    with torch.no_grad():
        net(ct2[:2], rna2[:2], clin2[:2])
    net.train()
    net.zero_grad(set_to_none=False)
    HL.cox_loss(h1, e1, t1).backward()
    torch.cuda.synchronize()
    ref = _oracle_backward(b["sd0"], batch1)
    assert_close(dict(net.named_parameters())[LAST].grad, dict(ref.named_parameters())[LAST].grad, 2e-4, "last conv2 weight gradient")


def test_second_backward_over_one_forward_raises():
    """The encoder's backward ADDS its BatchNorm-backward sums into accumulators that only a training forward zeroes (csrc/dn_net.hip: bb_y0,
    bb_y1, bb_in, bb_tr inside [stats_begin_packed, stats_end)), so a second backward over the same forward would normalise with doubled
    sums: it raises instead (decision recorded in DESIGN.md).  Whole model and stand-alone encoder; the first backward is unaffected."""
    from multimodal_survival_prediction_amd import losses as HL
    b, batch = _base(), _train_batch()
    net = _hip(b["sd0"]).train()
    ct, rna, clin, t, e = [v.to(DEV) for v in batch]
    hz = net(ct, rna, clin)
    HL.cox_loss(hz, e, t).backward(retain_graph=True)
    torch.cuda.synchronize()
    ref = _oracle_backward(b["sd0"], batch)
    assert_close(dict(net.named_parameters())[LAST].grad, dict(ref.named_parameters())[LAST].grad, 2e-4, "last conv2 weight gradient")
    with pytest.raises(RuntimeError, match="second backward over the same forward"):
        (2.0 * hz.sum()).backward()
    _, enc = _make(3)
    enc.train()
    x = structured_volumes(8, DIMS, 9).to(DEV)
    g = torch.Generator().manual_seed(2)
    y = enc(x)
    y.backward(torch.randn(8, 128, generator=g).to(DEV), retain_graph=True)
    with pytest.raises(RuntimeError, match="second backward over the same forward"):
        y.backward(torch.randn(8, 128, generator=g).to(DEV))


def test_encoder_backward_of_an_overwritten_forward_raises():
    """The stand-alone DenseNet121 module keeps ONE workspace (the latest input shape's): a second forward, whatever its mode or shape,
    takes it over, and the backward through the first raises; the backward through the second runs."""
    _, enc = _make(3)
    enc.train()
    x1, x2 = structured_volumes(8, DIMS, 9).to(DEV), structured_volumes(8, DIMS, 10).to(DEV)
    dout = torch.randn(8, 128, generator=torch.Generator().manual_seed(2)).to(DEV)
    y1 = enc(x1)
    y2 = enc(x2)
    with pytest.raises(RuntimeError, match="another forward ran on this model's workspace"):
        y1.backward(dout)
    y2.backward(dout)
    y1 = enc(x1)
    with torch.no_grad():
        enc(x2[:2])                                   # another shape: the module's workspace is re-made for it
    with pytest.raises(RuntimeError, match="another forward ran on this model's workspace"):
        y1.backward(dout)
    torch.cuda.synchronize()
