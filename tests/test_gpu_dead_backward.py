"""Dead-backward skip (MmsDnOpts.skip_dead_bwd, include/mmsurv.h): when the feature gradient `dout` of a model is exactly zero -- a batch
without a CT under PartialModalityNet's modality mask -- every launch of the DenseNet backward behind the head returns at once.

What must hold, and is checked here against the full backward (skip_dead_bwd = -1):
  * the full backward of a zero dout adds exact zeros (so skipping it changes nothing), and the skipped one touches nothing;
  * one element of magnitude 1e-30 anywhere in dout makes the step live (NaN would too; -0.0f does not);
  * in a fold group the test is per member;
  * nothing goes stale on a workspace that alternates dead and live steps, through one captured graph;
  * the SyncBN / staged drivers neither write nor read the word.

Tolerance of every "agrees" below: the run-to-run spread the suite allows for fp32 / fp64 atomic accumulation, as
tests/test_gpu_models.py::test_run_twice_spread states it -- every gradient tensor within 1e-4 of its maximum, tensors below 1e-5 of the
largest gradient (rounding noise only) left out.  The two sides of each comparison run the same kernels on the same saved activations, so
no ReLU mask can differ between them.

Shapes: B = 8, 32x32x32 (8 rows in block 4: the per-layer and tap-split forms) and B = 4, 64x64x32 (the block-4 cluster kernel, the
multi-tap block-1 kernels, the table-fed weight gradients), as tests/test_gpu_densenet.py.
"""
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, rel_err
from test_gpu_densenet import _make, structured_volumes

SHAPES = [(8, (32, 32, 32)), (4, (64, 64, 32))]
SPREAD = 1e-4          # tests/test_gpu_models.py::test_run_twice_spread


def _live_word(net_or_ws, dims4=None):
    """The workspace's "bwd_live" word (mms_dn121_region) as a 1-element int32 view."""
    if dims4 is None:
        return net_or_ws.workspace_region("bwd_live", 0, torch.int32)
    from multimodal_survival_prediction_amd import _lib
    off, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.check(_lib.load_library().mms_dn121_region(*dims4, b"bwd_live", 0, ctypes.byref(off), ctypes.byref(nb)), "mms_dn121_region")
    assert nb.value == 4
    return net_or_ws[off.value:off.value + 4].view(torch.int32)


def _pattern(net):
    """A fixed non-zero pattern in every .grad (the drivers accumulate into the caller's buffers)."""
    for i, p in enumerate(net.parameters()):
        n = p.numel()
        v = (torch.arange(n, dtype=torch.float32) % 7 + 1.0) * (0.125 if i % 2 else -0.375)
        p.grad = v.view_as(p).to(p.device).contiguous()
    return [p.grad.clone() for p in net.parameters()]


def _zero_grads(net):
    for p in net.parameters():
        p.grad = torch.zeros_like(p)


def _grads(net):
    return [p.grad.detach().clone() for p in net.parameters()]


def _spread(got, want):
    """worst per-tensor difference, relative to the tensor's maximum, over the tensors test_run_twice_spread compares"""
    gmax = max(float(g.abs().max()) for g in want)
    worst = 0.0
    for a, b in zip(want, got):
        if float(a.abs().max()) < 1e-5 * gmax:
            continue
        worst = max(worst, rel_err(b, a))
    return worst


_CASE = {}


def _case(B, dims):
    """One network, input, train forward and workspace snapshot per shape, shared by the single-model tests (left unchanged: every
    test restores the snapshot before its backward, so each backward sees the forward's zero-filled accumulators)."""
    key = (B, dims)
    if key not in _CASE:
        _, net = _make(7)
        net.train()
        x = structured_volumes(B, dims, 17).to(DEV)
        net.dn_opts = {}
        net._run_forward(x)
        torch.cuda.synchronize()
        _CASE[key] = dict(net=net, x=x, ws=net._eng["ws"].clone())
    c = _CASE[key]
    c["net"]._eng["ws"].copy_(c["ws"])
    return c


def _backward(c, dout, word=77, **opts):
    """Single-model backward on the shared case: workspace back to its state after the forward, the live word preset to `word`."""
    c["net"]._eng["ws"].copy_(c["ws"])
    _live_word(c["net"]).fill_(word)
    c["net"].dn_opts = dict(opts)
    c["net"]._run_backward(c["x"], dout)
    torch.cuda.synchronize()
    c["net"].dn_opts = {}


@pytest.mark.parametrize("B,dims", SHAPES)
def test_zero_dout_bitwise(B, dims):
    """dout = 0 into a pattern-filled gradient buffer: default and skip_dead_bwd = -1 both leave the pattern, bit for bit -- the second
    run proves that the full backward adds exact zeros, the first that the skip touches nothing; the word reads 0 / is not written."""
    c = _case(B, dims)
    net = c["net"]
    dout = torch.zeros(B, 128, device=DEV)
    res = {}
    for flag in (0, -1):
        want = _pattern(net)
        _backward(c, dout, skip_dead_bwd=flag)
        res[flag] = _grads(net)
        word = int(_live_word(net)[0])
        assert word == (0 if flag == 0 else 77), (flag, word)          # (-1: the head launch is given no word)
        for k, (a, b) in enumerate(zip(want, res[flag])):
            assert torch.equal(a, b), (flag, k)
    for a, b in zip(res[0], res[-1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("where", ["first", "last", "row_B-1_negzero_elsewhere"])
@pytest.mark.parametrize("B,dims", SHAPES)
def test_one_nonzero_element_is_live(B, dims, where):
    c = _case(B, dims)
    net = c["net"]
    dout = torch.zeros(B, 128, device=DEV)
    if where == "first":
        dout[0, 0] = 1e-30
    elif where == "last":
        dout[B - 1, 127] = -1e-30
    else:
        dout.fill_(-0.0)
        dout[B - 1, 61] = 1e-30
    res = {}
    for flag in (-1, 0):
        _zero_grads(net)
        _backward(c, dout, skip_dead_bwd=flag)
        res[flag] = _grads(net)
        if flag == 0:
            assert int(_live_word(net)[0]) == 1
    assert max(float(g.abs().max()) for g in res[-1]) > 0.0
    worst = _spread(res[0], res[-1])
    print(f"one element ({where}), B={B}: worst per-tensor difference skip-on vs skip-off {worst:.2e}")
    assert worst <= SPREAD


def test_negative_zero_and_nan():
    """-0.0f everywhere is a dead step; a NaN is a live one (the comparison is `!= 0.0f`)."""
    B, dims = SHAPES[0]
    c = _case(B, dims)
    net = c["net"]
    want = _pattern(net)
    _backward(c, torch.full((B, 128), -0.0, device=DEV))
    assert int(_live_word(net)[0]) == 0
    for a, b in zip(want, _grads(net)):
        assert torch.equal(a, b)
    d = torch.zeros(B, 128, device=DEV)
    d[3, 5] = float("nan")
    _zero_grads(net)
    _backward(c, d)
    assert int(_live_word(net)[0]) == 1


# ---- group of two ---------------------------------------------------------------------------------------------------------------
def _ptrs(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


@pytest.mark.parametrize("B,dims", SHAPES)
def test_group_of_two_one_dead(B, dims):
    """mms_dn121_backward_group with one dead and one live member, both ways round: the live member's gradients match its own
    single-model backward (on the same saved activations: the workspace is restored to its state after the group forward), the dead
    member's pattern-filled buffer is untouched, bit for bit."""
    from multimodal_survival_prediction_amd import _lib
    lib = _lib.load_library()
    nets, xs, es = [], [], []
    for g in range(2):
        _, net = _make(20 + g)
        net.train()
        x = structured_volumes(B, dims, 30 + g).to(DEV)
        nets.append(net); xs.append(x); es.append(net._tables(x))
    D, H, W = dims
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    opts = nets[0]._opts()
    outs = [torch.empty(B, 128, device=DEV) for _ in range(2)]
    ws, xp = _ptrs([e["ws"].data_ptr() for e in es]), _ptrs([x.data_ptr() for x in xs])
    pt, bt = _ptrs([ctypes.addressof(e["ptab"]) for e in es]), _ptrs([ctypes.addressof(e["btab"]) for e in es])
    _lib.check(lib.mms_dn121_forward_group(2, ws, B, D, H, W, xp, pt, bt, _ptrs([o.data_ptr() for o in outs]), 128, 1, ctypes.byref(opts), st),
               "mms_dn121_forward_group")
    torch.cuda.synchronize()
    snap = [e["ws"].clone() for e in es]
    live = torch.randn(B, 128, generator=torch.Generator().manual_seed(5)).to(DEV)
    zero = torch.zeros(B, 128, device=DEV)
    for dead in (0, 1):
        alive = 1 - dead
        for e, s in zip(es, snap):
            e["ws"].copy_(s)
        want_dead = _pattern(nets[dead])
        _zero_grads(nets[alive])
        douts = [zero, zero]
        douts[alive] = live
        gt = [net._grad_table() for net in nets]
        _lib.check(lib.mms_dn121_backward_group(2, ws, B, D, H, W, xp, pt, _ptrs([d.data_ptr() for d in douts]), 128,
                                                _ptrs([ctypes.addressof(t) for t in gt]), ctypes.byref(opts), st), "mms_dn121_backward_group")
        torch.cuda.synchronize()
        assert int(_live_word(es[dead]["ws"], (B, D, H, W))[0]) == 0 and int(_live_word(es[alive]["ws"], (B, D, H, W))[0]) == 1
        for k, (a, b) in enumerate(zip(want_dead, _grads(nets[dead]))):
            assert torch.equal(a, b), (dead, k)
        got = _grads(nets[alive])
        es[alive]["ws"].copy_(snap[alive])
        _zero_grads(nets[alive])
        nets[alive]._run_backward(xs[alive], live)
        torch.cuda.synchronize()
        worst = _spread(got, _grads(nets[alive]))
        print(f"group of two, member {dead} dead, B={B}: live member vs its single-model backward, worst per-tensor difference {worst:.2e}")
        assert worst <= SPREAD


# ---- a sequence on one workspace, through a captured graph ----------------------------------------------------------------------------
def _masked_cohort(dims, rna_dim):
    """16 patients, the first 8 with a CT, the last 8 without (all-zero volume, mask column 0) -- the convention of data.make_cohort."""
    from multimodal_survival_prediction_amd import data
    c = data.make_cohort(n=16, dims=dims, rna_dim=rna_dim, seed=11, complete=True)
    c["image"][8:] = 0.0
    c["mask"][8:, 0] = 0.0
    c["label"][:, 1] = torch.tensor([1.0, 0.0] * 8)            # events in every batch of four consecutive patients
    c = data.cohort_to(c, DEV)
    c["valid"] = c["has_survival"].float()
    return c


def _seq_models(rna_dim):
    """Two PartialModalityNet members with no all-zero parameter tensor (every tensor's maximum is >= ~0.05, so 'within 1e-4 of the
    tensor's maximum' is defined for every parameter) and dropout off."""
    from multimodal_survival_prediction_amd import models as HM
    out = []
    for g in range(2):
        torch.manual_seed(300 + g)
        m = HM.PartialModalityNet(rna_dim=rna_dim)
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, (torch.nn.BatchNorm3d, torch.nn.BatchNorm1d)):
                    mod.weight.uniform_(0.5, 1.5); mod.bias.normal_(0, 0.1)
                if isinstance(mod, torch.nn.Dropout):
                    mod.p = 0.0
            for p in m.parameters():
                if float(p.abs().max()) < 0.05:
                    p.normal_(0, 0.1)
        out.append(m)
    return out


def _tensors(engine, flat):
    """A copy of an engine's flat gradient cut into its per-parameter pieces."""
    base = engine.gflat.storage_offset()
    return [flat[v.storage_offset() - base:v.storage_offset() - base + v.numel()] for v in engine.gviews]


_SEQ_STEPS = [([[8, 9, 10, 11], [0, 1, 2, 3]], (0, 1)), ([[4, 5, 6, 7], [12, 13, 14, 15]], (1, 0)),
              ([[12, 13, 14, 15], [4, 5, 6, 7]], (0, 1))]          # (patient indices per member, live flag per member): 0 = no CT in the batch
_SEQ = {}


def _sequence_runs(lr=1e-7):
    """The three steps once with the default and once with skip_dead_bwd = -1, from the same seeded state; computed once per learning
    rate, shared by the tests below and left unchanged."""
    if lr in _SEQ:
        return _SEQ[lr]
    _SEQ[lr] = out = {}
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    B, dims, rna_dim = 4, (64, 64, 32), 64
    cohort = _masked_cohort(dims, rna_dim)
    base = _seq_models(rna_dim)
    for flag in (0, -1):
        ge = FoldGroupEngine([copy.deepcopy(m).to(DEV).train() for m in base], lr=lr, weight_decay=1e-4, dn_opts=dict(skip_dead_bwd=flag))
        losses, grads, words = [], [], []
        for idx, _ in _SEQ_STEPS:
            ge.reset_epoch_stats()
            ge.train_step_indexed(cohort, idx, skip_if_unusable=False, use_graph=True)
            torch.cuda.synchronize()
            losses.append([s["sum_loss"] for s in ge.epoch_stats()])
            grads.append([e.gflat.clone() for e in ge.engines])
            GP = next(iter(ge.plans.values()))
            words.append([int(_live_word(P.ws, (B,) + dims)[0]) for P in GP.Ps])
        out[flag] = dict(ge=ge, losses=losses, grads=grads, words=words)
    return out


def test_dead_live_sequence_through_graph():
    """FoldGroupEngine, two PartialModalityNet members, three graph-replayed steps: member 0 dead, live, dead; member 1 live, dead, live.
    Default against skip_dead_bwd = -1 from the same state: the words, the losses, the parameters and BatchNorm buffers after the three
    steps.  After a member's own dead step every gradient tensor is identical bit for bit in the two runs -- the encoder's (untouched
    zeros), every head's and the gate's, which dout does not gate (test_dead_step_gradient_buffer_bitwise below compares the whole flat
    buffer; here tensor by tensor, so a failure names its tensor).

    lr = 1e-7: an Adam step moves an element by at most ~3 lr whatever the gradient's size ((1 - b1) / sqrt(1 - b2) = 3.2), and an element
    whose gradient is rounding noise may move the other way in the other run, so two correct runs differ by up to 3 steps x 2 x 3.2 lr =
    1.9e-6 per element -- below 1e-4 of every tensor's maximum (>= 0.05, _seq_models), which is the bound asked of the parameters.
    Losses: the run-to-run spread of the hazards is 1e-6 (test_run_twice_spread); a Cox loss over 4 rows is a sum of <= 8 terms of them."""
    runs = _sequence_runs()
    a, b = runs[0], runs[-1]
    assert a["words"] == [list(lv) for _, lv in _SEQ_STEPS], a["words"]
    names = [k for k, _ in a["ge"].engines[0].model.named_parameters()]
    for it, (_, lv) in enumerate(_SEQ_STEPS):
        for g in range(2):
            la, lb = a["losses"][it][g], b["losses"][it][g]
            assert abs(la - lb) <= 1e-5 * max(1.0, abs(lb)), (it, g, la, lb)
            ta, tb = _tensors(a["ge"].engines[g], a["grads"][it][g]), _tensors(b["ge"].engines[g], b["grads"][it][g])
            assert len(ta) == len(names)
            if not lv[g]:
                for k, u, v in zip(names, ta, tb):
                    assert torch.equal(u, v), (it, g, k, float((u - v).abs().max()))
                    if k.startswith("ct_encoder."):
                        assert float(u.abs().max()) == 0.0, (it, g, k)             # the step's zero-fill, untouched
                assert max(float(u.abs().max()) for k, u in zip(names, ta) if not k.startswith("ct_encoder.")) > 0.0      # (the heads did get a gradient)
    for g in range(2):
        ma, mb = a["ge"].engines[g].model, b["ge"].engines[g].model
        for (k, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
            assert rel_err(p, q) <= SPREAD, (g, k, rel_err(p, q))
        for (k, p), (_, q) in zip(ma.named_buffers(), mb.named_buffers()):
            if "num_batches" in k:
                assert int(p) == int(q) == 3, k
            else:
                assert rel_err(p, q) <= SPREAD, (g, k, rel_err(p, q))


def test_live_step_after_dead_step_finds_what_it_needs():
    """The same sequence at lr = 0 (frozen weights; the BatchNorm buffers and the Adam moments still move): both runs then hold the same
    parameters at every step, so no ReLU mask can differ between them, and the gradients of EVERY step -- the live steps that follow a
    dead step on the same workspace, and the dead steps that follow a live one -- agree within the run-to-run spread.  A buffer gone
    stale across a skipped backward would show here.  (With lr > 0 the two runs' parameters part by an Adam step on every element whose
    gradient is rounding noise, and from the second step on a ReLU input within that distance of zero may take the other sign: single
    tensors then move by 1e-2 .. 1e-1 of their maximum, the flip lottery of tests/test_gpu_densenet.py -- measured here: 9.2e-2 on one
    tensor of member 1 at step 2.)"""
    runs = _sequence_runs(lr=0.0)
    a, b = runs[0], runs[-1]
    assert a["words"] == [list(lv) for _, lv in _SEQ_STEPS], a["words"]
    for it, (_, lv) in enumerate(_SEQ_STEPS):
        for g in range(2):
            la, lb = a["losses"][it][g], b["losses"][it][g]
            assert abs(la - lb) <= 1e-5 * max(1.0, abs(lb)), (it, g, la, lb)
            worst = _spread(_tensors(a["ge"].engines[g], a["grads"][it][g]), _tensors(b["ge"].engines[g], b["grads"][it][g]))
            print(f"lr = 0, step {it}, member {g} ({'live' if lv[g] else 'dead'}): worst per-tensor gradient difference skip-on vs skip-off {worst:.2e}")
            assert worst <= SPREAD, (it, g, worst)


def test_dead_step_gradient_buffer_bitwise():
    """The WHOLE flat gradient buffer of a member after its own dead step -- encoder, heads and gate -- is identical, bit for bit, with
    the default and with skip_dead_bwd = -1.  (The heads' and the gate's gradients are order-fixed sums at this batch size: up to 8 rows
    mms_gate_bwd runs one workgroup per model, csrc/heads.hip.  With a workgroup per row its fp32 atomics made the gate's four tensors
    differ by one or two units in the last place -- up to 1.1e-8 -- between any two runs, skip on or off alike.)"""
    runs = _sequence_runs()
    a, b = runs[0], runs[-1]
    for it, (_, lv) in enumerate(_SEQ_STEPS):
        for g in range(2):
            if not lv[g]:
                ga, gb = a["grads"][it][g], b["grads"][it][g]
                assert torch.equal(ga, gb), (it, g, float((ga - gb).abs().max()))


# ---- never on under SyncBN / in a backward stage -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["zero_dout", "poisoned_word"])
def test_sync_driver_never_skips(case):
    """mms_dn121_backward_stage with bn_world = 1 and a no-op statistics hook (a ctypes callback): the word is neither written nor read.
    zero_dout: default == skip_dead_bwd = -1 == the pattern, bit for bit, and the word keeps the value put there.  poisoned_word: the
    word is set to 0 ("dead") and dout is NOT zero -- a driver that consulted it would leave the gradients empty."""
    from multimodal_survival_prediction_amd import _lib
    B, dims = SHAPES[0]
    D, H, W = dims
    c = _case(B, dims)
    net, e = c["net"], c["net"]._eng
    lib = e["lib"]
    hook = _lib.SYNC_FN(lambda *a: 0)
    dout = torch.zeros(B, 128, device=DEV) if case == "zero_dout" else torch.randn(B, 128, generator=torch.Generator().manual_seed(3)).to(DEV)
    res = {}
    for flag in (0, -1):
        e["ws"].copy_(c["ws"])
        _live_word(net).fill_(0 if case == "poisoned_word" else 77)
        want = _pattern(net) if case == "zero_dout" else None
        if want is None:
            _zero_grads(net)
        net.dn_opts = dict(skip_dead_bwd=flag)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.mms_dn121_backward_stage(e["ws"].data_ptr(), B, D, H, W, c["x"].data_ptr(), e["ptab"], dout.data_ptr(), 128,
                                                net._grad_table(), 3, 0, 1, hook, None, ctypes.byref(net._opts()), st), "mms_dn121_backward_stage")
        torch.cuda.synchronize()
        net.dn_opts = {}
        res[flag] = _grads(net)
        assert int(_live_word(net)[0]) == (0 if case == "poisoned_word" else 77)
        if want is not None:
            for a, b in zip(want, res[flag]):
                assert torch.equal(a, b)
    if case == "zero_dout":
        for a, b in zip(res[0], res[-1]):
            assert torch.equal(a, b)
    else:
        assert max(float(g.abs().max()) for g in res[0]) > 0.0
        assert _spread(res[0], res[-1]) <= SPREAD
