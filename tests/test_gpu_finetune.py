"""Fine-tuning on the GPU: the segment-aware optimiser kernels (csrc/finetune.hip) against the CPU replica (tests/finetune_ref.py), the
backward that stops above the frozen DenseNet121 stages against the full backward, the engines with a plan against the torch-driven
oracle, the refusals and the untouched no-plan path, and one entry point run with MMS_PRETRAINED / MMS_FINETUNE."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import finetune_ref as R
from gpu_util import DEV, _Recorder, assert_close, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W2N = 32 * 27 * 128
N_PLAIN = 100_003          # ordinary elements; the three packed tensors (110 592 floats each) sit between them: n = 431 779, odd
FRAGMASK = 0b101
HYPER = (1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0)
HYPER32 = torch.tensor(HYPER, dtype=torch.float32).double().tolist()      # what the kernels read: AdamP.hyper is fp32 (0.999 -> 0.99900001...)


def _layout():
    """-> (n, packed offsets, bounds, lr_mult, wd_mult, l2sp flags).  Bounds are odd and unaligned; bound 1236 is the first element of packed
    tensor 0; segment 3 (frozen) holds packed tensor 1; segment 4 is a bias of one float; segment 6 is a frozen run of 5 floats."""
    offs = [1236, 1236 + W2N + 40_004, 1236 + 2 * W2N + 60_004]
    n = N_PLAIN + 3 * W2N
    b = [0, 617, 1236, 1236 + W2N + 1001, offs[1] + W2N + 7, offs[1] + W2N + 8, offs[2] + W2N + 13_001, offs[2] + W2N + 13_006, n]
    lr = [1.0, 0.5, 1.0, 0.0, 2.0, 0.1, 0.0, 1.0]
    wd = [1.0, 2.0, 1.0, 1.0, 0.0, 1.0, 1.0, 0.0]
    pull = [0, 1, 1, 0, 1, 1, 0, 0]
    assert offs[2] + W2N < b[6] and all(o % 4 == 0 for o in offs) and any(x % 4 for x in b[1:-1]) and n % 4 == 3
    return n, offs, b, lr, wd, pull


class _Member:
    """One model's buffers + AdamP / TuneP blocks over the layout above."""

    def __init__(self, seed, table, hyper, adamw, l2, skip=None):
        from multimodal_survival_prediction_amd import ops
        n, offs, b, lr, wd, pull = _layout()
        g_ = torch.Generator().manual_seed(seed)
        mk = lambda s: (torch.randn(n, generator=g_) * s).to(DEV)
        self.p, self.m, self.v = mk(0.05), mk(1e-3), mk(1e-3) ** 2
        self.g = torch.zeros(n, device=DEV)
        self.anchor = (self.p + mk(0.01)) if l2 else None
        self.packs = torch.zeros(3, 2, W2N, device=DEV)
        base = self.packs.data_ptr()
        self.w2 = dict(off=torch.tensor(offs, dtype=torch.int64, device=DEV),
                       pack_b=torch.tensor([base + 2 * i * W2N * 4 for i in range(3)], dtype=torch.int64, device=DEV),
                       pack_f=torch.tensor([base + (2 * i + 1) * W2N * 4 for i in range(3)], dtype=torch.int64, device=DEV), fragmask=FRAGMASK)
        self.sumsq, self.step = torch.zeros(1, dtype=torch.float64, device=DEV), torch.zeros(1, device=DEV)
        self.skip = None if skip is None else torch.tensor([skip], device=DEV)
        self.acc, self.rng = torch.zeros(4, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
        self.adam = ops.adam_params(self.p, self.g, self.m, self.v, hyper, self.sumsq, self.step, self.skip, adamw, acc=self.acc, rng=self.rng,
                                    w2=self.w2)
        ops.call("mms_w2_pack", self.adam)
        self.tune = ops.tune_params(self.adam, table, self.anchor) if table is not None else None

    def set_grad(self, seed, scale, frozen_mask):
        g = torch.randn(self.g.numel(), generator=torch.Generator().manual_seed(seed)) * scale
        g[frozen_mask] = 1e6                      # a leak of a frozen gradient into the norm cannot hide
        self.g.copy_(g)
        return g

    def cpu(self):
        return [t.detach().cpu().clone() for t in (self.p, self.m, self.v)]


def _table(l2):
    from multimodal_survival_prediction_amd import ops
    n, offs, b, lr, wd, pull = _layout()
    l2sp = [l2 * f for f in pull]
    return ops.tune_table(b, lr, wd, l2sp, DEV), (b, lr, wd, l2sp)


def _launch(members, name):
    from multimodal_survival_prediction_amd import _lib, ops
    lib = _lib.load_library()
    arr = (_lib.structs()["TuneP"] * len(members))(*[mb.tune for mb in members])
    if len(members) == 1:
        _lib.check(getattr(lib, name)(ctypes.byref(members[0].tune), ops.stream()), name)
    else:
        _lib.check(getattr(lib, name + "_group")(arr, len(members), ops.stream()), name + "_group")


@pytest.mark.parametrize("ng", [1, 3])
@pytest.mark.parametrize("adamw,l2", [(False, 0.0), (True, 0.0), (False, 0.05), (True, 0.05)])
def test_tuned_kernels_match_replica(adamw, l2, ng):
    """(a) frozen p / m / v bit for bit, (b) trainable elements against the replica to 2e-6 after 4 steps, (c) the sum-of-squares word
    against the fp64 sum of the trainable g^2 to 1e-5 (positive terms, at most 16 fp32 additions per thread partial at this size:
    16 * 2^-24 ~ 1e-6, times ten), (f) the packs the step leaves == mms_w2_pack of the new weights."""
    from multimodal_survival_prediction_amd import ops
    n, offs, b, lr, wd, _ = _layout()
    hyper = torch.tensor(HYPER, device=DEV)
    table, (b, lr, wd, l2sp) = _table(l2)
    frozen = ~R.trainable_mask(n, b, lr)
    members = [_Member(7 + i, table, hyper, adamw, l2 > 0) for i in range(ng)]
    start = [mb.cpu() for mb in members]
    ref = [[t.clone() for t in s] for s in start]
    anchors = [mb.anchor.cpu() if mb.anchor is not None else None for mb in members]
    for it in range(4):
        gs = [mb.set_grad(100 * it + i, 3.0 if it % 2 == 0 else 1e-3, frozen) for i, mb in enumerate(members)]     # clipped / unclipped
        for mb in members:
            mb.sumsq.zero_()
        _launch(members, "mms_grad_sumsq_tuned")
        torch.cuda.synchronize()
        for i, mb in enumerate(members):
            want = R.trainable_sumsq(gs[i], b, lr)
            got = float(mb.sumsq)
            print("step %d member %d: sumsq rel err %.3e" % (it, i, abs(got - want) / want))
            assert abs(got - want) <= 1e-5 * want, (it, i, got, want)
        _launch(members, "mms_clip_adam_tuned")
        for i in range(ng):
            R.step(ref[i][0], gs[i], ref[i][1], ref[i][2], it + 1, b, lr, wd, l2sp, HYPER32, adamw, anchors[i])
    torch.cuda.synchronize()
    tr = ~frozen
    for i, mb in enumerate(members):
        got = mb.cpu()
        assert float(mb.step) == 4.0 and int(mb.rng[1]) == 4 and float(mb.acc[3]) == 4.0
        for name, a, w, s0 in zip("pmv", got, ref[i], start[i]):
            assert torch.equal(a[frozen], s0[frozen]), "frozen %s of member %d moved" % (name, i)
            e = rel_err(a[tr], w[tr])
            print("member %d %s: rel err %.3e" % (i, name, e))
            assert e <= 2e-6, (name, i, e)
        assert not torch.equal(got[0][tr], start[i][0][tr])
        packs = mb.packs.clone()
        ops.call("mms_w2_pack", mb.adam)
        torch.cuda.synchronize()
        assert torch.equal(packs, mb.packs), "packs of member %d are not the packs of its weights" % i
        assert not torch.equal(packs[0], torch.zeros_like(packs[0]))


@pytest.mark.parametrize("adamw", [False, True])
def test_trivial_plan_gives_the_bits_of_clip_adam(adamw):
    """(d) one segment, multipliers 1, l2sp 0, the same preset sum word: p, m, v and both derived packs torch.equal to mms_clip_adam's."""
    from multimodal_survival_prediction_amd import ops
    n = _layout()[0]
    hyper = torch.tensor(HYPER, device=DEV)
    table = ops.tune_table([0, n], [1.0], [1.0], [0.0], DEV)
    a, t = _Member(3, None, hyper, adamw, False), _Member(3, table, hyper, adamw, False)
    none = torch.zeros(n, dtype=torch.bool)
    for it in range(2):
        a.set_grad(40 + it, 3.0 if it == 0 else 1e-3, none); t.set_grad(40 + it, 3.0 if it == 0 else 1e-3, none)
        a.sumsq.zero_(); t.sumsq.zero_()
        ops.call("mms_grad_sumsq", a.adam)
        ops.call("mms_grad_sumsq_tuned", t.tune)
        torch.cuda.synchronize()
        assert abs(float(t.sumsq) - float(a.sumsq)) <= 1e-5 * float(a.sumsq)
        t.sumsq.copy_(a.sumsq)                       # the same preset sum word
        ops.call("mms_clip_adam", a.adam)
        ops.call("mms_clip_adam_tuned", t.tune)
        torch.cuda.synchronize()
        for name, x, y in zip("pmv", (a.p, a.m, a.v), (t.p, t.m, t.v)):
            assert torch.equal(x, y), "step %d: %s differs in %d elements" % (it, name, int((x != y).sum()))
        assert torch.equal(a.packs, t.packs)
    assert float(a.step) == float(t.step) == 2.0 and torch.equal(a.acc, t.acc) and torch.equal(a.rng, t.rng)


def test_skipped_step_moves_nothing():
    """(e) skip_flag = 0: p, m, v, the packs and the step counter stay; the epoch bookkeeping still counts the batch, as in mms_grad_sumsq."""
    hyper = torch.tensor(HYPER, device=DEV)
    table, (b, lr, wd, l2sp) = _table(0.05)
    mb = _Member(5, table, hyper, False, True, skip=0.0)
    mb.set_grad(1, 3.0, ~R.trainable_mask(_layout()[0], b, lr))
    before, packs = mb.cpu(), mb.packs.clone()
    _launch([mb], "mms_grad_sumsq_tuned")
    _launch([mb], "mms_clip_adam_tuned")
    torch.cuda.synchronize()
    for x, y in zip(before, mb.cpu()):
        assert torch.equal(x, y)
    assert torch.equal(packs, mb.packs) and float(mb.step) == 0.0 and float(mb.acc[3]) == 1.0 and int(mb.rng[1]) == 1


def test_tune_check_reads_the_tables():
    from multimodal_survival_prediction_amd import _lib, ops
    n, offs, b, lr, wd, _ = _layout()
    hyper = torch.tensor(HYPER, device=DEV)
    mb = _Member(1, None, hyper, False, False)
    ok = lambda bb, ll, ww=None, l2=None, anchor=None: ops.tune_params(mb.adam, ops.tune_table(bb, ll, ww or [1.0] * len(ll), l2 or [0.0] * len(ll), DEV), anchor)
    ok(b, lr)
    bad = [([0, offs[0] + 5, n], [1.0, 1.0]),                      # a bound inside a packed tensor
           ([0, 700, 700, n], [1.0, 1.0, 1.0]),                    # not strictly ascending
           ([4, n], [1.0]), ([0, n - 1], [1.0]),                    # not from 0 to n
           ([0, n], [0.0]),                                         # nothing trainable
           ([0, n], [float("inf")]), ([0, n], [-1.0])]
    for bb, ll in bad:
        with pytest.raises(_lib.MmsError):
            ok(bb, ll)
    with pytest.raises(_lib.MmsError):
        ok([0, n], [1.0], [float("nan")])
    with pytest.raises(_lib.MmsError):
        ok([0, n], [1.0], None, [0.1])                              # l2sp without an anchor


# ---- truncated backward ----------------------------------------------------------------------------------
def _encoders(ng, seed=2):
    from multimodal_survival_prediction_amd.densenet import DenseNet121
    from test_gpu_densenet import structured_volumes
    nets, xs, douts = [], [], []
    for g in range(ng):
        torch.manual_seed(seed + g)
        nets.append(DenseNet121(out_channels=128).to(DEV).train())
        xs.append(structured_volumes(2, (32, 32, 32), seed + g).to(DEV))
        douts.append(torch.randn(2, 128, generator=torch.Generator().manual_seed(50 + g)).to(DEV) * 1e-2)
    return nets, xs, douts


def _backward(nets, xs, douts, block_lo):
    """Training forward, then the backward (block_lo None: the plain driver) -> per model the list of 364 gradient tensors."""
    from multimodal_survival_prediction_amd import _lib, ops
    lib, ng = _lib.load_library(), len(nets)
    P = ctypes.c_void_p
    es, gts = [], []
    for net, x in zip(nets, xs):
        for p in net.parameters():
            p.grad = None
        net._run_forward(x)
        es.append(net._tables(x))
        gts.append(net._grad_table())
    st, o = ops.stream(), ctypes.byref(nets[0]._opts())
    if ng == 1:
        e, a = es[0], (es[0]["ws"].data_ptr(), 2, 32, 32, 32, xs[0].data_ptr(), es[0]["ptab"], douts[0].data_ptr(), 128, gts[0])
        rc = lib.mms_dn121_backward(*a, o, st) if block_lo is None else lib.mms_dn121_backward_from(*a, block_lo, o, st)
    else:
        arr = lambda vals: (P * ng)(*vals)
        a = (ng, arr([e["ws"].data_ptr() for e in es]), 2, 32, 32, 32, arr([x.data_ptr() for x in xs]), arr([ctypes.addressof(e["ptab"]) for e in es]),
             arr([d.data_ptr() for d in douts]), 128, arr([ctypes.addressof(g) for g in gts]))
        rc = lib.mms_dn121_backward_group(*a, o, st) if block_lo is None else lib.mms_dn121_backward_group_from(*a, block_lo, o, st)
    _lib.check(rc, "backward")
    torch.cuda.synchronize()
    return [[p.grad.detach().clone() for p in net.parameters()] for net in nets]


@pytest.mark.parametrize("ng", [1, 2])
def test_backward_from_matches_the_full_backward(ng):
    """Stages >= block_lo agree with the full backward on the same forward within the run-to-run criterion of test_run_twice_spread (1e-4
    of each tensor's maximum); the gradient buffers of the frozen prefix stay exactly zero; block_lo = 0 is the full backward."""
    from multimodal_survival_prediction_amd.densenet import stage_table_ranges
    nets, xs, douts = _encoders(ng)
    full = _backward(nets, xs, douts, None)
    ranges = stage_table_ranges()
    for lo in (0, 1, 2, 3):
        got = _backward(nets, xs, douts, lo)
        first = ranges[lo][0]
        for g in range(ng):
            gmax = max(float(t.abs().max()) for t in full[g])
            worst = 0.0
            for i, (a, w) in enumerate(zip(got[g], full[g])):
                if i < first:
                    assert not bool(a.any()), "block_lo %d model %d: gradient %d of the frozen prefix was written" % (lo, g, i)
                    continue
                if float(w.abs().max()) < 1e-5 * gmax:
                    assert float(a.abs().max()) < 1e-4 * gmax
                    continue
                worst = max(worst, rel_err(a, w))
            print("ng %d block_lo %d model %d: worst per-tensor difference %.3e" % (ng, lo, g, worst))
            assert worst <= 1e-4, (lo, g, worst)
            assert bool(got[g][first].any()) and bool(got[g][first + 2].any())          # the stage's own first entries ARE written


# ---- engines against the oracle ----------------------------------------------------------------------------
def _oracle_optimizer(ref, net, plan, lr, wd):
    """torch's Adam over parameter groups as the plan sets them; frozen tensors: requires_grad_(False)."""
    groups = []
    for name, _, (lm, wm, l2) in plan.settings(net):          # (the plan reads the HIP model; the oracle's modules carry the same names)
        p = dict(ref.named_parameters())[name]
        assert l2 == 0.0
        if lm == 0.0:
            p.requires_grad_(False)
        else:
            groups.append(dict(params=[p], lr=lr * lm, weight_decay=wd * wm))
    return torch.optim.Adam(groups, lr=lr, weight_decay=wd)


# Cases of the engine tests.  Case c = the oracle/HIP model pair of seed c (test_gpu_models._pair) on batches 5c and 5c + 1 (case 4 is
# test_fused_graph_step_matches_reference_loop_body's own seed and batches).  That test's second bound -- 0.93 of the weights within 2e-5
# of the oracle's after two steps -- is a statement about Adam's first, sign-like steps, and at this 32^3 shape (dense block 4 has one
# voxel per sample) the fp32 CPU oracle often misses it against ITSELF in fp64: tools/finetune_oracle_scan.py, share of the TRAINABLE
# weights under freeze=2 + rna x0.1 for cases 4..13: 0.924 0.990 0.842 0.673 0.930 0.928 0.997 0.584 0.957 0.945 (whole encoder frozen,
# eval mode: 1.000 in every case).  The HIP path and the fp32 oracle are two fp32 implementations, each that far from exact arithmetic, so
# the bound can be asked of their difference only where the oracle's own loss is at most half of the 0.07 the bound allows: share >= 0.965.
# The cases are the first two of 4..13 that meet this premise, decided from the oracle alone: 5 and 10.
CASES = (5, 10)


def _check_against_oracle(ref, net, ref0, plan, max_mult):
    """test_fused_graph_step_matches_reference_loop_body's two bounds over the TRAINABLE weights, scaled by the plan's largest multiplier:
    worst difference of an update <= 4.2e-4, at least 0.93 of them within 2e-5; frozen tensors bit for bit.  Measured on the MI355X
    (share of the trainable weights): one engine, case 5, freeze=2 + rna x0.1: 0.9974; whole encoder frozen in eval mode: 1.0000; the
    group's members (cases 5, 10): 0.9968 and 0.9976."""
    frozen = {n for n, _, s in plan.settings(net) if s[0] == 0.0}
    worst, tot, close = 0.0, 0, 0.0
    for (k, p), (_, q), (_, p0) in zip(ref.named_parameters(), net.named_parameters(), ref0.named_parameters()):
        if k in frozen:
            assert torch.equal(q.detach().cpu(), p0.detach()), "frozen %s moved" % k
            assert torch.equal(p.detach(), p0.detach())
            continue
        du_ref, du_net = (p.detach() - p0.detach()).double(), (q.detach().cpu() - p0.detach()).double()
        worst = max(worst, float((du_ref - du_net).abs().max()))
        tot += p.numel()
        close += float(((p.detach() - q.detach().cpu()).abs() <= 2e-5 * max_mult).double().sum())
    print("worst update diff %.2e; %.4f of the trainable weights within %.1e" % (worst, close / tot, 2e-5 * max_mult))
    assert len(frozen) > 0
    assert worst <= 4.2e-4 * max_mult, worst
    assert close / tot >= 0.93, close / tot


def _plans():
    from multimodal_survival_prediction_amd.transfer import FineTunePlan
    return {"stages2_rna": FineTunePlan([("rna_encoder", 0.1)], freeze_stages=2), "enc_eval": FineTunePlan(freeze_stages=4, encoder_eval=True)}


def _oracle_step(ref, opt_ref, case, it, B, dims, rna_dim, valid):
    """One iteration of the reference loop body on the oracle; -> the batch"""
    from oracle import losses as OL
    from test_gpu_models import _batch
    ct, rna, clin, t, e, mask = _batch(B, dims, rna_dim, 5 * case + it)
    hz, gw = ref(ct, rna, clin, mask)
    sm = valid.bool()
    loss = OL.cox_loss(hz[sm], e[sm], t[sm]) + 0.01 * OL.gate_entropy_loss(gw)
    opt_ref.zero_grad(); loss.backward()
    torch.nn.utils.clip_grad_norm_([p for p in ref.parameters() if p.requires_grad], 1.0)
    opt_ref.step()
    return dict(ct=ct, rna=rna, clinical=clin, mask=mask, time=t, event=e, valid=valid)


@pytest.mark.parametrize("which", ["stages2_rna", "enc_eval"])
def test_engine_with_plan_matches_oracle(which):
    from multimodal_survival_prediction_amd.training import FusedOptimizer
    from test_gpu_models import _pair
    plan, case = _plans()[which], CASES[0]
    B, dims, rna_dim = 4, (32, 32, 32), 96
    ref, net = _pair("PartialModalityNet", case, rna_dim)
    ref0, _ = _pair("PartialModalityNet", case, rna_dim)
    opt_ref = _oracle_optimizer(ref, net, plan, 1e-4, 1e-4)
    eng = FusedOptimizer(net, lr=1e-4, weight_decay=1e-4, adamw=False, finetune=plan).engine
    assert eng.block_lo == (2 if which == "stages2_rna" else 0) and eng.enc_frozen == (which == "enc_eval") and eng.anchor is None
    ref.train(); net.train()
    if plan.encoder_eval:
        ref.ct_encoder.eval()
    bufs0 = {k: b.detach().cpu().clone() for k, b in net.named_buffers()}
    valid = torch.tensor([1, 1, 0, 1], dtype=torch.float32)
    for it in range(2):
        b = _oracle_step(ref, opt_ref, case, it, B, dims, rna_dim, valid)
        eng.train_step(b["ct"], b["rna"], b["clinical"], mask=b["mask"], time=b["time"], event=b["event"], valid=valid, skip_if_unusable=False)
    torch.cuda.synchronize()
    st = eng.epoch_stats()
    assert st["n_batches"] == 2 and st["n_usable"] == 2
    _check_against_oracle(ref, net, ref0, plan, 1.0)
    for (k, b), (_, c) in zip(ref.named_buffers(), net.named_buffers()):
        if plan.encoder_eval and k.startswith("ct_encoder."):
            assert torch.equal(c.cpu(), bufs0[k]), "encoder buffer %s moved under encoder_eval" % k       # (num_batches_tracked among them)
            assert torch.equal(b, bufs0[k])
        elif "num_batches" in k:
            assert int(b) == int(c), k
        else:
            assert_close(c, b, 2e-3, k)


def test_fold_group_with_plan_matches_oracle():
    """Two DIFFERENT members (cases 5 and 10: their own weights, their own batches) through FoldGroupEngine, each against its own oracle:
    a mix-up between the members' segment blocks, gradient tables or truncated-backward arguments would show in either.
    The group runs under GROUP_INDEPENDENT_OPTS, the launch forms this suite gives to group comparisons that must be tight (gpu_util):
    which K-split and tile forms a launch takes depends on how many models share it, and so does the summation order.  Under the
    default forms case 5 keeps 0.992 in either position of the group, case 10 keeps 0.915 there and 0.884 on one engine -- against 0.9976
    under these forms and 0.997 for the fp32 oracle against itself: one sign decided differently by rounding in the small blocks of this
    shape, the same in either position of the group, so no mix-up.  The default forms under a plan are what the one-engine test above and
    test_backward_from_matches_the_full_backward (ng = 2) run."""
    from gpu_util import GROUP_INDEPENDENT_OPTS
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    from test_gpu_models import _pair
    plan = _plans()["stages2_rna"]
    B, dims, rna_dim = 4, (32, 32, 32), 96
    pairs = [_pair("PartialModalityNet", c, rna_dim) for c in CASES]
    starts = [_pair("PartialModalityNet", c, rna_dim)[0] for c in CASES]
    opts = [_oracle_optimizer(ref, net, plan, 1e-4, 1e-4) for ref, net in pairs]
    grp = FoldGroupEngine([net for _, net in pairs], lr=1e-4, weight_decay=1e-4, adamw=False, finetune=plan, dn_opts=GROUP_INDEPENDENT_OPTS)
    assert grp.engines[0].tune_tab is grp.engines[1].tune_tab and grp.engines[0].block_lo == 2
    valid = torch.tensor([1, 1, 0, 1], dtype=torch.float32)
    for ref, net in pairs:
        ref.train(); net.train()
    for it in range(2):
        grp.train_step([_oracle_step(ref, opts[g], CASES[g], it, B, dims, rna_dim, valid) for g, (ref, _) in enumerate(pairs)],
                       skip_if_unusable=False)
    torch.cuda.synchronize()
    for (ref, net), ref0 in zip(pairs, starts):
        _check_against_oracle(ref, net, ref0, plan, 1.0)


# ---- refusals and the no-plan path ---------------------------------------------------------------------------
def _calls(finetune="absent"):
    from multimodal_survival_prediction_amd import models as HM
    from multimodal_survival_prediction_amd.engine import SurvivalEngine
    from test_gpu_models import _batch
    torch.manual_seed(1)
    net = HM.PartialModalityNet(rna_dim=96).to(DEV).train()
    eng = SurvivalEngine(net) if finetune == "absent" else SurvivalEngine(net, finetune=finetune)
    ct, rna, clin, t, e, mask = _batch(4, (32, 32, 32), 96, 3)
    eng.train_step(ct, rna, clin, mask=mask, time=t, event=e, use_graph=False)         # plan + first-use work
    eng.lib = rec = _Recorder(eng.lib)
    eng.train_step(ct, rna, clin, mask=mask, time=t, event=e, use_graph=False)
    torch.cuda.synchronize()
    return eng, rec.calls


def test_no_plan_enqueues_the_same_launches_and_refusals():
    from multimodal_survival_prediction_amd.distributed import DataParallel
    from multimodal_survival_prediction_amd.engine import engine_of
    from multimodal_survival_prediction_amd.transfer import FineTunePlan
    _, absent = _calls()
    eng, none = _calls(None)
    assert absent == none and len(none) > 5
    assert not any("tuned" in c or c.endswith("_from") for c in none) and "mms_clip_adam" in none and "mms_dn121_backward" in none
    assert eng.finetune is None and eng.tune_tab is None and eng.anchor is None
    plan = FineTunePlan([("fusion", 1.0, 1.0, 0.01)], freeze_stages=1)
    eng, tuned = _calls(plan)
    assert "mms_clip_adam_tuned" in tuned and "mms_grad_sumsq_tuned" in tuned and "mms_dn121_backward_from" in tuned
    assert "mms_clip_adam" not in tuned and "mms_dn121_backward" not in tuned
    assert eng.anchor is not None and all(eng.anchor is not t for t in eng._state())        # w0 is constant: not part of the step's state
    # weights loaded into a live engine: the L2-SP anchor follows them, in place (the launches hold its address)
    from multimodal_survival_prediction_amd.transfer import load_pretrained
    addr = eng.anchor.data_ptr()
    assert torch.equal(eng.anchor, eng.flat) is False                                        # (two steps have moved the weights)
    load_pretrained(eng.model, {k: v.detach().cpu() * 0.5 for k, v in eng.model.state_dict().items() if v.dtype.is_floating_point})
    assert torch.equal(eng.anchor, eng.flat) and eng.anchor.data_ptr() == addr
    eng4, frozen = _calls("freeze=4")
    assert not any(c.startswith("mms_dn121_backward") for c in frozen) and "mms_dn121_forward" in frozen
    # refusals
    with pytest.raises(RuntimeError, match="cannot be changed"):
        engine_of(eng.model, finetune="freeze=2")
    assert engine_of(eng.model, finetune=plan) is eng
    from test_gpu_models import _batch
    ct, rna, clin, t, e, mask = _batch(4, (32, 32, 32), 96, 3)
    with pytest.raises(RuntimeError, match="data-parallel"):
        eng.train_step(ct, rna, clin, mask=mask, time=t, event=e, ddp_world=2)
    with pytest.raises(RuntimeError, match="data-parallel"):
        DataParallel(eng).step(None, 2, False, False)
    with pytest.raises(RuntimeError, match="data-parallel"):
        DataParallel(eng).step_syncbn(None, 2)


# ---- one entry point ---------------------------------------------------------------------------------------
ENV = dict(MMS_PATIENTS="42", MMS_EPOCHS="4", MMS_FOLDS="3", MMS_BATCH_SIZE="4")


def _run(script, cwd, **extra):
    env = dict(os.environ, **ENV, **extra)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "scripts", "training", script)], cwd=cwd, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_rnaseq_entry_point_fine_tunes_a_checkpoint(tmp_path):
    """train_rnaseq_only.py plainly, then again from its fold checkpoints with a source gene list that lacks some of the cohort's genes
    (and orders the rest differently) and the first layer frozen: the second run's checkpoints keep that layer equal to the aligned source
    columns, and cv_results.json carries `transfer`."""
    from multimodal_survival_prediction_amd.transfer import default_gene_names
    src_dir, dst_dir = tmp_path / "source", tmp_path / "target"
    src_dir.mkdir(); dst_dir.mkdir()
    _run("train_rnaseq_only.py", src_dir)
    res0 = json.load(open(src_dir / "results" / "rnaseq_only" / "cv_results.json"))
    assert "transfer" not in res0
    names = default_gene_names(5005)
    src_genes = list(reversed(names))                       # the source's column j is the cohort's gene 5004 - j ...
    for j in range(0, 5005, 50):
        src_genes[j] = "SOURCE_ONLY_%d" % j                 # ... and the cohort's genes 5004 - j, j = 0, 50, ..., are unknown to the source
    genes = tmp_path / "genes.json"
    genes.write_text(json.dumps(dict(gene_names=src_genes)))
    out = _run("train_rnaseq_only.py", dst_dir, MMS_PRETRAINED=str(src_dir / "results" / "rnaseq_only" / "best_model_fold{fold}.pth"),
               MMS_PRETRAINED_GENES=str(genes), MMS_FINETUNE=r"rule=^mlp\.0\.:lr=0")
    assert "aligned by gene" in out and "frozen" in out
    res = json.load(open(dst_dir / "results" / "rnaseq_only" / "cv_results.json"))
    assert res["transfer"]["finetune"] == r"rule=^mlp\.0\.:lr=0.0:wd=1.0:l2sp=0.0" and res["transfer"]["pretrained"].endswith("best_model_fold{fold}.pth")
    assert res["transfer"]["folds"][0]["aligned_genes"]["mlp.0.weight"] == dict(shared=5005 - 101, new=101, dropped=101)
    assert set(res) - {"transfer"} == set(res0)
    for fold in (1, 2, 3):
        src = torch.load(src_dir / "results" / "rnaseq_only" / f"best_model_fold{fold}.pth", map_location="cpu")
        dst = torch.load(dst_dir / "results" / "rnaseq_only" / f"best_model_fold{fold}.pth", map_location="cpu")
        shared = torch.tensor([j for j in range(5005) if (5004 - j) % 50 != 0])
        assert torch.equal(dst["mlp.0.weight"][:, shared], src["mlp.0.weight"][:, 5004 - shared])
        assert torch.equal(dst["mlp.0.bias"], src["mlp.0.bias"])
        new = torch.tensor([5004 - j for j in range(0, 5005, 50)])
        assert not torch.equal(dst["mlp.0.weight"][:, new], src["mlp.0.weight"][:, 5004 - new])
        assert not torch.equal(dst["mlp.4.weight"], src["mlp.4.weight"])            # the rest trained on
