"""The launches of the training step outside the encoder whose chain was shortened (gate forward with every load in flight, one launch for a
layer's two Linear-backward roles, one zeroing launch per step, Cox in one launch for small batches) and the DenseNet head forward at the
fold groups' row counts, through the C ABI against plain torch on the CPU at the 1e-4 of tests/test_gpu_heads.py, and -- where an earlier
launch form is still selectable -- against that form bit for bit."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_util import DEV, assert_close


@pytest.fixture(scope="module")
def env():
    from multimodal_survival_prediction_amd import _lib, ops
    return _lib.load_library(), _lib.structs(), ops, _lib


def _d(t):
    return t.detach().to(DEV).contiguous()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# =====================================================================================================================
# gate forward
# =====================================================================================================================
@pytest.mark.parametrize("ng", [1, 2])
@pytest.mark.parametrize("M", [1, 4, 33])
def test_gate_fwd(env, M, ng):
    lib, S, ops, _lib = env
    arr = (S["GateP"] * ng)()
    live, want = [], []
    for g in range(ng):
        gen = torch.Generator().manual_seed(7 * M + g)
        feats = torch.randn(M, 288, generator=gen)
        mask = (torch.rand(M, 3, generator=gen) < 0.6).float()
        mask[:, 1] = 0.0                                   # a modality nobody has
        mask[0, 0] = 1.0
        w1, b1 = torch.randn(64, 291, generator=gen) / 291 ** 0.5, torch.randn(64, generator=gen) * 0.1
        w2, b2 = torch.randn(3, 64, generator=gen) / 8, torch.randn(3, generator=gen) * 0.1
        segs = [slice(0, 128), slice(128, 256), slice(256, 288)]
        masked = torch.cat([feats[:, s] * mask[:, i:i + 1] for i, s in enumerate(segs)], 1)
        hidden = F.relu(F.linear(torch.cat([masked, mask], 1), w1, b1))
        gate = F.softmax(F.linear(hidden, w2, b2), dim=1)
        fused = torch.cat([masked[:, s] * gate[:, i:i + 1] for i, s in enumerate(segs)], 1)
        ent = (gate * torch.log(gate + 1e-8)).sum(1).mean()
        want.append((gate, hidden, fused, ent.reshape(1)))
        d = [_d(t) for t in (feats, mask, w1, b1, w2, b2)]
        out = [torch.full((M, 64), float("nan"), device=DEV), torch.full((M, 3), float("nan"), device=DEV),
               torch.full((M, 288), float("nan"), device=DEV), torch.zeros(1, device=DEV)]
        arr[g] = ops.gate_params(d[0], d[1], d[2], d[3], d[4], d[5], out[0], out[1], out[2], entropy=out[3])
        live.append((d, out))
    runs = []
    for _ in range(2):
        for _, out in live:
            out[3].zero_()
        _lib.check(lib.mms_gate_fwd_group(arr, ng, ops.stream()), "mms_gate_fwd_group")
        torch.cuda.synchronize()
        runs.append([[t.clone() for t in out] for _, out in live])
    for g in range(ng):
        hid, gt, fu, en = runs[0][g]
        assert_close(gt, want[g][0], 1e-4, "gate"); assert_close(hid, want[g][1], 1e-4, "hidden")
        assert_close(fu, want[g][2], 1e-4, "fused"); assert_close(en, want[g][3], 1e-4, "entropy")
        for a, b in zip(runs[0][g][:3], runs[1][g][:3]):      # (the entropy word is an fp32 atomic sum over the rows' workgroups)
            assert torch.equal(_bits(a), _bits(b))
        if M == 1:
            assert torch.equal(_bits(runs[0][g][3]), _bits(runs[1][g][3]))


# =====================================================================================================================
# DenseNet head forward: norm5 + relu + global average pool + Linear
# =====================================================================================================================
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("N", [4, 6])
@pytest.mark.parametrize("B,V,C", [(4, 4, 1024), (4, 1, 1024), (3, 8, 1024), (2, 4, 1056)])
def test_head_fwd(env, B, V, C, N, train):
    """16, 4, 24 and 8 rows (two full row batches, half a batch, three batches, one); C = 1056 has a second, partial channel chunk and a 17th
    weight piece per lane; N = 6 leaves the last workgroup two waves without a column.  (The kernel is the one tests/test_gpu_large_batch.py
    covers from 16 samples up; a form with all rows requested at once was measured slower and is not in the library -- DESIGN.md section 5,
    round 11 -- and these are the cases any such form has to pass.)"""
    lib, S, ops, _lib = env
    gen = torch.Generator().manual_seed(1000 * B + 10 * V + N)
    x = torch.randn(B * V, C, generator=gen) + 0.2
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.1
    rmean, rvar = torch.randn(C, generator=gen) * 0.1, torch.rand(C, generator=gen) + 0.5
    w, bias = torch.randn(N, C, generator=gen) / C ** 0.5, torch.randn(N, generator=gen) * 0.1
    if train:
        mu, var = x.double().mean(0), x.double().var(0, unbiased=False)
    else:
        mu, var = rmean.double(), rvar.double()
    a = torch.relu((x.double() - mu) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double())
    pooled = a.view(B, V, C).mean(1)
    out = pooled @ w.double().t() + bias.double()
    d = [_d(t) for t in (x, gamma, beta, rmean, rvar, w, bias)]
    s, q = d[0].double().sum(0), (d[0].double() ** 2).sum(0)
    pd_, od = torch.full((B, C), float("nan"), device=DEV), torch.full((B, N + 3), float("nan"), device=DEV)
    bn = ops.bnsrc(d[1], d[2], B * V, train, s, q, d[3], d[4])
    p = S["HeadFwdP"](d[0].data_ptr(), C, C, B, V, bn, d[5].data_ptr(), d[6].data_ptr(), N, pd_.data_ptr(), od.data_ptr(), N + 3)
    _lib.check(lib.mms_head_fwd(ctypes.byref(p), ops.stream()), "mms_head_fwd")
    torch.cuda.synchronize()
    assert_close(pd_, pooled, 1e-4, "pooled")
    assert_close(od[:, :N], out, 1e-4, "out")
    assert bool(torch.isnan(od[:, N:]).all())              # columns past N are not the launch's


# =====================================================================================================================
# Linear backward: both roles in one launch
# =====================================================================================================================
def _linear_case(M, K, N, bn, relu, seed):
    """-> inputs and torch's gradients of  y = [relu](dropout_mask * relu(bn(x)) W^T + b)  (bn = False: y = [relu](x W^T + b))."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=gen).requires_grad_(True)
    w = (torch.randn(N, K, generator=gen) / max(K, 1) ** 0.5).requires_grad_(True)
    b = (torch.randn(N, generator=gen) * 0.1).requires_grad_(True)
    dy = torch.randn(M, N, generator=gen)
    dw0 = torch.randn(N, K, generator=gen)                 # the gradient buffer is accumulated into
    mod = keep = None
    train = M > 1                                          # (BatchNorm1d over one row: eval-mode statistics, as torch requires)
    if bn:
        mod = torch.nn.BatchNorm1d(K)
        with torch.no_grad():
            mod.weight.copy_(torch.rand(K, generator=gen) + 0.5); mod.bias.copy_(torch.randn(K, generator=gen) * 0.2)
            mod.running_mean.copy_(torch.randn(K, generator=gen) * 0.3); mod.running_var.copy_(torch.rand(K, generator=gen) + 0.5)
        mod.train(train)
        keep = (torch.rand(M, K, generator=gen) > 0.3).float() / 0.7 if train else None
        a = F.relu(mod(x))
        if keep is not None:
            a = a * keep
    else:
        a = x
    y = F.linear(a, w, b)
    if relu:
        y = F.relu(y)
    y.backward(dy)
    return dict(x=x, w=w, b=b, dy=dy, dw0=dw0, y=y.detach(), mod=mod, keep=keep, train=train)


@pytest.mark.parametrize("ng", [1, 2])
@pytest.mark.parametrize("bn,relu", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("K,N", [(32, 3), (512, 128), (5005, 8), (1, 32)])
@pytest.mark.parametrize("M", [1, 4, 5])
def test_linear_bwd_merged(env, M, K, N, bn, relu, ng):
    """(K, N) = (1, 32) has no dx (a single-role launch); 5005 columns take the row-split weight kernel; M = 5 the 8-row instantiation.
    Form 0 (merged where the layer has both roles) against torch, and against form 1 (one launch per role) bit for bit."""
    lib, S, ops, _lib = env
    want_dx = (K, N) != (1, 32)
    res = {}
    cases = [_linear_case(M, K, N, bn, relu, 31 * M + K + N + 5 * g) for g in range(ng)]
    for form in (0, 1):
        arr = (S["LinearBwdP"] * ng)()
        live = []
        for g, c in enumerate(cases):
            mod = copy.deepcopy(c["mod"]).to(DEV) if bn else None
            keepd = _d(c["keep"]) if c["keep"] is not None else None
            pro = ops.inprolog(mod, train=c["train"], drop_mask=keepd)
            xd, wd, dyd, yd = _d(c["x"]), _d(c["w"]), _d(c["dy"]), _d(c["y"])
            dw, db = _d(c["dw0"]), torch.zeros(N, device=DEV)
            dx = torch.full((M, K + 2), float("nan"), device=DEV) if want_dx else None
            dg, dbt = (torch.zeros(K, device=DEV), torch.zeros(K, device=DEV)) if bn and want_dx else (None, None)      # (the input role's outputs)
            arr[g] = S["LinearBwdP"](dyd.data_ptr(), dyd.stride(0), yd.data_ptr(), yd.stride(0), 1 if relu else 0, xd.data_ptr(), xd.stride(0),
                                     M, K, pro, wd.data_ptr(), N, dw.data_ptr(), db.data_ptr(), ops.ptr(dx), dx.stride(0) if want_dx else 0,
                                     ops.ptr(dg), ops.ptr(dbt))
            live.append((mod, keepd, xd, wd, dyd, yd, dw, db, dx, dg, dbt))
        _lib.check(lib.mms_linear_bwd_group_form(arr, ng, form, ops.stream()), "mms_linear_bwd_group_form")
        torch.cuda.synchronize()
        res[form] = live
    for g, c in enumerate(cases):
        _, _, _, _, _, _, dw, db, dx, dg, dbt = res[0][g]
        assert_close(dw, c["dw0"] + c["w"].grad, 1e-4, "dw (accumulated)")
        assert_close(db, c["b"].grad, 1e-4, "dbias")
        if want_dx:
            assert_close(dx[:, :K], c["x"].grad, 1e-4, "dx")
            assert bool(torch.isnan(dx[:, K:]).all())
        if bn and want_dx:
            assert_close(dg, c["mod"].weight.grad, 1e-4, "dgamma"); assert_close(dbt, c["mod"].bias.grad, 1e-4, "dbeta")
        for a, b in zip(res[0][g][6:], res[1][g][6:]):
            if a is not None:
                assert torch.equal(_bits(a), _bits(b)), "the merged launch differs from the two launches"
    assert lib.mms_linear_bwd_group_form(arr, ng, 2, ops.stream()) == -1


# =====================================================================================================================
# zero spans
# =====================================================================================================================
ZS_SIZES = [4, 8, 12, 16, 20, 4096 + 4, (1 << 20) + 8]


@pytest.mark.parametrize("n", [1, 3, 30])
def test_zero_spans(env, n):
    """Every size with a 4-byte guard word before and after each span, the first span 4 bytes past a 16-byte boundary (the guard words
    then walk the spans through the other alignments); n = 30 is the cap."""
    lib, S, ops, _lib = env
    sizes = [ZS_SIZES[(i + (n == 1) * 6) % len(ZS_SIZES)] for i in range(n)]
    total = 32 + sum(sizes) + 4 * (n + 1) + 32
    buf = torch.full((total // 4 + 4,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    base = buf.data_ptr()
    off = (-base) % 16 + 16 + 4 - 4                        # the first guard word: 16-byte aligned, so the span starts 4 bytes past
    want = buf.cpu().numpy().copy()
    arr = (S["MmsZeroSpan"] * n)()
    for i, sz in enumerate(sizes):
        off += 4                                           # guard
        arr[i] = S["MmsZeroSpan"](base + off, sz)
        if i == 0:
            assert (base + off) % 16 == 4
        want[off // 4:(off + sz) // 4] = 0
        off += sz
    assert off + 4 <= buf.numel() * 4
    _lib.check(lib.mms_zero_spans_group(arr, n, ops.stream()), "mms_zero_spans_group")
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got, want), "bytes outside the spans were written, or bytes inside were not"


def test_zero_spans_odd_bytes_and_arguments(env):
    """Byte-granular spans (1, 3, 17, 35 bytes at odd addresses) and the argument checks."""
    lib, S, ops, _lib = env
    buf = torch.full((256,), 0x5A, dtype=torch.uint8, device=DEV)
    base = buf.data_ptr()
    spans = [(1, 1), (5, 3), (19, 17), (77, 35)]
    arr = (S["MmsZeroSpan"] * 31)()
    want = buf.cpu().numpy().copy()
    for i, (o, sz) in enumerate(spans):
        arr[i] = S["MmsZeroSpan"](base + o, sz)
        want[o:o + sz] = 0
    _lib.check(lib.mms_zero_spans_group(arr, len(spans), ops.stream()), "mms_zero_spans_group")
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), want)
    for i in range(31):
        arr[i] = S["MmsZeroSpan"](base, 4)
    assert lib.mms_zero_spans_group(arr, 0, ops.stream()) == -1
    assert lib.mms_zero_spans_group(arr, 31, ops.stream()) == -1
    assert lib.mms_zero_spans_group(None, 1, ops.stream()) == -1
    arr[1] = S["MmsZeroSpan"](None, 4)
    assert lib.mms_zero_spans_group(arr, 2, ops.stream()) == -1
    arr[1] = S["MmsZeroSpan"](base, 0)
    assert lib.mms_zero_spans_group(arr, 2, ops.stream()) == -1
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), want)         # nothing was launched


# =====================================================================================================================
# Cox: one launch for n <= 256
# =====================================================================================================================
def _cox_inputs(n, scenario, seed):
    rng = np.random.default_rng(seed)
    h = rng.normal(0, 1.5, n).astype(np.float32)
    time = (rng.exponential(500, n) + 1).astype(np.float32)
    event = (rng.random(n) < 0.6).astype(np.float32)
    valid = None
    if scenario == "censored":
        event[:] = 0
    elif scenario == "events":
        event[:] = 1
    elif scenario == "ties":
        time = np.floor(time / 400).astype(np.float32) + 1          # a handful of distinct times
    elif scenario == "invalid":
        valid = (rng.random(n) < 0.7).astype(np.float32)
        valid[0] = 0
    return h, time, event, valid


@pytest.mark.parametrize("ties", ["breslow", "efron"])
@pytest.mark.parametrize("scenario", ["plain", "censored", "events", "ties", "invalid"])
@pytest.mark.parametrize("n", [1, 2, 4, 5, 256, 257])
def test_cox_one_launch_equals_two(env, n, scenario, ties):
    """Form 0 (n <= 256: one launch; 257: the two kernels) against form 1 (always the two kernels), two models per launch: lse, tie_frac,
    out and dh bit for bit."""
    lib, S, ops, _lib = env
    ng, mode = 2, ops.TIE_MODES[ties]
    ins = [_cox_inputs(n, scenario, 17 * n + g) for g in range(ng)]
    res = {}
    for form in (0, 1):
        arr = (S["CoxP"] * ng)()
        live = []
        for g, (h, t, e, v) in enumerate(ins):
            hd = torch.zeros(n, 3, device=DEV); hd[:, 1] = torch.tensor(h)          # (a strided hazard column, as the engines pass it)
            td, ed = torch.tensor(t, device=DEV), torch.tensor(e, device=DEV)
            vd = torch.tensor(v, device=DEV) if v is not None else None
            lse, dh = torch.full((n,), float("nan"), device=DEV), torch.full((n, 2), float("nan"), device=DEV)
            out = torch.full((2,), float("nan"), device=DEV)
            frac = torch.full((n,), float("nan"), device=DEV) if mode == 1 else None
            arr[g] = S["CoxP"](hd[:, 1:].data_ptr(), 3, td.data_ptr(), ed.data_ptr(), ops.ptr(vd), n, 0.5 + g, lse.data_ptr(), dh.data_ptr(), 2,
                               out.data_ptr(), mode, ops.ptr(frac))
            live.append((hd, td, ed, vd, lse, dh, out, frac))
        _lib.check(lib.mms_cox_fwd_bwd_group_form(arr, ng, form, ops.stream()), "mms_cox_fwd_bwd_group_form")
        torch.cuda.synchronize()
        res[form] = live
    for g in range(ng):
        for name, a, b in zip(("lse", "dh", "out", "tie_frac"), res[0][g][4:], res[1][g][4:]):
            if a is not None:
                assert torch.equal(_bits(a), _bits(b)), (name, a, b)
        lse, dh, out = res[0][g][4:7]
        assert not bool(torch.isnan(lse).any()) and not bool(torch.isnan(dh[:, 0]).any()) and not bool(torch.isnan(out).any())
        assert bool(torch.isnan(dh[:, 1]).all())
    assert lib.mms_cox_fwd_bwd_group_form(arr, ng, 2, ops.stream()) == -1


# =====================================================================================================================
# gradient norm
# =====================================================================================================================
@pytest.mark.parametrize("ng", [1, 2])
@pytest.mark.parametrize("n", [3, 16, 4099, (1 << 15) + 5, (1 << 20) + 5, (1 << 22) + 7])
def test_grad_sumsq(env, n, ng):
    """sumsq of mms_grad_sumsq_group (form 0: 1024-thread workgroups) against torch's fp64 sum of the same buffer.  The bound is measured
    here, not chosen: twice the relative error of the form before round 11 (form 1) on that buffer; both errors and the bound are printed.
    n = 3 and 16 are one thread's tail and one float4; 4099 a full 256-thread workgroup's four loads plus a 3-float tail; 2^20 + 5 gives 257
    workgroups of 256 threads, a ragged last trip and a tail -- not a multiple of four, so form 0 keeps them; 2^15 + 5 (8 workgroups -> 2 of
    1024 threads) and 2^22 + 7 (the capped grid: 1024 -> 256, the form the training step runs) are where form 0 differs.  step, acc and rng
    advance exactly once per call and per model in both forms."""
    lib, S, ops, _lib = env
    arr = (S["AdamP"] * ng)()
    live = []
    for g in range(ng):
        gen = torch.Generator().manual_seed(n + g)
        grad = _d(torch.randn(n, generator=gen) * (0.5 + g))
        st = dict(sumsq=torch.zeros(1, dtype=torch.float64, device=DEV), step=torch.zeros(1, device=DEV), acc=torch.zeros(4, device=DEV),
                  cox_out=torch.tensor([0.75 + g, 1.0], device=DEV), entropy=torch.tensor([-1.25 - g], device=DEV),
                  rng=torch.tensor([11, 40 + g], dtype=torch.int32, device=DEV), hyper=torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0], device=DEV))
        arr[g] = ops.adam_params(grad, grad, grad, grad, st["hyper"], st["sumsq"], st["step"], None, False, acc=st["acc"], cox_out=st["cox_out"],
                                 entropy=st["entropy"], rng=st["rng"])
        live.append((grad, st, float((grad.double() ** 2).sum())))
    err = {}
    for call, form in enumerate((1, 0)):
        for _, st, _ in live:
            st["sumsq"].zero_()
        _lib.check(lib.mms_grad_sumsq_group_form(arr, ng, form, ops.stream()), "mms_grad_sumsq_group_form")
        torch.cuda.synchronize()
        err[form] = [abs(float(st["sumsq"]) - want) / want for _, st, want in live]
        for g, (_, st, _) in enumerate(live):
            assert float(st["step"]) == call + 1 and int(st["rng"][1]) == 40 + g + call + 1 and int(st["rng"][0]) == 11
            assert st["acc"].tolist() == [(call + 1) * (0.75 + g), call + 1.0, (call + 1) * (-1.25 - g), call + 1.0]
    for g in range(ng):
        print(f"n={n} ng={ng} model {g}: relative error of the earlier form {err[1][g]:.3e}, bound {2 * err[1][g]:.3e}, this form {err[0][g]:.3e}")
        assert err[0][g] <= 2 * err[1][g], (err[0][g], err[1][g])
    assert lib.mms_grad_sumsq_group_form(arr, ng, 2, ops.stream()) == -1


# =====================================================================================================================
# the step in a graph
# =====================================================================================================================
def test_fold_group_graph_replay_equals_eager():
    """Two PartialModalityNet members (gate, entropy word, every changed head launch but the DenseNet head) on the 3-conv encoder, batch 4:
    three graph-replayed training steps against three eager ones of twin models, on three different batches.  lr = 0: the encoder's weight
    gradients are fp32 atomic sums whose order differs between any two runs, so with moving weights the later losses would differ in their
    last bits between two EAGER runs as well; with the weights at rest every loss is a function of the forward alone and must be the same
    bits -- while the zeroing launch, the Cox launch, the merged backward launches and the bookkeeping in the gradient-norm launch all run
    inside the graph (an accumulator that was not zeroed, or zeroed out of order, shows in the entropy sums and the step counters).
    The zeroing launch's main spans are seen through the gradients: after every step each member's flat gradient and its sum of squares,
    graph against eager.  They are not the same bits (the atomic sums above), so the flat gradient is held to the 2e-5 of its largest
    element that tests/test_gpu_fold_group.py holds two runs of one step to, and the sum of squares to the 1e-4 of tests/gpu_util.py; a span
    that was not zeroed, or zeroed after the backward had started, is off by the whole previous gradient -- a factor, not a rounding."""
    from multimodal_survival_prediction_amd import models as HM
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    from test_gpu_models import _batch
    B, dims, rna_dim, G = 4, (16, 16, 8), 64, 2
    old = HM.USE_MONAI
    HM.USE_MONAI = False
    try:
        base = []
        for g in range(G):
            torch.manual_seed(200 + g)
            base.append(HM.PartialModalityNet(rna_dim=rna_dim))
    finally:
        HM.USE_MONAI = old
    eng = {k: FoldGroupEngine([copy.deepcopy(m).to(DEV).train() for m in base], lr=0.0, weight_decay=1e-4) for k in ("graph", "eager")}
    valid = torch.tensor([1, 1, 0, 1], dtype=torch.float32)
    losses, grads = {k: [] for k in eng}, {k: [] for k in eng}
    for it in range(3):
        batches = []
        for g in range(G):
            ct, rna, clin, t, e, mask = _batch(B, dims, rna_dim, 70 + 10 * it + g)
            batches.append(dict(ct=ct, rna=rna, clinical=clin, mask=mask, time=t, event=e, valid=valid))
        for k, ge in eng.items():
            ge.train_step(batches, skip_if_unusable=False, use_graph=(k == "graph"))
            torch.cuda.synchronize()
            GP = ge.plan(B, dims)
            losses[k].append([P.cox_out.clone() for P in GP.Ps])
            grads[k].append([(e_.gflat.clone(), e_.sumsq.clone()) for e_ in ge.engines])
    for it in range(3):
        for a, b in zip(losses["graph"][it], losses["eager"][it]):
            assert torch.equal(_bits(a), _bits(b)), (it, a, b)
        for (ga, sa), (gb, sb) in zip(grads["graph"][it], grads["eager"][it]):
            assert float(gb.abs().max()) > 0 and float(sb) > 0
            assert_close(ga, gb, 2e-5, f"flat gradient after step {it}")
            assert_close(sa, sb, 1e-4, f"sum of squares after step {it}")
    sg, se = eng["graph"].epoch_stats(), eng["eager"].epoch_stats()
    for g in range(G):
        assert sg[g]["n_batches"] == se[g]["n_batches"] == 3 and sg[g]["n_usable"] == se[g]["n_usable"]
        assert sg[g]["sum_loss"] == se[g]["sum_loss"]
        # a step's entropy word is the fp32 atomic sum of 4 rows' terms of one sign, in any order: <= 3 roundings of 2^-24 relative per step
        assert abs(sg[g]["sum_entropy"] - se[g]["sum_entropy"]) <= 4e-7 * abs(se[g]["sum_entropy"])
        assert int(eng["graph"].engines[g].rng[1]) == int(eng["eager"].engines[g].rng[1]) == 3
        assert float(eng["graph"].engines[g].step_count) == float(eng["eager"].engines[g].step_count) == 3.0
