"""Duplicate zero samples (MmsDnOpts.dup_zero, include/mmsurv.h): the all-zero volumes of a model's batch are identical to one another
through the whole forward, so the multi-tap conv2 forward kernel (dense block 1 of the real volumes) computes the first of them and stores
its tiles to the others; the statistic partials are multiplied by the number of zero samples.  Which samples are zero is read from words
that the boxed conv0 forward leaves (mms_conv0_fwd_group_zw): a sample is zero iff its word equals the boxes per sample.

Checked here, through the group entry points, for the compacting form (dup_zero = 0), the masking form (1) and off (-1):
  * op level: volume 32x32x16 -> conv0 16x16x8 (32 boxes per sample) -> block-1 grid 8x8x4 = 256 rows per sample, two models;
    B = 3 on the 32-row tiles (conv3_mt = 3), B = 4 on the 64-row tiles (conv3_mt = 2 needs M >= 1024).  The words come from a real conv0
    forward of the volumes.  Slab columns: bit-identical to dup_zero = -1 and within 1e-4 of the maximum of torch's
    (tests/test_gpu_dn_fwd_ops.py).  Statistics: |difference| <= 1e-10 * sum |terms| (tests/test_gpu_conv0_zero_skip.py).
  * hand-written words, a grid whose rows per sample are no multiple of the tile height, eval mode;
  * network level and the words' lifetime across graph replays: see the tests.
"""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_util import DEV, assert_close, cl, rel_err

DIMS, OD, PD = (32, 32, 16), (16, 16, 8), (8, 8, 4)
ZBPS = (OD[0] // 4) * (OD[1] // 4) * (OD[2] // 4)        # 32 boxes per sample
RPS = PD[0] * PD[1] * PD[2]                                # 256 rows per sample in block 1
# zero samples per pattern (B = 3; at B = 4 sample 3 is real unless "all"), and what else the pattern does
PATTERNS = {"none": (), "one": (1,), "z02": (0, 2), "z12": (1, 2), "all": None, "negzero": (0, 2), "corner": (0, 1, 2)}
PAIRS = [("none", "z02"), ("one", "z12"), ("all", "corner"), ("negzero", "all"), ("z12", "z12")]
MODES = (0, 1, -1)


def _env():
    from multimodal_survival_prediction_amd import _lib, ops
    return _lib.load_library(), _lib.structs(), ops


def _zero_set(kind, B):
    """the samples that are all-zero volumes"""
    if kind == "all":
        return tuple(range(B))
    if kind == "corner":
        return (0, 1)               # sample 2 holds one non-zero voxel: it must count as real
    return PATTERNS[kind]


def _volume(kind, B, seed):
    x = torch.rand(B, *DIMS, generator=torch.Generator().manual_seed(seed)) + 0.05
    for b in (range(B) if kind == "all" else PATTERNS[kind]):
        x[b] = -0.0 if kind == "negzero" else 0.0
    if kind == "corner":
        x[2, DIMS[0] - 1, DIMS[1] - 1, DIMS[2] - 1] = 1.5
    return x


_STEM = {}


def _stem(kind, B, slot):
    """Per (pattern, B, member slot): the volume and the zero-sample words a real conv0 forward of it leaves -- computed once, left unchanged."""
    key = (kind, B, slot)
    if key in _STEM:
        return _STEM[key]
    lib, S, ops = _env()
    seed = 1000 + 100 * list(PATTERNS).index(kind) + 10 * B + slot
    g = torch.Generator().manual_seed(seed)
    x = _volume(kind, B, seed + 1)
    w = torch.randn(64, 343, generator=g) / 343 ** 0.5
    M0 = B * OD[0] * OD[1] * OD[2]
    xd, wd = x.to(DEV).contiguous(), w.to(DEV).contiguous()
    y0 = torch.full((M0, 64), float("nan"), device=DEV)
    s, q = torch.zeros(64, dtype=torch.float64, device=DEV), torch.zeros(64, dtype=torch.float64, device=DEV)
    words = torch.zeros(64, dtype=torch.int32, device=DEV)
    coords = ops.init_coords(B, OD, DEV)
    p = S["Conv0FwdP"](xd.data_ptr(), ops.dims3(DIMS), ops.dims3(OD), coords.data_ptr(), M0, wd.data_ptr(), y0.data_ptr(), s.data_ptr(), q.data_ptr())
    zw = (ctypes.c_void_p * 1)(words.data_ptr())
    from multimodal_survival_prediction_amd import _lib
    _lib.check(lib.mms_conv0_fwd_group_zw(ctypes.byref(p), zw, 1, None, ops.stream()), "mms_conv0_fwd_group_zw")
    torch.cuda.synchronize()
    zs = _zero_set(kind, B)
    assert [int(v) == ZBPS for v in words[:B].cpu()] == [b in zs for b in range(B)], (kind, words[:B].cpu())
    assert int(words[B:].abs().max()) == 0
    assert not bool(torch.isnan(y0).any())
    _STEM[key] = dict(kind=kind, B=B, zs=zs, words=words)
    return _STEM[key]


def _check_stats(s, s2, terms, what):
    d = (s - s2).abs()
    print(f"{what}: statistics against dup_zero = -1: {float(d.max()):.2e}")
    assert bool((d <= 1e-10 * terms).all()), what


# ---- conv2 (multi-tap kernel) -----------------------------------------------------------------------------------------------------------
_C3 = {}


def _c3_case(kind, B, slot, distinct=False):
    """y1 of a block-1 layer: random per sample, the zero samples' rows identical (as the layers before leave them) unless `distinct`;
    weights, BatchNorm block and the torch references.  Once per key, left unchanged."""
    key = (kind, B, slot, distinct)
    if key in _C3:
        return _C3[key]
    st = _stem(kind, B, slot)
    g = torch.Generator().manual_seed(5000 + 100 * list(PATTERNS).index(kind) + 10 * B + slot)
    y1 = torch.randn(B, 128, *PD, generator=g) + 0.1
    if not distinct and len(st["zs"]) > 1:
        for b in st["zs"][1:]:
            y1[b] = y1[st["zs"][0]]
    gamma, beta = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g) * 0.1
    rm, rv = torch.randn(128, generator=g) * 0.2, torch.rand(128, generator=g) + 0.5
    w = torch.randn(32, 128, 3, 3, 3, generator=g) / (128 * 27) ** 0.5
    ref = {t: cl(F.conv3d(F.relu(F.batch_norm(y1, None if t else rm.clone(), None if t else rv.clone(), gamma, beta, training=bool(t), momentum=0.0, eps=1e-5)),
                          w, padding=1)) for t in (1, 0)}
    _, _, ops = _env()
    y1d = cl(y1).to(DEV)
    wpf, _ = ops.pack_conv3(w.to(DEV))
    _C3[key] = dict(kind=kind, B=B, zs=st["zs"], words=st["words"], y1=y1d, s=y1d.double().sum(0), q=(y1d.double() ** 2).sum(0), wpf=wpf, ref=ref,
                    gamma=gamma.to(DEV), beta=beta.to(DEV), rm=rm.to(DEV), rv=rv.to(DEV))
    return _C3[key]


def _run_c3(cases, mode, train, mt, words=None, dims=PD):
    """mms_conv3_fwd_group on the members -> [(slab [M, 256], sum, sumsq)]"""
    lib, S, ops = _env()
    from multimodal_survival_prediction_amd import _lib
    keep, blocks = [], []
    for i, c in enumerate(cases):
        M = c["y1"].shape[0]
        B = M // (dims[0] * dims[1] * dims[2])
        coords = ops.init_coords(B, dims, DEV)
        bn = ops.bnsrc(c["gamma"], c["beta"], M, train, c["s"], c["q"], c["rm"], c["rv"])
        slab = torch.full((M, 256), float("nan"), device=DEV)
        s1, q1 = torch.zeros(32, dtype=torch.float64, device=DEV), torch.zeros(32, dtype=torch.float64, device=DEV)
        p = S["Conv3FwdP"](c["y1"].data_ptr(), coords.data_ptr(), ops.dims3(dims), M, c["wpf"].data_ptr(), slab[:, 64:96].data_ptr(), 256, bn,
                           s1.data_ptr() if train else None, q1.data_ptr() if train else None, None, 27)
        wd = c["words"] if words is None else words[i]
        p.zwords, p.zbps = wd.data_ptr(), ZBPS           # (dup_zero = -1 must ignore them)
        keep.append((slab, s1, q1, coords, wd))
        blocks.append(p)
    arr = (S["Conv3FwdP"] * len(cases))(*blocks)
    o = ops.dn_opts(conv3_mt=mt, conv3_small=-1, dup_zero=mode)
    _lib.check(lib.mms_conv3_fwd_group(arr, len(cases), ctypes.byref(o), ops.stream()), "mms_conv3_fwd_group")
    torch.cuda.synchronize()
    return [k[:3] for k in keep]


def _check_c3(cases, res, train, tag):
    for i, c in enumerate(cases):
        slab2, s2, q2 = res[-1][i]
        ref = c["ref"][1 if train else 0]
        v = slab2[:, 64:96].double()
        for m in (0, 1):
            slab, s, q = res[m][i]
            what = "conv2 %s %s mode %d %s" % (c["kind"], tag, m, "train" if train else "eval")
            assert torch.equal(slab[:, 64:96], slab2[:, 64:96]), what
            assert bool(torch.isnan(slab[:, :64]).all()) and bool(torch.isnan(slab[:, 96:]).all()), what
            assert_close(slab[:, 64:96], ref, 1e-4, what)
            if train:
                _check_stats(s, s2, v.abs().sum(0), what + " sum")
                _check_stats(q, q2, (v * v).sum(0), what + " sumsq")
                assert_close(s, ref.double().sum(0), 1e-4, what + " sum")
                assert_close(q, (ref.double() ** 2).sum(0), 1e-4, what + " sumsq")


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B,mt", [(3, 3), (4, 2)], ids=["tile32", "tile64"])
@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(p) for p in PAIRS])
def test_conv3_fwd(pair, B, mt, train):
    cases = [_c3_case(k, B, i) for i, k in enumerate(pair)]
    res = {m: _run_c3(cases, m, train, mt) for m in MODES}
    _check_c3(cases, res, train, "tile%d" % (32 if mt == 3 else 64))


def _hand(vals):
    w = torch.zeros(64, dtype=torch.int32, device=DEV)
    w[:len(vals)] = torch.tensor(vals, dtype=torch.int32)
    return w


@pytest.mark.parametrize("B,mt", [(3, 3), (4, 2)], ids=["tile32", "tile64"])
def test_hand_written_words(B, mt):
    """Samples with DIFFERENT rows.  Words unequal to the boxes per sample -- smaller, larger, never written -- give the full computation;
    words that do say 'zero' for samples 0 and 2 give sample 2 the rows of sample 0, which shows that the words are what decides (and
    that the comparisons above are not between two full computations)."""
    cases = [_c3_case("none", B, i, distinct=True) for i in range(2)]
    full = _run_c3(cases, -1, True, mt)
    for vals in ([ZBPS - 1, 0, ZBPS - 1], [ZBPS + 1, ZBPS + 1, ZBPS + 1], [0, 0, 0], [ZBPS, 1, ZBPS - 1], [2 * ZBPS, ZBPS, 7]):
        words = [_hand(vals), _hand(vals[::-1])]
        for m in (0, 1):
            for (a, s, q), (a2, s2, q2) in zip(_run_c3(cases, m, True, mt, words), full):
                assert torch.equal(a[:, 64:96], a2[:, 64:96]), (vals, m)
                assert bool((s - s2).abs().max() <= 1e-10 * a2[:, 64:96].double().abs().sum(0).max())
    words = [_hand([ZBPS, 0, ZBPS]), _hand([0, 0, 0])]
    for m in (0, 1):
        (a, s, q), (b, _, _) = _run_c3(cases, m, True, mt, words)
        a2, b2 = full[0][0], full[1][0]
        assert torch.equal(a[:2 * RPS, 64:96], a2[:2 * RPS, 64:96]) and torch.equal(a[3 * RPS:, 64:96], a2[3 * RPS:, 64:96])
        assert torch.equal(a[2 * RPS:3 * RPS, 64:96], a2[:RPS, 64:96]) and not torch.equal(a[2 * RPS:3 * RPS, 64:96], a2[2 * RPS:3 * RPS, 64:96])
        assert torch.equal(b[:, 64:96], b2[:, 64:96])
        v0 = a2[:RPS, 64:96].double().sum(0)            # the statistics count sample 0 twice, sample 2 not
        want = full[0][1] - a2[2 * RPS:3 * RPS, 64:96].double().sum(0) + v0
        assert bool(((s - want).abs() <= 1e-9 * a2[:, 64:96].double().abs().sum(0)).all())


def test_rows_per_sample_not_a_multiple_of_the_tile():
    """Block-1 grid 5x4x4 = 80 rows per sample (B = 3 on the 32-row tiles; B = 13, 1040 rows, on the 64-row tiles): a sample is no whole
    number of tiles, so the feature turns itself off for the launch -- words that say 'zero' for samples with different rows change nothing,
    and the result is torch's."""
    _, _, ops = _env()
    dims = (5, 4, 4)
    for B, mt in ((3, 3), (13, 2)):
        g = torch.Generator().manual_seed(77 + B)
        y1 = torch.randn(B, 128, *dims, generator=g) + 0.1
        gamma, beta = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g) * 0.1
        w = torch.randn(32, 128, 3, 3, 3, generator=g) / (128 * 27) ** 0.5
        ref = cl(F.conv3d(F.relu(F.batch_norm(y1, None, None, gamma, beta, training=True, eps=1e-5)), w, padding=1))
        y1d = cl(y1).to(DEV)
        c = dict(y1=y1d, s=y1d.double().sum(0), q=(y1d.double() ** 2).sum(0), wpf=ops.pack_conv3(w.to(DEV))[0], gamma=gamma.to(DEV), beta=beta.to(DEV),
                 rm=None, rv=None)
        words = [_hand([ZBPS] * B)]
        full = _run_c3([c], -1, True, mt, words, dims)[0]
        assert_close(full[0][:, 64:96], ref, 1e-4, "conv2 80 rows per sample")
        for m in (0, 1):
            got = _run_c3([c], m, True, mt, words, dims)[0]
            assert torch.equal(got[0][:, 64:96], full[0][:, 64:96]), (B, m)
            assert bool(((got[1] - full[1]).abs() <= 1e-10 * full[0][:, 64:96].double().abs().sum(0)).all())


# ---- network level ----------------------------------------------------------------------------------------------------------------------
def _network(train):
    """mms_dn121_forward_group (+ mms_dn121_backward_group), 2 members, B = 8 at 32x32x32 (block 1: 512 rows per sample on the multi-tap
    kernel's 32-row tiles): member 0's batch is all zero, member 1 has two zero samples.  -> per dup_zero setting: outputs, buffers, gradients,
    the words"""
    from multimodal_survival_prediction_amd import _lib, ops
    from test_gpu_dead_backward import _grads, _ptrs, _zero_grads
    from test_gpu_densenet import _make, structured_volumes
    lib = _lib.load_library()
    Bn, dims = 8, (32, 32, 32)
    D, H, W = dims
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dout = [torch.randn(Bn, 128, generator=torch.Generator().manual_seed(5 + g)).to(DEV) for g in range(2)]
    res = {}
    for flag in MODES:
        nets, xs, es = [], [], []
        for g in range(2):
            _, net = _make(20 + g)
            net.train(train)
            x = structured_volumes(Bn, dims, 30 + g).to(DEV)
            if g == 0:
                x.zero_()
            else:
                x[3] = 0.0
                x[6] = 0.0
            nets.append(net); xs.append(x); es.append(net._tables(x))
        opts = ops.dn_opts(nets[0]._opts(), dup_zero=flag)
        outs = [torch.empty(Bn, 128, device=DEV) for _ in range(2)]
        ws, xp = _ptrs([e["ws"].data_ptr() for e in es]), _ptrs([x.data_ptr() for x in xs])
        pt, bt = _ptrs([ctypes.addressof(e["ptab"]) for e in es]), _ptrs([ctypes.addressof(e["btab"]) for e in es])
        for net in nets:
            net.workspace_region("zero_words", 0, torch.int32).fill_(123)          # stale words: every forward clears them itself
        _lib.check(lib.mms_dn121_forward_group(2, ws, Bn, D, H, W, xp, pt, bt, _ptrs([o.data_ptr() for o in outs]), 128, 1 if train else 0,
                                               ctypes.byref(opts), st), "mms_dn121_forward_group")
        torch.cuda.synchronize()
        words = [net.workspace_region("zero_words", 0, torch.int32)[:Bn].cpu().tolist() for net in nets]
        slab = [net.workspace_region("slab", 0).clone() for net in nets]
        grads = None
        if train:
            for net in nets:
                _zero_grads(net)
            gt = [net._grad_table() for net in nets]
            _lib.check(lib.mms_dn121_backward_group(2, ws, Bn, D, H, W, xp, pt, _ptrs([d.data_ptr() for d in dout]), 128,
                                                    _ptrs([ctypes.addressof(t) for t in gt]), ctypes.byref(opts), st), "mms_dn121_backward_group")
            torch.cuda.synchronize()
            grads = [_grads(net) for net in nets]
        res[flag] = dict(outs=[o.clone() for o in outs], bufs=[[b.detach().clone() for b in net.buffers()] for net in nets], grads=grads, words=words,
                         slab=slab)
    return res


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_network_group(train):
    """Default (and the masking form) against dup_zero = -1 over forward + backward, at the criterion of
    tests/test_gpu_conv0_zero_skip.py::test_network_group: the statistics of every BatchNorm layer are accumulated with fp64 atomics whose
    order varies from run to run under either setting, so features and BatchNorm buffers are held to 1e-6 of their maximum (two runs of the
    same code: tests/test_gpu_models.py::test_run_twice_spread), every gradient tensor to 1e-4 of its maximum, tensors below 1e-5 of the
    largest left out.  Eval mode has no such sums: features bit for bit."""
    from test_gpu_dead_backward import _spread
    res = _network(train)
    bps = 4 * 4 * 4
    for flag in MODES:
        w = res[flag]["words"]
        if flag < 0:
            assert w == [[0] * 8, [0] * 8], w                    # cleared, never written
        else:
            assert w[0] == [bps] * 8 and [v == bps for v in w[1]] == [b in (3, 6) for b in range(8)], w
    for flag in (0, 1):
        for g in range(2):
            a, b = res[flag], res[-1]
            assert not bool(torch.isnan(a["outs"][g]).any())
            if not train:
                assert torch.equal(a["outs"][g], b["outs"][g]) and torch.equal(a["slab"][g], b["slab"][g]), (flag, g)
                continue
            e = rel_err(a["outs"][g], b["outs"][g])
            worst_buf = 0.0
            for u, v in zip(a["bufs"][g], b["bufs"][g]):
                if u.dtype.is_floating_point:
                    worst_buf = max(worst_buf, rel_err(u, v))
                else:
                    assert torch.equal(u, v)
            worst = _spread(a["grads"][g], b["grads"][g])
            print(f"dup_zero {flag}, member {g}: features {e:.2e}, BatchNorm buffers {worst_buf:.2e}, gradients (worst tensor) {worst:.2e}")
            assert e <= 1e-6 and worst_buf <= 1e-6 and worst <= 1e-4, (flag, g, e, worst_buf, worst)


def test_word_lifetime_through_graph():
    """FoldGroupEngine, two PartialModalityNet members, graph-replayed steps at lr = 0 on the same engine and the same graph: a step whose
    batches hold zero volumes (member 0: all four; member 1: none), then a step on all-real volumes, then one with the roles swapped.  The
    default against dup_zero = -1 from the same state: the words after every step say what the step's batch held -- they are cleared by every
    forward -- and losses and gradients of every step agree within the run-to-run spread (tests/test_gpu_dead_backward.py: 1e-4 of a tensor's
    maximum, tensors below 1e-5 of the largest left out; losses 1e-5)."""
    from multimodal_survival_prediction_amd import _lib
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    from test_gpu_dead_backward import _masked_cohort, _seq_models, _spread, _tensors
    B, dims, rna_dim = 4, (64, 64, 32), 64
    cohort = _masked_cohort(dims, rna_dim)            # patients 8..15 have no CT: all-zero volumes
    steps = [([[8, 9, 10, 11], [0, 1, 2, 3]], ((0, 1, 2, 3), ())), ([[4, 5, 6, 7], [0, 1, 2, 3]], ((), ())),
             ([[0, 1, 12, 13], [12, 4, 13, 14]], ((2, 3), (0, 2, 3)))]
    base = _seq_models(rna_dim)
    bps = (dims[0] // 8) * (dims[1] // 8) * (dims[2] // 8)
    off, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.check(_lib.load_library().mms_dn121_region(B, *dims, b"zero_words", 0, ctypes.byref(off), ctypes.byref(nb)), "mms_dn121_region")
    runs = {}
    for flag in (0, -1):
        ge = FoldGroupEngine([copy.deepcopy(m).to(DEV).train() for m in base], lr=0.0, weight_decay=1e-4, dn_opts=dict(dup_zero=flag))
        losses, grads, words = [], [], []
        for idx, _ in steps:
            ge.reset_epoch_stats()
            ge.train_step_indexed(cohort, idx, skip_if_unusable=False, use_graph=True)
            torch.cuda.synchronize()
            losses.append([s["sum_loss"] for s in ge.epoch_stats()])
            grads.append([e.gflat.clone() for e in ge.engines])
            GP = next(iter(ge.plans.values()))
            words.append([P.ws[off.value:off.value + 4 * B].view(torch.int32).cpu().tolist() for P in GP.Ps])
        runs[flag] = dict(ge=ge, losses=losses, grads=grads, words=words)
    a, b = runs[0], runs[-1]
    for it, (_, zs) in enumerate(steps):
        assert [[v == bps for v in w] for w in a["words"][it]] == [[s in z for s in range(B)] for z in zs], (it, a["words"][it])
        assert b["words"][it] == [[0] * B, [0] * B], (it, b["words"][it])
        for g in range(2):
            la, lb = a["losses"][it][g], b["losses"][it][g]
            assert abs(la - lb) <= 1e-5 * max(1.0, abs(lb)), (it, g, la, lb)
            worst = _spread(_tensors(a["ge"].engines[g], a["grads"][it][g]), _tensors(b["ge"].engines[g], b["grads"][it][g]))
            print(f"step {it}, member {g}: worst per-tensor gradient difference dup_zero 0 vs -1 {worst:.2e}")
            assert worst <= 1e-4, (it, g, worst)
