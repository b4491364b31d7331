"""Identical samples in the backward of block 1's conv2 (MmsDnOpts.dup_zero_bwd, include/mmsurv.h): the gradient rows of a batch's all-zero
volumes are identical where their rows of dout are all zero.  The head launch leaves the bit mask of those samples in the word "bwd_dup";
the multi-tap backward-data kernel computes the lowest of them and stores its tiles to the others, the multi-tap weight-gradient kernel
walks the remaining rows and counts the lowest sample's once per sample of the mask.

Checked here through the group entry points, on the shapes of tests/test_gpu_dup_zero.py (block-1 grid 8x8x4 = 256 rows per sample, B = 3
and 4, two members per launch, conv3_mt = 3 / conv3w_mt = 2 to reach the two kernels):
  * the word's producer (mms_head_bwd_group_dup) on zero-word patterns x dout rows;
  * backward-data: dbn bit-identical to dup_zero_bwd = -1, sums within 1e-10 x sum |terms| of it, both within 1e-4 of torch;
  * weight gradient, three layouts, msplit 1 and 5: within 1e-4 of torch and of the off setting (fp32 atomics: neither side is bit-stable);
  * hand-written masks on samples with DIFFERENT rows -- the word decides; rows per sample of 80 -- the feature turns itself off;
  * network level and the word's lifetime through one captured graph.
"""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_util import DEV, assert_close, cl, rel_err

PD = (8, 8, 4)
RPS = PD[0] * PD[1] * PD[2]                # 256 rows per sample
ZBPS = 32                                  # boxes per sample of the conv0 grid 16x16x8 above it
SETS = {"none": (), "one": (1,), "z02": (0, 2), "z12": (1, 2), "all": None}
PAIRS = [("none", "z02"), ("one", "z12"), ("all", "z02"), ("z12", "all")]


def _env():
    from multimodal_survival_prediction_amd import _lib, ops
    return _lib.load_library(), _lib.structs(), ops, _lib


def _set(kind, B):
    return tuple(range(B)) if kind == "all" else SETS[kind]


def _mask(samples):
    return sum(1 << b for b in samples) if len(samples) >= 2 else 0


def _word(v):
    return torch.tensor([v if v < 2 ** 31 else v - 2 ** 32], dtype=torch.int32, device=DEV)


# ---- the word's producer ----------------------------------------------------------------------------------------------------------------
def _head(douts, words, zbps=ZBPS, N=128, preset=0x5A5A5A5A):
    """mms_head_bwd_group_dup on one member per (dout, zero words) pair -> [(bwd_live, bwd_dup)]"""
    lib, S, ops, _lib = _env()
    C, V = 64, 2
    keep, blocks, lives, dups, zws = [], [], [], [], []
    for dout, zw in zip(douts, words):
        B = dout.shape[0]
        g = torch.Generator().manual_seed(3)
        slab = (torch.randn(B * V, C, generator=g) + 0.2).to(DEV)
        gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.1).to(DEV)
        s, q = slab.double().sum(0), (slab.double() ** 2).sum(0)
        bn = ops.bnsrc(gamma, beta, B * V, True, s, q)
        pooled, w = torch.randn(B, C, generator=g).to(DEV), torch.randn(N, C, generator=g).to(DEV)
        dw, db, dg, dbe = torch.zeros(N, C, device=DEV), torch.zeros(N, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        dslab = torch.zeros(B * V, C, device=DEV)
        d = dout.to(DEV).contiguous()
        blocks.append(S["HeadBwdP"](d.data_ptr(), d.stride(0), pooled.data_ptr(), slab.data_ptr(), C, C, B, V, bn, w.data_ptr(), N,
                                    dw.data_ptr(), db.data_ptr(), dg.data_ptr(), dbe.data_ptr(), dslab.data_ptr(), C, None))
        live, dup = torch.full((1,), 77, dtype=torch.int32, device=DEV), torch.full((1,), preset, dtype=torch.int32, device=DEV)
        z = None if zw is None else zw.to(DEV)
        keep.append((slab, gamma, beta, s, q, pooled, w, dw, db, dg, dbe, dslab, d, z))
        lives.append(live); dups.append(dup); zws.append(z)
    n = len(blocks)
    arr = (S["HeadBwdP"] * n)(*blocks)
    P = ctypes.c_void_p * n
    _lib.check(lib.mms_head_bwd_group_dup(arr, P(*[t.data_ptr() for t in lives]), P(*[None if z is None else z.data_ptr() for z in zws]), zbps,
                                          P(*[t.data_ptr() for t in dups]), n, ops.stream()), "mms_head_bwd_group_dup")
    torch.cuda.synchronize()
    return [(int(a[0]), int(b[0]) & 0xffffffff) for a, b in zip(lives, dups)]


def _zw(B, zero, val=ZBPS):
    w = torch.zeros(64, dtype=torch.int32)
    for b in zero:
        w[b] = val
    return w


def _dout(B, zero_rows, N=128, seed=9):
    d = torch.randn(B, N, generator=torch.Generator().manual_seed(seed))
    for b in zero_rows:
        d[b] = 0.0
    return d


@pytest.mark.parametrize("B", [3, 4])
def test_word_producer(B):
    """Zero-word patterns x dout rows -> the expected masks (fewer than two samples -> 0); two members per launch."""
    cases = []          # (zero words' samples, zero dout rows, expected D)
    for kind in SETS:
        z = _set(kind, B)
        cases.append((z, z, z))                                  # every zero sample has a zero row
        cases.append((z, (), ()))                                # no zero row at all
        cases.append((z, tuple(range(B)), z))                    # a dead batch: every row zero, the zero samples still decide
        cases.append((tuple(range(B)), z, z))                    # every sample zero, the rows decide
    for i in range(0, len(cases), 2):
        pair = cases[i:i + 2]
        got = _head([_dout(B, rows) for _, rows, _ in pair], [_zw(B, z) for z, _, _ in pair])
        for (z, rows, want), (live, dup) in zip(pair, got):
            assert dup == _mask(want), (B, z, rows, want, bin(dup))
            assert live == (1 if len(rows) < B else 0), (B, rows, live)


def test_word_producer_values():
    """One element of 1e-30 in a row of D takes the sample out; -0.0f is zero; NaN is not; words unequal to the boxes per sample -- smaller,
    larger, never written -- are no zero samples; a dout beyond the live scan, more than 32 samples, no words or no boxes per sample give 0."""
    B = 4
    tiny = _dout(B, (0, 1, 2)); tiny[1, 77] = 1e-30
    negz = _dout(B, (0, 2, 3)); negz[2] = -0.0; negz[3, 5] = -0.0
    nan = _dout(B, (0, 1, 3)); nan[3, 127] = float("nan")
    got = _head([tiny, negz], [_zw(B, range(B))] * 2)
    assert [g[1] for g in got] == [0b0101, 0b1101], got
    got = _head([nan, _dout(B, (1, 3))], [_zw(B, range(B))] * 2)
    assert [g[1] for g in got] == [0b0011, 0b1010], got
    zero = _dout(B, range(B))
    for vals in ([ZBPS - 1] * 4, [ZBPS + 1] * 4, [0] * 4, [ZBPS, 1, ZBPS - 1, 2 * ZBPS]):
        w = torch.zeros(64, dtype=torch.int32); w[:4] = torch.tensor(vals, dtype=torch.int32)
        assert _head([zero], [w])[0] == (0, 0), vals
    w = torch.zeros(64, dtype=torch.int32); w[:4] = torch.tensor([ZBPS, 0, ZBPS, ZBPS + 1], dtype=torch.int32)
    assert _head([zero], [w])[0] == (0, 0b0101)
    # dout larger than the scan (3 x 6000 > 16384 elements): live, nothing shared
    assert _head([torch.zeros(3, 6000)], [_zw(3, range(3))], N=6000)[0] == (1, 0)
    # 33 samples; no words; no boxes per sample
    assert _head([torch.zeros(33, 128)], [_zw(33, range(33))])[0] == (0, 0)
    assert _head([zero], [None])[0] == (0, 0)
    assert _head([zero], [_zw(B, range(B), 0)], zbps=0)[0] == (0, 0)


# ---- one block-1 layer: operands and torch references -----------------------------------------------------------------------------------
_LAYER = {}


def _layer(B, slot, D, distinct=False, dims=PD):
    """y1 and dz of a block-1 layer, random per sample, the rows of the samples in D identical (as the launches before leave them) unless
    `distinct`; weights, BatchNorm block, and torch's dbn / sums / dW.  Once per key, left unchanged."""
    key = (B, slot, tuple(D), distinct, dims)
    if key in _LAYER:
        return _LAYER[key]
    _, _, ops, _ = _env()
    g = torch.Generator().manual_seed(7000 + 100 * B + 10 * slot + len(D) + (5 if distinct else 0) + dims[0])
    y1 = torch.randn(B, 128, *dims, generator=g) + 0.1
    dz = torch.randn(B, 32, *dims, generator=g)
    if not distinct:
        for b in D[1:]:
            y1[b] = y1[D[0]]; dz[b] = dz[D[0]]
    gamma, beta = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g) * 0.1
    w = (torch.randn(32, 128, 3, 3, 3, generator=g) / (128 * 27) ** 0.5).requires_grad_(True)
    c = dict(B=B, D=tuple(D), dims=dims, M=B * dims[0] * dims[1] * dims[2])
    c.update(_reference(y1, dz, gamma, beta, w))
    c["y1"], c["dz"] = cl(y1).to(DEV), cl(dz).to(DEV)
    c["s"], c["q"] = c["y1"].double().sum(0), (c["y1"].double() ** 2).sum(0)
    c["gamma"], c["beta"] = gamma.to(DEV), beta.to(DEV)
    c["w"], c["wpb"] = w, ops.pack_conv3(w.detach().to(DEV))[1]
    c["coords"] = ops.init_coords(B, dims, DEV)
    _LAYER[key] = c
    return c


def _reference(y1, dz, gamma, beta, w, weight=None):
    """torch: dbn = gradient at norm2's output behind the relu mask, its BatchNorm-backward sums, dW.  weight: per-sample factors of dz in dW
    (the hand-written masks' expectation)."""
    yd = y1.double()
    mean, var = yd.mean((0, 2, 3, 4), keepdim=True), yd.var((0, 2, 3, 4), unbiased=False, keepdim=True)
    xh = ((yd - mean) / torch.sqrt(var + 1e-5)).float()
    pre = (gamma.view(1, -1, 1, 1, 1) * xh + beta.view(1, -1, 1, 1, 1)).requires_grad_(True)
    if w.grad is not None:
        w.grad = None
    F.conv3d(F.relu(pre), w, padding=1).backward(dz)
    dbn = pre.grad
    out = dict(dbn=cl(dbn), s1=cl(dbn).double().sum(0), s2=cl(dbn * xh).double().sum(0), dw=w.grad.clone(),
               t1=cl(dbn).double().abs().sum(0), t2=cl(dbn * xh).double().abs().sum(0), xh=cl(xh))
    if weight is not None:
        w.grad = None
        pre2 = pre.detach().requires_grad_(True)
        F.conv3d(F.relu(pre2), w, padding=1).backward(dz * torch.tensor(weight, dtype=dz.dtype).view(-1, 1, 1, 1, 1))
        out["dw"] = w.grad.clone()
    return out


def _run_data(cases, flag, words):
    """mms_conv3_bwd_data_group on the members -> [(dbn, s1, s2)]"""
    lib, S, ops, _lib = _env()
    keep, blocks = [], []
    for c, wd in zip(cases, words):
        bn = ops.bnsrc(c["gamma"], c["beta"], c["M"], True, c["s"], c["q"])
        dbn = torch.full((c["M"], 128), float("nan"), device=DEV)
        s1, s2 = torch.zeros(128, dtype=torch.float64, device=DEV), torch.zeros(128, dtype=torch.float64, device=DEV)
        p = S["Conv3BwdDataP"](c["dz"].data_ptr(), 32, c["coords"].data_ptr(), ops.dims3(c["dims"]), c["M"], c["wpb"].data_ptr(), c["y1"].data_ptr(), bn,
                               dbn.data_ptr(), s1.data_ptr(), s2.data_ptr(), None, 27)
        p.dup = wd.data_ptr()                               # (dup_zero_bwd = -1 must ignore it)
        keep.append((dbn, s1, s2, wd))
        blocks.append(p)
    arr = (S["Conv3BwdDataP"] * len(cases))(*blocks)
    o = ops.dn_opts(conv3_mt=3, conv3_small=-1, dup_zero_bwd=flag)
    _lib.check(lib.mms_conv3_bwd_data_group(arr, len(cases), ctypes.byref(o), ops.stream()), "mms_conv3_bwd_data_group")
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(k[0]).any()) for k in keep)
    return [k[:3] for k in keep]


def _run_weight(cases, flag, words, layout, msplit):
    """mms_conv3_bwd_weight_group on the members -> [dW as [32, 128, 3, 3, 3]]"""
    lib, S, ops, _lib = _env()
    keep, blocks = [], []
    for c, wd in zip(cases, words):
        bn = ops.bnsrc(c["gamma"], c["beta"], c["M"], True, c["s"], c["q"])
        dw = torch.zeros({0: (32, 128, 27), 1: (27, 32, 128), 2: (32, 27, 128)}[layout], device=DEV)
        p = S["Conv3BwdWP"](c["y1"].data_ptr(), c["coords"].data_ptr(), ops.dims3(c["dims"]), c["M"], bn, c["dz"].data_ptr(), 32, dw.data_ptr(), msplit, layout)
        p.dup = wd.data_ptr()
        keep.append((dw, wd))
        blocks.append(p)
    arr = (S["Conv3BwdWP"] * len(cases))(*blocks)
    o = ops.dn_opts(conv3w_mt=2, dup_zero_bwd=flag)
    _lib.check(lib.mms_conv3_bwd_weight_group(arr, len(cases), ctypes.byref(o), ops.stream()), "mms_conv3_bwd_weight_group")
    torch.cuda.synchronize()
    perm = {0: lambda t: t, 1: lambda t: t.permute(1, 2, 0), 2: lambda t: t.permute(0, 2, 1)}[layout]
    return [perm(k[0]).reshape(32, 128, 3, 3, 3) for k in keep]


def _check_sums(a, b, terms, what):
    d = (a - b).abs()
    print(f"{what}: against dup_zero_bwd = -1: {float(d.max()):.2e}")
    assert bool((d <= 1e-10 * terms).all()), what


# ---- backward-data ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(p) for p in PAIRS])
def test_bwd_data(pair, B, flag):
    cases = [_layer(B, i, _set(k, B) if len(_set(k, B)) >= 2 else ()) for i, k in enumerate(pair)]
    words = [_word(_mask(c["D"])) for c in cases]
    off = _run_data(cases, -1, words)
    got = _run_data(cases, flag, words)
    for c, (dbn, s1, s2), (dbn0, s10, s20) in zip(cases, got, off):
        what = "backward-data B %d D %s" % (B, c["D"])
        assert torch.equal(dbn, dbn0), what
        assert_close(dbn, c["dbn"], 1e-4, what + " dbn")
        _check_sums(s1, s10, c["t1"].to(DEV), what + " s1")
        _check_sums(s2, s20, c["t2"].to(DEV), what + " s2")
        assert_close(s1, c["s1"], 1e-4, what + " s1"); assert_close(s2, c["s2"], 1e-4, what + " s2")


# ---- weight gradient --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [0, 2])
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("B,kinds,msplit", [(3, ("z02", "none"), 1), (3, ("z02", "z12"), 5), (4, ("all", "z02"), 3), (4, ("one", "z12"), 8)])
def test_bwd_weight(B, kinds, msplit, layout, flag):
    """B = 3, D = {0, 2}, msplit = 5: 768 rows give 160-row chunks that straddle samples; compacted, 512 rows give 128-row chunks and one
    empty chunk."""
    cases = [_layer(B, i, _set(k, B) if len(_set(k, B)) >= 2 else ()) for i, k in enumerate(kinds)]
    words = [_word(_mask(c["D"])) for c in cases]
    off = _run_weight(cases, -1, words, layout, msplit)
    got = _run_weight(cases, flag, words, layout, msplit)
    for c, dw, dw0 in zip(cases, got, off):
        what = "weight gradient B %d D %s msplit %d layout %d" % (B, c["D"], msplit, layout)
        print(f"{what}: torch {rel_err(dw, c['dw']):.2e}, off setting {rel_err(dw, dw0):.2e}")
        assert_close(dw0, c["dw"], 1e-4, what + " (off) against torch")
        assert_close(dw, c["dw"], 1e-4, what + " against torch")
        assert_close(dw, dw0, 1e-4, what + " against the off setting")


def test_one_consumer_options():
    """dup_zero_bwd = 2 leaves backward-data alone, 1 the weight gradient: with samples of DIFFERENT rows and a mask naming two of them the
    other consumer's result is the full one."""
    cases = [_layer(3, i, (), distinct=True) for i in range(2)]
    words = [_word(0b101)] * 2
    for (a, _, _), (b, _, _) in zip(_run_data(cases, 2, words), _run_data(cases, -1, words)):
        assert torch.equal(a, b)
    for a, c in zip(_run_weight(cases, 1, words, 2, 3), cases):
        assert_close(a, c["dw"], 1e-4, "weight gradient under dup_zero_bwd = 1")


# ---- hand-written masks, samples with different rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 4])
def test_hand_written_masks(B):
    """A mask naming samples 0 and 2 gives sample 2 the dbn rows of sample 0 and a dW that counts sample 0's rows twice and sample 2's not at
    all -- the word decides, and the comparisons above are not between two full computations.  Mask 0, a single bit, or bits >= B: the full
    result."""
    cases = [_layer(B, i, (), distinct=True) for i in range(2)]
    zero = [_word(0)] * 2
    full = _run_data(cases, -1, zero)
    for m in (0, 0b100, 1 << B, (1 << B) | 0b10, 0xffffffff & ~((1 << B) - 1), (0xffffffff & ~((1 << B) - 1)) | 1):
        words = [_word(m), _word(m)]
        for (a, s1, s2), (a0, s10, s20), c in zip(_run_data(cases, 0, words), full, cases):
            assert torch.equal(a, a0), bin(m)
            _check_sums(s1, s10, c["t1"].to(DEV), "mask %x s1" % m)
            _check_sums(s2, s20, c["t2"].to(DEV), "mask %x s2" % m)
        for a, c in zip(_run_weight(cases, 0, words, 1, 5), cases):
            assert_close(a, c["dw"], 1e-4, "weight gradient, mask %x" % m)
    words = [_word(0b101), _word(0)]
    (a, s1, s2), (b, _, _) = _run_data(cases, 0, words)
    a0, b0 = full[0][0], full[1][0]
    assert torch.equal(b, b0)
    assert torch.equal(a[:2 * RPS], a0[:2 * RPS]) and torch.equal(a[3 * RPS:], a0[3 * RPS:])
    assert torch.equal(a[2 * RPS:3 * RPS], a0[:RPS]) and not torch.equal(a[2 * RPS:3 * RPS], a0[2 * RPS:3 * RPS])
    c = cases[0]
    xh = c["xh"].to(DEV).double()
    want1 = full[0][1] - a0[2 * RPS:3 * RPS].double().sum(0) + a0[:RPS].double().sum(0)          # the sums count sample 0 twice, sample 2 not
    want2 = full[0][2] - (a0[2 * RPS:3 * RPS].double() * xh[2 * RPS:3 * RPS]).sum(0) + (a0[:RPS].double() * xh[:RPS]).sum(0)
    assert bool(((s1 - want1).abs() <= 1e-9 * c["t1"].to(DEV)).all())
    assert bool(((s2 - want2).abs() <= 1e-6 * c["t2"].to(DEV)).all())          # (xh is torch's here: fp32 rounding of the factor)
    # dW: sample 0's rows twice, sample 2's not at all, from torch
    weight = [2.0, 1.0, 0.0] + [1.0] * (B - 3)
    y1 = c["y1"].cpu().reshape(B, *PD, 128).permute(0, 4, 1, 2, 3).contiguous()
    dz = c["dz"].cpu().reshape(B, *PD, 32).permute(0, 4, 1, 2, 3).contiguous()
    want = _reference(y1, dz, c["gamma"].cpu(), c["beta"].cpu(), c["w"], weight)["dw"]
    for layout, ms in ((0, 1), (1, 5), (2, 3)):
        dw, dwb = _run_weight(cases, 0, words, layout, ms)
        assert_close(dw, want, 1e-4, "weight gradient with sample 0 counted twice (layout %d, msplit %d)" % (layout, ms))
        assert rel_err(dw, c["dw"]) > 1e-2
        assert_close(dwb, cases[1]["dw"], 1e-4, "the other member")


# ---- other placements of the workgroups ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,ng", [(PD, 1), (PD, 3), ((4, 4, 2), 1), ((4, 4, 2), 2)], ids=["one-member", "three-members", "3-tiles", "3-tiles-two"])
def test_placements(dims, ng):
    """One member and three members (every member on all eight XCDs), and a grid of 3 tiles (32 rows per sample: no XCD placement): B = 3,
    D = {0, 2} and {1, 2}."""
    cases = [_layer(3, 4 + i, ((0, 2), (1, 2), (0, 1, 2))[i], dims=dims) for i in range(ng)]
    words = [_word(_mask(c["D"])) for c in cases]
    for (a, s1, s2), (a0, s10, s20), c in zip(_run_data(cases, 0, words), _run_data(cases, -1, words), cases):
        assert torch.equal(a, a0), (dims, ng, c["D"])
        assert_close(a, c["dbn"], 1e-4, "dbn")
        _check_sums(s1, s10, c["t1"].to(DEV), "s1"); _check_sums(s2, s20, c["t2"].to(DEV), "s2")
    for a, c in zip(_run_weight(cases, 0, words, 2, 2), cases):
        assert_close(a, c["dw"], 1e-4, "dW")


# ---- the feature turns itself off -------------------------------------------------------------------------------------------------------
def test_rows_per_sample_not_a_multiple_of_32():
    """Block-1 grid 5x4x4 = 80 rows per sample: a mask naming samples with different rows changes nothing."""
    dims = (5, 4, 4)
    cases = [_layer(3, i, (), distinct=True, dims=dims) for i in range(2)]
    words = [_word(0b101), _word(0b111)]
    for (a, s1, s2), (a0, s10, s20), c in zip(_run_data(cases, 0, words), _run_data(cases, -1, words), cases):
        assert torch.equal(a, a0)
        assert_close(a, c["dbn"], 1e-4, "80 rows per sample: dbn")
        _check_sums(s1, s10, c["t1"].to(DEV), "80 rows s1"); _check_sums(s2, s20, c["t2"].to(DEV), "80 rows s2")
    for a, a0, c in zip(_run_weight(cases, 0, words, 2, 2), _run_weight(cases, -1, words, 2, 2), cases):
        assert_close(a, c["dw"], 1e-4, "80 rows per sample: dW")
        assert_close(a, a0, 1e-4, "80 rows per sample: dW against the off setting")


# ---- network level ----------------------------------------------------------------------------------------------------------------------
_NET = {}


def _network(variant):
    """mms_dn121_forward_group + _backward_group, 2 members, B = 8 at 32x32x32 (block 1: 512 rows per sample).  Member 0: all volumes zero,
    dout zero (dead).  Member 1: volumes 3 and 6 zero with zero rows of dout -- variant "row6": sample 6's row of dout is non-zero.
    -> per dup_zero_bwd setting: gradients and the words"""
    if variant in _NET:
        return _NET[variant]
    from multimodal_survival_prediction_amd import _lib, ops
    from test_gpu_dead_backward import _grads, _ptrs, _zero_grads
    from test_gpu_densenet import _make, structured_volumes
    lib = _lib.load_library()
    Bn, dims = 8, (32, 32, 32)
    D, H, W = dims
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dout = [torch.zeros(Bn, 128), torch.randn(Bn, 128, generator=torch.Generator().manual_seed(6))]
    dout[1][3] = 0.0
    if variant != "row6":
        dout[1][6] = 0.0
    dout = [d.to(DEV) for d in dout]
    res = {}
    for flag in (0, -1):
        nets, xs, es = [], [], []
        for g in range(2):
            _, net = _make(20 + g)
            net.train()
            x = structured_volumes(Bn, dims, 30 + g).to(DEV)
            if g == 0:
                x.zero_()
            else:
                x[3] = 0.0
                x[6] = 0.0
            nets.append(net); xs.append(x); es.append(net._tables(x))
        opts = ops.dn_opts(nets[0]._opts(), conv3_mt=3, conv3w_mt=2, dup_zero_bwd=flag)
        outs = [torch.empty(Bn, 128, device=DEV) for _ in range(2)]
        ws, xp = _ptrs([e["ws"].data_ptr() for e in es]), _ptrs([x.data_ptr() for x in xs])
        pt, bt = _ptrs([ctypes.addressof(e["ptab"]) for e in es]), _ptrs([ctypes.addressof(e["btab"]) for e in es])
        _lib.check(lib.mms_dn121_forward_group(2, ws, Bn, D, H, W, xp, pt, bt, _ptrs([o.data_ptr() for o in outs]), 128, 1,
                                               ctypes.byref(opts), st), "mms_dn121_forward_group")
        for net in nets:
            _zero_grads(net)
            net.workspace_region("bwd_dup", 0, torch.int32).fill_(0x7777)          # a stale word: every backward that reads it writes it
        gt = [net._grad_table() for net in nets]
        _lib.check(lib.mms_dn121_backward_group(2, ws, Bn, D, H, W, xp, pt, _ptrs([d.data_ptr() for d in dout]), 128,
                                                _ptrs([ctypes.addressof(t) for t in gt]), ctypes.byref(opts), st), "mms_dn121_backward_group")
        torch.cuda.synchronize()
        res[flag] = dict(grads=[_grads(net) for net in nets], names=[n for n, _ in nets[0].named_parameters()],
                         dup=[int(net.workspace_region("bwd_dup", 0, torch.int32)[0]) for net in nets],
                         live=[int(net.workspace_region("bwd_live", 0, torch.int32)[0]) for net in nets])
    _NET[variant] = res
    return res


@pytest.mark.parametrize("variant", ["both", "row6"])
def test_network_group(variant):
    """Default against dup_zero_bwd = -1 at the criterion of tests/test_gpu_dup_zero.py::test_network_group: every gradient tensor within 1e-4
    of its maximum, tensors below 1e-5 of the largest left out -- and denseblock1's conv2 weight and norm2 weight / bias gradients of every
    layer must be among the compared ones, or the test would not see this change."""
    res = _network(variant)
    a, b = res[0], res[-1]
    assert a["live"] == [0, 1] and b["live"] == [0, 1]
    assert a["dup"] == [0xff, 0b1001000 if variant == "both" else 0], a["dup"]           # member 0: dead, the live word wins
    assert b["dup"] == [0x7777, 0x7777], b["dup"]                                         # off: never written
    for g in range(2):
        if g == 0:
            assert all(float(t.abs().max()) == 0.0 for t in a["grads"][0])
            continue
        want, got = b["grads"][g], a["grads"][g]
        gmax = max(float(t.abs().max()) for t in want)
        worst, seen = 0.0, set()
        for name, u, v in zip(a["names"], got, want):
            if float(v.abs().max()) < 1e-5 * gmax:
                continue
            seen.add(name)
            worst = max(worst, rel_err(u, v))
        need = [n for n in a["names"] if "denseblock1." in n and (n.endswith("conv2.weight") or ".norm2." in n)]
        assert len(need) == 6 * 3 and all(n in seen for n in need), [n for n in need if n not in seen]
        print(f"{variant}, member {g}: worst per-tensor gradient difference dup_zero_bwd 0 vs -1 {worst:.2e}")
        assert worst <= 1e-4, (variant, g, worst)


# ---- lifetime through one captured graph ------------------------------------------------------------------------------------------------
def test_word_lifetime_through_graph():
    """FoldGroupEngine, two PartialModalityNet members, graph-replayed steps at lr = 0 on the same engine and the same graph: a step with an
    all-absent member, one on all-real volumes, one mixed (D = {2, 3} and {0, 2, 3}).  "bwd_dup" after each step says what that step's batch
    held; losses within 1e-5 and gradients within 1e-4 (tests/test_gpu_dead_backward.py) of dup_zero_bwd = -1 from the same state."""
    from multimodal_survival_prediction_amd import _lib
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    from test_gpu_dead_backward import _masked_cohort, _seq_models, _spread, _tensors
    B, dims, rna_dim = 4, (64, 64, 32), 64
    cohort = _masked_cohort(dims, rna_dim)            # patients 8..15 have no CT: all-zero volumes, mask 0
    steps = [([[8, 9, 10, 11], [0, 1, 2, 3]], (0b1111, 0)), ([[4, 5, 6, 7], [0, 1, 2, 3]], (0, 0)),
             ([[0, 1, 12, 13], [12, 4, 13, 14]], (0b1100, 0b1101))]
    base = _seq_models(rna_dim)
    off, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.check(_lib.load_library().mms_dn121_region(B, *dims, b"bwd_dup", 0, ctypes.byref(off), ctypes.byref(nb)), "mms_dn121_region")
    assert nb.value == 4
    runs = {}
    for flag in (0, -1):
        ge = FoldGroupEngine([copy.deepcopy(m).to(DEV).train() for m in base], lr=0.0, weight_decay=1e-4, dn_opts=dict(dup_zero_bwd=flag))
        losses, grads, words = [], [], []
        for idx, _ in steps:
            ge.reset_epoch_stats()
            ge.train_step_indexed(cohort, idx, skip_if_unusable=False, use_graph=True)
            torch.cuda.synchronize()
            losses.append([s["sum_loss"] for s in ge.epoch_stats()])
            grads.append([e.gflat.clone() for e in ge.engines])
            GP = next(iter(ge.plans.values()))
            words.append([int(P.ws[off.value:off.value + 4].view(torch.int32)[0]) for P in GP.Ps])
        runs[flag] = dict(ge=ge, losses=losses, grads=grads, words=words)
    a, b = runs[0], runs[-1]
    for it, (_, want) in enumerate(steps):
        assert tuple(a["words"][it]) == want, (it, a["words"][it])
        for g in range(2):
            la, lb = a["losses"][it][g], b["losses"][it][g]
            assert abs(la - lb) <= 1e-5 * max(1.0, abs(lb)), (it, g, la, lb)
            worst = _spread(_tensors(a["ge"].engines[g], a["grads"][it][g]), _tensors(b["ge"].engines[g], b["grads"][it][g]))
            print(f"step {it}, member {g}: worst per-tensor gradient difference dup_zero_bwd 0 vs -1 {worst:.2e}")
            assert worst <= 1e-4, (it, g, worst)
