"""Zero-box skip of the boxed conv0 kernels (MmsDnOpts.c0_zero_skip, include/mmsurv.h): a box whose staged input region -- halo included --
compares equal to 0.0f everywhere is not multiplied.  conv0_fwd_box_kernel stores +0.0f for it and adds nothing to the statistics;
conv0_bwd_weight_kernel skips its MFMAs, and a workgroup whose boxes of a model were all zero skips its flush.  Both kernels walk a model's
boxes sample-minor (position j = box j / B of sample j % B), whatever the option says.

Checked here against the option's other setting (-1: every box does its work) and against torch on the CPU, through the group entry points:
  * shapes: input 16x16x8 -> output 8x8x4 (4 forward and 8 weight-gradient boxes per sample), B = 3 (no divisor of either count: a
    workgroup's range ends in the middle of a sample cycle), 2 models, 1 / 3 / default workgroups (at 3 a range crosses the model boundary);
  * input patterns per model: "dense", "one_zero" (sample 1 all zero), "zero", "corner" (one voxel, in the halo of several boxes of one
    sample, everything else zero), "negzero" (samples 0 and 2 filled with -0.0f).

Tolerances: 1e-4 of the reference's maximum against torch (tests/test_gpu_dn_fwd_ops.py, tests/test_gpu_dn_bwd_ops.py).  Statistics of the
two settings: |difference| <= 1e-10 * sum |terms| -- an order-of-summation bound of fp64 sums of fewer than 2^17 terms (n * 2^-53 ~ 1.5e-11).
Network level: see test_network_group.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_util import DEV, assert_close, cl, rel_err

B, DIMS, OD = 3, (16, 16, 8), (8, 8, 4)
M = B * OD[0] * OD[1] * OD[2]
PATTERNS = ("dense", "one_zero", "zero", "corner", "negzero")
PAIRS = [("dense", "one_zero"), ("one_zero", "zero"), ("zero", "corner"), ("corner", "negzero"), ("negzero", "dense"), ("zero", "zero")]
NWG = [1, 3, 0]


def _volume(kind, seed):
    x = torch.randn(B, *DIMS, generator=torch.Generator().manual_seed(seed))
    if kind == "one_zero":
        x[1] = 0.0
    elif kind == "zero":
        x.zero_()
    elif kind == "corner":
        x.zero_()
        x[2, 8, 8, 3] = 1.5         # d = h = 8: inside the 13-wide regions of both forward boxes along d and h, and of 2 of the 4 gradient boxes along d
    elif kind == "negzero":
        x[0] = -0.0
        x[2] = -0.0
    return x


def _zero_boxes(x, bd):
    """[B, OD0/bd, 2, 1] bool: the box's input region (outputs 2 o - 3 .. 2 o + 3 of its bd x 4 x 4 outputs, zero padding) is all zero"""
    xp = F.pad(x, (3, 3, 3, 3, 3, 3))
    out = torch.zeros(B, OD[0] // bd, OD[1] // 4, OD[2] // 4, dtype=torch.bool)
    for b in range(B):
        for z in range(out.shape[1]):
            for y in range(out.shape[2]):
                for w in range(out.shape[3]):
                    r = xp[b, 2 * bd * z:2 * bd * z + 2 * bd + 5, 8 * y:8 * y + 13, 8 * w:8 * w + 13]
                    out[b, z, y, w] = bool((r == 0).all())
    return out


_CASES = {}


def _case(kind, slot):
    """Per (pattern, member slot): volume, weights, CPU forward, random dbn0 -- computed once, left unchanged."""
    key = (kind, slot)
    if key not in _CASES:
        seed = 100 + 10 * PATTERNS.index(kind) + slot
        g = torch.Generator().manual_seed(seed)
        x = _volume(kind, seed + 1)
        w = torch.randn(64, 343, generator=g) * 0.05
        y = cl(F.conv3d(x[:, None], w.view(64, 1, 7, 7, 7), stride=2, padding=3))
        gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.3
        dbn = torch.randn(M, 64, generator=g)
        _CASES[key] = dict(kind=kind, x=x, w=w, y=y, gamma=gamma, beta=beta, dbn=dbn, zf=_zero_boxes(x, 4), zw=_zero_boxes(x, 2))
    return _CASES[key]


def _env():
    from multimodal_survival_prediction_amd import _lib, ops
    return _lib.load_library(), _lib.structs(), ops


def _forward(cases, nwg, flag):
    """mms_conv0_fwd_group on the members -> [(y [M, 64] pre-filled with NaN, sum, sumsq)]"""
    lib, S, ops = _env()
    coords = ops.init_coords(B, OD, DEV)
    keep, blocks = [], []
    for c in cases:
        x, w = c["x"].to(DEV).contiguous(), c["w"].to(DEV).contiguous()
        y = torch.full((M, 64), float("nan"), device=DEV)
        s, q = torch.zeros(64, dtype=torch.float64, device=DEV), torch.zeros(64, dtype=torch.float64, device=DEV)
        keep.append((x, w, y, s, q))
        blocks.append(S["Conv0FwdP"](x.data_ptr(), ops.dims3(DIMS), ops.dims3(OD), coords.data_ptr(), M, w.data_ptr(), y.data_ptr(),
                                     s.data_ptr(), q.data_ptr()))
    arr = (S["Conv0FwdP"] * len(cases))(*blocks)
    opts = ops.dn_opts(c0f_nwg=nwg, c0_zero_skip=flag)
    _lib_check(lib.mms_conv0_fwd_group(arr, len(cases), ctypes.byref(opts), ops.stream()), "mms_conv0_fwd_group")
    torch.cuda.synchronize()
    return [(k[2], k[3], k[4]) for k in keep]


def _lib_check(rc, what):
    from multimodal_survival_prediction_amd import _lib
    _lib.check(rc, what)


@pytest.mark.parametrize("nwg", NWG)
@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(p) for p in PAIRS])
def test_forward(pair, nwg):
    cases = [_case(k, i) for i, k in enumerate(pair)]
    on, off = _forward(cases, nwg, 0), _forward(cases, nwg, -1)
    for c, (y, s, q), (y2, s2, q2) in zip(cases, on, off):
        what = "%s nwg=%d" % (c["kind"], nwg)
        assert not bool(torch.isnan(y).any()) and not bool(torch.isnan(y2).any()), what          # every output written
        assert torch.equal(y, y2), what
        yb = y.view(torch.int32).view(B, OD[0] // 4, 4, OD[1] // 4, 4, OD[2] // 4, 4, 64).permute(0, 1, 3, 5, 2, 4, 6, 7)
        zf = c["zf"].to(DEV)
        assert int(yb[zf].abs().max() if bool(zf.any()) else 0) == 0, what                       # zero boxes read +0.0
        if c["kind"] == "dense":
            assert not bool(zf.any())
        if c["kind"] in ("one_zero", "zero", "corner", "negzero"):
            assert bool(zf.any())
        if float(c["y"].abs().max()) > 0:
            assert_close(y, c["y"], 1e-4, "conv0 " + what)
        else:
            assert float(y.abs().max()) == 0.0
        y64 = y.double()
        ds, dq = float((s - s2).abs().max()), float((q - q2).abs().max())
        print(f"{what}: statistics on vs off: sum {ds:.2e}, sumsq {dq:.2e}")
        assert bool(((s - s2).abs() <= 1e-10 * y64.abs().sum(0)).all()), what
        assert bool(((q - q2).abs() <= 1e-10 * (y64 * y64).sum(0)).all()), what
        if float(c["y"].abs().max()) > 0:
            assert_close(s, c["y"].double().sum(0), 1e-4, "conv0 sum " + what)
        if c["kind"] == "zero":
            for t in (s, q, s2, q2):
                assert float(t.abs().max()) == 0.0


def _pattern(n, k):
    return ((torch.arange(n, dtype=torch.float32) % 7 + 1.0) * (0.125 if k % 2 else -0.375)).to(DEV)


def _wgrad_reference(c, y0, s, q):
    """torch fp64: norm0's backward of dbn0 on the forward's own y0 and statistics, then conv0's weight gradient -> dW [64, 343], dgamma, dbeta"""
    y, dbn = y0.double().cpu(), c["dbn"].double()
    mean = s.cpu() / M
    var = (q.cpu() / M - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    xhat = (y - mean) * rstd
    t1, t2 = dbn.sum(0), (dbn * xhat).sum(0)
    dy = c["gamma"].double() * rstd * (dbn - t1 / M - xhat * t2 / M)
    w = c["w"].double().view(64, 1, 7, 7, 7).requires_grad_(True)
    out = F.conv3d(c["x"].double()[:, None], w, stride=2, padding=3)
    (cl(out) * dy).sum().backward()
    return w.grad.view(64, 343), t2, t1, (t1, t2)


def _wgrad(cases, fwd, nwg, flag, rep, dead=None):
    """mms_conv0_bwd_weight_group on the forward's y0 -> per member dict(dw, dw0 (what dw held before), dg, db, rep)"""
    lib, S, ops = _env()
    coords = ops.init_coords(B, OD, DEV)
    keep, blocks = [], []
    for i, (c, (y0, s, q)) in enumerate(zip(cases, fwd)):
        _, _, _, (t1, t2) = c["ref"]
        x, dbn = c["x"].to(DEV).contiguous(), c["dbn"].to(DEV).contiguous()
        gamma, beta = c["gamma"].to(DEV), c["beta"].to(DEV)
        a1, a2 = t1.to(DEV), t2.to(DEV)
        bn, bb = ops.bnsrc(gamma, beta, M, True, s, q), ops.bnbwd(a1, a2)
        patterned = c["kind"] == "zero" or dead == i
        dw = _pattern(64 * 343, i) if patterned else torch.zeros(64 * 343, device=DEV)
        dg, db = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
        r = torch.zeros(3, 64 * 343, device=DEV) if rep else None
        live = None
        if dead is not None:
            live = torch.tensor([0 if dead == i else 1], dtype=torch.int32, device=DEV)
        keep.append(dict(dw=dw, dw0=dw.clone(), dg=dg, db=db, rep=r, hold=(x, dbn, gamma, beta, a1, a2, live, y0, s, q)))
        blocks.append(S["Conv0BwdWP"](dbn.data_ptr(), y0.data_ptr(), bn, bb, x.data_ptr(), ops.dims3(DIMS), ops.dims3(OD), coords.data_ptr(), M,
                                      dw.data_ptr(), 1, dg.data_ptr(), db.data_ptr(), r.data_ptr() if rep else None, 3 if rep else 0,
                                      live.data_ptr() if live is not None else None))
    arr = (S["Conv0BwdWP"] * len(cases))(*blocks)
    opts = ops.dn_opts(c0_nwg=nwg, c0_zero_skip=flag)
    _lib_check(lib.mms_conv0_bwd_weight_group(arr, len(cases), ctypes.byref(opts), ops.stream()), "mms_conv0_bwd_weight_group")
    torch.cuda.synchronize()
    return keep


_REFS = {}


def _with_refs(pair):
    """The pair's forward on the GPU (y0 and its statistics) and the fp64 reference on them: once per pair, left unchanged."""
    if pair not in _REFS:
        cases = [dict(_case(k, i)) for i, k in enumerate(pair)]
        fwd = _forward(cases, 0, 0)
        for c, (y0, s, q) in zip(cases, fwd):
            c["ref"] = _wgrad_reference(c, y0, s, q)
        _REFS[pair] = (cases, fwd)
    return _REFS[pair]


@pytest.mark.parametrize("rep", [False, True], ids=["direct", "replicas"])
@pytest.mark.parametrize("nwg", NWG)
@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(p) for p in PAIRS])
def test_weight_gradient(pair, nwg, rep):
    """("dense" with nwg = 3 against the reference is the case that a box dealt twice or not at all cannot pass.)"""
    cases, fwd = _with_refs(pair)
    res = {flag: _wgrad(cases, fwd, nwg, flag, rep) for flag in (0, -1)}
    for i, c in enumerate(cases):
        want, dgam, dbet, _ = c["ref"]
        what = "%s nwg=%d %s" % (c["kind"], nwg, "replicas" if rep else "direct")
        if c["kind"] in ("dense", "one_zero", "negzero"):
            assert float(want.abs().max()) > 0
        for flag in (0, -1):
            k = res[flag][i]
            got = (k["dw"] - k["dw0"]).view(64, 343)
            if c["kind"] == "zero":
                assert float(want.abs().max()) == 0.0
                assert torch.equal(k["dw"], k["dw0"]), (what, flag)                # exact zeros added, or nothing
            else:
                print(f"{what} flag {flag}: dW0 rel err {rel_err(got, want):.2e}")
                assert_close(got, want, 1e-4, "dW0 %s flag %d" % (what, flag))
            if rep:
                assert float(k["rep"].abs().max()) == 0.0, (what, flag)            # left zeroed for the next call
            assert_close(k["dg"], dgam, 1e-4, "dgamma0 " + what)
            assert_close(k["db"], dbet, 1e-4, "dbeta0 " + what)
        assert torch.equal(res[0][i]["dg"], res[-1][i]["dg"]) and torch.equal(res[0][i]["db"], res[-1][i]["db"]), what


@pytest.mark.parametrize("flag", [0, -1])
@pytest.mark.parametrize("dead", [0, 1])
def test_weight_gradient_dead_member(dead, flag):
    """A member whose `live` word is 0 beside a live one (workgroup ranges cross the model boundary at 3 workgroups): its pattern-filled
    gradient and its replicas stay as they were, bit for bit; the live member matches the reference."""
    cases, fwd = _with_refs(("one_zero", "dense"))
    for rep in (False, True):
        res = _wgrad(cases, fwd, 3, flag, rep, dead=dead)
        assert torch.equal(res[dead]["dw"], res[dead]["dw0"])
        if rep:
            assert float(res[dead]["rep"].abs().max()) == 0.0 and float(res[1 - dead]["rep"].abs().max()) == 0.0
        k = res[1 - dead]
        assert_close((k["dw"] - k["dw0"]).view(64, 343), cases[1 - dead]["ref"][0], 1e-4, "dW0 of the live member")


def test_network_group():
    """mms_dn121_forward_group + mms_dn121_backward_group, 2 members, B = 8 at 32x32x32 (the smallest volume of
    tests/test_gpu_dead_backward.py): member 0's volume is all zero, member 1 has one zero sample.  Default options against c0_zero_skip = -1.

    What holds, and why: conv0's output y0 (workspace region "y0") is bit-identical -- the skip stores the +0.0f the MFMAs would produce and
    the non-zero boxes run the same instructions.  norm0's statistics get the same per-workgroup partial sums (a skipped box adds exactly
    nothing to an fp64 partial sum that the full path adds 0.0 to), but those partial sums, like the statistics of every later BatchNorm
    layer, are accumulated with fp64 atomics whose order varies from run to run under EITHER setting.  So the features and the BatchNorm
    buffers are compared at the bound the suite sets for two runs of the same code (tests/test_gpu_models.py::test_run_twice_spread:
    outputs within 1e-6 of their maximum), the gradients at that file's and tests/test_gpu_dead_backward.py's own criterion (every tensor
    within 1e-4 of its maximum, tensors below 1e-5 of the largest gradient left out)."""
    from multimodal_survival_prediction_amd import _lib, ops
    from test_gpu_dead_backward import _grads, _ptrs, _spread, _zero_grads
    from test_gpu_densenet import _make, structured_volumes
    lib = _lib.load_library()
    Bn, dims = 8, (32, 32, 32)
    D, H, W = dims
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dout = [torch.randn(Bn, 128, generator=torch.Generator().manual_seed(5 + g)).to(DEV) for g in range(2)]
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
            nets.append(net); xs.append(x); es.append(net._tables(x))
        opts = ops.dn_opts(nets[0]._opts(), c0_zero_skip=flag)
        outs = [torch.empty(Bn, 128, device=DEV) for _ in range(2)]
        ws, xp = _ptrs([e["ws"].data_ptr() for e in es]), _ptrs([x.data_ptr() for x in xs])
        pt, bt = _ptrs([ctypes.addressof(e["ptab"]) for e in es]), _ptrs([ctypes.addressof(e["btab"]) for e in es])
        _lib.check(lib.mms_dn121_forward_group(2, ws, Bn, D, H, W, xp, pt, bt, _ptrs([o.data_ptr() for o in outs]), 128, 1, ctypes.byref(opts), st),
                   "mms_dn121_forward_group")
        torch.cuda.synchronize()
        y0 = [net.workspace_region("y0").clone() for net in nets]
        for net in nets:
            _zero_grads(net)
        gt = [net._grad_table() for net in nets]
        _lib.check(lib.mms_dn121_backward_group(2, ws, Bn, D, H, W, xp, pt, _ptrs([d.data_ptr() for d in dout]), 128,
                                                _ptrs([ctypes.addressof(t) for t in gt]), ctypes.byref(opts), st), "mms_dn121_backward_group")
        torch.cuda.synchronize()
        res[flag] = dict(y0=y0, outs=[o.clone() for o in outs], bufs=[[b.detach().clone() for b in net.buffers()] for net in nets],
                         grads=[_grads(net) for net in nets])
    for g in range(2):
        assert torch.equal(res[0]["y0"][g], res[-1]["y0"][g]), g
        assert not bool(torch.isnan(res[0]["outs"][g]).any())
        e = rel_err(res[0]["outs"][g], res[-1]["outs"][g])
        worst_buf = 0.0
        for a, b in zip(res[0]["bufs"][g], res[-1]["bufs"][g]):
            if a.dtype.is_floating_point:
                worst_buf = max(worst_buf, rel_err(a, b))
            else:
                assert torch.equal(a, b)
        worst = _spread(res[0]["grads"][g], res[-1]["grads"][g])
        print(f"network member {g}: features {e:.2e}, BatchNorm buffers {worst_buf:.2e}, gradients (worst tensor) {worst:.2e}")
        assert e <= 1e-6 and worst_buf <= 1e-6 and worst <= 1e-4
    assert float(res[0]["y0"][0].abs().max()) == 0.0
