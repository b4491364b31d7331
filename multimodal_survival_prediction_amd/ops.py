"""Thin per-op wrappers over the C ABI taking torch tensors (used by tests and by the autograd-compatible
host path).  Pointers are taken with .data_ptr(); all launches go to torch's current stream."""
import ctypes

import torch

from . import _lib


def _S():
    return _lib.structs()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else t.data_ptr()


def dims3(d):
    return _S()["Dims3"](int(d[0]), int(d[1]), int(d[2]))


def bnsrc(gamma, beta, count, train, sum=None, sumsq=None, rmean=None, rvar=None, eps=1e-5):
    return _S()["BnSrc"](ptr(sum), ptr(sumsq), ptr(rmean), ptr(rvar), ptr(gamma), ptr(beta),
                         1.0 / float(count), float(eps), 1 if train else 0)


def dn_opts(base=None, **kw):
    """MmsDnOpts (include/mmsurv.h): launch-shape options of the DenseNet121 drivers and convolution entry points.  All-zero = the
    defaults; the library reads no environment variable, so this block is the only way to select a kernel form (A/B measurements, the
    parity tests that must reach one form).  base: another block or a dict to start from."""
    S = _S()["MmsDnOpts"]
    names = {f[0] for f in S._fields_}
    o = S()
    if isinstance(base, dict):
        kw = dict(base, **kw)
    elif base is not None:
        ctypes.memmove(ctypes.byref(o), ctypes.byref(base), ctypes.sizeof(S))
    for k, v in kw.items():
        if k not in names:
            raise AttributeError("MmsDnOpts has no field %r (include/mmsurv.h)" % k)
        setattr(o, k, int(v))
    return o


def opts_ref(o):
    """ctypes argument for a `const MmsDnOpts*` parameter: NULL (defaults) for None."""
    return None if o is None else ctypes.byref(o)


def call(name, p, opts=None):
    """Single-model entry point name(p, stream); with opts: its fold-group form name_group(p, 1, opts, stream) (the entry points that
    have several kernel forms take the launch-shape options there)."""
    lib = _lib.load_library()
    if opts is None:
        _lib.check(getattr(lib, name)(ctypes.byref(p), stream()), name)
    else:
        _lib.check(getattr(lib, name + "_group")(ctypes.byref(p), 1, ctypes.byref(opts), stream()), name + "_group")


# mms_dn_launch_form: the header's MMS_OP_* by lower-case name ("conv1_fwd", ...) and, per op, its MMS_FORM_<family>_* values by lower-case
# name ("wholek8", "tile32", "small2", "mt", ...) -- read from include/mmsurv.h like every layout, not typed again
LAUNCH_OPS = {k.lower(): v for k, v in _lib.defines("MMS_OP_").items()}
_FORM_FAMILY = {"conv1_fwd": "C1_", "conv1_bwd_data": "C1_", "conv3_fwd": "C3_", "conv3_bwd_data": "C3_", "conv3_bwd_weight": "C3W_"}
LAUNCH_FORMS = {op: {v: k.lower() for k, v in _lib.defines("MMS_FORM_" + fam).items()} for op, fam in _FORM_FAMILY.items()}


def launch_form(op, p, ng, opts=None):
    """The kernel form the op's *_group entry point takes for ng members shaped like the parameter block p (host only, no launch):
    a name from LAUNCH_FORMS[op]; raises for a block the entry point would refuse."""
    rc = _lib.load_library().mms_dn_launch_form(LAUNCH_OPS[op], ctypes.byref(p), int(ng), opts_ref(opts))
    _lib.check(min(rc, 0), "mms_dn_launch_form")
    return LAUNCH_FORMS[op][rc]


def init_coords(B, dims, device):
    D, H, W = dims
    out = torch.empty(B * D * H * W, dtype=torch.int32, device=device)
    _lib.check(_lib.load_library().mms_init_coords(out.data_ptr(), B, D, H, W, stream()), "mms_init_coords")
    return out


def conv1_fwd(x, K, w, y, bn, M, osum=None, osumsq=None, pool=False, in_dims=(0, 0, 0), partial=None, ksplit=0,
              counters=None, opts=None):
    """x: [Min, ldx] slab (first K columns); w: [N, K]; y: [M, ldy] view (column offset applied by slicing).
    partial/ksplit/counters: split the K loop over workgroups with a last-arriver fixup (Conv1FwdP in mmsurv.h)."""
    p = _S()["Conv1FwdP"](ptr(x), x.stride(0), M, K, ptr(w), w.shape[0], ptr(y), y.stride(0), bn,
                          ptr(osum), ptr(osumsq), 1 if pool else 0, dims3(in_dims), 0, 0, ptr(partial), ksplit, ptr(counters))
    call("mms_conv1_fwd", p, opts)


def conv3_fwd(y1, coords, dims, wp, out, bn, osum=None, osumsq=None, partial=None, nsplit=27, wfrag=False, opts=None):
    """wfrag: wp is the fragment-ordered pack (pack_conv3_frag) -- small grids only (Conv3FwdP.wfrag in mmsurv.h)."""
    M = y1.shape[0]
    p = _S()["Conv3FwdP"](ptr(y1), ptr(coords), dims3(dims), M, ptr(wp), ptr(out), out.stride(0), bn,
                          ptr(osum), ptr(osumsq), ptr(partial), nsplit)
    p.wfrag = 1 if wfrag else 0
    call("mms_conv3_fwd", p, opts)


def conv0_fwd(x, in_dims, out_dims, coords, w, y, osum=None, osumsq=None):
    p = _S()["Conv0FwdP"](ptr(x), dims3(in_dims), dims3(out_dims), ptr(coords), y.shape[0], ptr(w), ptr(y),
                          ptr(osum), ptr(osumsq))
    call("mms_conv0_fwd", p)


def pool_fwd(y0, in_dims, out_dims, B, slab, argmax, bn, osum=None, osumsq=None):
    p = _S()["PoolFwdP"](ptr(y0), dims3(in_dims), dims3(out_dims), B, ptr(slab), slab.stride(0), ptr(argmax), bn,
                         ptr(osum), ptr(osumsq))
    call("mms_pool_fwd", p)


def head_fwd(slab, C, B, V, bn, w, bias, pooled, out):
    p = _S()["HeadFwdP"](ptr(slab), slab.stride(0), C, B, V, bn, ptr(w), ptr(bias), w.shape[0], ptr(pooled), ptr(out), out.stride(0))
    call("mms_head_fwd", p)


def pack_conv3(w):
    wpf = torch.empty(32 * 27 * 128, dtype=torch.float32, device=w.device)
    wpb = torch.empty(128 * 27 * 32, dtype=torch.float32, device=w.device)
    _lib.check(_lib.load_library().mms_pack_conv3(w.data_ptr(), wpf.data_ptr(), wpb.data_ptr(), stream()), "mms_pack_conv3")
    return wpf, wpb


def pack_conv3_frag(w):
    """canonical conv2 weight -> the two MFMA-fragment-ordered packs the small-grid kernels read with contiguous 1-KB loads."""
    wff = torch.empty(32 * 27 * 128, dtype=torch.float32, device=w.device)
    wfb = torch.empty(128 * 27 * 32, dtype=torch.float32, device=w.device)
    _lib.check(_lib.load_library().mms_pack_conv3_frag(w.data_ptr(), wff.data_ptr(), wfb.data_ptr(), stream()), "mms_pack_conv3_frag")
    return wff, wfb


# ---- backward ops ---------------------------------------------------------------------------------------
def bnbwd(s1, s2):
    return _S()["BnBwd"](ptr(s1), ptr(s2))


def conv3_bwd_data(dz, coords, dims, wpb, y1, bn, dbn, s1, s2, partial=None, nsplit=27, wfrag=False, opts=None):
    p = _S()["Conv3BwdDataP"](ptr(dz), dz.stride(0), ptr(coords), dims3(dims), y1.shape[0], ptr(wpb), ptr(y1), bn,
                              ptr(dbn), ptr(s1), ptr(s2), ptr(partial), nsplit)
    p.wfrag = 1 if wfrag else 0
    call("mms_conv3_bwd_data", p, opts)


def conv3_bwd_weight(y1, coords, dims, bn, dz, dw, msplit=1, tapmajor=False, opts=None, layout=None):
    p = _S()["Conv3BwdWP"](ptr(y1), ptr(coords), dims3(dims), y1.shape[0], bn, ptr(dz), dz.stride(0), ptr(dw), msplit,
                           layout if layout is not None else (1 if tapmajor else 0))          # Conv3BwdWP.dw_layout
    call("mms_conv3_bwd_weight", p, opts)


def conv1_bwd(which, dyraw, M, N, x, K, bn_in, w, dw, dbn, s1, s2, y=None, bn_out=None, bb_out=None, pool=False,
              in_dims=(0, 0, 0), msplit=1, dgamma_out=None, dbeta_out=None, fuse_dx=None, fuse_accumulate=True, fuse_dgamma=None,
              fuse_dbeta=None, opts=None):
    S = _S()
    p = S["Conv1BwdP"]()
    p.dyraw, p.lddy = ptr(dyraw), dyraw.stride(0)
    p.y, p.ldy = (ptr(y), y.stride(0)) if y is not None else (None, 0)
    p.has_bn_out = 1 if bn_out is not None else 0
    p.bn_out = bn_out if bn_out is not None else bn_in
    p.bb_out = bb_out if bb_out is not None else S["BnBwd"](None, None)
    p.M, p.N = M, N
    p.x, p.ldx, p.K, p.bn_in = ptr(x), x.stride(0), K, bn_in
    setattr(p, "in", dims3(in_dims))
    p.w = ptr(w)
    p.pool = 1 if pool else 0
    p.dw = ptr(dw)
    p.dbn, p.lddbn = ptr(dbn), dbn.stride(0)
    p.s1, p.s2 = ptr(s1), ptr(s2)
    p.msplit = msplit
    p.dgamma_out, p.dbeta_out = ptr(dgamma_out), ptr(dbeta_out)
    if fuse_dx is not None:          # norm1 backward in the data kernel's epilogue (Conv1BwdP.fuse_dx, M <= 128)
        p.fuse_dx, p.fuse_lddx, p.fuse_accumulate = ptr(fuse_dx), fuse_dx.stride(0), 1 if fuse_accumulate else 0
        p.fuse_dgamma, p.fuse_dbeta = ptr(fuse_dgamma), ptr(fuse_dbeta)
    if which == "weight":
        call("mms_conv1_bwd_weight", p)
    else:
        call("mms_conv1_bwd_data", p, opts)


def bn_bwd_apply(dbn, x, dx, M, C, bn, bb, accumulate, dgamma, dbeta):
    p = _S()["BnBwdApplyP"](ptr(dbn), dbn.stride(0), ptr(x), x.stride(0), ptr(dx), dx.stride(0), M, C, bn, bb,
                            1 if accumulate else 0, ptr(dgamma), ptr(dbeta))
    call("mms_bn_bwd_apply", p)


def head_bwd(dout, pooled, slab, C, B, V, bn, w, dw, dbias, dgamma, dbeta, dslab):
    p = _S()["HeadBwdP"](ptr(dout), dout.stride(0), ptr(pooled), ptr(slab), slab.stride(0), C, B, V, bn, ptr(w), w.shape[0],
                         ptr(dw), ptr(dbias), ptr(dgamma), ptr(dbeta), ptr(dslab), dslab.stride(0))
    call("mms_head_bwd", p)


def pool_bwd(dslab, argmax, out_dims, in_dims, B, y0, bn, dbn, s1, s2, coords=None):
    p = _S()["PoolBwdP"](ptr(dslab), dslab.stride(0), ptr(argmax), dims3(out_dims), dims3(in_dims), B, ptr(y0), bn,
                         ptr(dbn), ptr(s1), ptr(s2), ptr(coords))
    call("mms_pool_bwd", p)


def pool_act(x, K, bn, in_dims, y):
    """Transition pre-pass: y[m'][:K] = AvgPool3d(2, 2)(relu(bn(x)))[m'] for channels-last x [B*in][ldx] (mms_pool_act)."""
    p = _S()["PoolActP"](ptr(x), x.stride(0), K, bn, dims3(in_dims), y.shape[0], ptr(y), y.stride(0))
    _lib.check(_lib.load_library().mms_pool_act_group(ctypes.byref(p), 1, stream()), "mms_pool_act_group")


def conv0_bwd_weight(dbn, y0, bn, bb, x, in_dims, out_dims, coords, dw, msplit, dgamma, dbeta, dw_rep=None):
    """dw_rep: optional zeroed [nrep <= 8][64 * 343] replica scratch (Conv0BwdWP.dw_rep: spreads the gradient atomics, a second launch adds
    the replicas into dw and leaves them zeroed)"""
    p = _S()["Conv0BwdWP"](ptr(dbn), ptr(y0), bn, bb, ptr(x), dims3(in_dims), dims3(out_dims), ptr(coords),
                           y0.shape[0], ptr(dw), msplit, ptr(dgamma), ptr(dbeta), ptr(dw_rep), 0 if dw_rep is None else dw_rep.shape[0])
    call("mms_conv0_bwd_weight", p)


def conv0_bwd_data(dbn, bn, w, in_dims, out_dims, dx, group=None):
    """norm0 (frozen: bn.train = 0) backward + conv0 with respect to the volume (mms_conv0_bwd_data): dbn [B*out, 64] -> dx [B, D, H, W],
    written.  group: a list of (dbn, bn, w, dx) members of identical shape for ONE mms_conv0_bwd_data_group launch (grid z = member)."""
    S = _S()["Conv0BwdDataP"]
    mk = lambda d, b, w_, x_: S(ptr(d), b, ptr(w_), dims3(in_dims), dims3(out_dims), d.shape[0], ptr(x_))
    if group is None:
        call("mms_conv0_bwd_data", mk(dbn, bn, w, dx))
        return
    arr = (S * len(group))(*[mk(*m) for m in group])
    _lib.check(_lib.load_library().mms_conv0_bwd_data_group(arr, len(group), stream()), "mms_conv0_bwd_data_group")


# ---- heads ------------------------------------------------------------------------------------------------
def inprolog(bn=None, train=False, drop_p=0.0, drop_mask=None, rng=None, stream_id=0):
    """bn: None or a torch.nn.BatchNorm1d-like holder with weight/bias/running_mean/running_var/num_batches_tracked."""
    S = _S()["InProlog"]
    if bn is None:
        return S(0, None, None, None, None, None, 1e-5, 0.1, 1 if train else 0, float(drop_p), ptr(drop_mask), ptr(rng), stream_id)
    return S(1, ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var), ptr(bn.num_batches_tracked),
             float(bn.eps), float(bn.momentum), 1 if train else 0, float(drop_p), ptr(drop_mask), ptr(rng), stream_id)


def linear_fwd(x, K, pro, w, bias, y, out_relu):
    p = _S()["LinearFwdP"](ptr(x), x.stride(0), x.shape[0], K, pro, ptr(w), ptr(bias), w.shape[0], ptr(y), y.stride(0),
                           1 if out_relu else 0)
    call("mms_linear_fwd", p)


def linear_bwd(dy, y, out_relu, x, K, pro, w, dw, dbias, dx=None, dgamma=None, dbeta=None):
    p = _S()["LinearBwdP"](ptr(dy), dy.stride(0), ptr(y), y.stride(0), 1 if out_relu else 0, ptr(x), x.stride(0),
                           x.shape[0], K, pro, ptr(w), w.shape[0], ptr(dw), ptr(dbias), ptr(dx),
                           dx.stride(0) if dx is not None else 0, ptr(dgamma), ptr(dbeta))
    call("mms_linear_bwd", p)


def gate_params(feats, mask, w1, b1, w2, b2, hidden, gate, fused, dfused=None, ent_weight=0.0, dfeats=None,
                dw1=None, db1=None, dw2=None, db2=None, entropy=None, dgate_ext=None):
    return _S()["GateP"](ptr(feats), ptr(mask), feats.shape[0], ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(hidden), ptr(gate),
                         ptr(fused), ptr(dfused), float(ent_weight), ptr(dgate_ext), ptr(dfeats), ptr(dw1), ptr(db1),
                         ptr(dw2), ptr(db2), ptr(entropy))


def zero_spans(tensors):
    """-> the MmsZeroSpan array of mms_zero_spans_group over `tensors` (contiguous device tensors; the caller keeps them alive)."""
    S = _S()["MmsZeroSpan"]
    for t in tensors:
        if not t.is_contiguous():
            raise ValueError("zero_spans: contiguous tensors only")
    return (S * len(tensors))(*[S(t.data_ptr(), t.numel() * t.element_size()) for t in tensors])


def gather_params(idx_dev, B, srcs, device_only=None):
    """GatherP (include/mmsurv.h) of B rows named by idx_dev over srcs = [(source, destination, width or None = all columns,
    availability flags or None)]: fp32 rows in device or pinned host memory (the caller keeps them alive).  device_only: the message
    that refuses pinned sources too."""
    G = _S()["GatherP"]()
    G.idx, G.B, G.nsrc = idx_dev.data_ptr(), B, len(srcs)
    for i, (a, b, w, flag) in enumerate(srcs):
        if a.dtype != torch.float32 or not (a.is_cuda or (device_only is None and a.is_pinned())):
            raise TypeError(device_only or "gather sources must be fp32 tensors in device or pinned host memory")
        G.src[i], G.dst[i], G.src_ld[i], G.dst_ld[i] = a.data_ptr(), b.data_ptr(), a.stride(0), b.stride(0)
        G.width[i] = w if w is not None else a.shape[1]
        if flag is not None:
            G.present[i], G.present_ld[i] = flag.data_ptr(), flag.stride(0)
    return G


TIE_MODES = {"breslow": 0, "efron": 1}


def _cox_p(h, time, event, valid, scale, want_grad, ties):
    """-> (CoxP, out, dh, scratch tensors the launch writes)"""
    n = h.shape[0]
    lse = torch.empty(n, device=h.device)
    out = torch.empty(2, device=h.device)
    dh = torch.empty(n, device=h.device) if want_grad else None
    frac = torch.empty(n, device=h.device) if TIE_MODES[ties] == 1 else None
    p = _S()["CoxP"](ptr(h), h.stride(0), ptr(time), ptr(event), ptr(valid), n, float(scale), ptr(lse), ptr(dh), 1, ptr(out),
                     TIE_MODES[ties], ptr(frac))
    return p, out, dh, (lse, frac)


def cox_fwd_bwd(h, time, event, valid=None, scale=1.0, want_grad=True, ties="breslow"):
    """h: [n] or [n,1] fp32 on device -> (out[2] = {loss, usable}, dh or None).  ties: CoxP.tie_mode (include/mmsurv.h)."""
    p, out, dh, _scratch = _cox_p(h, time, event, valid, scale, want_grad, ties)
    call("mms_cox_fwd_bwd", p)
    return out, dh


def cox_fwd_bwd_group(members):
    """The fold-group form: ONE mms_cox_fwd_bwd_group launch pair over `members`, dicts of cox_fwd_bwd's arguments (h, time, event
    [, valid, scale, ties]) with the same n -> [(out, dh)] per member."""
    built = [_cox_p(m["h"], m["time"], m["event"], m.get("valid"), m.get("scale", 1.0), True, m.get("ties", "breslow")) for m in members]
    arr = (_S()["CoxP"] * len(built))(*[b[0] for b in built])
    _lib.check(_lib.load_library().mms_cox_fwd_bwd_group(arr, len(built), stream()), "mms_cox_fwd_bwd_group")
    return [(b[1], b[2]) for b in built]


def cindex_counts(h, time, event):
    counts = torch.zeros(3, dtype=torch.int64, device=h.device)
    p = _S()["CindexP"](ptr(h), ptr(time), ptr(event), h.shape[0], ptr(counts))
    call("mms_cindex_counts", p)
    return counts


def cindex_boot(hrank, trank, event, w, stratum=None, pair_rule=0):
    """Weighted (bootstrap) Harrell-C pair counts (CbootP in mmsurv.h).  hrank: int32 [M, n] (or [n]) dense ranks of the risk scores, trank /
    event / stratum: int32 [n], w: int8 [R, n] multiplicities 0..127 -> int64 [M + 1, R]: row m = 2*concordant + tied of model m, row M =
    comparable pairs.  w is padded here to the 64-byte row length the kernel reads."""
    hrank = hrank.reshape(1, -1) if hrank.dim() == 1 else hrank
    M, n = hrank.shape
    if w.dim() != 2 or w.shape[1] != n or w.dtype != torch.int8:
        raise ValueError("w must be int8 [R, n]")
    if trank.numel() != n or event.numel() != n or (stratum is not None and stratum.numel() != n):
        raise ValueError("trank / event / stratum must have n = %d elements" % n)
    dev = hrank.device
    i32 = lambda t: None if t is None else t.to(device=dev, dtype=torch.int32).contiguous()
    hrank, trank, event, stratum = i32(hrank), i32(trank), i32(event), i32(stratum)
    R, ldw = w.shape[0], (n + 63) // 64 * 64
    if ldw == n and w.is_contiguous() and w.data_ptr() % 16 == 0:
        wp = w
    else:
        wp = torch.zeros(R, ldw, dtype=torch.int8, device=dev)
        wp[:, :n] = w
    out = torch.zeros(M + 1, R, dtype=torch.int64, device=dev)
    p = _S()["CbootP"](ptr(hrank), n, M, ptr(trank), ptr(event), ptr(stratum), n, ptr(wp), ldw, R, ptr(out), int(pair_rule))
    call("mms_cindex_boot", p)
    return out


def _upload(a, dtype, dev):
    """a host array -> flat device tensor of dtype; an empty one becomes a single zero (never a NULL pointer)"""
    import numpy as np
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).reshape(-1) if a.size else np.zeros(1, dtype)).to(dev)


def _launch_or_plan(name, p, keep, res, plan_only):
    """The tail of the evaluation wrappers: launch `name` on p -> res.  plan_only: launch nothing -> (p, keep = whatever p points to,
    res; a tuple res is spliced in), for call(name, p) by the caller (the tools/bench_*.py time the launch alone)."""
    if plan_only:
        return (p, keep) + (res if isinstance(res, tuple) else (res,))
    call(name, p)
    return res


def gene_screen(x, off, row, coef, G=None, plan_only=False):
    """Univariate Cox score screen (GeneScreenP in mmsurv.h).  x: fp32 [N, >= G] device matrix (row pitch x.stride(0)); off: [P + 1]
    problem offsets, row: [off[P]] patient rows in risk order, coef: [off[P], 3] float64 (a, b, q) -- host arrays (numpy or CPU
    tensors).  The launch cannot check row / off, so both are checked HERE, before the upload (as augment.check_records checks its
    records): rows in [0, N), off non-decreasing from 0 and ending at len(row).  -> (U, V): two [P, G] float64 device tensors.
    plan_only: upload and check, do not launch -> (GeneScreenP, the tensors it points to, U, V), for call("mms_gene_screen", p) by
    the caller (tools/bench_gene_screen.py times the launch alone)."""
    import numpy as np
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise TypeError("x must be a 2-D fp32 device tensor with unit column stride")
    N, G = x.shape[0], x.shape[1] if G is None else int(G)
    off, row = np.asarray(off, dtype=np.int64).reshape(-1), np.asarray(row, dtype=np.int64).reshape(-1)
    coef = np.ascontiguousarray(np.asarray(coef, dtype=np.float64)).reshape(-1, 3)
    P = len(off) - 1
    if N < 1 or not 1 <= G <= x.shape[1]:
        raise ValueError("x must have N >= 1 rows and 1 <= G <= %d columns" % x.shape[1])
    if P < 0 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != len(row) or len(coef) != len(row):
        raise ValueError("off must be non-decreasing from 0 to len(row) = len(coef)")
    if len(row) >= 2 ** 31:
        raise ValueError("the problems' row lists together must stay below 2^31 entries")
    if len(row) and (row.min() < 0 or row.max() >= N):
        raise ValueError("rows must lie in [0, %d)" % N)
    dev = x.device
    off_d, row_d, coef_d = _upload(off, np.int32, dev), _upload(row, np.int32, dev), _upload(coef, np.float64, dev)
    U, V = torch.empty(max(P, 1), G, dtype=torch.float64, device=dev), torch.empty(max(P, 1), G, dtype=torch.float64, device=dev)
    p = _S()["GeneScreenP"](ptr(x), N, x.stride(0), G, P, ptr(off_d), ptr(row_d), ptr(coef_d), ptr(U), ptr(V))
    return _launch_or_plan("mms_gene_screen", p, (x, off_d, row_d, coef_d), (U[:P], V[:P]), plan_only)


def _check_permutations(perm, n, what):
    """perm: int64 [R, n]; every row must hold each of 0 .. n - 1 once"""
    import numpy as np
    if perm.size and (perm.min() < 0 or perm.max() >= n):
        raise ValueError("%s must hold values in [0, %d)" % (what, n))
    seen = np.zeros(perm.shape, dtype=bool)
    np.put_along_axis(seen, perm, True, axis=1)
    if not seen.all():
        raise ValueError("every row of %s must be a permutation of 0 .. %d" % (what, n - 1))


def gsea_scores(x, row, m, perm, G=None, plan_only=False):
    """Permutation Z of every gene under R1 relabellings (GseaScoreP in mmsurv.h).  x: fp32 [N, >= G] device matrix (row pitch
    x.stride(0)); row: [n] patient rows in list order, m: [n] float64 null martingale residuals, perm: [R1, n] the residual each list
    position gets per replicate -- host arrays.  The launch cannot check row / perm, so both are checked HERE, before the upload (as
    ops.gene_screen checks its rows): rows in [0, N), every perm row a permutation of 0 .. n - 1, m finite.  -> (scale [G], Z [R1, G]):
    float64 device tensors.  plan_only: upload and check, do not launch -> (GseaScoreP, the tensors it points to, scale, Z), for
    call("mms_gsea_scores", p) by the caller (tools/bench_gsea.py times the launches alone)."""
    import numpy as np
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise TypeError("x must be a 2-D fp32 device tensor with unit column stride")
    N, G = x.shape[0], x.shape[1] if G is None else int(G)
    row = np.asarray(row, dtype=np.int64).reshape(-1)
    m = np.ascontiguousarray(np.asarray(m, dtype=np.float64)).reshape(-1)
    n = len(row)
    perm = np.asarray(perm, dtype=np.int64).reshape(-1, n) if n else np.zeros((0, 0), np.int64)
    R1 = perm.shape[0]
    lim = _lib.defines("MMS_GSEA_MAX_")
    if N < 1 or not 1 <= G <= min(x.shape[1], lim["G"]):
        raise ValueError("x must have N >= 1 rows and 1 <= G <= %d columns" % min(x.shape[1], lim["G"]))
    if n < 2 or len(m) != n or not np.isfinite(m).all():
        raise ValueError("row and m must hold the same n >= 2 entries, m finite")
    if R1 > lim["R1"]:
        raise ValueError("at most %d replicates a launch" % lim["R1"])
    if row.min() < 0 or row.max() >= N:
        raise ValueError("rows must lie in [0, %d)" % N)
    _check_permutations(perm, n, "perm")
    dev = x.device
    row_d, m_d, perm_d = _upload(row, np.int32, dev), _upload(m, np.float64, dev), _upload(perm, np.int32, dev)
    scale = torch.zeros(G, dtype=torch.float64, device=dev)
    Z = torch.zeros(max(R1, 1), G, dtype=torch.float64, device=dev)
    p = _S()["GseaScoreP"](n, N, x.stride(0), G, R1, G, ptr(x), ptr(row_d), ptr(m_d), ptr(perm_d), ptr(scale), ptr(Z))
    return _launch_or_plan("mms_gsea_scores", p, (x, row_d, m_d, perm_d), (scale, Z[:R1]), plan_only)


def check_gene_sets(set_off, set_gene, G):
    """The CSR contract of GseaEsP on host arrays: set_off non-decreasing from 0 to len(set_gene), every set's genes distinct and in
    [0, G), 1 <= k <= G - 1.  -> (set_off, set_gene) as int64."""
    import numpy as np
    off, gene = np.asarray(set_off, dtype=np.int64).reshape(-1), np.asarray(set_gene, dtype=np.int64).reshape(-1)
    if len(off) < 1 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != len(gene):
        raise ValueError("set_off must be non-decreasing from 0 to len(set_gene)")
    if len(gene) >= 2 ** 31:
        raise ValueError("the sets together must stay below 2^31 members")
    if len(gene) and (gene.min() < 0 or gene.max() >= G):
        raise ValueError("set genes must lie in [0, %d)" % G)
    k = np.diff(off)
    if len(k) and (k.min() < 1 or k.max() > G - 1):
        raise ValueError("every set must hold 1 .. G - 1 = %d genes" % (G - 1))
    sid = np.repeat(np.arange(len(k)), k)
    if len(np.unique(sid * G + gene)) != len(gene):
        raise ValueError("a set lists a gene twice")
    return off, gene


def gsea_es(Z, set_off, set_gene, gperm=None, weight=1, peak=True, plan_only=False):
    """Enrichment score of S gene sets in every replicate (GseaEsP in mmsurv.h).  Z: float64 [R1, G] gene statistics, a device tensor
    (row pitch Z.stride(0); ops.gsea_scores' Z: finite by construction) or a host array (a non-finite value is refused HERE); set_off
    [S + 1], set_gene: the sets in CSR form; gperm: None, or int [R, G] gene permutations (preranked mode: Z must have ONE row and
    R1 = R + 1; replicate r >= 1 ranks z[gperm[r - 1][g]]); weight 0 / 1 -- host arrays, checked here before the upload
    (check_gene_sets; every gperm row a permutation).  -> (es float64 [R1, S], peak int32 [R1, S] or None): device tensors.
    plan_only: upload and check, do not launch -> (GseaEsP, the tensors it points to, es, peak), for call("mms_gsea_es", p)."""
    import numpy as np
    if torch.is_tensor(Z) and Z.is_cuda:
        if Z.dtype != torch.float64 or Z.dim() != 2 or (Z.shape[1] > 1 and Z.stride(1) != 1):
            raise TypeError("Z must be float64 [R1, G] with unit column stride")
        if not bool(torch.isfinite(Z).all()):
            raise ValueError("Z must be finite")
        dev = Z.device
    else:
        Zh = np.asarray(Z.cpu() if torch.is_tensor(Z) else Z, dtype=np.float64)
        Zh = Zh.reshape(1, -1) if Zh.ndim == 1 else Zh
        if Zh.ndim != 2 or not np.isfinite(Zh).all():
            raise ValueError("Z must be a finite float64 [R1, G] array")
        dev = torch.device("cuda")
        Z = torch.from_numpy(np.ascontiguousarray(Zh)).to(dev) if Zh.size else torch.zeros(Zh.shape, dtype=torch.float64, device=dev)
    rows, G = Z.shape
    if rows > 1 and Z.stride(0) < G:                 # (an expanded view: rows that overlap have no pitch)
        Z = Z.contiguous()
    lim = _lib.defines("MMS_GSEA_MAX_")
    if weight not in (0, 1):
        raise ValueError("weight must be 0 or 1")
    if not 2 <= G <= lim["G"]:
        raise ValueError("Z must have 2 .. %d gene columns" % lim["G"])
    off, gene = check_gene_sets(set_off, set_gene, G)
    S = len(off) - 1
    gperm_d = None
    if gperm is None:
        R1 = rows
    else:
        gperm = np.asarray(gperm, dtype=np.int64).reshape(-1, G)
        if rows != 1:
            raise ValueError("preranked mode ranks ONE row of scores, got %d" % rows)
        _check_permutations(gperm, G, "gperm")
        R1 = gperm.shape[0] + 1
        gperm_d = _upload(gperm, np.int32, dev)
    if R1 > lim["R1"]:
        raise ValueError("at most %d replicates a launch" % lim["R1"])
    ldz = max(Z.stride(0), G) if rows > 1 else G
    off_d, gene_d = _upload(off, np.int32, dev), _upload(gene, np.int32, dev)
    lde = max(S, 1)
    es = torch.zeros(max(R1, 1), lde, dtype=torch.float64, device=dev)
    pk = torch.zeros(max(R1, 1), lde, dtype=torch.int32, device=dev) if peak else None
    Zp = Z if Z.numel() else torch.zeros(1, dtype=torch.float64, device=dev)
    p = _S()["GseaEsP"](G, S, R1, int(weight), ldz, lde, ptr(Zp), ptr(gperm_d), ptr(off_d), ptr(gene_d), ptr(es), ptr(pk))
    return _launch_or_plan("mms_gsea_es", p, (Zp, gperm_d, off_d, gene_d), (es[:R1, :S], None if pk is None else pk[:R1, :S]), plan_only)


def logrank_scan(rank, pflag, coef, coff, cut, cset=None, at=None, tables=False, plan_only=False):
    """Log-rank statistic of every cut of Q problems (LogrankScanP in mmsurv.h).  rank: int32 [Q, n] ranks over the shared time-descending
    positions -- a device tensor (row pitch rank.stride(0)) or a host array; pflag: [n], coef: [n, 2] float64 (h, c) from
    risk_strata.logrank_coefficients; coff: [S + 1] offsets of the S cut sets in cut; cset: [Q] the set of each problem (None: S = Q, set
    q); at: [S] the designated cut index of each set, -1 = none (None: none) -- host arrays.  The launch cannot check them, so they are
    checked HERE (as ops.gene_screen checks its rows): coff non-decreasing from 0 to len(cut), every set ascending, cset in [0, S), at in
    [-1, the set's size), pflag's bits against coef.  -> dict of device tensors chi2_max, chi2_at (float64 [Q]), arg_max (int32 [Q]) and,
    with tables, U, V (float64 [Q, C]), n_high, d_high (int32 [Q, C]), C = the largest set (columns past a problem's own cuts are not
    written).  plan_only: upload and check, do not launch -> (LogrankScanP, the tensors it points to, the dict), for
    call("mms_logrank_scan", p) by the caller (tools/bench_logrank_scan.py times the launch alone)."""
    import numpy as np
    dev = rank.device if torch.is_tensor(rank) and rank.is_cuda else torch.device("cuda")
    if not torch.is_tensor(rank):
        rank = torch.from_numpy(np.ascontiguousarray(np.asarray(rank, dtype=np.int32)))
    if rank.dim() != 2 or rank.dtype != torch.int32 or (rank.shape[0] and rank.shape[1] and rank.stride(1) != 1):
        raise TypeError("rank must be int32 [Q, n] with unit column stride")
    rank = rank.to(dev)
    Q, n = rank.shape
    if Q > 1 and rank.stride(0) < n:                 # (an expanded view: rows that overlap have no pitch)
        rank = rank.contiguous()
    pflag = np.asarray(pflag, dtype=np.int64).reshape(-1)
    coef = np.ascontiguousarray(np.asarray(coef, dtype=np.float64)).reshape(-1, 2)
    coff, cut = np.asarray(coff, dtype=np.int64).reshape(-1), np.asarray(cut, dtype=np.int64).reshape(-1)
    S = len(coff) - 1
    if n < 1 or len(pflag) != n or len(coef) != n:
        raise ValueError("rank must have n >= 1 columns, pflag n entries and coef [n, 2]")
    if ((pflag & ~3) != 0).any() or not np.array_equal((pflag & 2) != 0, (coef != 0).any(1)) or not np.isfinite(coef).all():
        raise ValueError("pflag must be [event] | 2 [coef != 0] and coef finite")
    if S < 0 or coff[0] != 0 or (np.diff(coff) < 0).any() or coff[-1] != len(cut):
        raise ValueError("coff must be non-decreasing from 0 to len(cut)")
    if len(cut) >= 2 ** 31 or (len(cut) and (np.abs(cut) >= 2 ** 31).any()):
        raise ValueError("cuts must be int32 and fewer than 2^31")
    inner = np.ones(len(cut), bool)
    inner[coff[:-1][coff[:-1] < len(cut)]] = False                       # (the first cut of a set has no predecessor in it)
    if len(cut) > 1 and ((np.diff(cut) < 0) & inner[1:]).any():
        raise ValueError("every cut set must be ascending")
    if cset is None:
        if S != Q:
            raise ValueError("without cset there is one cut set per problem: %d sets, %d problems" % (S, Q))
    else:
        cset = np.asarray(cset, dtype=np.int64).reshape(-1)
        if len(cset) != Q or (Q and (cset.min() < 0 or cset.max() >= S)):
            raise ValueError("cset must name one of the %d cut sets for each of the %d problems" % (S, Q))
    sizes = np.diff(coff)
    if at is not None:
        at = np.asarray(at, dtype=np.int64).reshape(-1)
        if len(at) != S or (at < -1).any() or (at >= sizes).any():
            raise ValueError("at must hold one cut index per set (-1: none)")
    maxc = int(sizes.max()) if S else 0
    t = {k: None if a is None else _upload(a, np.int32, dev) for k, a in dict(pflag=pflag, coff=coff, cut=cut, cset=cset, at=at).items()}
    t.update(rank=rank if rank.numel() else torch.zeros(1, dtype=torch.int32, device=dev), coef=_upload(coef, np.float64, dev))
    ldo = max(maxc, 1)
    out = dict(chi2_max=torch.zeros(max(Q, 1), dtype=torch.float64, device=dev), arg_max=torch.zeros(max(Q, 1), dtype=torch.int32, device=dev),
               chi2_at=torch.zeros(max(Q, 1), dtype=torch.float64, device=dev))
    if tables:
        out.update(U=torch.zeros(max(Q, 1), ldo, dtype=torch.float64, device=dev), V=torch.zeros(max(Q, 1), ldo, dtype=torch.float64, device=dev),
                   n_high=torch.zeros(max(Q, 1), ldo, dtype=torch.int32, device=dev), d_high=torch.zeros(max(Q, 1), ldo, dtype=torch.int32, device=dev))
    p = _S()["LogrankScanP"](n, max(rank.stride(0), n) if Q else n, Q, maxc, ptr(t["rank"]), ptr(t["pflag"]), ptr(t["coef"]), ptr(t["coff"]),
                             ptr(t["cut"]), ptr(t["cset"]), ptr(t["at"]), ptr(out["chi2_max"]), ptr(out["arg_max"]), ptr(out["chi2_at"]),
                             ptr(out.get("U")), ptr(out.get("V")), ptr(out.get("n_high")), ptr(out.get("d_high")), ldo)
    res = {k: (v[:Q, :maxc] if v.dim() == 2 else v[:Q]) for k, v in out.items()}
    return _launch_or_plan("mms_logrank_scan", p, (t, out), res, plan_only)


def _rsf_dev(t, dtype, what, dims=None):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or (dims is not None and t.dim() != dims):
        raise TypeError("%s must be a contiguous %s device tensor%s" % (what, dtype, "" if dims is None else " of %d dimensions" % dims))
    return t


def rsf_split(xt, mult, event, tgroup, node, tables, level, mtry, nsplit, min_leaf, seed, tree_id=None, candidates=False, plan_only=False):
    """One level of T lock-step survival trees (RsfSplitP in mmsurv.h).  Device tensors: xt fp32 [p, n] feature-major in position order,
    mult uint8 [T, n], event / tgroup int32 [n], node int32 [T, n] (updated), tables = dict(feat int32, thr fp32, stat fp64, n_node,
    d_node int32), each [T, nn] (updated), tree_id int32 [T] or None.  candidates: also return dict(U, V float64, n_left, d_left int32)
    [T, 2^level, C] of every candidate (zero where a node's workgroup returned at once)."""
    _rsf_dev(xt, torch.float32, "xt", 2); _rsf_dev(mult, torch.uint8, "mult", 2); _rsf_dev(node, torch.int32, "node", 2)
    _rsf_dev(event, torch.int32, "event", 1); _rsf_dev(tgroup, torch.int32, "tgroup", 1)
    p_, n = xt.shape
    T = mult.shape[0]
    if mult.shape[1] != n or tuple(node.shape) != (T, n) or len(event) != n or len(tgroup) != n:
        raise ValueError("mult / node must be [T, n] and event / tgroup [n] for xt [p, n]")
    kinds = dict(feat=torch.int32, thr=torch.float32, stat=torch.float64, n_node=torch.int32, d_node=torch.int32)
    nn = tables["feat"].shape[1] if T else 1
    for k, dt in kinds.items():
        _rsf_dev(tables[k], dt, k, 2)
        if tuple(tables[k].shape) != (T, nn):
            raise ValueError("the tree tables must all be [T, nn]")
    if tree_id is not None:
        _rsf_dev(tree_id, torch.int32, "tree_id", 1)
        if len(tree_id) != T:
            raise ValueError("tree_id must name one hash stream per tree")
    C = int(mtry) * int(nsplit)
    out = None
    if candidates:
        shape = (max(T, 1), 1 << int(level), max(C, 1))
        out = dict(U=torch.zeros(shape, dtype=torch.float64, device=xt.device), V=torch.zeros(shape, dtype=torch.float64, device=xt.device),
                   n_left=torch.zeros(shape, dtype=torch.int32, device=xt.device), d_left=torch.zeros(shape, dtype=torch.int32, device=xt.device))
    if T == 0:                                                       # an empty forest: nothing to launch (and no pointer to give)
        return None if out is None else {k: v[:0] for k, v in out.items()}
    g = (lambda k: ptr(out[k])) if candidates else (lambda k: None)
    p = _S()["RsfSplitP"](n, n, p_, T, int(level), nn, int(mtry), int(nsplit), int(min_leaf), int(seed) & 0xffffffff, ptr(xt), ptr(mult),
                          ptr(event), ptr(tgroup), ptr(tree_id), ptr(node), ptr(tables["feat"]), ptr(tables["thr"]), ptr(tables["stat"]),
                          ptr(tables["n_node"]), ptr(tables["d_node"]), g("U"), g("V"), g("n_left"), g("d_left"), max(C, 1) if candidates else 0)
    res = None if out is None else {k: v[:T] for k, v in out.items()}
    return _launch_or_plan("mms_rsf_split", p, (xt, mult, event, tgroup, node, tables, tree_id, out), res, plan_only)


def rsf_leaves(mult, event, tgroup, node, feat, n_node, weight, wset, hpos, plan_only=False):
    """Mortality and cumulative hazard at the horizons of every leaf of T trees (RsfLeavesP in mmsurv.h).  Device tensors: mult uint8
    [T, n], event / tgroup int32 [n], node int32 [T, n], feat / n_node int32 [T, nn], weight float64 [F, n], wset int32 [T] or None (row
    0), hpos int32 [nh].  -> (mort float64 [T, nn], H float64 [T, nn, nh]), zero at nodes that are no leaf."""
    _rsf_dev(mult, torch.uint8, "mult", 2); _rsf_dev(node, torch.int32, "node", 2); _rsf_dev(event, torch.int32, "event", 1)
    _rsf_dev(tgroup, torch.int32, "tgroup", 1); _rsf_dev(feat, torch.int32, "feat", 2); _rsf_dev(n_node, torch.int32, "n_node", 2)
    _rsf_dev(weight, torch.float64, "weight", 2); _rsf_dev(hpos, torch.int32, "hpos", 1)
    T, n = mult.shape
    nn, F, nh = feat.shape[1], weight.shape[0], len(hpos)
    if tuple(node.shape) != (T, n) or len(event) != n or len(tgroup) != n or weight.shape[1] != n or tuple(n_node.shape) != (T, nn):
        raise ValueError("node must be [T, n], event / tgroup [n], weight [F, n], n_node like feat")
    if wset is not None:
        _rsf_dev(wset, torch.int32, "wset", 1)
        if len(wset) != T or (T and (int(wset.min()) < 0 or int(wset.max()) >= F)):
            raise ValueError("wset must name one of the %d weight rows for each tree" % F)
    if nh and (int(hpos.min()) < 0 or int(hpos.max()) > n):
        raise ValueError("hpos must lie in [0, n]")
    mort = torch.zeros(T, nn, dtype=torch.float64, device=mult.device)
    H = torch.zeros(T, nn, max(nh, 1), dtype=torch.float64, device=mult.device)
    if T == 0:
        return mort, H[:, :, :nh]
    p = _S()["RsfLeavesP"](n, n, T, nn, nh, F, ptr(mult), ptr(event), ptr(tgroup), ptr(node), ptr(feat), ptr(n_node), ptr(weight), ptr(wset),
                           ptr(hpos) if nh else None, ptr(mort), ptr(H))
    return _launch_or_plan("mms_rsf_leaves", p, (mult, event, tgroup, node, feat, n_node, weight, wset, hpos), (mort, H[:, :, :nh]), plan_only)


def rsf_predict(x, feat, thr, mort, H, use=None, plan_only=False):
    """Masked forest means of R rows (RsfPredictP in mmsurv.h).  x fp32 [R, p] device (row pitch x.stride(0)); feat int32, thr fp32, mort
    float64 [T, nn], H float64 [T, nn, nh] contiguous; use uint8 [T, R] or None (all trees).  feat is checked HERE against p (the launch
    cannot).  -> (mortality float64 [R], H float64 [R, nh], count int32 [R]); NaN where count is 0."""
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise TypeError("x must be a float32 [R, p] device tensor with unit column stride")
    _rsf_dev(feat, torch.int32, "feat", 2); _rsf_dev(thr, torch.float32, "thr", 2); _rsf_dev(mort, torch.float64, "mort", 2)
    _rsf_dev(H, torch.float64, "H", 3)
    R, p_ = x.shape
    T, nn = feat.shape
    nh = H.shape[2]
    if tuple(thr.shape) != (T, nn) or tuple(mort.shape) != (T, nn) or tuple(H.shape[:2]) != (T, nn):
        raise ValueError("thr, mort and H must match feat [T, nn]")
    if T and int(feat.max()) >= p_:
        raise ValueError("the forest splits on feature %d; x has %d columns" % (int(feat.max()), p_))
    if use is not None:
        _rsf_dev(use, torch.uint8, "use", 2)
        if tuple(use.shape) != (T, R):
            raise ValueError("use must be [T, R]")
    dev = x.device
    om = torch.zeros(max(R, 1), dtype=torch.float64, device=dev)
    oh = torch.zeros(max(R, 1), max(nh, 1), dtype=torch.float64, device=dev)
    cnt = torch.zeros(max(R, 1), dtype=torch.int32, device=dev)
    d = torch.zeros(1, dtype=torch.float64, device=dev)            # never a NULL pointer for an empty table
    pz = lambda t: ptr(t) if t.numel() else ptr(d)
    p = _S()["RsfPredictP"](R, max(x.stride(0), p_) if R else p_, p_, T, max(nn, 1), nh, pz(x), pz(feat), pz(thr), pz(mort), pz(H), ptr(use),
                            R if use is not None else 0, ptr(om), ptr(oh), ptr(cnt))
    return _launch_or_plan("mms_rsf_predict", p, (x, feat, thr, mort, H, use, om, oh, cnt, d), (om[:R], oh[:R, :nh], cnt[:R]), plan_only)


def rsf_vimp(x, feat, thr, mort, use, donor, M0, cnt, event, tgroup, pset, pgene, poff, ptree, delta=False, plan_only=False):
    """Permutation importance counts of P (set, gene) problems x R repeats in one launch (RsfVimpP in mmsurv.h).  Device tensors: x fp32
    [n, p] (row pitch x.stride(0)); feat int32, thr fp32, mort float64 [T, nn]; use uint8 [T, n]; donor int32 [R, T, n] (both contiguous,
    or views of one row pitch: donor.stride() == (T * use.stride(0), use.stride(0), 1)); M0 float64 and
    cnt int32 [F, n]; event / tgroup int32 [n] per row of x (tgroup: a larger number is a shorter time); the problem table pset, pgene
    [P], poff [P + 1], ptree [poff[P]] as int32 device tensors or host arrays.  The launch cannot check table contents, so they are checked
    HERE: feat < p, genes in [0, p), donors in [0, n), trees in [0, T), sets in [0, F), tgroup in [0, n), poff non-decreasing from 0 to
    len(ptree).  -> dict(conc2, comparable int64 [P, R]) and, with delta, D, M float64 [P, R, n].  P = 0 or T = 0 launches nothing."""
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise TypeError("x must be a float32 [n, p] device tensor with unit column stride")
    _rsf_dev(feat, torch.int32, "feat", 2); _rsf_dev(thr, torch.float32, "thr", 2); _rsf_dev(mort, torch.float64, "mort", 2)
    _rsf_dev(M0, torch.float64, "M0", 2)
    for t, dt, dims, what in ((use, torch.uint8, 2, "use"), (donor, torch.int32, 3, "donor")):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or t.dim() != dims:
            raise TypeError("%s must be a %s device tensor of %d dimensions" % (what, dt, dims))
    _rsf_dev(cnt, torch.int32, "cnt", 2); _rsf_dev(event, torch.int32, "event", 1); _rsf_dev(tgroup, torch.int32, "tgroup", 1)
    dev = x.device
    n, p_ = x.shape
    T, nn = feat.shape
    R, F = donor.shape[0], M0.shape[0]
    lim = _lib.defines("MMS_RSF_")
    ldu = use.stride(0) if use.dim() == 2 and use.shape[0] else n
    if not (use.numel() and donor.numel() and ldu >= n and use.stride(1) == 1 and donor.stride() == (T * ldu, ldu, 1)):
        use, donor, ldu = use.contiguous(), donor.contiguous(), n
    P, nt = len(poff) - 1, len(ptree)
    if P < 0 or len(pset) != P or len(pgene) != P:
        raise ValueError("pset and pgene must be [P] and poff [P + 1]")
    tab = [t.to(dev) if torch.is_tensor(t) else _upload(t, "int32", dev) for t in (pset, pgene, poff, ptree)]
    if any(t.dtype != torch.int32 or t.dim() != 1 for t in tab):
        raise TypeError("pset, pgene, poff and ptree must be one-dimensional int32")
    pset, pgene, poff, ptree = (t.contiguous() for t in tab)
    if not (1 <= n <= lim["MAX_N"]) or not (1 <= R <= lim["VIMP_MAX_R"]) or F < 1 or P < 0 or P * R >= 2 ** 31:
        raise ValueError("n must be in 1..%d, repeats in 1..%d, sets >= 1, problems x repeats < 2^31" % (lim["MAX_N"], lim["VIMP_MAX_R"]))
    if tuple(thr.shape) != (T, nn) or tuple(mort.shape) != (T, nn) or tuple(use.shape) != (T, n) or tuple(donor.shape) != (R, T, n):
        raise ValueError("thr and mort must match feat [T, nn], use be [T, n] and donor [R, T, n]")
    if tuple(cnt.shape) != (F, n) or len(event) != n or len(tgroup) != n:
        raise ValueError("cnt must match M0 [F, n]; event and tgroup must be [n]")
    if T and int(feat.max()) >= p_:
        raise ValueError("the forest splits on feature %d; x has %d columns" % (int(feat.max()), p_))
    if T and (int(donor.min()) < 0 or int(donor.max()) >= n):
        raise ValueError("donors must lie in [0, %d)" % n)
    if int(tgroup.min()) < 0 or int(tgroup.max()) >= n:
        raise ValueError("tgroup must lie in [0, %d)" % n)
    if int(poff[0]) != 0 or int(poff[P]) != nt or bool((poff[1:] < poff[:-1]).any()):
        raise ValueError("poff must be non-decreasing from 0 to len(ptree)")
    if P and (int(pset.min()) < 0 or int(pset.max()) >= F or int(pgene.min()) < 0 or int(pgene.max()) >= p_):
        raise ValueError("sets must lie in [0, %d) and genes in [0, %d)" % (F, p_))
    if nt and (int(ptree.min()) < 0 or int(ptree.max()) >= T):
        raise ValueError("tree lists must lie in [0, %d)" % T)
    out = dict(conc2=torch.zeros(max(P, 1), R, dtype=torch.int64, device=dev), comparable=torch.zeros(max(P, 1), R, dtype=torch.int64, device=dev))
    if delta:
        out.update(D=torch.zeros(max(P, 1), R, n, dtype=torch.float64, device=dev), M=torch.zeros(max(P, 1), R, n, dtype=torch.float64, device=dev))
    res = {k: v[:P] for k, v in out.items()}
    d = torch.zeros(1, dtype=torch.float64, device=dev)            # never a NULL pointer for an empty table
    pz = lambda t: ptr(t) if t.numel() else ptr(d)
    p = _S()["RsfVimpP"](n, max(x.stride(0), p_), p_, T, max(nn, 1), F, R, P, ldu, n, ptr(x), pz(feat), pz(thr), pz(mort), pz(use), pz(donor),
                         ptr(M0), ptr(cnt), ptr(event), ptr(tgroup), pz(pset), pz(pgene), pz(poff), pz(ptree), ptr(out["conc2"]),
                         ptr(out["comparable"]), ptr(out.get("D")), ptr(out.get("M")))
    return _launch_or_plan("mms_rsf_vimp", p, (x, feat, thr, mort, use, donor, M0, cnt, event, tgroup, pset, pgene, poff, ptree, out, d), res,
                           plan_only)


GBM_TABLES = dict(feat=torch.int32, bin=torch.int32, thr=torch.float32, gain=torch.float64, value=torch.float64, n_node=torch.int32,
                  G=torch.int64, H=torch.int64)
GBM_PARAMS = dict(lr=torch.float64, depth=torch.int32, min_leaf=torch.int32, l2=torch.float64, min_gain=torch.float64)
_GBM_LIM = {}


def _gbm_lim():
    """the header's MMS_GBM_* limits, parsed once (these wrappers run five times a boosting round)"""
    if not _GBM_LIM:
        _GBM_LIM.update(_lib.defines("MMS_GBM_"))
    return _GBM_LIM


def gbm_tables(P, M, nn, device):
    """The heap-indexed booster tables [P, M, nn] as mms_gbm_* expect them before round 0: feat = -1, every other table 0."""
    return {k: (torch.full((P, M, nn), -1, dtype=dt, device=device) if k == "feat" else torch.zeros(P, M, nn, dtype=dt, device=device))
            for k, dt in GBM_TABLES.items()}


def gbm_state(P, n, M, device):
    """The per-problem state of a fit: F (0), qg, qh, wt, node [P, n], loglik [P, M + 1], conc2 / comparable [P, M]."""
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
    return dict(F=z((P, n), torch.float64), qg=z((P, n), torch.int64), qh=z((P, n), torch.int64), wt=z((P, n), torch.uint8),
                node=z((P, n), torch.int32), loglik=z((P, M + 1), torch.float64), conc2=z((P, M), torch.int64),
                comparable=z((P, M), torch.int64))


def _gbm_common(mult, state, tables, params, n, need_tables=GBM_TABLES):
    """Shapes and dtypes shared by the gbm wrappers -> (P, M, nn).  params: dict of [P] device tensors (GBM_PARAMS), each optional here."""
    lim = _gbm_lim()
    _rsf_dev(mult, torch.uint8, "mult", 2)
    P = mult.shape[0]
    if mult.shape[1] != n or not (1 <= n <= lim["MAX_N"]) or P > lim["MAX_P"]:
        raise ValueError("mult must be [P, n] with n in 1..%d and P <= %d" % (lim["MAX_N"], lim["MAX_P"]))
    kinds = dict(F=torch.float64, qg=torch.int64, qh=torch.int64, wt=torch.uint8, node=torch.int32)
    for k, dt in kinds.items():
        _rsf_dev(state[k], dt, k, 2)
        if tuple(state[k].shape) != (P, n):
            raise ValueError("state[%r] must be [P, n]" % k)
    _rsf_dev(tables["feat"], torch.int32, "feat", 3)
    _, M, nn = tables["feat"].shape
    for k in need_tables:
        _rsf_dev(tables[k], GBM_TABLES[k], k, 3)
        if tuple(tables[k].shape) != (P, M, nn):
            raise ValueError("the booster tables must all be [P, M, nn]")
    if M < 1 or not (1 <= nn <= (2 << lim["MAX_DEPTH"]) - 1):
        raise ValueError("M must be >= 1 and nn in 1..%d" % ((2 << lim["MAX_DEPTH"]) - 1))
    for k, v in params.items():
        _rsf_dev(v, GBM_PARAMS[k] if k in GBM_PARAMS else torch.int32, k, 1)
        if len(v) != P:
            raise ValueError("%s must be [P]" % k)
    return P, M, nn


def _gbm_u32(t):
    """int64 values in 0 .. 2^32 - 1 -> the same bits as an int32 tensor (what a `const unsigned*` reads)"""
    if t.numel() and (int(t.min()) < 0 or int(t.max()) > 0xFFFFFFFF):
        raise ValueError("a hash threshold must lie in 0 .. 2^32 - 1")
    return torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32).contiguous()


def gbm_grad(mult, event, tgroup, rowid, subsample_u32, state, tables, round, seed, pid=None, last=False, plan_only=False):
    """Quantised Cox gradients of one round of P lock-step boosters (GbmGradP in mmsurv.h).  Device tensors: mult uint8 [P, n], event /
    tgroup / rowid int32 [n] in position (time-descending) order, subsample_u32 int32 [P] (the threshold's bits: _gbm_u32), state =
    gbm_state(...), tables = gbm_tables(...), pid int32 [P] or None.  Writes state qg / qh / wt / node / loglik[:, round] and the root of
    tables n_node / G / H [:, round]; last: only loglik[:, round] (round = M allowed)."""
    n = mult.shape[1] if torch.is_tensor(mult) and mult.dim() == 2 else 0
    params = dict(pid=pid) if pid is not None else {}
    P, M, nn = _gbm_common(mult, state, tables, params, n, ("n_node", "G", "H"))
    for t, what in ((event, "event"), (tgroup, "tgroup"), (rowid, "rowid"), (subsample_u32, "subsample")):
        _rsf_dev(t, torch.int32, what, 1)
    _rsf_dev(state["loglik"], torch.float64, "loglik", 2)
    if len(event) != n or len(tgroup) != n or len(rowid) != n or len(subsample_u32) != P or tuple(state["loglik"].shape) != (P, M + 1):
        raise ValueError("event / tgroup / rowid must be [n], subsample [P] and loglik [P, M + 1]")
    round = int(round)
    if not (0 <= round < M or (last and round == M)):
        raise ValueError("round must lie in [0, M) ([0, M] with last)")
    if P == 0:
        return None
    p = _S()["GbmGradP"](n, n, P, round, M, nn, 1 if last else 0, int(seed) & 0xffffffff, ptr(mult), ptr(event), ptr(tgroup), ptr(rowid), ptr(pid),
                         ptr(subsample_u32), ptr(state["F"]), ptr(state["qg"]), ptr(state["qh"]), ptr(state["wt"]), ptr(state["node"]),
                         ptr(state["loglik"]), ptr(tables["n_node"]), ptr(tables["G"]), ptr(tables["H"]))
    return _launch_or_plan("mms_gbm_grad", p, (mult, event, tgroup, rowid, pid, subsample_u32, state, tables), None, plan_only)


def gbm_scratch(P, p_, level, device):
    """The partial tables of mms_gbm_split for one level: (part_gain, part_cut, part_sum)"""
    nt = (int(p_) + _gbm_lim()["TILE"] - 1) // _gbm_lim()["TILE"]
    c = max(P, 1) * nt * (1 << int(level))
    return (torch.zeros(c, dtype=torch.float64, device=device), torch.zeros(4 * c, dtype=torch.int32, device=device),
            torch.zeros(2 * c, dtype=torch.int64, device=device))


def gbm_split(xb, edges, state, tables, params, colsample_u32, level, round, seed, pid=None, form=0, trace=False, scratch=None,
              plan_only=False):
    """One level of one round of P lock-step boosters: histograms, cuts, argmax, routing (GbmSplitP in mmsurv.h).  Device tensors: xb uint8
    [p, n] bins, feature-major in position order (the CALLER guarantees xb < B: boosting.bin_matrix does; checked by fit once), edges fp32
    [p, B - 1], state / tables as gbm_grad, params = dict(depth, min_leaf int32, l2, min_gain float64) [P], colsample_u32 int32 [P].
    form: 0 default, 1 members, 2 private (header: MMS_GBM_FORM_*).  trace: also return dict(n, G, H) [P, 2^level, p, B], the prefixed
    histograms of every admitted feature of every live node (zero elsewhere).  scratch: gbm_scratch(...) to reuse."""
    lim = _gbm_lim()
    _rsf_dev(xb, torch.uint8, "xb", 2); _rsf_dev(edges, torch.float32, "edges", 2)
    p_, n = xb.shape
    B = edges.shape[1] + 1
    need = {k: params[k] for k in ("depth", "min_leaf", "l2", "min_gain")}
    if pid is not None:
        need["pid"] = pid
    P, M, nn = _gbm_common(state["wt"], state, tables, need, n, ("feat", "bin", "thr", "gain", "n_node", "G", "H"))
    _rsf_dev(colsample_u32, torch.int32, "colsample", 1)
    level, round, form = int(level), int(round), int(form)
    if edges.shape[0] != p_ or not (2 <= B <= lim["MAX_BINS"]) or len(colsample_u32) != P:
        raise ValueError("edges must be [p, B - 1] with B in 2..%d and colsample [P]" % lim["MAX_BINS"])
    if not (0 <= level < lim["MAX_DEPTH"]) or nn < (4 << level) - 1 or not (0 <= round < M) or form not in (0, 1, 2):
        raise ValueError("level must lie in [0, %d) with nn >= 2^(level + 2) - 1, round in [0, M), form in 0..2" % lim["MAX_DEPTH"])
    if (1 << level) * (B + 1) > lim["LDS_CELLS"]:
        raise ValueError("the histograms of one feature at this level do not fit the workgroup's LDS")
    dev = xb.device
    out = None
    if trace:
        shape = (max(P, 1), 1 << level, p_, B)
        out = dict(n=torch.zeros(shape, dtype=torch.int32, device=dev), G=torch.zeros(shape, dtype=torch.int64, device=dev),
                   H=torch.zeros(shape, dtype=torch.int64, device=dev))
    if P == 0:
        return None if out is None else {k: v[:0] for k, v in out.items()}
    sc = gbm_scratch(P, p_, level, dev) if scratch is None else scratch
    nt = (p_ + lim["TILE"] - 1) // lim["TILE"]
    if sc[0].dtype != torch.float64 or sc[1].dtype != torch.int32 or sc[2].dtype != torch.int64 or sc[0].numel() < P * nt * (1 << level) \
            or sc[1].numel() < 4 * P * nt * (1 << level) or sc[2].numel() < 2 * P * nt * (1 << level):
        raise ValueError("scratch too small for this level (gbm_scratch)")
    g = (lambda k: ptr(out[k])) if trace else (lambda k: None)
    p = _S()["GbmSplitP"](n, n, p_, P, B, level, round, M, nn, form, int(seed) & 0xffffffff, nt, ptr(xb), ptr(state["wt"]), ptr(state["qg"]),
                          ptr(state["qh"]), ptr(edges), ptr(params["depth"]), ptr(params["min_leaf"]), ptr(params["l2"]), ptr(params["min_gain"]),
                          ptr(colsample_u32), ptr(pid), ptr(state["node"]), ptr(tables["feat"]), ptr(tables["bin"]), ptr(tables["thr"]),
                          ptr(tables["gain"]), ptr(tables["n_node"]), ptr(tables["G"]), ptr(tables["H"]), ptr(sc[0]), ptr(sc[1]), ptr(sc[2]),
                          g("n"), g("G"), g("H"))
    res = None if out is None else {k: v[:P] for k, v in out.items()}
    return _launch_or_plan("mms_gbm_split", p, (xb, edges, state, tables, params, colsample_u32, pid, sc, out), res, plan_only)


def gbm_update(event, tgroup, state, tables, params, round, evalm=None, plan_only=False):
    """Leaf values, F of every position and the evaluation pair counts of one round (GbmUpdateP in mmsurv.h).  params = dict(lr, l2
    float64 [P]); evalm uint8 [P, n] or None (no counts).  Writes tables value[:, round], state F and conc2 / comparable[:, round]."""
    _rsf_dev(event, torch.int32, "event", 1); _rsf_dev(tgroup, torch.int32, "tgroup", 1)
    n = len(event)
    P, M, nn = _gbm_common(state["wt"], state, tables, {k: params[k] for k in ("lr", "l2")}, n, ("feat", "G", "H", "value"))
    round = int(round)
    if len(tgroup) != n or not (0 <= round < M):
        raise ValueError("tgroup must be [n] and round lie in [0, M)")
    if evalm is not None:
        _rsf_dev(evalm, torch.uint8, "evalm", 2); _rsf_dev(state["conc2"], torch.int64, "conc2", 2); _rsf_dev(state["comparable"], torch.int64, "comparable", 2)
        if tuple(evalm.shape) != (P, n) or tuple(state["conc2"].shape) != (P, M) or tuple(state["comparable"].shape) != (P, M):
            raise ValueError("evalm must be [P, n] and conc2 / comparable [P, M]")
    if P == 0:
        return None
    p = _S()["GbmUpdateP"](n, n, P, round, M, nn, ptr(state["node"]), ptr(event), ptr(tgroup), ptr(evalm), ptr(params["lr"]), ptr(params["l2"]),
                           ptr(tables["feat"]), ptr(tables["G"]), ptr(tables["H"]), ptr(tables["value"]), ptr(state["F"]),
                           ptr(state["conc2"]) if evalm is not None else None, ptr(state["comparable"]) if evalm is not None else None)
    return _launch_or_plan("mms_gbm_update", p, (event, tgroup, state, tables, params, evalm), None, plan_only)


def gbm_predict(x, feat, thr, value, at, plan_only=False):
    """F of R raw rows after each of K round counts, for P boosters (GbmPredictP in mmsurv.h).  x fp32 [R, p] device (row pitch
    x.stride(0)); feat int32, thr fp32, value float64 [P, M, nn]; at: K ascending round counts in 0..M (host sequence).  feat is checked
    HERE against p.  -> float64 [P, K, R]."""
    import numpy as np
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise TypeError("x must be a float32 [R, p] device tensor with unit column stride")
    _rsf_dev(feat, torch.int32, "feat", 3); _rsf_dev(thr, torch.float32, "thr", 3); _rsf_dev(value, torch.float64, "value", 3)
    R, p_ = x.shape
    P, M, nn = feat.shape
    at = np.asarray(at, np.int64).reshape(-1)
    K = len(at)
    lim = _gbm_lim()
    if tuple(thr.shape) != (P, M, nn) or tuple(value.shape) != (P, M, nn) or M < 1 or not (1 <= nn <= (2 << lim["MAX_DEPTH"]) - 1):
        raise ValueError("thr and value must match feat [P, M, nn]")
    if K < 1 or at.min() < 0 or at.max() > M or (np.diff(at) < 0).any():
        raise ValueError("at must hold ascending round counts in 0..%d" % M)
    if P and int(feat.max()) >= p_:
        raise ValueError("the booster splits on feature %d; x has %d columns" % (int(feat.max()), p_))
    dev = x.device
    out = torch.zeros(max(P, 1), K, max(R, 1), dtype=torch.float64, device=dev)
    if P == 0 or R == 0:
        return out[:P, :, :R]
    at_d = _upload(at, "int32", dev)
    p = _S()["GbmPredictP"](R, max(x.stride(0), p_), p_, P, M, nn, K, 0, ptr(x), ptr(feat), ptr(thr), ptr(value), ptr(at_d), ptr(out))
    return _launch_or_plan("mms_gbm_predict", p, (x, feat, thr, value, at_d, out), out, plan_only)


def tree_shap(x, feat, thr, value, cover, goff, slot, U, use=None, plan_only=False, out=None):
    """Path-dependent TreeSHAP of G groups of trees for R raw rows (TreeShapP in mmsurv.h).  x fp32 [R, p] device (row pitch
    x.stride(0)); feat int32, thr fp32, value float64, cover int32, slot int32 [T, nn] device; goff: G + 1 ascending tree offsets from 0
    to T (host sequence); U >= 1 output columns; use uint8 [T, R] device (row pitch use.stride(0)) or None (every tree admits every
    row).  What the launch cannot check is checked HERE: feat < p, slot in [0, U) and the cover rule (tree_shap.check_tables: at every
    split node the children's covers are > 0 and sum to the node's).  out = (phi float64 [G, U, ldr], base float64 [G, ldr]) device
    tensors to write into (ldr >= R; columns >= R are left alone), None: fresh ones with ldr = R.
    -> (phi [G, U, R], base [G, R]) float64 device tensors, SLOT-major: phi[g][slot][row]."""
    import numpy as np
    from . import tree_shap as _ts
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise TypeError("x must be a float32 [R, p] device tensor with unit column stride")
    _rsf_dev(feat, torch.int32, "feat", 2); _rsf_dev(thr, torch.float32, "thr", 2); _rsf_dev(value, torch.float64, "value", 2)
    _rsf_dev(cover, torch.int32, "cover", 2); _rsf_dev(slot, torch.int32, "slot", 2)
    R, p_ = x.shape
    T, nn = feat.shape
    U = int(U)
    goff = np.asarray(goff, np.int64).reshape(-1)
    G = len(goff) - 1
    lim = _lib.defines("MMS_SHAP_")
    if any(tuple(t.shape) != (T, nn) for t in (thr, value, cover, slot)) or not (1 <= nn <= (2 << lim["MAX_DEPTH"]) - 1):
        raise ValueError("thr, value, cover and slot must match feat [T, nn], nn in 1..%d" % ((2 << lim["MAX_DEPTH"]) - 1))
    if G < 0 or p_ < 1 or U < 1 or (G >= 0 and len(goff) and (goff[0] != 0 or goff[-1] != T or (np.diff(goff) < 0).any())):
        raise ValueError("goff must ascend from 0 to T = %d, U >= 1 and x have a column" % T)
    if T:
        if int(feat.max()) >= p_:
            raise ValueError("a tree splits on feature %d; x has %d columns" % (int(feat.max()), p_))
        split = _ts.split_nodes(feat)
        sl = slot[:, :split.shape[1]][split]
        if sl.numel() and (int(sl.min()) < 0 or int(sl.max()) >= U):
            raise ValueError("slot must lie in [0, U) at every split node")
        _ts.check_tables(feat, cover)
    ldu = 0
    if use is not None:
        if not torch.is_tensor(use) or not use.is_cuda or use.dtype != torch.uint8 or use.dim() != 2 or tuple(use.shape) != (T, R) \
                or (R > 1 and use.stride(1) != 1) or (T > 1 and use.stride(0) < R):
            raise TypeError("use must be a uint8 [T, R] device tensor with unit column stride")
        ldu = max(int(use.stride(0)), R) if T > 1 else R
    dev = x.device
    if out is None:
        phi, base = torch.empty(max(G, 1), U, max(R, 1), dtype=torch.float64, device=dev), torch.empty(max(G, 1), max(R, 1), dtype=torch.float64, device=dev)
    else:
        phi, base = out
        _rsf_dev(phi, torch.float64, "phi", 3); _rsf_dev(base, torch.float64, "base", 2)
        if phi.shape[0] != max(G, 1) or phi.shape[1] != U or base.shape[0] != max(G, 1) or phi.shape[2] != base.shape[1] or base.shape[1] < max(R, 1):
            raise ValueError("out must be (phi [G, U, ldr], base [G, ldr]) with ldr >= R")
    ldr = int(base.shape[1])
    res = (phi[:G, :, :R], base[:G, :R])
    if T == 0:                                                      # groups without a tree: zeros, and nothing to launch
        res[0].zero_(); res[1].zero_()
    if G == 0 or R == 0 or T == 0:
        return ((None, ()) + res) if plan_only else res
    goff_d = _upload(goff, "int32", dev)
    p = _S()["TreeShapP"](R, max(x.stride(0), p_), p_, T, nn, G, U, ldr, ldu, 0, ptr(x), ptr(feat), ptr(thr), ptr(value), ptr(cover), ptr(goff_d),
                          ptr(slot), ptr(use), ptr(phi), ptr(base))
    return _launch_or_plan("mms_tree_shap", p, (x, feat, thr, value, cover, goff_d, slot, use, phi, base), res, plan_only)


def td_metrics(trank, event, hcut, rord, surv, w, plan_only=False):
    """IPCW Brier / dynamic AUC sums of M models at H horizons under R multiplicity rows (TdMetricsP in mmsurv.h).  trank, event: [n] dense
    time ranks and event flags of the TIME-ASCENDING positions (events before censorings at equal times), hcut: [H] positions with
    t <= tau_h, rord: [M, n] 2 * position + [last of its risk tie group] in risk-ascending order -- host arrays
    (absolute_risk.metric_inputs makes them); surv: float64 [M, n, H] predicted survival per position, w: int8 [R, n] multiplicities --
    host arrays or device tensors.  The launch cannot check the tables, so they are checked HERE (as ops.logrank_scan checks its cuts):
    trank dense and non-decreasing from 0, no event after a censoring inside a time group, hcut non-decreasing in [0, n] and on
    group boundaries, every rord row a permutation whose last entry ends a group, surv finite, w in 0..127 with a positive sum in every
    row.  -> dict of float64 device tensors G, km, wcase, wctrl [R, H], brier, auc_num [R, M, H].  plan_only: upload and check, do not
    launch -> (TdMetricsP, the tensors it points to, the dict), for call("mms_td_metrics", p) by the caller (tools/bench_td_metrics.py
    times the launch alone)."""
    import numpy as np
    dev = next((t.device for t in (surv, w) if torch.is_tensor(t) and t.is_cuda), torch.device("cuda"))
    trank, event = np.asarray(trank, dtype=np.int64).reshape(-1), np.asarray(event, dtype=np.int64).reshape(-1)
    hcut, rord = np.asarray(hcut, dtype=np.int64).reshape(-1), np.asarray(rord, dtype=np.int64)
    n, H = len(trank), len(hcut)
    if n < 1 or H < 1 or len(event) != n or rord.ndim != 2 or rord.shape[0] < 1 or rord.shape[1] != n:
        raise ValueError("trank / event must have n >= 1 entries, hcut H >= 1 and rord must be [M >= 1, n]")
    M = rord.shape[0]
    step = np.diff(trank)
    if trank[0] != 0 or ((step != 0) & (step != 1)).any():
        raise ValueError("trank must be dense ranks of ascending times: from 0, every step 0 or 1")
    if ((event != 0) & (event != 1)).any() or ((step == 0) & (np.diff(event) > 0)).any():
        raise ValueError("event must be 0 / 1 and, inside a group of equal times, events must precede censorings")
    inner = hcut[(hcut > 0) & (hcut < n)]
    if (hcut < 0).any() or (hcut > n).any() or (np.diff(hcut) < 0).any() or (trank[inner - 1] == trank[inner]).any():
        raise ValueError("hcut must be non-decreasing in [0, n] and must not split a group of equal times")
    if (rord < 0).any() or not (np.sort(rord >> 1, 1) == np.arange(n)).all() or not (rord[:, -1] & 1).all():
        raise ValueError("every row of rord must be 2 * (a permutation of 0..n-1) + flag, the last entry flagged")
    if not torch.is_tensor(surv):
        surv = torch.from_numpy(np.ascontiguousarray(np.asarray(surv, dtype=np.float64)))
    if not torch.is_tensor(w):
        w = torch.from_numpy(np.ascontiguousarray(np.asarray(w)))
    if surv.dtype != torch.float64 or tuple(surv.shape) != (M, n, H) or not bool(torch.isfinite(surv).all()):
        raise ValueError("surv must be finite float64 [M, n, H] = [%d, %d, %d]" % (M, n, H))
    if w.dtype != torch.int8 or w.dim() != 2 or w.shape[1] != n:
        raise ValueError("w must be int8 [R, n]")
    R = w.shape[0]
    if R and (bool((w < 0).any()) or bool((w.sum(1, dtype=torch.int64) < 1).any())):
        raise ValueError("w must hold multiplicities 0..127 and every row must draw a patient")
    surv, w = surv.to(dev).contiguous(), w.to(dev).contiguous()
    t = {k: _upload(a, np.int32, dev) for k, a in dict(trank=trank, event=event, hcut=hcut, rord=rord).items()}
    t.update(surv=surv, w=w if R else torch.zeros(1, n, dtype=torch.int8, device=dev))               # (never a NULL pointer)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
    out = dict(G=z(max(R, 1), H), km=z(max(R, 1), H), wcase=z(max(R, 1), H), wctrl=z(max(R, 1), H), brier=z(max(R, 1), M, H),
               auc_num=z(max(R, 1), M, H))
    p = _S()["TdMetricsP"](n, H, M, R, ptr(t["trank"]), ptr(t["event"]), ptr(t["hcut"]), ptr(t["rord"]), n, ptr(t["surv"]), H, ptr(t["w"]), n,
                           ptr(out["G"]), ptr(out["km"]), ptr(out["wcase"]), ptr(out["wctrl"]), ptr(out["brier"]), ptr(out["auc_num"]))
    res = {k: v[:R] for k, v in out.items()}
    return _launch_or_plan("mms_td_metrics", p, (t, out), res, plan_only)


COX_NEWTON_STATUS = {1: "converged", 2: "max_iter", 3: "singular", 4: "monotone likelihood", 5: "no step accepted", 6: "no events"}


def cox_newton(x, time, event, glast, w, cmask, tol=1e-9, max_iter=30, beta_max=30.0, info=False, plan_only=False):
    """Newton-Raphson Cox fits of R multiplicity rows x S covariate subsets (CoxNewtonP in mmsurv.h).  x: float64 [n, p] covariates of
    the TIME-DESCENDING positions, w: int8 [R, n] multiplicities -- host arrays or device tensors (a view's row pitch x.stride(0) /
    w.stride(0) is passed on); time, event, glast: [n] the positions' times, event flags and 1 at the last position of each group of
    equal times, cmask: [S] column sets (bit a = column a) -- host arrays.  The launch cannot check the tables, so they are checked
    HERE (as ops.td_metrics checks its own): times
    non-increasing, glast exactly the ends of the groups of equal times, x finite, w >= 0, every mask non-empty and below 2^p.
    -> dict of device tensors beta, se (float64 [R, S, p]), loglik, loglik0 (float64 [R, S]), iters, status (int32 [R, S]) and, with
    info, info (float64 [R, S, p, p]).  plan_only: upload and check, do not launch -> (CoxNewtonP, the tensors it points to, the dict),
    for call("mms_cox_newton", p) by the caller (tools/bench_cox_newton.py times the launch alone)."""
    import numpy as np
    dev = next((t.device for t in (x, w) if torch.is_tensor(t) and t.is_cuda), torch.device("cuda"))
    time, event = np.asarray(time, dtype=np.float64).reshape(-1), np.asarray(event, dtype=np.int64).reshape(-1)
    glast, cmask = np.asarray(glast, dtype=np.int64).reshape(-1), np.asarray(cmask, dtype=np.int64).reshape(-1)
    n, S = len(time), len(cmask)
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64)))
    if not torch.is_tensor(w):
        w = torch.from_numpy(np.ascontiguousarray(np.asarray(w)))
    if x.dtype != torch.float64 or x.dim() != 2 or x.shape[0] != n or n < 1 or x.shape[1] < 1 or x.stride(1) != 1:
        raise ValueError("x must be float64 [n, p] with n = len(time) >= 1, p >= 1 and unit column stride")
    p = x.shape[1]
    if len(event) != n or len(glast) != n or ((event != 0) & (event != 1)).any():
        raise ValueError("event and glast must have n entries and event must be 0 / 1")
    if not np.isfinite(time).all() or (np.diff(time) > 0).any():
        raise ValueError("the positions must stand in time-descending order (finite times)")
    if not np.array_equal(glast != 0, np.concatenate([time[1:] != time[:-1], [True]])):
        raise ValueError("glast must be 1 exactly at the last position of every group of equal times")
    if not bool(torch.isfinite(x).all()):
        raise ValueError("x must be finite")
    if w.dtype != torch.int8 or w.dim() != 2 or w.shape[1] != n or (w.shape[0] > 1 and w.stride(1) != 1):
        raise ValueError("w must be int8 [R, n]")
    R = w.shape[0]
    if R and bool((w < 0).any()):
        raise ValueError("w must hold multiplicities 0..127")
    if ((cmask <= 0) | (cmask >= (1 << p))).any():
        raise ValueError("every mask must name at least one of the %d columns and none beyond them" % p)
    x, w = x.to(dev), w.to(dev)
    if n > 1 and x.stride(0) < p:
        x = x.contiguous()
    if R == 0 or (R > 1 and w.stride(0) < n) or w.stride(1) != 1:
        w = w.contiguous() if R else torch.zeros(1, n, dtype=torch.int8, device=dev)          # (never a NULL pointer)
    t = dict(x=x, w=w, event=_upload(event, np.int32, dev), glast=_upload(glast != 0, np.int32, dev), cmask=_upload(cmask, np.int32, dev))
    Q = max(R * S, 1)
    zd = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
    zi = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)
    out = dict(beta=zd(Q, p), se=zd(Q, p), loglik=zd(Q), loglik0=zd(Q), iters=zi(Q), status=zi(Q))
    if info:
        out["info"] = zd(Q, p, p)
    P = _S()["CoxNewtonP"](n, p, R, S, ptr(x), max(x.stride(0), p) if n > 1 else p, ptr(t["event"]), ptr(t["glast"]), ptr(w),
                           max(w.stride(0), n) if R > 1 else n, ptr(t["cmask"]), float(tol), int(max_iter), float(beta_max), ptr(out["beta"]),
                           ptr(out["se"]), ptr(out["loglik"]), ptr(out["loglik0"]), ptr(out["iters"]), ptr(out["status"]), ptr(out.get("info")))
    res = {k: v[:R * S].reshape((R, S) + tuple(v.shape[1:])) for k, v in out.items()}
    return _launch_or_plan("mms_cox_newton", P, (t, out), res, plan_only)


COXNET_STATUS = {-1: "new", 0: "not converged", 1: "converged", 2: "not converged"}


def coxnet_plan(x, row, event, glast, mult, lam, alpha, scale=None, beta=None, G=None, tol=1e-6, max_iter=5000):
    """Upload and check the problems of one elastic-net Cox call (CoxnetP in mmsurv.h) -> (CoxnetP, dict of the device tensors it points
    to).  x: fp32 [N, >= G] device matrix; row / event / glast: [n] the shared row list (time descending), its event flags and tie-group
    end flags; mult: [P, n] integer multiplicities; lam, alpha: [P]; scale: None or [P, G]; beta: None (zeros) or [P, G] start / point of
    evaluation -- host arrays.  The launch cannot check them, so they are checked HERE (as ops.gene_screen checks its rows): rows in
    [0, N), mult >= 0, lam >= 0 and finite, alpha in [0, 1], scale > 0 and finite (the device gets its reciprocal).  The state is that of NEW problems: status -1,
    trial = beta, step 1, iters 0, counter P."""
    import numpy as np
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise TypeError("x must be a 2-D fp32 device tensor with unit column stride")
    N, G = x.shape[0], x.shape[1] if G is None else int(G)
    if N < 1 or not 1 <= G <= x.shape[1]:
        raise ValueError("x must have N >= 1 rows and 1 <= G <= %d columns" % x.shape[1])
    row = np.asarray(row, dtype=np.int64).reshape(-1)
    n = len(row)
    event, glast = np.asarray(event).reshape(-1) != 0, np.asarray(glast).reshape(-1) != 0
    mult = np.asarray(mult)
    if mult.ndim != 2 or mult.shape[1] != n or len(event) != n or len(glast) != n:
        raise ValueError("mult must be [P, n] and event / glast [n] for the n = %d rows of the list" % n)
    P = mult.shape[0]
    if not np.array_equal(mult, np.floor(mult)) or (mult < 0).any() or (mult >= 2 ** 31).any():
        raise ValueError("multiplicities must be integers >= 0")
    if n and (row.min() < 0 or row.max() >= N):
        raise ValueError("rows must lie in [0, %d)" % N)
    if n and not glast[-1]:
        raise ValueError("the last row of the list ends a tie group: glast[-1] must be set")
    if P * max(n, G) >= 2 ** 31:
        raise ValueError("P * max(rows, G) must stay below 2^31")
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (P,)).copy()
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (P,)).copy()
    if not (np.isfinite(lam).all() and (lam >= 0).all()):
        raise ValueError("lambda must be finite and >= 0")
    if not ((alpha >= 0).all() and (alpha <= 1).all()):
        raise ValueError("alpha must lie in [0, 1]")
    if scale is not None:
        scale = np.ascontiguousarray(np.asarray(scale, dtype=np.float64))
        if scale.shape != (P, G) or not (np.isfinite(scale).all() and (scale > 0).all()):
            raise ValueError("scale must be [P, G], finite and > 0")
    beta = np.zeros((P, G)) if beta is None else np.ascontiguousarray(np.asarray(beta, dtype=np.float64))
    if beta.shape != (P, G) or not np.isfinite(beta).all():
        raise ValueError("beta must be [P, G] and finite")
    if not (0 < float(tol) <= 1.0) or not 1 <= int(max_iter) <= 100000000:
        raise ValueError("tol must lie in (0, 1] and max_iter in [1, 1e8]")
    dev = x.device
    f64 = lambda *s: torch.zeros(max(int(np.prod(s)), 1), dtype=torch.float64, device=dev)
    i32 = lambda k: torch.zeros(max(k, 1), dtype=torch.int32, device=dev)
    t = {k: _upload(a, np.int32, dev) for k, a in dict(row=row, event=event, glast=glast, mult=mult).items()}
    t.update({k: _upload(a, np.float64, dev) for k, a in dict(lam=lam, alpha=alpha, beta=beta, trial=beta).items()})
    t.update(x=x, scale=None if scale is None else _upload(1.0 / scale, np.float64, dev), grad=f64(P, G), f=f64(P), step=f64(P) + 1.0,
             iters=i32(P), status=i32(P) - 1, loss=f64(P), nsum=f64(P), kkt=f64(P), obj=f64(P), E=f64(P, n), R=f64(P, n), Gr=f64(P, G),
             counter=i32(1) + P)
    p = _S()["CoxnetP"](ptr(x), N, x.stride(0), G, n, ptr(t["row"]), ptr(t["event"]), ptr(t["glast"]), P, ptr(t["mult"]), ptr(t["lam"]),
                        ptr(t["alpha"]), ptr(t["scale"]), ptr(t["beta"]), ptr(t["trial"]), ptr(t["grad"]), ptr(t["f"]), ptr(t["step"]),
                        ptr(t["iters"]), ptr(t["status"]), ptr(t["loss"]), ptr(t["nsum"]), ptr(t["kkt"]), ptr(t["obj"]), ptr(t["E"]),
                        ptr(t["R"]), ptr(t["Gr"]), ptr(t["counter"]), float(tol), int(max_iter))
    t.update(P=P, G=G, n=n)
    return p, t


def _coxnet_out(t, names):
    P, G, n = t["P"], t["G"], t["n"]
    shape = dict(beta=(P, G), grad=(P, G), E=(P, n), R=(P, n))
    import math
    return {k: t[k][:math.prod(shape.get(k, (P,)))].reshape(shape.get(k, (P,))).cpu().numpy() for k in names}


def coxnet_eval(x, row, event, glast, mult, lam, alpha, beta, scale=None, G=None):
    """One evaluation of P elastic-net Cox problems at beta (mms_coxnet_eval; arguments as coxnet_plan) -> dict of float64 numpy arrays:
    eta, r [P, n]; grad [P, G] (the smooth part's gradient, on the scaled genes); loss (the negative partial log-likelihood, not divided
    by n), n, f (smooth part), obj, kkt [P].  An empty row list launches nothing: loss 0 and gradient lam (1 - alpha) beta, by the same
    rule as a problem without rows."""
    p, t = coxnet_plan(x, row, event, glast, mult, lam, alpha, scale=scale, beta=beta, G=G)
    if t["P"] and t["n"]:
        _lib.check(_lib.load_library().mms_coxnet_eval(ctypes.byref(p), stream()), "mms_coxnet_eval")
        o = _coxnet_out(t, ("E", "R", "grad", "loss", "nsum", "f", "obj", "kkt"))
        return dict(eta=o["E"], r=o["R"], grad=o["grad"], loss=o["loss"], n=o["nsum"], f=o["f"], obj=o["obj"], kkt=o["kkt"])
    return _coxnet_no_rows(t)


def _coxnet_no_rows(t):
    """What the definitions give a call without rows (nothing to launch): loss 0, gradient lam (1 - alpha) beta."""
    import numpy as np
    P, G = t["P"], t["G"]
    o = _coxnet_out(t, ("beta", "lam", "alpha"))
    b, l1, l2 = o["beta"], (o["lam"] * o["alpha"])[:, None], (o["lam"] * (1 - o["alpha"]))[:, None]
    g = l2 * b
    rho = np.where(b != 0, np.abs(g + l1 * np.sign(b)), np.maximum(np.abs(g) - l1, 0.0)).max(1) if P else np.zeros(0)
    f = 0.5 * l2[:, 0] * (b * b).sum(1)
    return dict(eta=np.zeros((P, 0)), r=np.zeros((P, 0)), grad=g, loss=np.zeros(P), n=np.zeros(P), f=f,
                obj=f + l1[:, 0] * np.abs(b).sum(1), kkt=rho, beta=b)


def coxnet_fit(x, row, event, glast, mult, lam, alpha, scale=None, beta=None, G=None, tol=1e-6, max_iter=5000, check_every=50):
    """Fit P elastic-net Cox problems in lock-step (mms_coxnet_iterate; arguments as coxnet_plan, beta = the start, zeros by default):
    enqueue check_every rounds, read the device counter of unfinished problems (one 4-byte copy), until it is zero; max_iter bounds every
    problem's own count on the device.  -> dict of numpy arrays: beta, grad [P, G]; f, obj, kkt, step [P]; iters, status [P] (1 =
    converged, 2 = max_iter reached without convergence: not a fit) and eta [P, n] of the last evaluated point."""
    import numpy as np
    p, t = coxnet_plan(x, row, event, glast, mult, lam, alpha, scale=scale, beta=beta, G=G, tol=tol, max_iter=max_iter)
    check_every = max(1, int(check_every))
    if t["P"] and t["n"]:
        lib = _lib.load_library()
        rounds = 0
        while rounds <= int(max_iter) + 1:
            _lib.check(lib.mms_coxnet_iterate(ctypes.byref(p), check_every, stream()), "mms_coxnet_iterate")
            rounds += check_every
            if int(t["counter"].item()) <= 0:
                break
        o = _coxnet_out(t, ("beta", "grad", "f", "obj", "kkt", "step", "iters", "status", "E"))
        o["eta"] = o.pop("E")
        return o
    o = _coxnet_no_rows(t)
    P = t["P"]
    conv = o["kkt"] <= tol
    return dict(beta=o["beta"], grad=o["grad"], f=o["f"], obj=o["obj"], kkt=o["kkt"], step=np.ones(P), iters=np.zeros(P, np.int32),
                status=np.where(conv, 1, 2).astype(np.int32), eta=o["eta"])


def adam_params(p_, g, m, v, hyper, sumsq, step, skip_flag=None, adamw=False, acc=None, cox_out=None, entropy=None,
                rng=None, w2=None):
    """w2: None or dict(off=int64[n] device tensor, pack_b=ptr table (int64[n] device tensor of addresses), pack_f=the same,
    fragmask=int): the conv2 tensors kept in packed primary storage inside the flat buffers (AdamP.w2_*, include/mmsurv.h)."""
    a = _S()["AdamP"](ptr(p_), ptr(g), ptr(m), ptr(v), p_.numel(), ptr(hyper), ptr(sumsq), ptr(step), ptr(skip_flag),
                      1 if adamw else 0, ptr(acc), ptr(cox_out), ptr(entropy), ptr(rng))
    if w2 is not None:
        a.w2_off, a.w2_pack_b, a.w2_pack_f = ptr(w2["off"]), ptr(w2["pack_b"]), ptr(w2["pack_f"])
        a.n_w2, a.w2_fragmask = int(w2["off"].numel()), int(w2["fragmask"])
    return a


def tune_table(bounds, lr_mult, wd_mult, l2sp, device):
    """The device tables of TuneP (include/mmsurv.h) from host sequences: one table serves every plan of an engine and every member of a
    fold group."""
    nseg = len(lr_mult)
    if len(bounds) != nseg + 1 or len(wd_mult) != nseg or len(l2sp) != nseg:
        raise ValueError("tune_table: bounds needs one entry more than the multipliers")
    return dict(nseg=nseg, bounds=torch.tensor([int(b) for b in bounds], dtype=torch.int64, device=device),
                lr_mult=torch.tensor([float(x) for x in lr_mult], dtype=torch.float32, device=device),
                wd_mult=torch.tensor([float(x) for x in wd_mult], dtype=torch.float32, device=device),
                l2sp=torch.tensor([float(x) for x in l2sp], dtype=torch.float32, device=device))


def tune_params(adam, table, anchor=None, check=True):
    """TuneP around an AdamP block (adam_params) and a tune_table.  check: mms_tune_check reads the tables back and validates them
    against the block (it synchronises: not inside a graph capture)."""
    t = _S()["TuneP"]()
    t.a = adam
    t.bounds, t.lr_mult, t.wd_mult, t.l2sp = ptr(table["bounds"]), ptr(table["lr_mult"]), ptr(table["wd_mult"]), ptr(table["l2sp"])
    t.nseg, t.anchor = int(table["nseg"]), ptr(anchor)
    if check:
        _lib.check(_lib.load_library().mms_tune_check(ctypes.byref(t)), "mms_tune_check")
    return t


_WORKER_STREAMS = {}


def worker_streams(device, n):
    """The process-wide HIP streams that concurrent fold (sub-)groups step on: created once, in a fixed order, and shared by every
    consumer (training epoch, validation pass, the benchmark's legs).  HIP multiplexes streams onto a few hardware queues in the order
    they were first created/used, so side streams created later in a process (after graph-capture warm-up streams, per-engine streams ...)
    can end up sharing a queue: measured on the 2 x 10-model leg of bench.py -- 3550 vs 2740 patients/s depending only on how many
    streams the legs before it had created.  One early, fixed set keeps the mapping the same for the whole run."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    lst = _WORKER_STREAMS.setdefault(key, [])
    if n > len(lst):
        import os, warnings
        cap = int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4)        # ROCm's cap on hardware queues per device; the null stream takes one
        if n + 1 > cap:
            warnings.warn(f"{n} worker streams + the null stream on GPU_MAX_HW_QUEUES={cap} hardware queues: two streams will share a queue and "
                          f"serialise (K = 5 epoch, four sub-groups: 1879 patients/s against 2696 with GPU_MAX_HW_QUEUES=5; "
                          f"profiles/r03_cu_partition_experiments.txt).  Set GPU_MAX_HW_QUEUES >= {n + 1} before the process starts, "
                          f"or use <= {cap - 1} streams.", RuntimeWarning, stacklevel=2)
    while len(lst) < n:
        lst.append(torch.cuda.Stream(device=device))
    return lst[:n]


def cluster_workgroups(B, dims):
    """Workgroups per model of the persistent per-block ("cluster") launches of dense blocks 3 and 4 (csrc/dn_cl.hip; the rule of
    csrc/dn_net.hip make_plan): clusters of 8 workgroups, each owning whole samples with <= 16 or <= 32 rows; 0 = the block has too many
    voxels per sample (or too many clusters) and runs per layer."""
    out = []
    for shift in (4, 5):
        vox = max(1, (dims[0] >> shift) * (dims[1] >> shift) * (dims[2] >> shift))
        rt = 1 if vox <= 16 else (2 if vox <= 32 else 0)
        if not rt:
            out.append(0)
            continue
        spc = min(B, (16 * rt) // vox)
        ncl = -(-B // spc)
        out.append(8 * ncl if ncl <= 8 else 0)
    return tuple(out)


def fused_layer_workgroups(B, dims):
    """(producers, consumers) per model of the fused block-3 forward launch (csrc/dn_c3s.hip mms_c3s_c1s_fwd: conv2 of layer l as
    16-row tiles x two 16-column halves, conv1 of layer l + 1 as 16 x 16 tiles of its 128 outputs; the rule of csrc/dn_net.hip
    fuse_block); (0, 0) = more than 128 rows, never fused."""
    M = B * max(1, (dims[0] >> 4) * (dims[1] >> 4) * (dims[2] >> 4))
    if M > 128:
        return (0, 0)
    tiles = -(-M // 16)
    return (2 * tiles, 8 * tiles)


def persistent_opts(base, device, ng, B, dims):
    """MmsDnOpts for a driver call of ng lock-step models: `base` with persist_b3 / persist_b4 switched to the per-layer path (-1) where
    the persistent launches of all worker streams could not be co-resident -- their workgroups hand data to each other inside the
    launch, one such launch per worker stream may be in flight, and the chip has a fixed number of CUs (the kernels' bounded sweeps +
    time-out word stay as the backstop).  The rule shared by SurvivalEngine, FoldGroupEngine and bench.py; decided at launch (=
    graph-capture) time and passed to the drivers as an argument."""
    if dims is None or len(dims) != 3:
        return base
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    w3, w4 = cluster_workgroups(B, dims)
    kw = {}
    if base.persist_b3 > 0 and w3 * ng * max_worker_streams() > cus:
        kw["persist_b3"] = -1
    if base.persist_b4 >= 0 and w4 * ng * max_worker_streams() > cus:
        kw["persist_b4"] = -1
    # fused block-3 forward (fuse_layers): its conv1 workgroups wait inside the launch for its conv2 ones.  Every worker stream may have
    # one such launch in flight, and one block-4 persistent launch; the fused kernel holds two workgroups per CU (256 VGPRs, 78 KB of
    # LDS), a block-4 cluster workgroup is counted as one of them.  The waiting workgroups of all streams must leave room for one
    # launch's producers (3 streams x 2 models -> 3 x 2 x (64 + 8) + 2 x 16 = 464 <= 512).
    fp, fc = fused_layer_workgroups(B, dims)
    if base.fuse_layers >= 0 and fc:
        b4 = w4 if kw.get("persist_b4", base.persist_b4) >= 0 else 0
        if max_worker_streams() * ng * (fc + b4) + ng * fp > 2 * cus:
            kw["fuse_layers"] = -1
    return dn_opts(base, **kw) if kw else base


def persistent_b4_fits(device, ng, B=4, dims=(64, 64, 32)):
    """Whether dense block 4 runs as one persistent launch per pass for ng lock-step models per worker stream (bench.py's mirror of the drivers)."""
    return persistent_opts(dn_opts(), device, ng, B, dims).persist_b4 >= 0


def max_worker_streams():
    """How many worker streams this process has created (over all devices: an upper bound on concurrently stepping sub-groups)."""
    return max([len(v) for v in _WORKER_STREAMS.values()] or [1])
