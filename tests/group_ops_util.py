"""Builders for tests/test_gpu_group_ops.py: the DenseNet ops through their fold-group entry points (mms_*_group) with ng > 1.

A *member* is one model's problem for one op: its own activations, weights, BatchNorm parameters and statistics and gradients, seeded by
(case, member index), its device copies and its CPU references -- torch's F.batch_norm / F.conv3d / pooling under autograd, fp64 column sums
for the statistics; the functions tests/test_gpu_dn_fwd_ops.py and tests/test_gpu_dn_bwd_ops.py compare with.  Built once per key and left
unchanged.

A *launch* function takes any list of members (a group, one member alone, the group reversed), fills a ctypes array of the op's parameter
blocks and calls the _group entry directly.  Store-written outputs of all members live in ONE allocation [n + 1, rows, ld] pre-filled with
NaN whose slot n is never passed to the launch; after the launch every member's window must hold no NaN and everything outside the windows
must still be NaN (check_windows).  Accumulators (fp64 statistics, fp32 weight gradients) start from zero.  Each launch returns the members'
results and the kernel form the launcher takes for it (ops.launch_form: the library's own answer, from the launcher's predicates).
"""
import ctypes
import zlib

import torch
import torch.nn.functional as F

from gpu_util import DEV, cl

NAN = float("nan")
_MEM = {}


def env():
    from multimodal_survival_prediction_amd import _lib, ops
    return _lib.load_library(), _lib.structs(), ops, _lib


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def cached(key, make):
    if key not in _MEM:
        _MEM[key] = make()
    return _MEM[key]


def dev(t):
    return t.detach().to(DEV).contiguous()


def colsums(t):
    d = t.double()
    return d.sum(0).contiguous(), (d * d).sum(0).contiguous()


def zeros64(n):
    return torch.zeros(n, dtype=torch.float64, device=DEV)


def nan_slots(n, rows, ld):
    return torch.full((n + 1, rows, ld), NAN, device=DEV)


def check_windows(buf, n, c0, c1, what):
    """(c) of the file's docstring: windows written completely, nothing else touched."""
    for g in range(n):
        assert not bool(torch.isnan(buf[g][:, c0:c1]).any()), "%s: member %d left NaN in its window" % (what, g)
        assert bool(torch.isnan(buf[g][:, :c0]).all()) and bool(torch.isnan(buf[g][:, c1:]).all()), "%s: member %d wrote outside its columns" % (what, g)
    assert bool(torch.isnan(buf[n]).all()), "%s: the slot behind the last member was written" % what


def group_call(entry, S, blocks, opts=None, takes_opts=True):
    """-> the entry's return code"""
    lib, _, ops, _ = env()
    arr = (S * len(blocks))(*blocks)
    fn = getattr(lib, entry)
    rc = fn(arr, len(blocks), ops.opts_ref(opts), ops.stream()) if takes_opts else fn(arr, len(blocks), ops.stream())
    torch.cuda.synchronize()
    return rc


def order_spread(terms):
    """What the ORDER of fp32 additions alone does to a sum of these terms ([T, ...], CPU fp32): the largest element-wise difference between
    two random orders, each started from 0 as the atomics on a zeroed gradient are -- the largest over eight such pairs, so that one pair
    of orders that happen to agree does not make the value 0."""
    g = torch.Generator().manual_seed(7)

    def total(perm):
        a = torch.zeros_like(terms[0])
        for i in perm.tolist():
            a = a + terms[i]
        return a
    T = terms.shape[0]
    return max(float((total(torch.randperm(T, generator=g)) - total(torch.randperm(T, generator=g))).abs().max()) for _ in range(8))


def chunks(M, msplit):
    mc = ((M + msplit - 1) // msplit + 31) // 32 * 32
    return [(z * mc, min(M, z * mc + mc)) for z in range(msplit) if z * mc < M]


def _bn_params(g, C):
    return (torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2, torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5)


def _rows5(m):
    """[M, C] -> [1, C, M, 1, 1]: any row count as a volume for torch's 3-d ops"""
    return m.t().reshape(1, m.shape[1], m.shape[0], 1, 1).contiguous()


def bnsrc(m, pre, rows, train=True):
    _, _, ops, _ = env()
    return ops.bnsrc(m[pre + "gamma"], m[pre + "beta"], rows, train, m[pre + "sum"], m[pre + "sumsq"], m.get(pre + "rm"), m.get(pre + "rv"))


# ---- 1x1x1 convolution, forward -----------------------------------------------------------------------------------------------------------
def c1f_member(case, g, M, K, N=128, pool_dims=None):
    """pool_dims = (B, dims): a transition (M = B * dims / 8 pooled rows); else M plain rows"""
    def make():
        r = gen("c1f", case, g)
        if pool_dims:
            B, dims = pool_dims
            x5 = torch.randn(B, K, *dims, generator=r) + 0.2
        else:
            x5 = _rows5(torch.randn(M, K, generator=r) * 1.5 + 0.3)
        gamma, beta, rm, rv = _bn_params(r, K)
        w = torch.randn(N, K, generator=r) / K ** 0.5
        ref, act = {}, {}
        for t in (1, 0):
            a = F.relu(F.batch_norm(x5, None if t else rm.clone(), None if t else rv.clone(), gamma, beta, training=bool(t), momentum=0.0, eps=1e-5))
            y = F.conv3d(a, w.view(N, K, 1, 1, 1))
            ref[t] = cl(F.avg_pool3d(y, 2, 2) if pool_dims else y)
            act[t] = cl(F.avg_pool3d(a, 2, 2)) if pool_dims else None
        xm = cl(x5)
        slab = torch.randn(xm.shape[0], K + 4, generator=r)          # finite columns behind K: a kernel that reads them gets wrong sums
        slab[:, :K] = xm
        slab = dev(slab)
        s, q = colsums(slab[:, :K])
        return dict(M=M, K=K, N=N, pool=pool_dims, slab=slab, w=dev(w), ref=ref, act=act, gamma=dev(gamma), beta=dev(beta), rm=dev(rm), rv=dev(rv),
                    sum=s, sumsq=q)
    return cached(("c1f", case, g, M, K, N, pool_dims), make)


def launch_c1f(members, opts=None, train=True, ksplit=0, pooled=None):
    """mms_conv1_fwd_group.  pooled: the members' pooled operands (launch_pool_act) -> plain convolution over them with the identity BatchNorm
    block.  -> ([dict(y, sum, sumsq)], form)"""
    _, S, ops, _ = env()
    n, m0 = len(members), members[0]
    M, K, N = m0["M"], m0["K"], m0["N"]
    buf = nan_slots(n, M, N + 8)
    keep, blocks = [], []
    for g, m in enumerate(members):
        os_, oq = zeros64(N), zeros64(N)
        part = torch.full((ksplit * m["M"] * N,), NAN, device=DEV) if ksplit else None
        cnt = torch.zeros(256, dtype=torch.int32, device=DEV) if ksplit else None
        if pooled is not None:
            x, bn, pool, dims = pooled[g], S["BnSrc"](), 0, (0, 0, 0)
        else:
            x, bn = m["slab"], bnsrc(m, "", m["slab"].shape[0], train)
            pool, dims = (1, m["pool"][1]) if m["pool"] else (0, (0, 0, 0))
        blocks.append(S["Conv1FwdP"](x.data_ptr(), x.stride(0), m["M"], m["K"], m["w"].data_ptr(), N, buf[g][:, 4:4 + N].data_ptr(), N + 8, bn,
                                     os_.data_ptr() if train else None, oq.data_ptr() if train else None, pool, ops.dims3(dims), 0, 0,
                                     ops.ptr(part), ksplit, ops.ptr(cnt)))
        keep.append((os_, oq, part, cnt, x))
    form = ops.launch_form("conv1_fwd", blocks[0], n, opts)
    rc = group_call("mms_conv1_fwd_group", S["Conv1FwdP"], blocks, opts)
    assert rc == 0, rc
    check_windows(buf, n, 4, 4 + N, "conv1 forward")
    for k in keep:
        if k[3] is not None:
            assert int(k[3].abs().sum()) == 0, "K-split ticket counters not re-armed"
    return [dict(y=buf[g][:, 4:4 + N], sum=keep[g][0], sumsq=keep[g][1]) for g in range(n)], form


def launch_pool_act(members):
    """mms_pool_act_group on transition members -> the pooled operands [Mout, K] (views of one NaN-filled allocation, pitch K + 4)"""
    _, S, ops, _ = env()
    n, m0 = len(members), members[0]
    buf = nan_slots(n, m0["M"], m0["K"] + 4)
    blocks = [S["PoolActP"](m["slab"].data_ptr(), m["slab"].stride(0), m["K"], bnsrc(m, "", m["slab"].shape[0]), ops.dims3(m["pool"][1]), m["M"],
                            buf[g].data_ptr(), m["K"] + 4) for g, m in enumerate(members)]
    rc = group_call("mms_pool_act_group", S["PoolActP"], blocks, takes_opts=False)
    assert rc == 0, rc
    check_windows(buf, n, 0, m0["K"], "pool_act")
    return [buf[g][:, :m0["K"]] for g in range(n)]


# ---- 1x1x1 convolution, backward ----------------------------------------------------------------------------------------------------------
def c1b_member(case, g, M, K, N=128, pool_dims=None):
    """A dense layer's conv1 with norm1 before and norm2 behind it (has_bn_out = 1), or a transition's (pool_dims = (B, dims), no norm behind):
    inputs and every gradient the two backward kernels produce, from autograd."""
    def make():
        r = gen("c1b", case, g)
        if pool_dims:
            B, dims = pool_dims
            x = (torch.randn(B, K, *dims, generator=r) + 0.3).requires_grad_(True)
        else:
            x = _rows5(torch.randn(M, K, generator=r) * 1.3 + 0.2).requires_grad_(True)
        g1, b1 = (torch.rand(K, generator=r) + 0.5).requires_grad_(True), (torch.randn(K, generator=r) * 0.3).requires_grad_(True)
        w = (torch.randn(N, K, generator=r) / K ** 0.5).requires_grad_(True)
        h = F.batch_norm(x, None, None, g1, b1, training=True, eps=1e-5)
        h.retain_grad()
        a = F.relu(h)
        y = F.conv3d(a, w.view(N, K, 1, 1, 1))
        y.retain_grad()
        m = dict(M=M, K=K, N=N, pool=pool_dims)
        if pool_dims:
            out = F.avg_pool3d(y, 2, 2)
            G = torch.randn(out.shape, generator=r)
            (out * G).sum().backward()
        else:
            g2, b2 = (torch.rand(N, generator=r) + 0.5).requires_grad_(True), (torch.randn(N, generator=r) * 0.3).requires_grad_(True)
            out = F.batch_norm(y, None, None, g2, b2, training=True, eps=1e-5)
            G = torch.randn(out.shape, generator=r)
            (out * G).sum().backward()
            yd, Gd = dev(cl(y)), dev(cl(G))
            s, q = colsums(yd)
            mean, var = s / M, q / M - (s / M) ** 2
            yhat = (yd.double() - mean) / torch.sqrt(var + 1e-5)
            m.update(y=yd, o_gamma=dev(g2), o_beta=dev(b2), o_sum=s, o_sumsq=q, bb1=Gd.double().sum(0).contiguous(),
                     bb2=(Gd.double() * yhat).sum(0).contiguous(), ref_dg2=g2.grad, ref_db2=b2.grad)
        xm = cl(x)
        slab = torch.randn(xm.shape[0], K + 4, generator=r)
        slab[:, :K] = xm.detach()
        slab = dev(slab)
        s, q = colsums(slab[:, :K])
        dbn = cl(h.grad)
        xhat = (xm.detach().double() - xm.detach().double().mean(0)) / torch.sqrt(xm.detach().double().var(0, unbiased=False) + 1e-5)
        m.update(slab=slab, gamma=dev(g1), beta=dev(b1), sum=s, sumsq=q, w=dev(w), dy=dev(cl(G)), ref_dbn=dbn, ref_s1=dbn.double().sum(0),
                 ref_s2=(dbn.double() * xhat).sum(0), ref_dx=cl(x.grad), ref_dg1=g1.grad, ref_db1=b1.grad, ref_dw=w.grad,
                 cpu_dy=cl(G) if pool_dims else cl(y.grad),          # the gradient at the convolution's (pooled) output
                 cpu_a=cl(F.avg_pool3d(a, 2, 2) if pool_dims else a).detach(),
                 base=dev(torch.randn(M, K, generator=r)))
        return m
    return cached(("c1b", case, g, M, K, N, pool_dims), make)


def _c1b_block(m, S, ops):
    p = S["Conv1BwdP"]()
    p.dyraw, p.lddy = m["dy"].data_ptr(), m["dy"].stride(0)
    rows = m["slab"].shape[0]
    if m["pool"]:
        p.has_bn_out, p.bn_out, p.pool = 0, bnsrc(m, "", rows), 1
        setattr(p, "in", ops.dims3(m["pool"][1]))
    else:
        p.y, p.ldy, p.has_bn_out = m["y"].data_ptr(), m["y"].stride(0), 1
        p.bn_out, p.bb_out = bnsrc(m, "o_", m["M"]), ops.bnbwd(m["bb1"], m["bb2"])
    p.M, p.N = m["M"], m["N"]
    p.x, p.ldx, p.K, p.bn_in = m["slab"].data_ptr(), m["slab"].stride(0), m["K"], bnsrc(m, "", rows)
    p.w, p.msplit = m["w"].data_ptr(), 1
    return p


def launch_c1b_data(members, opts=None, fuse=False, accumulate=False):
    """mms_conv1_bwd_data_group.  fuse: norm1's backward in the launch (Conv1BwdP.fuse_dx): dx is assigned, or added to the member's `base`.
    -> ([dict(dbn, s1, s2) or dict(dx, dgamma, dbeta)], form)"""
    _, S, ops, _ = env()
    n, m0 = len(members), members[0]
    K, rows = m0["K"], m0["slab"].shape[0]
    buf = nan_slots(n, rows, K + 8)
    keep, blocks = [], []
    for g, m in enumerate(members):
        p = _c1b_block(m, S, ops)
        s1, s2 = zeros64(K), zeros64(K)
        p.s1, p.s2 = s1.data_ptr(), s2.data_ptr()
        dg, db = torch.zeros(K, device=DEV), torch.zeros(K, device=DEV)
        if fuse:
            scratch = torch.full((rows, K), NAN, device=DEV)
            p.dbn, p.lddbn = scratch.data_ptr(), K
            if accumulate:
                buf[g][:, 4:4 + K] = m["base"]
            p.fuse_dx, p.fuse_lddx, p.fuse_accumulate = buf[g][:, 4:4 + K].data_ptr(), K + 8, 1 if accumulate else 0
            p.fuse_dgamma, p.fuse_dbeta = dg.data_ptr(), db.data_ptr()
            keep.append((s1, s2, dg, db, scratch))
        else:
            p.dbn, p.lddbn = buf[g][:, 4:4 + K].data_ptr(), K + 8
            keep.append((s1, s2, dg, db))
        blocks.append(p)
    form = ops.launch_form("conv1_bwd_data", blocks[0], n, opts)
    rc = group_call("mms_conv1_bwd_data_group", S["Conv1BwdP"], blocks, opts)
    assert rc == 0, rc
    check_windows(buf, n, 4, 4 + K, "conv1 backward-data")
    if fuse:
        for k in keep:       # the fused forms leave the dbn scratch and the statistic accumulators alone
            assert bool(torch.isnan(k[4]).all()) and float(k[0].abs().sum()) == 0.0 and float(k[1].abs().sum()) == 0.0
        return [dict(dx=buf[g][:, 4:4 + K], dgamma=keep[g][2], dbeta=keep[g][3]) for g in range(n)], form
    return [dict(dbn=buf[g][:, 4:4 + K], s1=keep[g][0], s2=keep[g][1]) for g in range(n)], form


def launch_c1b_weight(members, msplit):
    """mms_conv1_bwd_weight_group; members may differ in K.  The gradients of all members are zeroed windows of one NaN-filled allocation.
    -> [dict(dw [N, K], dgamma, dbeta)]"""
    _, S, ops, _ = env()
    n, N = len(members), members[0]["N"]
    kmax = max(m["K"] for m in members)
    buf = torch.full((n + 1, N * kmax), NAN, device=DEV)
    keep, blocks = [], []
    for g, m in enumerate(members):
        buf[g][:N * m["K"]] = 0.0
        p = _c1b_block(m, S, ops)
        dg, db = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
        p.dw, p.msplit = buf[g].data_ptr(), msplit
        if not m["pool"]:
            p.dgamma_out, p.dbeta_out = dg.data_ptr(), db.data_ptr()
        keep.append((dg, db))
        blocks.append(p)
    rc = group_call("mms_conv1_bwd_weight_group", S["Conv1BwdP"], blocks, takes_opts=False)
    assert rc == 0, rc
    for g, m in enumerate(members):
        assert not bool(torch.isnan(buf[g][:N * m["K"]]).any()) and bool(torch.isnan(buf[g][N * m["K"]:]).all()), "conv1 dW: member %d" % g
    assert bool(torch.isnan(buf[n]).all())
    return [dict(dw=buf[g][:N * m["K"]].view(N, m["K"]), dgamma=keep[g][0], dbeta=keep[g][1]) for g, m in enumerate(members)]


def c1b_terms(m, msplit):
    """the fp32 partial weight gradients of the row chunks, on the CPU: the terms the kernel's atomics add up"""
    return torch.stack([m["cpu_dy"][a:b].t() @ m["cpu_a"][a:b] for a, b in chunks(m["M"], msplit)])


# ---- 3x3x3 convolution --------------------------------------------------------------------------------------------------------------------
def c3_member(case, g, B, dims):
    def make():
        r = gen("c3", case, g)
        y1 = (torch.randn(B, 128, *dims, generator=r) + 0.1).requires_grad_(True)
        gamma, beta, rm, rv = _bn_params(r, 128)
        w = (torch.randn(32, 128, 3, 3, 3, generator=r) / (128 * 27) ** 0.5).requires_grad_(True)
        G = torch.randn(B, 32, *dims, generator=r)
        h = F.batch_norm(y1, None, None, gamma, beta, training=True, eps=1e-5)
        h.retain_grad()
        a = F.relu(h)
        z = F.conv3d(a, w, padding=1)
        (z * G).sum().backward()
        with torch.no_grad():
            z0 = F.conv3d(F.relu(F.batch_norm(y1, rm.clone(), rv.clone(), gamma, beta, training=False, eps=1e-5)), w, padding=1)
        _, _, ops, _ = env()
        y1d = dev(cl(y1))
        s, q = colsums(y1d)
        xhat = (y1d.double() - s / y1d.shape[0]) / torch.sqrt(q / y1d.shape[0] - (s / y1d.shape[0]) ** 2 + 1e-5)
        dbn = cl(h.grad)
        wd = dev(w)
        wpf, wpb = ops.pack_conv3(wd)
        wff, wfb = ops.pack_conv3_frag(wd)
        dz = torch.randn(y1d.shape[0], 40, generator=r)
        dz[:, 4:36] = cl(G)
        dz = dev(dz)
        torch.cuda.synchronize()
        return dict(B=B, dims=dims, M=y1d.shape[0], y1=y1d, sum=s, sumsq=q, gamma=dev(gamma), beta=dev(beta), rm=dev(rm), rv=dev(rv),
                    wpf=wpf, wpb=wpb, wff=wff, wfb=wfb, dz=dz, coords=ops.init_coords(B, dims, DEV),
                    ref={1: cl(z.detach()), 0: cl(z0)}, ref_dbn=dbn, ref_s1=dbn.double().sum(0), ref_s2=(dbn.double() * xhat.cpu()).sum(0),
                    ref_dw=w.grad.view(32, 128, 27), cpu_a=a.detach(), cpu_G=G)
    return cached(("c3", case, g, B, dims), make)


def launch_c3f(members, opts=None, train=True, split=0, frag=False):
    """mms_conv3_fwd_group -> ([dict(out [M, 32], sum, sumsq)], form)"""
    _, S, ops, _ = env()
    n, M = len(members), members[0]["M"]
    buf = nan_slots(n, M, 64)
    keep, blocks = [], []
    for g, m in enumerate(members):
        os_, oq = zeros64(32), zeros64(32)
        part = torch.full((split * M * 32,), NAN, device=DEV) if split else None
        p = S["Conv3FwdP"](m["y1"].data_ptr(), m["coords"].data_ptr(), ops.dims3(m["dims"]), m["M"], (m["wff"] if frag else m["wpf"]).data_ptr(),
                           buf[g][:, 16:48].data_ptr(), 64, bnsrc(m, "", m["M"], train), os_.data_ptr() if train else None,
                           oq.data_ptr() if train else None, ops.ptr(part), split or 27)
        p.wfrag = 1 if frag else 0
        keep.append((os_, oq, part))
        blocks.append(p)
    form = ops.launch_form("conv3_fwd", blocks[0], n, opts)
    rc = group_call("mms_conv3_fwd_group", S["Conv3FwdP"], blocks, opts)
    assert rc == 0, rc
    check_windows(buf, n, 16, 48, "conv2 forward")
    return [dict(out=buf[g][:, 16:48], sum=keep[g][0], sumsq=keep[g][1]) for g in range(n)], form


def launch_c3bd(members, opts=None, split=0, frag=False):
    """mms_conv3_bwd_data_group -> ([dict(dbn [M, 128], s1, s2)], form)"""
    _, S, ops, _ = env()
    n, M = len(members), members[0]["M"]
    buf = nan_slots(n, M, 128)
    keep, blocks = [], []
    for g, m in enumerate(members):
        s1, s2 = zeros64(128), zeros64(128)
        part = torch.full((split * M * 128,), NAN, device=DEV) if split else None
        p = S["Conv3BwdDataP"](m["dz"][:, 4:36].data_ptr(), 40, m["coords"].data_ptr(), ops.dims3(m["dims"]), m["M"], (m["wfb"] if frag else m["wpb"]).data_ptr(),
                               m["y1"].data_ptr(), bnsrc(m, "", m["M"]), buf[g].data_ptr(), s1.data_ptr(), s2.data_ptr(), ops.ptr(part), split or 27)
        p.wfrag = 1 if frag else 0
        keep.append((s1, s2, part))
        blocks.append(p)
    form = ops.launch_form("conv3_bwd_data", blocks[0], n, opts)
    rc = group_call("mms_conv3_bwd_data_group", S["Conv3BwdDataP"], blocks, opts)
    assert rc == 0, rc
    check_windows(buf, n, 0, 128, "conv2 backward-data")
    return [dict(dbn=buf[g], s1=keep[g][0], s2=keep[g][1]) for g in range(n)], form


def launch_c3bw(members, opts, msplit, layout):
    """mms_conv3_bwd_weight_group -> ([dW in the canonical order [32, 128, 27]], form)"""
    _, S, ops, _ = env()
    n = len(members)
    buf = torch.full((n + 1, 32 * 128 * 27), NAN, device=DEV)
    buf[:n] = 0.0
    blocks = [S["Conv3BwdWP"](m["y1"].data_ptr(), m["coords"].data_ptr(), ops.dims3(m["dims"]), m["M"], bnsrc(m, "", m["M"]), m["dz"][:, 4:36].data_ptr(), 40,
                              buf[g].data_ptr(), msplit, layout) for g, m in enumerate(members)]
    form = ops.launch_form("conv3_bwd_weight", blocks[0], n, opts)
    rc = group_call("mms_conv3_bwd_weight_group", S["Conv3BwdWP"], blocks, opts)
    assert rc == 0, rc
    assert not bool(torch.isnan(buf[:n]).any()) and bool(torch.isnan(buf[n]).all()), "conv2 dW"
    return [buf[g].view(32, 128, 27) if layout == 0 else buf[g].view(32, 27, 128).permute(0, 2, 1) for g in range(n)], form


def c3w_terms(m, msplit):
    """the fp32 partial weight gradients of the row chunks, on the CPU (torch's own weight-gradient routine on dz masked to a chunk)"""
    out = []
    Gm = cl(m["cpu_G"])
    for a, b in chunks(m["M"], msplit):
        keep = torch.zeros(m["M"], 1)
        keep[a:b] = 1.0
        Gc = (Gm * keep).reshape(m["B"], *m["dims"], 32).permute(0, 4, 1, 2, 3).contiguous()
        out.append(torch.nn.grad.conv3d_weight(m["cpu_a"], (32, 128, 3, 3, 3), Gc, padding=1).reshape(32, 128, 27))
    return torch.stack(out)
