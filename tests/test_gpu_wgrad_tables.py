"""Table-fed weight-gradient launches of dense blocks 2-4 (csrc/dn_bwd.hip mms_wgrad_tab_group; MmsDnOpts.wgrad_tab = 0, the default):
every (model, layer) member of a block in one conv2 and one conv1 launch, the members' parameter blocks rebuilt on the device from
compact records, against torch on the CPU and against the launches of at most MMS_MAX_GROUP by-value members they replace
(wgrad_tab = -1)."""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from gpu_util import DEV, assert_close, cl, rel_err, uncl

C0 = 256            # input channels of layer 0 of the synthetic block: conv1 members have K = 256, 288, ... in steps of 32


def _S():
    from multimodal_survival_prediction_amd import _lib
    return _lib.structs()


def _launch(models, members, shape, which=3, nmodels=None, nmembers=None):
    from multimodal_survival_prediction_amd import _lib, ops
    S = _S()
    ma = (S["MmsWgradModel"] * max(1, len(models)))(*models)
    me = (S["MmsWgradMember"] * max(1, len(members)))(*members)
    st = ops.stream() if torch.cuda.is_available() else None
    return _lib.load_library().mms_wgrad_tab_group(ma, len(models) if nmodels is None else nmodels, me,
                                                   len(members) if nmembers is None else nmembers, ctypes.byref(shape), which, st)


def _d(t):
    return t.detach().to(DEV).contiguous()


# (members, batch, grid, conv2 row chunks, conv1 row chunks, conv2 gradient layout): the block-4 and block-3 shapes of the workload at one
# row chunk, and 512 rows at two chunks per op (the atomic-accumulate path; the chunk counts the driver picks for >= 4 members of 512 rows)
CASES = [(11, 4, (2, 2, 1), 1, 1, 2), (12, 2, (4, 4, 2), 1, 1, 1), (11, 2, (8, 8, 4), 2, 2, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("nmem,B,dims,ms3,ms1,layout", CASES)
def test_wgrad_table_launch_ops(nmem, B, dims, ms3, ms1, layout):
    """Both ops through one table-fed launch of 11 / 12 members spread over two models (6 + 5 / 6 + 6: layers 0-5 of model 0, the rest
    of model 1, so every member has its own K), each member with its own BatchNorm blocks and zero-filled gradient buffers: 1e-4 against
    torch autograd on the CPU, and bit for bit against single-member launches of the by-value entry points where every gradient element
    receives one atomic add (M <= 128)."""
    from multimodal_survival_prediction_amd import ops
    S = _S()
    torch.manual_seed(100 * nmem + B)
    M = B * dims[0] * dims[1] * dims[2]
    ld = C0 + 32 * 12
    coords = ops.init_coords(B, dims, DEV)
    keep, models, xs, dslabs, slabs, sts, tabs = [], [], [], [], [], [], []
    for m in range(2):
        x = torch.randn(B, ld, *dims) * 1.3 + 0.2
        slab = _d(cl(x))
        dslab = torch.randn(M, ld, device=DEV)
        st = torch.cat([slab.double().sum(0), (slab.double() ** 2).sum(0)]).contiguous()
        tab = torch.zeros(12, 15, dtype=torch.int64)
        xs.append(x); slabs.append(slab); dslabs.append(dslab); sts.append(st); tabs.append(tab)
    mem = []
    for j in range(nmem):
        m, l = (0, j) if j < 6 else (1, j)
        K = C0 + 32 * l
        n1, n2 = nn.BatchNorm3d(K), nn.BatchNorm3d(128)
        c1, c2 = nn.Conv3d(K, 128, 1, bias=False), nn.Conv3d(128, 32, 3, padding=1, bias=False)
        with torch.no_grad():
            for n in (n1, n2):
                n.weight.uniform_(0.5, 1.5); n.bias.normal_(0, 0.3)
        z = c2(F.relu(n2(c1(F.relu(n1(xs[m][:, :K]))))))
        z.backward(uncl(dslabs[m][:, K:K + 32].cpu(), B, dims))
        g1, b1, g2, b2 = _d(n1.weight), _d(n1.bias), _d(n2.weight), _d(n2.bias)
        w1, w2 = _d(c1.weight.view(128, K)), _d(c2.weight)
        slab, dslab, st = slabs[m], dslabs[m], sts[m]
        bn1 = ops.bnsrc(g1, b1, M, True, st[:ld], st[ld:])
        y1 = torch.empty(M, 128, device=DEV)
        sty = torch.zeros(256, dtype=torch.float64, device=DEV)
        ops.conv1_fwd(slab, K, w1, y1, bn1, M, sty[:128], sty[128:])
        bn2 = ops.bnsrc(g2, b2, M, True, sty[:128], sty[128:])
        _, wpb = ops.pack_conv3(w2)
        dmid = torch.empty(M, 128, device=DEV)
        bb = torch.zeros(256, dtype=torch.float64, device=DEV)
        ops.conv3_bwd_data(dslab[:, K:K + 32], coords, dims, wpb, y1, bn2, dmid, bb[:128], bb[128:], None, 27)
        tabs[m][l] = torch.tensor([g1.data_ptr(), b1.data_ptr(), w1.data_ptr(), g2.data_ptr(), b2.data_ptr(), 0, 0, 0, 0, 0, 0,
                                   y1.data_ptr(), sty.data_ptr(), dmid.data_ptr(), bb.data_ptr()], dtype=torch.int64)
        # the launches of at most MMS_MAX_GROUP by-value members: here one member each, the same row chunks
        r = dict(dw2=torch.zeros(27 * 32 * 128, device=DEV), dw1=torch.zeros(128, K, device=DEV), dg2=torch.zeros(128, device=DEV),
                 db2=torch.zeros(128, device=DEV))
        ops.conv3_bwd_weight(y1, coords, dims, bn2, dslab[:, K:K + 32], r["dw2"], ms3, layout=layout, opts=ops.dn_opts(conv3w_mt=-1))
        ops.conv1_bwd("weight", dmid, M, 128, slab, K, bn1, w1, r["dw1"], torch.empty(M, ld, device=DEV),
                      torch.zeros(1024, dtype=torch.float64, device=DEV), torch.zeros(1024, dtype=torch.float64, device=DEV),
                      y=y1, bn_out=bn2, bb_out=ops.bnbwd(bb[:128], bb[128:]), msplit=ms1, dgamma_out=r["dg2"], dbeta_out=r["db2"])
        t = dict(dw2=torch.zeros(27 * 32 * 128, device=DEV), dw1=torch.zeros(128, K, device=DEV), dg2=torch.zeros(128, device=DEV),
                 db2=torch.zeros(128, device=DEV))
        want = dict(dw2=c2.weight.grad, dw1=c1.weight.grad.view(128, K), dg2=n2.weight.grad, db2=n2.bias.grad)
        mem.append(dict(m=m, l=l, K=K, ref=r, tab=t, want=want))
        keep.append((g1, b1, g2, b2, w1, w2, y1, sty, dmid, bb, wpb))
    tabs = [t.to(DEV) for t in tabs]
    torch.cuda.synchronize()
    for m in range(2):
        models.append(S["MmsWgradModel"](tabs[m].data_ptr(), slabs[m].data_ptr(), dslabs[m].data_ptr(), coords.data_ptr(), sts[m].data_ptr(),
                                         M, ops.dims3(dims), 1))
    members = [S["MmsWgradMember"](e["tab"]["dw2"].data_ptr(), e["tab"]["dw1"].data_ptr(), e["tab"]["dg2"].data_ptr(),
                                   e["tab"]["db2"].data_ptr(), e["m"], e["l"]) for e in mem]
    assert _launch(models, members, S["MmsWgradShape"](ld, C0, ms3, ms1, layout, M)) == 0
    torch.cuda.synchronize()
    canon = (lambda t: t.view(32, 27, 128).permute(0, 2, 1).reshape(32, 128, 3, 3, 3)) if layout == 2 else \
            (lambda t: t.view(27, 32, 128).permute(1, 2, 0).reshape(32, 128, 3, 3, 3))
    for j, e in enumerate(mem):
        for k in ("dw2", "dw1", "dg2", "db2"):
            got, ref = e["tab"][k], e["ref"][k]
            what = "member %d (model %d, K %d) %s" % (j, e["m"], e["K"], k)
            assert_close(canon(got) if k == "dw2" else got, e["want"][k], 1e-4, what)
            if M <= 128:
                assert torch.equal(got, ref), what + ": differs from the by-value launch"
            else:
                assert_close(got, ref, 1e-4, what + " against the by-value launch")


def _block_of(name):
    for b in (1, 2, 3, 4):
        if "denseblock%d." % b in name:
            return b
    return 0


def _compare(new, old, what):
    """Parameter gradients of one run with wgrad_tab = 0 against one with -1: blocks 3 and 4 (one row chunk: one atomic add onto zero per
    element in both) bit for bit, every other tensor within 1e-4 of its maximum."""
    assert new.keys() == old.keys()
    for k, g in old.items():
        if _block_of(k) in (3, 4):
            assert torch.equal(new[k], g), "%s: %s differs (rel err %.3e)" % (what, k, rel_err(new[k], g))
    errs = {k: rel_err(new[k], g) for k, g in old.items()}
    worst = max(errs, key=errs.get)
    assert errs[worst] <= 1e-4, (what, worst, errs[worst])


@pytest.mark.gpu
def test_whole_net_equals_by_value_launches_twice():
    """One training forward + backward of DenseNet121 at 4 x (64, 64, 32) with the table-fed launches and with the by-value ones, same
    weights, input and dout; then the gradients zeroed and a second pass on the same workspace (records valid only once would show)."""
    from test_gpu_densenet import _make, structured_volumes
    ref, net = _make(7)
    x = structured_volumes(4, (64, 64, 32), 51).to(DEV)
    dout = torch.randn(4, 128, generator=torch.Generator().manual_seed(3)).to(DEV)
    res = {}
    for flag in (-1, 0):
        net.dn_opts = dict(wgrad_tab=flag)
        net.load_state_dict(ref.state_dict())
        net.train()
        res[flag] = []
        for rep in range(2):
            net.zero_grad(set_to_none=True)
            y = net(x)
            y.backward(dout)
            torch.cuda.synchronize()
            res[flag].append({k: q.grad.clone() for k, q in net.named_parameters()})
    for rep in range(2):
        _compare(res[0][rep], res[-1][rep], "pass %d" % (rep + 1))


def _fold_models(n):
    from multimodal_survival_prediction_amd import models as HM
    base = []
    for g in range(n):
        torch.manual_seed(200 + g)
        m = HM.PartialModalityNet(rna_dim=1024)
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, (torch.nn.BatchNorm3d, torch.nn.BatchNorm1d)):
                    mod.weight.uniform_(0.5, 1.5); mod.bias.normal_(0, 0.1)
                if isinstance(mod, torch.nn.Dropout):
                    mod.p = 0.0
        base.append(m)
    return base


@pytest.mark.gpu
@pytest.mark.parametrize("ng", [2, 3])
def test_fold_group_three_replayed_steps(ng):
    """Fold groups of 2 and 3 models (3: 72 / 48 / 36 members per launch) through the engine's captured-graph step, lr = 0, three steps on
    the same batches: the gradients of every step agree between the two flag values, and with the table-fed launches steps 2 and 3 agree
    with step 1 (a host pointer baked into the replayed launch would not survive)."""
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    from test_gpu_models import _batch
    base = _fold_models(ng)
    valid = torch.tensor([1, 1, 0, 1], dtype=torch.float32)
    batches = []
    for g in range(ng):
        ct, rna, clin, t, e, mask = _batch(4, (64, 64, 32), 1024, 70 + g)
        batches.append(dict(ct=ct, rna=rna, clinical=clin, mask=mask, time=t, event=e, valid=valid))
    grads = {}
    for flag in (-1, 0):
        nets = [copy.deepcopy(m).to(DEV).train() for m in base]
        ge = FoldGroupEngine(nets, lr=0.0, weight_decay=1e-4, dn_opts=dict(wgrad_tab=flag))
        grads[flag] = []
        for step in range(3):
            ge.train_step(copy.deepcopy(batches), skip_if_unusable=False)
            torch.cuda.synchronize()
            per_model = []
            for net, eng in zip(nets, ge.engines):
                names = {id(p): k for k, p in net.named_parameters()}
                per_model.append({names[id(p)]: v.clone() for p, v in zip(eng.params, eng.gviews)})
            grads[flag].append(per_model)
        ge.epoch_stats()
    for step in range(3):
        for g in range(ng):
            _compare(grads[0][step][g], grads[-1][step][g], "step %d model %d" % (step + 1, g))
    for step in (1, 2):
        for g in range(ng):
            _compare(grads[0][step][g], grads[0][0][g], "table-fed step %d against step 1, model %d" % (step + 1, g))


def test_wgrad_table_argument_checks():
    """CPU-side return codes, nothing is launched: no members, more members than the kernel argument holds, models of unequal M (and the
    other ranges of include/mmsurv.h: model count, member indices, layer range, row chunk, which)."""
    from multimodal_survival_prediction_amd import _lib
    S = _S()
    lib = _lib.load_library()
    assert lib.mms_abi_sizeof(b"MmsWgradMember") == 40 and lib.mms_abi_sizeof(b"MmsWgradModel") == 64
    cap, capm = 90, 5                    # MMS_WGRAD_MAX_MEMBERS, MMS_WGRAD_MAX_MODELS
    p = 0x10000                          # never dereferenced on the host
    model = lambda M=64: S["MmsWgradModel"](p, p, p, p, p, M, S["Dims3"](4, 4, 2), 1)
    member = lambda m=0, l=0: S["MmsWgradMember"](p, p, p, p, m, l)
    shape = lambda **kw: S["MmsWgradShape"](**dict(dict(ld=640, C0=256, ms3=1, ms1=1, dw_layout=2, count=64), **kw))
    ERR = -1
    assert _launch([model()], [], shape()) == ERR
    assert _launch([model()], [member()] * (cap + 1), shape()) == ERR
    assert _launch([model(), model(128)], [member(0), member(1)], shape()) == ERR
    assert _launch([model(), model(128)], [member(0), member(0, 1)], shape()) == ERR          # (even when no member names the odd model)
    assert _launch([], [member()], shape()) == ERR
    assert _launch([model()] * (capm + 1), [member()], shape()) == ERR
    assert _launch([model()], [member(1)], shape()) == ERR                                    # model index out of range
    assert _launch([model()], [member(0, 12)], shape()) == ERR                                # K + 32 > ld
    assert _launch([model()], [member(0, -1)], shape()) == ERR
    assert _launch([model(4096)], [member()], shape(count=4096)) == ERR                       # conv2 row chunk over 1024 rows
    assert _launch([model()], [member()], shape(ms1=0)) == ERR
    assert _launch([model()], [member()], shape(dw_layout=3)) == ERR
    assert _launch([model()], [member()], shape(), which=0) == ERR
    assert _launch([model()], [S["MmsWgradMember"](0, p, p, p, 0, 0)], shape(), which=1) == ERR
