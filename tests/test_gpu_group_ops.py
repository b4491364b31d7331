"""Op-level parity of the DenseNet ops launched as FOLD GROUPS (ng > 1) through their mms_*_group entries.

csrc/common.h: "Per-model work is exactly the single-model kernel's: grouping changes placement only, never results."  The op suites
(test_gpu_dn_fwd_ops.py, test_gpu_dn_bwd_ops.py) launch every kernel form with ng = 1; what exists only when ng > 1 -- the member placement
(xcd_place / xcd_place_parts in its three branches, c3s_place, blockIdx.z / zdim of the tile-GEMM core) and the kernel forms chosen from ng --
is checked here, op by op, members with DIFFERENT data, per member:
  (a) against torch on the CPU (tests/group_ops_util.py) at the op-level tolerance 1e-4: outputs, statistics, every gradient;
  (b) against the same member launched alone in the same form, wherever the options can pin the form: store-written tensors bit for bit; fp64
      statistics |difference| <= 1e-10 * sum |terms| (tests/test_gpu_dup_zero.py::_check_stats); fp32-atomic weight gradients within 4 x what
      the order of the additions does to the same terms on the CPU (group_ops_util.order_spread);
  (c) no member writes outside its window of a NaN-filled allocation shared by all members (group_ops_util.check_windows, in every launch);
  (d) the members in reversed order give the same bits, member for member, in store-written tensors.
Every case asserts the kernel form it was written for through mms_dn_launch_form; a case whose form flips with ng asserts the other form at
ng = 1.  A group whose second member differs in a field the launcher compares is refused with MMS_ERR_ARG before any launch.

Not here: the launches whose workgroups wait for each other inside the launch (mms_c3s_c1s_fwd, mms_cl_*_group, the persistent block-3 / 4
drivers): tests/test_gpu_layer_fusion.py and tests/test_gpu_densenet.py.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import group_ops_util as U
from gpu_util import DEV, assert_close, cl


def _opts(d):
    return U.env()[2].dn_opts(**d)


def _sums_same(a, b, terms, what):
    d = (a - b).abs()
    assert bool((d <= 1e-10 * terms).all()), "%s: group vs alone %.2e" % (what, float(d.max()))


def _stat_terms(v):
    v = v.double()
    return v.abs().sum(0), (v * v).sum(0)


# ---- conv1 forward ------------------------------------------------------------------------------------------------------------------------
# (id, M, K, ng, options, ksplit, form, form of ONE member under the same options, options that pin the group's form for one member or None)
# tile counts of the tile-GEMM cases (gridDim.x of xcd_place): flip 32 (ng = 2), tile64 32 (ng = 4), tile32-ng8 / -ng10 8, ragged 4 (100 rows);
# the whole-K kernel takes its member from blockIdx.z as it stands.
C1F = [("wholek8", 128, 224, 5, {}, 0, "wholek8", "wholek8", {}),
       ("wholek16", 128, 992, 5, {}, 0, "wholek16", "wholek16", {}),
       ("flip", 1024, 256, 2, {}, 0, "tile32", "wholek8", {"conv1_small": -1}),             # 512 tiles alone, 1024 > 640 as a pair
       ("tile64", 2048, 64, 4, {}, 0, "tile64", "tile32", None),                            # M N ng = 2^20; one member: 2^18
       ("tile32-ng10", 256, 96, 10, {"conv1_small": -1}, 0, "tile32", "tile32", {"conv1_small": -1}),
       ("tile32-ng8", 256, 96, 8, {"conv1_small": -1}, 0, "tile32", "tile32", {"conv1_small": -1}),         # one XCD per member
       ("ragged", 100, 288, 3, {"conv1_small": -1}, 0, "tile32", "tile32", {"conv1_small": -1}),
       ("ksplit8", 16, 992, 3, {"conv1_small": -1}, 8, "ksplit", "ksplit", {"conv1_small": -1}),
       ("ksplit5", 128, 640, 3, {"conv1_small": -1}, 5, "ksplit", "ksplit", {"conv1_small": -1}),
       # ng and the split with a common factor: a member index taken modulo ng instead of by division is a permutation when they are coprime
       ("ksplit8-ng4", 16, 992, 4, {"conv1_small": -1}, 8, "ksplit", "ksplit", {"conv1_small": -1}),
       ("ksplit5-ng5", 128, 640, 5, {"conv1_small": -1}, 5, "ksplit", "ksplit", {"conv1_small": -1})]


def _check_c1f(mem, res, train, what):
    for g, (m, r) in enumerate(zip(mem, res)):
        ref = m["ref"][1 if train else 0]
        assert_close(r["y"], ref, 1e-4, "%s member %d y" % (what, g))
        if train:
            assert_close(r["sum"], ref.double().sum(0), 1e-4, "%s member %d sum" % (what, g))
            assert_close(r["sumsq"], (ref.double() ** 2).sum(0), 1e-4, "%s member %d sumsq" % (what, g))


def _same_c1f(a, b, what):
    assert torch.equal(a["y"], b["y"]), what
    t1, t2 = _stat_terms(b["y"])
    _sums_same(a["sum"], b["sum"], t1, what + " sum")
    _sums_same(a["sumsq"], b["sumsq"], t2, what + " sumsq")


@pytest.mark.parametrize("name,M,K,ng,o,ksplit,form,form1,pin", C1F, ids=[c[0] for c in C1F])
def test_conv1_fwd(name, M, K, ng, o, ksplit, form, form1, pin):
    mem = [U.c1f_member(name, g, M, K) for g in range(ng)]
    res, f = U.launch_c1f(mem, _opts(o), True, ksplit)
    assert f == form, f
    _check_c1f(mem, res, True, name)
    ev, f = U.launch_c1f(mem, _opts(o), False, ksplit)
    assert f == form, f
    _check_c1f(mem, ev, False, name + " eval")
    one, f = U.launch_c1f(mem[:1], _opts(o), True, ksplit)
    assert f == form1, f                                        # (the flip cases: another form for one member)
    _check_c1f(mem[:1], one, True, name + " alone")
    if pin is not None:
        for g in range(ng):
            one, f = U.launch_c1f([mem[g]], _opts(pin), True, ksplit)
            assert f == form, f
            _same_c1f(res[g], one[0], "%s member %d" % (name, g))
    rev, _ = U.launch_c1f(mem[::-1], _opts(o), True, ksplit)
    for g in range(ng):
        assert torch.equal(res[g]["y"], rev[ng - 1 - g]["y"]), (name, g)


def _transition(ng):
    return [U.c1f_member("transition", g, 128, 64, 32, (4, (8, 8, 4))) for g in range(ng)]


def test_conv1_fwd_pooled():
    """pool = 1: AvgPool3d of relu(norm(x)) while loading, 128 pooled rows = 4 row tiles, ng = 2"""
    mem = _transition(2)
    res, f = U.launch_c1f(mem)
    assert f == "tile32", f
    _check_c1f(mem, res, True, "pooled")
    for g in range(2):
        one, f = U.launch_c1f([mem[g]])
        assert f == "tile32"
        _same_c1f(res[g], one[0], "pooled member %d" % g)
    rev, _ = U.launch_c1f(mem[::-1])
    assert torch.equal(res[0]["y"], rev[1]["y"]) and torch.equal(res[1]["y"], rev[0]["y"])


def test_transition_default_form():
    """What the driver runs: mms_pool_act_group, then the plain convolution over the pooled rows with the identity BatchNorm block
    (ng = 10 = MMS_MAX_GROUP: 8 x 2 tiles x 10 members stay on the whole-K kernel)."""
    ng = 10
    mem = _transition(ng)
    pooled = U.launch_pool_act(mem)
    for g, m in enumerate(mem):
        assert_close(pooled[g], m["act"][1], 1e-4, "pooled operand, member %d" % g)
        assert torch.equal(pooled[g], U.launch_pool_act([m])[0]), g
    rev = U.launch_pool_act(mem[::-1])
    assert all(torch.equal(pooled[g], rev[ng - 1 - g]) for g in range(ng))
    res, f = U.launch_c1f(mem, pooled=pooled)
    assert f == "wholek8", f
    _check_c1f(mem, res, True, "transition (pre-pass)")
    for g in range(ng):
        one, f = U.launch_c1f([mem[g]], pooled=[pooled[g]])
        assert f == "wholek8"
        _same_c1f(res[g], one[0], "transition (pre-pass) member %d" % g)


# ---- conv1 backward-data ------------------------------------------------------------------------------------------------------------------
# row tiles (gridDim.x): 8 (ng = 2: a model per XCD set), 8 (ng = 10), 4 with a ragged last one (ng = 3), 32 of 64 rows (ng = 4)
C1B = [("tile32-ng2", 256, 96, 2, "tile32", "tile32"), ("tile32-ng10", 256, 64, 10, "tile32", "tile32"), ("ragged", 100, 352, 3, "tile32", "tile32"),
       ("tile64", 2048, 128, 4, "tile64", "tile32")]       # M K ng = 2^20; one member: 2^18


def _check_c1b(mem, res, what):
    for g, (m, r) in enumerate(zip(mem, res)):
        assert_close(r["dbn"], m["ref_dbn"], 1e-4, "%s member %d dbn" % (what, g))
        assert_close(r["s1"], m["ref_s1"], 1e-4, "%s member %d s1" % (what, g))
        assert_close(r["s2"], m["ref_s2"], 1e-4, "%s member %d s2" % (what, g))


def _same_c1b(a, b, m, what):
    assert torch.equal(a["dbn"], b["dbn"]), what
    d = b["dbn"].double()
    xh = (m["slab"][:, :m["K"]].double() - m["sum"] / d.shape[0]) / torch.sqrt(m["sumsq"] / d.shape[0] - (m["sum"] / d.shape[0]) ** 2 + 1e-5)
    _sums_same(a["s1"], b["s1"], d.abs().sum(0), what + " s1")
    _sums_same(a["s2"], b["s2"], (d * xh).abs().sum(0), what + " s2")


@pytest.mark.parametrize("name,M,K,ng,form,form1", C1B, ids=[c[0] for c in C1B])
def test_conv1_bwd_data(name, M, K, ng, form, form1):
    mem = [U.c1b_member(name, g, M, K) for g in range(ng)]
    res, f = U.launch_c1b_data(mem)
    assert f == form, f
    _check_c1b(mem, res, name)
    for g in range(ng):
        one, f = U.launch_c1b_data([mem[g]])
        assert f == form1, f
        if form1 == form:                      # no option gives one member the 64x64 tiles of the group: (a) only there
            _same_c1b(res[g], one[0], mem[g], "%s member %d" % (name, g))
        elif g == 0:
            _check_c1b(mem[:1], one, name + " alone")
    rev, _ = U.launch_c1b_data(mem[::-1])
    for g in range(ng):
        assert torch.equal(res[g]["dbn"], rev[ng - 1 - g]["dbn"]), (name, g)


def test_conv1_bwd_data_pooled():
    """a transition's backward-data (pool = 1, no norm behind the convolution): 64 pooled rows -> 512 rows of dbn, ng = 2"""
    mem = [U.c1b_member("transition", g, 64, 64, 32, (2, (8, 8, 4))) for g in range(2)]
    res, f = U.launch_c1b_data(mem)
    assert f == "tile32", f
    _check_c1b(mem, res, "pooled")
    for g in range(2):
        _same_c1b(res[g], U.launch_c1b_data([mem[g]])[0][0], mem[g], "pooled member %d" % g)


@pytest.mark.parametrize("small_bwd,form", [(0, "fused_wholem"), (-1, "fused_tile")])
@pytest.mark.parametrize("M,C", [(M, C) for M in (16, 100, 128) for C in (352, 992)])
def test_conv1_bwd_data_fused_norm1(M, C, small_bwd, form):
    """norm1's backward inside the launch, ng = 5: the whole-M kernel (conv1s_bwd_kernel) and the tile-GEMM epilogue; dx assigned and added"""
    ng = 5
    mem = [U.c1b_member("fused", g, M, C) for g in range(ng)]
    o = {"conv1_small_bwd": small_bwd}
    for acc in (False, True):
        res, f = U.launch_c1b_data(mem, _opts(o), fuse=True, accumulate=acc)
        assert f == form, f
        for g, (m, r) in enumerate(zip(mem, res)):
            what = "fused %s M %d C %d member %d" % (form, M, C, g)
            assert_close(r["dx"] - m["base"] if acc else r["dx"], m["ref_dx"], 1e-4, what + " dx")
            assert_close(r["dgamma"], m["ref_dg1"], 1e-4, what + " dgamma1")
            assert_close(r["dbeta"], m["ref_db1"], 1e-4, what + " dbeta1")
            one, f = U.launch_c1b_data([m], _opts(o), fuse=True, accumulate=acc)
            assert f == form
            assert torch.equal(r["dx"], one[0]["dx"]) and torch.equal(r["dgamma"], one[0]["dgamma"]) and torch.equal(r["dbeta"], one[0]["dbeta"]), what
    rev, _ = U.launch_c1b_data(mem[::-1], _opts(o), fuse=True, accumulate=True)
    for g in range(ng):
        assert torch.equal(res[g]["dx"], rev[ng - 1 - g]["dx"]), g


# ---- conv1 weight gradient ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,M,Ks,msplit", [("layers", 256, (64, 96, 128, 160), 4), ("ragged", 100, (352,) * 4, 2), ("ng5", 100, (352,) * 5, 2)],
                         ids=["layers-ng4-ms4", "ragged-ng4-ms2", "ragged-ng5-ms2"])
def test_conv1_bwd_weight(name, M, Ks, msplit):
    """row chunks over blockIdx.z (member = blockIdx.z / msplit); members of one launch may differ in K (the layers of a dense block).
    Two cases have ng and msplit with a common factor (see the K-split cases of the forward)."""
    ng = len(Ks)
    mem = [U.c1b_member(name, g, M, K) for g, K in enumerate(Ks)]
    res = U.launch_c1b_weight(mem, msplit)
    rev = U.launch_c1b_weight(mem[::-1], msplit)
    for g, (m, r) in enumerate(zip(mem, res)):
        what = "conv1 dW %s member %d" % (name, g)
        assert_close(r["dw"], m["ref_dw"], 1e-4, what)
        assert_close(r["dgamma"], m["ref_dg2"], 1e-4, what + " dgamma2")
        assert_close(r["dbeta"], m["ref_db2"], 1e-4, what + " dbeta2")
        one = U.launch_c1b_weight([m], msplit)[0]
        assert torch.equal(r["dgamma"], one["dgamma"]) and torch.equal(r["dbeta"], one["dbeta"]), what
        assert torch.equal(r["dgamma"], rev[ng - 1 - g]["dgamma"]) and torch.equal(r["dbeta"], rev[ng - 1 - g]["dbeta"]), what
        # fp32 atomics of msplit chunk partials per element.  Measured (the largest of eight pairs of random orders of the same terms on the CPU):
        # 7.6e-6 to 1.5e-5 (layers: four terms per element, |dW| up to 138, i.e. one or two ulps there); exactly 0 (ragged: two terms, addition commutes).
        # Margin 4 x, because the atomic order differs from run to run
        spread = U.order_spread(U.c1b_terms(m, msplit))
        d = float((r["dw"] - one["dw"]).abs().max())
        print("%s: group vs alone %.2e, order spread of the terms %.2e" % (what, d, spread))
        assert d <= 4 * spread, (what, d, spread)


# ---- conv2 forward / backward-data --------------------------------------------------------------------------------------------------------
# (id, B, grid, ng, options, tap split, fragment-ordered weights, forward form, backward-data form, options that pin the form for ONE member)
# row tiles: 8x8x4 B 4 = 64 tiles of 16 (JN: 64 ng > 128), 32 of 32; 4x4x2 B 4 = 8 / 4; 5x3x2 B 3 = 90 rows, ragged; 7x7x8 B 3 = 1176 rows
# (37 tiles of 32, 19 of 64: ragged); 8x16x16 B 2 = 4096 rows (128 / 64 tiles)
_G = {"conv3_small": -1, "conv3_mt": -1}
C3 = [("jn1-ng2", 4, (8, 8, 4), 2, {}, 0, False, "small1", "small1", {"conv3_small": 1}),
      ("jn2-ng3", 4, (8, 8, 4), 3, {}, 0, False, "small2", "small2", {"conv3_small": 2}),
      ("jn2-ng3-frag", 4, (8, 8, 4), 3, {}, 0, True, "small2", "small2", {"conv3_small": 2}),
      ("jn1-ng5", 4, (4, 4, 2), 5, {}, 0, False, "small1", "small1", {"conv3_small": 1}),
      ("jn1-ng10-frag", 4, (4, 4, 2), 10, {}, 0, True, "small1", "small1", {"conv3_small": 1}),
      ("jn1-ragged-ng4", 3, (5, 3, 2), 4, {}, 0, False, "small1", "small1", {"conv3_small": 1}),
      ("jn2-ragged-ng4-frag", 3, (5, 3, 2), 4, {"conv3_small": 2}, 0, True, "small2", "small2", {"conv3_small": 2}),
      ("tapsplit-ng3", 4, (4, 4, 2), 3, {}, 3, False, "tapsplit", "tapsplit", {}),
      ("tapsplit-ragged-ng2", 3, (5, 3, 2), 2, {}, 27, False, "tapsplit", "tapsplit", {}),
      ("mt32-ragged-ng3", 3, (7, 7, 8), 3, {"conv3_mt": 3}, 0, False, "mt32", "mt32", {"conv3_mt": 3}),
      ("mt32-ragged-ng4", 3, (7, 7, 8), 4, {"conv3_mt": 3}, 0, False, "mt32", "mt32", {"conv3_mt": 3}),
      ("mt32-ng3", 2, (8, 16, 16), 3, {"conv3_mt": 3}, 0, False, "mt32", "mt32", {"conv3_mt": 3}),
      ("mt32-ng4", 2, (8, 16, 16), 4, {"conv3_mt": 3}, 0, False, "mt32", "mt32", {"conv3_mt": 3}),
      ("mt32-ng8", 2, (8, 16, 16), 8, {"conv3_mt": 3}, 0, False, "mt32", "mt32", {"conv3_mt": 3}),
      ("mt64-ng3", 2, (8, 16, 16), 3, {"conv3_mt": 2}, 0, False, "mt64", None, {"conv3_mt": 2}),
      ("mt64-ng4", 2, (8, 16, 16), 4, {"conv3_mt": 2}, 0, False, "mt64", None, {"conv3_mt": 2}),          # 64 tiles: a model per two XCDs
      ("mt64-ragged-ng4", 3, (7, 7, 8), 4, {"conv3_mt": 2}, 0, False, "mt64", None, {"conv3_mt": 2}),
      ("tapgemm-ng2", 4, (8, 8, 4), 2, _G, 0, False, "tapgemm", "tapgemm", _G),
      ("tapgemm-ng5", 4, (8, 8, 4), 5, _G, 0, False, "tapgemm", "tapgemm", _G),
      ("tapgemm-ng8", 4, (8, 8, 4), 8, _G, 0, False, "tapgemm", "tapgemm", _G),
      ("tapgemm-ragged-ng3", 3, (5, 3, 2), 3, _G, 0, False, "tapgemm", "tapgemm", _G)]


def _c3_members(B, dims, ng):
    return [U.c3_member("c3", g, B, dims) for g in range(ng)]       # (keyed by shape and member: shared by the cases of a shape)


@pytest.mark.parametrize("name,B,dims,ng,o,split,frag,form,formb,pin", C3, ids=[c[0] for c in C3])
def test_conv3_fwd(name, B, dims, ng, o, split, frag, form, formb, pin):
    mem = _c3_members(B, dims, ng)
    res, f = U.launch_c3f(mem, _opts(o), True, split, frag)
    assert f == form, f
    if name.startswith("jn2-ng3"):                                   # the form flips with ng: one member alone takes JN = 1
        assert U.launch_c3f(mem[:1], _opts(o), True, split, frag)[1] == "small1"
    ev, f = U.launch_c3f(mem, _opts(o), False, split, frag)
    assert f == form, f
    rev, _ = U.launch_c3f(mem[::-1], _opts(o), True, split, frag)
    for g, m in enumerate(mem):
        what = "conv2 forward %s member %d" % (name, g)
        assert_close(res[g]["out"], m["ref"][1], 1e-4, what)
        assert_close(res[g]["sum"], m["ref"][1].double().sum(0), 1e-4, what + " sum")
        assert_close(res[g]["sumsq"], (m["ref"][1].double() ** 2).sum(0), 1e-4, what + " sumsq")
        assert_close(ev[g]["out"], m["ref"][0], 1e-4, what + " eval")
        one, f = U.launch_c3f([m], _opts(pin), True, split, frag)
        assert f == form, f
        assert torch.equal(res[g]["out"], one[0]["out"]), what
        t1, t2 = _stat_terms(one[0]["out"])
        _sums_same(res[g]["sum"], one[0]["sum"], t1, what + " sum")
        _sums_same(res[g]["sumsq"], one[0]["sumsq"], t2, what + " sumsq")
        assert torch.equal(res[g]["out"], rev[ng - 1 - g]["out"]), what + " reversed"


@pytest.mark.parametrize("name,B,dims,ng,o,split,frag,form,formb,pin", [c for c in C3 if c[8]], ids=[c[0] for c in C3 if c[8]])
def test_conv3_bwd_data(name, B, dims, ng, o, split, frag, form, formb, pin):
    mem = _c3_members(B, dims, ng)
    res, f = U.launch_c3bd(mem, _opts(o), split, frag)
    assert f == formb, f
    if name.startswith("jn2-ng3"):
        assert U.launch_c3bd(mem[:1], _opts(o), split, frag)[1] == "small1"
    rev, _ = U.launch_c3bd(mem[::-1], _opts(o), split, frag)
    for g, m in enumerate(mem):
        what = "conv2 backward-data %s member %d" % (name, g)
        assert_close(res[g]["dbn"], m["ref_dbn"], 1e-4, what)
        assert_close(res[g]["s1"], m["ref_s1"], 1e-4, what + " s1")
        assert_close(res[g]["s2"], m["ref_s2"], 1e-4, what + " s2")
        one, f = U.launch_c3bd([m], _opts(pin), split, frag)
        assert f == formb, f
        assert torch.equal(res[g]["dbn"], one[0]["dbn"]), what
        d = one[0]["dbn"].double()
        xh = (m["y1"].double() - m["sum"] / m["M"]) / torch.sqrt(m["sumsq"] / m["M"] - (m["sum"] / m["M"]) ** 2 + 1e-5)
        _sums_same(res[g]["s1"], one[0]["s1"], d.abs().sum(0), what + " s1")
        _sums_same(res[g]["s2"], one[0]["s2"], (d * xh).abs().sum(0), what + " s2")
        assert torch.equal(res[g]["dbn"], rev[ng - 1 - g]["dbn"]), what + " reversed"


# ---- conv2 weight gradient ----------------------------------------------------------------------------------------------------------------
# (id, B, grid, ng, options, msplit or None = the driver's rule mms_conv3_bwd_weight_msplit(M, ng, options), dw_layout, form)
C3W = [("default-ng2", 4, (8, 8, 4), 2, {}, None, 0, "tapgemm"),
       ("default-ng5", 4, (8, 8, 4), 5, {}, None, 2, "tapgemm"),
       ("mt-ng2", 4, (8, 8, 4), 2, {"conv3w_mt": 2}, None, 2, "mt"),
       ("mt-ng5", 4, (8, 8, 4), 5, {"conv3w_mt": 2}, None, 0, "mt"),
       ("tapgemm-ng5", 4, (8, 8, 4), 5, {"conv3w_mt": -1}, None, 0, "tapgemm"),
       ("mt-ng10", 4, (4, 4, 2), 10, {"conv3w_mt": 2}, 1, 0, "mt"),
       ("tapgemm-ng10", 4, (4, 4, 2), 10, {"conv3w_mt": -1}, 1, 2, "tapgemm"),
       ("mt-ragged-ng3", 3, (5, 3, 2), 3, {"conv3w_mt": 2}, 2, 2, "mt"),
       ("tapgemm-ragged-ng3", 3, (5, 3, 2), 3, {"conv3w_mt": -1}, 2, 0, "tapgemm")]


@pytest.mark.parametrize("name,B,dims,ng,o,msplit,layout,form", C3W, ids=[c[0] for c in C3W])
def test_conv3_bwd_weight(name, B, dims, ng, o, msplit, layout, form):
    lib, _, ops, _ = U.env()
    mem = _c3_members(B, dims, ng)
    M = mem[0]["M"]
    if msplit is None:
        msplit = lib.mms_conv3_bwd_weight_msplit(M, ng, ops.opts_ref(_opts(o)))
        assert msplit == {2: 8, 5: 4}[ng], msplit                   # 1024 rows: 128-row chunks below 4 members, 256-row chunks from 4
    res, f = U.launch_c3bw(mem, _opts(o), msplit, layout)
    assert f == form, f
    for g, m in enumerate(mem):
        assert_close(res[g], m["ref_dw"], 1e-4, "conv2 dW %s member %d" % (name, g))
    for g in range(ng):
        one, f = U.launch_c3bw([mem[g]], _opts(o), msplit, layout)
        assert f == form, f
        # fp32 atomics of msplit chunk partials per element.  Measured (the largest of eight pairs of random orders of the same terms on the CPU):
        # 1.5e-5 with 8 chunks of 128 rows and with 4 chunks of 256 rows (|dW| up to 127: two ulps there), exactly 0 with one or two terms.  Margin 4 x, because the atomic order differs from run to run
        spread = U.order_spread(U.c3w_terms(mem[g], msplit))
        d = float((res[g] - one[0]).abs().max())
        print("conv2 dW %s member %d: group vs alone %.2e, order spread of the terms %.2e" % (name, g, d, spread))
        assert d <= 4 * spread, (name, g, d, spread)


# ---- the ops with one form: one case each -------------------------------------------------------------------------------------------------
def test_bn_bwd_apply():
    """norm1 backward into the gradient slab: 100 rows, 96 channels, ng = 10 (dx assigned into the members' windows)"""
    _, S, ops, _ = U.env()
    ng, M, C = 10, 100, 96

    def member(g):
        r = U.gen("bnapply", g)
        x = (torch.randn(1, C, M, 1, 1, generator=r) * 1.3 + 0.2).requires_grad_(True)
        ga, be = (torch.rand(C, generator=r) + 0.5).requires_grad_(True), (torch.randn(C, generator=r) * 0.3).requires_grad_(True)
        G = torch.randn(1, C, M, 1, 1, generator=r)
        (F.batch_norm(x, None, None, ga, be, training=True, eps=1e-5) * G).sum().backward()
        xd, Gd = U.dev(cl(x)), U.dev(cl(G))
        s, q = U.colsums(xd)
        xh = (xd.double() - s / M) / torch.sqrt(q / M - (s / M) ** 2 + 1e-5)
        return dict(x=xd, G=Gd, gamma=U.dev(ga), beta=U.dev(be), sum=s, sumsq=q, s1=Gd.double().sum(0).contiguous(), s2=(Gd.double() * xh).sum(0).contiguous(),
                    ref_dx=cl(x.grad), ref_dg=ga.grad, ref_db=be.grad)
    mem = [U.cached(("bnapply", g), lambda g=g: member(g)) for g in range(ng)]

    def launch(ms):
        buf = U.nan_slots(len(ms), M, C + 8)
        grads = [(torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)) for _ in ms]
        blocks = [S["BnBwdApplyP"](m["G"].data_ptr(), C, m["x"].data_ptr(), C, buf[g][:, 4:4 + C].data_ptr(), C + 8, M, C, U.bnsrc(m, "", M),
                                   ops.bnbwd(m["s1"], m["s2"]), 0, grads[g][0].data_ptr(), grads[g][1].data_ptr()) for g, m in enumerate(ms)]
        assert U.group_call("mms_bn_bwd_apply_group", S["BnBwdApplyP"], blocks, takes_opts=False) == 0
        U.check_windows(buf, len(ms), 4, 4 + C, "bn_bwd_apply")
        return [(buf[g][:, 4:4 + C], grads[g][0], grads[g][1]) for g in range(len(ms))]
    res, rev = launch(mem), launch(mem[::-1])
    for g, m in enumerate(mem):
        assert_close(res[g][0], m["ref_dx"], 1e-4, "dx member %d" % g)
        assert_close(res[g][1], m["ref_dg"], 1e-4, "dgamma member %d" % g)
        assert_close(res[g][2], m["ref_db"], 1e-4, "dbeta member %d" % g)
        one = launch([m])[0]
        assert all(torch.equal(a, b) for a, b in zip(res[g], one)), g
        assert all(torch.equal(a, b) for a, b in zip(res[g], rev[ng - 1 - g])), g


def test_pool_fwd_and_bwd():
    """norm0 + relu0 + MaxPool3d(3, 2, 1) and its backward (the brick kernel the driver's grids take: W % 16 == 0): conv0 grid 4x4x16 -> 2x2x8,
    B = 2, ng = 10"""
    _, S, ops, _ = U.env()
    ng, B, od, pd = 10, 2, (4, 4, 16), (2, 2, 8)
    M0, M1 = B * 4 * 4 * 16, B * 2 * 2 * 8

    def member(g):
        r = U.gen("pool", g)
        y0 = (torch.randn(B, 64, *od, generator=r) + 0.2).requires_grad_(True)
        ga, be = torch.rand(64, generator=r) + 0.5, torch.randn(64, generator=r) * 0.3
        h = F.batch_norm(y0, None, None, ga, be, training=True, eps=1e-5)
        h.retain_grad()
        p0 = F.max_pool3d(F.relu(h), 3, 2, 1)
        G = torch.randn(p0.shape, generator=r)
        (p0 * G).sum().backward()
        yd = U.dev(cl(y0))
        s, q = U.colsums(yd)
        xh = (yd.double() - s / M0) / torch.sqrt(q / M0 - (s / M0) ** 2 + 1e-5)
        dbn = cl(h.grad)
        return dict(y0=yd, gamma=U.dev(ga), beta=U.dev(be), sum=s, sumsq=q, G=U.dev(cl(G)), pad=U.dev(torch.randn(M1, 8, generator=r)), xh=xh, ref=cl(p0.detach()), ref_dbn=dbn, ref_s1=dbn.double().sum(0),
                    ref_s2=(dbn.double() * xh.cpu()).sum(0))
    mem = [U.cached(("pool", g), lambda g=g: member(g)) for g in range(ng)]

    def launch(ms):
        n = len(ms)
        slab, dbn = U.nan_slots(n, M1, 72), U.nan_slots(n, M0, 64)
        am = torch.full((n, M1, 64), 255, dtype=torch.uint8, device=DEV)
        st = [[U.zeros64(64) for _ in range(4)] for _ in ms]
        fb = [S["PoolFwdP"](m["y0"].data_ptr(), ops.dims3(od), ops.dims3(pd), B, slab[g][:, 4:68].data_ptr(), 72, am[g].data_ptr(), U.bnsrc(m, "", M0),
                            st[g][0].data_ptr(), st[g][1].data_ptr()) for g, m in enumerate(ms)]
        assert U.group_call("mms_pool_fwd_group", S["PoolFwdP"], fb, takes_opts=False) == 0
        U.check_windows(slab, n, 4, 68, "pool_fwd")
        assert int(am.max()) < 27
        dsl = [torch.cat([m["G"], m["pad"]], 1).contiguous() for m in ms]
        bb = [S["PoolBwdP"](dsl[g].data_ptr(), 72, am[g].data_ptr(), ops.dims3(pd), ops.dims3(od), B, m["y0"].data_ptr(), U.bnsrc(m, "", M0), dbn[g].data_ptr(),
                            st[g][2].data_ptr(), st[g][3].data_ptr(), None) for g, m in enumerate(ms)]
        assert U.group_call("mms_pool_bwd_group", S["PoolBwdP"], bb, takes_opts=False) == 0
        U.check_windows(dbn, n, 0, 64, "pool_bwd")
        return [(slab[g][:, 4:68], am[g], dbn[g], st[g]) for g in range(n)]
    res, rev = launch(mem), launch(mem[::-1])
    for g, m in enumerate(mem):
        out, am, dbn, st = res[g]
        assert_close(out, m["ref"], 1e-4, "pool member %d" % g)
        assert_close(st[0], m["ref"].double().sum(0), 1e-4, "pool sum"); assert_close(st[1], (m["ref"].double() ** 2).sum(0), 1e-4, "pool sumsq")
        assert_close(dbn, m["ref_dbn"], 1e-4, "pool dbn member %d" % g)
        assert_close(st[2], m["ref_s1"], 1e-4, "pool s1"); assert_close(st[3], m["ref_s2"], 1e-4, "pool s2")
        o1, a1, d1, s1 = launch([m])[0]
        assert torch.equal(out, o1) and torch.equal(am, a1) and torch.equal(dbn, d1), g
        t1, t2 = _stat_terms(o1)
        _sums_same(st[0], s1[0], t1, "pool sum"); _sums_same(st[1], s1[1], t2, "pool sumsq")
        _sums_same(st[2], s1[2], d1.double().abs().sum(0), "pool s1")
        _sums_same(st[3], s1[3], (d1.double() * m["xh"]).abs().sum(0), "pool s2")
        ro, ra, rd, _ = rev[ng - 1 - g]
        assert torch.equal(out, ro) and torch.equal(am, ra) and torch.equal(dbn, rd), g


def test_head_bwd():
    """class_layers + norm5 backward: B = 4, V = 4, C = 1024, ng = 10"""
    _, S, ops, _ = U.env()
    ng, B, V, C, N = 10, 4, 4, 1024, 128

    def member(g):
        r = U.gen("head", g)
        x = (torch.randn(B, C, V, 1, 1, generator=r) + 0.2).requires_grad_(True)
        ga, be = (torch.rand(C, generator=r) + 0.5).requires_grad_(True), (torch.randn(C, generator=r) * 0.3).requires_grad_(True)
        w, bias = (torch.randn(N, C, generator=r) / C ** 0.5).requires_grad_(True), (torch.randn(N, generator=r) * 0.1).requires_grad_(True)
        pooled = F.relu(F.batch_norm(x, None, None, ga, be, training=True, eps=1e-5)).mean(dim=(2, 3, 4))
        out = pooled @ w.t() + bias
        dout = torch.randn(out.shape, generator=r)
        out.backward(dout)
        xd = U.dev(cl(x))
        s, q = U.colsums(xd)
        return dict(x=xd, gamma=U.dev(ga), beta=U.dev(be), sum=s, sumsq=q, w=U.dev(w), pooled=U.dev(pooled), dout=U.dev(dout),
                    ref=dict(dw=w.grad, dbias=bias.grad, dgamma=ga.grad, dbeta=be.grad, dslab=cl(x.grad)))
    mem = [U.cached(("head", g), lambda g=g: member(g)) for g in range(ng)]

    def launch(ms):
        n = len(ms)
        buf = U.nan_slots(n, B * V, C + 8)
        acc = [dict(dw=torch.zeros(N, C, device=DEV), dbias=torch.zeros(N, device=DEV), dgamma=torch.zeros(C, device=DEV), dbeta=torch.zeros(C, device=DEV)) for _ in ms]
        blocks = [S["HeadBwdP"](m["dout"].data_ptr(), N, m["pooled"].data_ptr(), m["x"].data_ptr(), C, C, B, V, U.bnsrc(m, "", B * V), m["w"].data_ptr(), N,
                                acc[g]["dw"].data_ptr(), acc[g]["dbias"].data_ptr(), acc[g]["dgamma"].data_ptr(), acc[g]["dbeta"].data_ptr(),
                                buf[g][:, 4:4 + C].data_ptr(), C + 8) for g, m in enumerate(ms)]
        assert U.group_call("mms_head_bwd_group", S["HeadBwdP"], blocks, takes_opts=False) == 0
        U.check_windows(buf, n, 4, 4 + C, "head_bwd")
        return [dict(acc[g], dslab=buf[g][:, 4:4 + C]) for g in range(n)]
    res, rev = launch(mem), launch(mem[::-1])
    for g, m in enumerate(mem):
        one = launch([m])[0]
        for k, ref in m["ref"].items():
            assert_close(res[g][k], ref, 1e-4, "head %s member %d" % (k, g))
            assert torch.equal(res[g][k], one[k]), (k, g)             # no atomics in these kernels: every tensor bit for bit
            assert torch.equal(res[g][k], rev[ng - 1 - g][k]), (k, g)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
# Per entry: a valid two-member group's scalar fields, and the fields of the SECOND member whose change the launcher must refuse BEFORE its
# first launch -- each of them read off the launcher's member comparison (csrc/dn_fwd.hip, csrc/dn_bwd.hip).  Every pointer of both blocks
# points into one NaN-filled allocation that is large enough for any of these shapes; it must come back untouched.
_BN = dict(inv_count=1.0 / 64, eps=1e-5, train=1)
_D = lambda d, h, w: dict(D=d, H=h, W=w)
REFUSALS = [
    ("mms_conv1_fwd_group", "Conv1FwdP", True, dict(ldx=64, M=64, K=64, N=128, ldy=128), [dict(M=96), dict(pool=1), {"in": _D(2, 2, 2)}]),
    ("mms_pool_act_group", "PoolActP", False, {"ldx": 64, "K": 64, "in": _D(4, 4, 4), "Mout": 8, "ldy": 64}, [dict(Mout=16), {"in": _D(8, 4, 4)}]),
    ("mms_conv1_bwd_data_group", "Conv1BwdP", True, dict(lddy=128, ldy=128, has_bn_out=1, M=64, N=128, ldx=64, K=64, lddbn=64, msplit=1),
     [dict(M=96), dict(pool=1), {"in": _D(2, 2, 2)}]),
    ("mms_conv1_bwd_weight_group", "Conv1BwdP", False, dict(lddy=128, ldy=128, has_bn_out=1, M=64, N=128, ldx=64, K=64, lddbn=64, msplit=1),
     [dict(M=96), dict(pool=1), dict(msplit=2)]),
    ("mms_conv3_fwd_group", "Conv3FwdP", True, dict(g=_D(2, 8, 8), M=128, ldo=32, nsplit=27), [dict(M=256), dict(g=_D(4, 8, 8)), dict(g=_D(2, 8, 4))]),
    ("mms_conv3_bwd_data_group", "Conv3BwdDataP", True, dict(lddz=32, g=_D(2, 8, 8), M=128, nsplit=27), [dict(M=256), dict(g=_D(2, 4, 8))]),
    ("mms_conv3_bwd_weight_group", "Conv3BwdWP", True, dict(g=_D(2, 8, 8), M=128, lddz=32, msplit=1), [dict(M=256), dict(g=_D(4, 8, 8)), dict(msplit=2)]),
    ("mms_bn_bwd_apply_group", "BnBwdApplyP", False, dict(lddbn=64, ldx=64, lddx=64, M=64, C=64), [dict(M=96), dict(C=32)]),
    ("mms_pool_fwd_group", "PoolFwdP", False, {"in": _D(4, 4, 4), "out": _D(2, 2, 2), "B": 1, "ld": 64}, [dict(B=2), {"in": _D(6, 4, 4)}, dict(out=_D(2, 2, 3))]),
    ("mms_pool_bwd_group", "PoolBwdP", False, {"ld": 64, "out": _D(2, 2, 2), "in": _D(4, 4, 4), "B": 1}, [dict(B=2), {"in": _D(4, 6, 4)}, dict(out=_D(3, 2, 2))]),
    ("mms_head_bwd_group", "HeadBwdP", False, dict(lddout=8, ld=64, C=64, B=2, V=2, N=8, ldd=64), [dict(B=3), dict(V=4)]),
]


def _fill(S, st, ptr, fields):
    """every pointer of the block (nested blocks included) -> ptr; then the given scalar / Dims3 fields"""
    p = st()
    for name, ct in st._fields_:
        if ct is ctypes.c_void_p:
            setattr(p, name, ptr)
        elif ct is S["BnSrc"]:
            setattr(p, name, S["BnSrc"](ptr, ptr, ptr, ptr, ptr, ptr, _BN["inv_count"], _BN["eps"], _BN["train"]))
        elif ct is S["BnBwd"]:
            setattr(p, name, S["BnBwd"](ptr, ptr))
    for k, v in fields.items():
        setattr(p, k, S["Dims3"](v["D"], v["H"], v["W"]) if isinstance(v, dict) else v)
    return p


@pytest.mark.parametrize("entry,sname,takes_opts,base,changes", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(entry, sname, takes_opts, base, changes):
    _, S, _, _ = U.env()
    buf = torch.full((1 << 20,), U.NAN, device=DEV)
    ok = [_fill(S, S[sname], buf.data_ptr(), base) for _ in range(2)]
    for ch in changes:
        blocks = [ok[0], _fill(S, S[sname], buf.data_ptr(), dict(base, **ch))]
        assert U.group_call(entry, S[sname], blocks, takes_opts=takes_opts) == -1, (entry, ch)       # MMS_ERR_ARG
        assert bool(torch.isnan(buf).all()), (entry, ch)
