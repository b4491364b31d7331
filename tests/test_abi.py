"""CPU: the C-ABI library loads, exports every symbol include/mmsurv.h declares, and its struct layouts
match the host's parsed view of the header (no compute calls)."""
import ctypes
import os

import pytest

from multimodal_survival_prediction_amd import _build, _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.lib_path()):
        _build.build()
    return _lib.load_library()


def test_exports_every_declared_symbol(lib):
    protos = _lib.protos()
    assert len(protos) >= 10
    for name in protos:
        assert hasattr(lib, name), name


def test_struct_layouts_match(lib):
    for name, st in _lib.structs().items():
        assert lib.mms_abi_sizeof(name.encode()) == ctypes.sizeof(st), name
    assert lib.mms_abi_sizeof(b"NoSuchStruct") == -1
    assert lib.mms_abi_version() >= 1


def test_launch_form_query(lib):
    """mms_dn_launch_form (a host function: no GPU, the blocks' pointers are never followed): the kernel form a *_group launcher takes for a
    parameter block, ng and options -- the function each launcher switches on.  The thresholds that depend on ng, on both sides."""
    from multimodal_survival_prediction_amd import ops
    assert "mms_dn_launch_form" in _lib.protos() and hasattr(lib, "mms_dn_launch_form")
    S, fake = _lib.structs(), 0x10000
    form = lambda op, p, ng, **o: ops.launch_form(op, p, ng, ops.dn_opts(**o))

    def c1f(M, K, **kw):
        p = S["Conv1FwdP"](x=fake, ldx=K, M=M, K=K, w=fake, N=128, y=fake, ldy=128)
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    # conv1 forward: whole-K kernel while tiles * ng <= 640 (template by K), 64x64 tiles from M N ng >= 2^20, K split on request
    assert [form("conv1_fwd", c1f(128, K), 5) for K in (224, 512, 544, 992)] == ["wholek8", "wholek8", "wholek16", "wholek16"]
    assert [form("conv1_fwd", c1f(1024, 256), ng) for ng in (1, 2)] == ["wholek8", "tile32"]
    assert [form("conv1_fwd", c1f(2048, 64), ng) for ng in (1, 3, 4)] == ["tile32", "tile32", "tile64"]
    assert form("conv1_fwd", c1f(2048, 64), 4, big_ng=-1) == "tile32" and form("conv1_fwd", c1f(1024, 256), 2, conv1_small=1) == "wholek8"
    ks = dict(partial=fake, counters=fake, ksplit=5)
    assert form("conv1_fwd", c1f(128, 640, **ks), 3, conv1_small=-1) == "ksplit" and form("conv1_fwd", c1f(128, 640, **ks), 3) == "wholek16"
    assert form("conv1_fwd", c1f(128, 64, pool=1), 2) == "tile32"
    assert lib.mms_dn_launch_form(1, ctypes.byref(c1f(128, 48)), 2, None) == -1 and lib.mms_dn_launch_form(99, ctypes.byref(c1f(128, 64)), 2, None) == -1
    assert lib.mms_dn_launch_form(1, ctypes.byref(c1f(128, 224, x=fake + 4)), 5, None) == -1          # the whole-K kernel wants x and w 16-byte aligned ...
    assert form("conv1_fwd", c1f(128, 224, x=fake + 4), 5, conv1_small=-1) == "tile32"                 # ... the tile GEMM does not
    assert lib.mms_dn_launch_form(1, None, 2, None) == -1 and lib.mms_dn_launch_form(1, ctypes.byref(c1f(128, 64)), 11, None) == -1

    # conv1 backward-data: the same tile rule on M K ng; the two fused-norm1 forms
    def c1b(M, K, **kw):
        p = S["Conv1BwdP"](dyraw=fake, lddy=128, y=fake, ldy=128, has_bn_out=1, M=M, N=128, x=fake, ldx=K, K=K, w=fake)
        p.bn_in.train = p.bn_out.train = 1
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    assert [form("conv1_bwd_data", c1b(2048, 128), ng) for ng in (1, 4)] == ["tile32", "tile64"]
    fu = dict(fuse_dx=fake, fuse_lddx=352)
    assert form("conv1_bwd_data", c1b(100, 352, **fu), 5) == "fused_wholem" and form("conv1_bwd_data", c1b(100, 352, **fu), 5, conv1_small_bwd=-1) == "fused_tile"

    # conv2 forward / backward-data: JN of the small-grid kernels from ceil(M / 16) * ng > 128; tap split; multi-tap forms
    def c3(name, M, dims, **kw):
        p = S[name](M=M, g=ops.dims3(dims), nsplit=27)
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    for op, name in (("conv3_fwd", "Conv3FwdP"), ("conv3_bwd_data", "Conv3BwdDataP")):
        assert [form(op, c3(name, 1024, (8, 8, 4)), ng) for ng in (1, 2, 3)] == ["small1", "small1", "small2"]
        assert form(op, c3(name, 1024, (8, 8, 4), wfrag=1), 3) == "small2" and form(op, c3(name, 90, (5, 3, 2)), 4, conv3_small=2) == "small2"
        assert form(op, c3(name, 128, (4, 4, 2), partial=fake, nsplit=3), 3) == "tapsplit"
        assert form(op, c3(name, 1024, (8, 8, 4)), 2, conv3_small=-1, conv3_mt=-1) == "tapgemm"
        assert form(op, c3(name, 1176, (7, 7, 8)), 3, conv3_mt=3) == "mt32" and form(op, c3(name, 4096, (8, 16, 16)), 4) == "mt32"
    assert form("conv3_fwd", c3("Conv3FwdP", 4096, (8, 16, 16)), 3, conv3_mt=2) == "mt64"

    # conv2 weight gradient: the multi-tap kernel from chunks of >= 512 rows whose grid fills the chip, or forced
    w3 = lambda M, ms: S["Conv3BwdWP"](M=M, g=ops.dims3((8, 8, 4)), msplit=ms)
    assert form("conv3_bwd_weight", w3(1024, 4), 5) == "tapgemm" and form("conv3_bwd_weight", w3(1024, 4), 5, conv3w_mt=2) == "mt"
    assert form("conv3_bwd_weight", w3(8192, 8), 10) == "mt" and form("conv3_bwd_weight", w3(8192, 8), 10, conv3w_mt=-1) == "tapgemm"
    assert form("conv3_bwd_weight", w3(8192, 8), 8) == "tapgemm"                 # 576 workgroups: three quarters of a round


def test_weight_gradient_chunk_rule(lib):
    """mms_conv3_bwd_weight_msplit (a host function: no GPU): the row-chunk count the whole-encoder drivers give a conv2 weight-gradient launch of
    `members` (model, layer) members of M rows.  Chunks of 512..1024 rows whose 9-per-chunk grid fills >= 90 % of whole rounds of 3 x 256 workgroups
    put the launch on the multi-tap kernel; otherwise rows / 1024 (>= 4 members) or rows / 512 chunks of the one-tap form; levels of <= 1024 rows:
    256- / 128-row chunks.  MmsDnOpts.ms3_rows fixes the rows per chunk (the tests' group-independent setting)."""
    from multimodal_survival_prediction_amd import ops
    ms = lambda M, n, o=None: lib.mms_conv3_bwd_weight_msplit(M, n, ops.opts_ref(o))
    assert [ms(8192, n) for n in range(1, 11)] == [16, 16, 16, 8, 16, 14, 12, 10, 9, 8]
    for n in (5, 6, 7, 8, 9, 10):                   # the chosen grids fill their rounds, chunks stay within the kernel's 1024-row mask table
        c, w = ms(8192, n), ms(8192, n) * n * 9
        assert 512 <= ((8192 + c - 1) // c + 31) // 32 * 32 <= 1024 and w * 10 >= -(-w // 768) * 768 * 9
    assert [ms(1024, n) for n in (1, 3, 4, 10)] == [8, 8, 4, 4] and ms(128, 10) == 1 and ms(16, 1) == 1
    assert ms(8192, 6, ops.dn_opts(ms3_rows=512)) == 16 and ms(8192, 6, ops.dn_opts(conv3w_mt=-1)) == 8
    assert ms(0, 1) == 0 and ms(8192, 0) == 0 and ms(8192, 11) == 0
