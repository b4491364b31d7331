"""The input-gradient attribution entry points (mms_conv0_bwd_data[_group], mms_dn121_input_grad, mms_fb3_input_grad) are declared in
include/mmsurv.h, bound through _lib's header parse, exported by the library and check their arguments on the host; no existing structure
changed; the host-side bookkeeping of multimodal_survival_prediction_amd.attribution on hand-made arrays.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from multimodal_survival_prediction_amd import _lib

EXPECTED = {"mms_conv0_bwd_data": 2, "mms_conv0_bwd_data_group": 3, "mms_dn121_input_grad": 13, "mms_fb3_input_grad": 14}


def test_header_declares_the_entry_points():
    protos = _lib.protos()
    for name, nargs in EXPECTED.items():
        assert name in protos, name
        assert len(protos[name]) == nargs, (name, protos[name])
        assert protos[name][-1].strip() == "hipStream_t"
    assert "Conv0BwdDataP" in protos["mms_conv0_bwd_data"][0] and "Conv0BwdDataP" in protos["mms_conv0_bwd_data_group"][0]
    # mms_dn121_backward's shape with (buffers, dx) in place of the gradient table; mms_fb3_backward's likewise
    assert len(protos["mms_dn121_input_grad"]) == len(protos["mms_dn121_backward"]) + 1
    assert len(protos["mms_fb3_input_grad"]) == len(protos["mms_fb3_backward"]) + 1
    assert "MmsDnOpts" in protos["mms_dn121_input_grad"][-2]


def test_structs():
    S = _lib.structs()
    assert [f[0] for f in S["Conv0BwdDataP"]._fields_] == ["dbn", "bn", "w", "in", "out", "M", "dx"]
    assert 10 * ctypes.sizeof(S["Conv0BwdDataP"]) + 8 <= 4096                    # ten members by value in the kernel-argument segment
    # unchanged: the blocks this path hands to the training backward's kernels
    assert [f[0] for f in S["BnSrc"]._fields_] == ["sum", "sumsq", "rmean", "rvar", "gamma", "beta", "inv_count", "eps", "train", "nrep", "rep_stride"]
    assert [f[0] for f in S["BnBwd"]._fields_] == ["s1", "s2", "nrep", "rep_stride"]
    assert [f[0] for f in S["Conv0FwdP"]._fields_] == ["x", "in", "out", "coords", "M", "w", "y", "osum", "osumsq", "srep", "sstride"]
    assert [f[0] for f in S["PoolBwdP"]._fields_] == ["dslab", "ld", "argmax", "out", "in", "B", "y0", "bn", "dbn", "s1", "s2", "coords", "srep", "sstride"]
    assert [f[0] for f in S["HeadBwdP"]._fields_][-3:] == ["dslab", "ldd", "ext_sums"]
    assert ctypes.sizeof(S["BnSrc"]) == 72 and ctypes.sizeof(S["FbConvP"]) * 10 + 8 <= 4096


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.lib_path()):
        pytest.fail("libmmsurv_hip.so is not built")
    return _lib.load_library()


def test_library_exports_and_sizes(lib):
    for name in EXPECTED:
        assert hasattr(lib, name), name
    assert lib.mms_abi_sizeof(b"Conv0BwdDataP") == ctypes.sizeof(_lib.structs()["Conv0BwdDataP"])


def _c0(in_dims=(16, 16, 8), out_dims=None, B=2, train=0, **null):
    """a Conv0BwdDataP whose pointers are non-NULL dummies: every case below must be refused on the host, before any launch"""
    S = _lib.structs()
    out_dims = out_dims or tuple((d + 1) // 2 for d in in_dims)
    d = lambda k: None if null.get(k) else 0x1000
    bn = S["BnSrc"](None, None, d("rmean"), d("rvar"), d("gamma"), d("beta"), 1.0, 1e-5, train)
    return S["Conv0BwdDataP"](d("dbn"), bn, d("w"), S["Dims3"](*in_dims), S["Dims3"](*out_dims), B * out_dims[0] * out_dims[1] * out_dims[2], d("dx"))


def test_conv0_bwd_data_checks_arguments_on_the_host(lib):
    bad = [_c0(dbn=True), _c0(w=True), _c0(dx=True), _c0(gamma=True), _c0(rvar=True), _c0(train=1),
           _c0(out_dims=(8, 8, 5)), _c0(out_dims=(16, 16, 8)), _c0(in_dims=(0, 16, 8), out_dims=(1, 8, 4)), _c0(in_dims=(4096, 16, 8))]
    for i, p in enumerate(bad):
        assert lib.mms_conv0_bwd_data(ctypes.byref(p), None) == -1, i
        assert lib.mms_conv0_bwd_data_group(ctypes.byref(p), 1, None) == -1, i
    p = _c0()
    p.M = 0
    assert lib.mms_conv0_bwd_data(ctypes.byref(p), None) == -1
    p.M = 2 * 8 * 8 * 4 + 1                                                      # not a whole number of samples
    assert lib.mms_conv0_bwd_data(ctypes.byref(p), None) == -1
    assert lib.mms_conv0_bwd_data(None, None) == -1
    ok = _c0()
    assert lib.mms_conv0_bwd_data_group(ctypes.byref(ok), 0, None) == -1 and lib.mms_conv0_bwd_data_group(ctypes.byref(ok), 11, None) == -1
    two = (_lib.structs()["Conv0BwdDataP"] * 2)(_c0(), _c0(in_dims=(16, 16, 16)))     # members of different shape
    assert lib.mms_conv0_bwd_data_group(two, 2, None) == -1


def test_drivers_check_arguments_on_the_host(lib):
    P = ctypes.c_void_p
    tab = (P * 512)(*([0x1000] * 512))
    d = 0x1000
    # DenseNet121: the workspace plan's domain (multiples of 32, B > 0), NULL pointers, a dout pitch below the feature width
    for B, D, H, W in ((0, 32, 32, 32), (2, 48, 32, 32), (2, 32, 32, 16), (2, 32, 32, 4096)):
        assert lib.mms_dn121_input_grad(d, B, D, H, W, d, tab, tab, d, 128, d, None, None) == -1, (B, D, H, W)
    for k in range(6):
        a = [d, d, tab, tab, d, d]
        a[k] = None
        assert lib.mms_dn121_input_grad(a[0], 2, 32, 32, 32, a[1], a[2], a[3], a[4], 128, a[5], None, None) == -1, k
    assert lib.mms_dn121_input_grad(d, 2, 32, 32, 32, d, tab, tab, d, 64, d, None, None) == -1
    # 3-conv encoder: widths, workspace size, NULL pointers, NULL table entries
    w = (ctypes.c_int * 3)(32, 64, 128)
    n = ctypes.c_size_t(0)
    assert lib.mms_fb3_workspace_bytes(w, 2, 16, 16, 8, ctypes.byref(n)) == 0
    call = lambda **kw: lib.mms_fb3_input_grad(kw.get("ws", d), kw.get("nb", n.value), kw.get("w", w), kw.get("B", 2), 16, 16, 8, kw.get("x", d),
                                               kw.get("prm", tab), kw.get("buf", tab), kw.get("dout", d), kw.get("ld", 128), kw.get("dx", d), None)
    for kw in (dict(ws=None), dict(x=None), dict(prm=None), dict(buf=None), dict(dout=None), dict(dx=None), dict(nb=n.value + 256), dict(B=0),
               dict(ld=64), dict(w=None), dict(w=(ctypes.c_int * 3)(8, 64, 128)), dict(w=(ctypes.c_int * 3)(48, 64, 128))):
        assert call(**kw) == -1, kw
    hole = (P * 12)(*([0x1000] * 11 + [None]))
    assert call(prm=hole) == -1 and call(buf=(P * 9)(*([0x1000] * 8 + [None]))) == -1


def test_modality_shares_and_gene_scores_on_hand_made_arrays():
    from multimodal_survival_prediction_amd import attribution
    res = dict(ct=np.array([[[[[1., -1.]]]], [[[[2., 0.]]]]]), rna=np.array([[0.5, 0., -2.], [0., 0., 0.]]), clinical=np.array([[1.], [4.]]))
    batch = dict(ct=np.array([[[[[2., 1.]]]], [[[[1., 5.]]]]]), rna=np.array([[2., 7., 1.], [3., 3., 3.]]), clinical=np.array([[-1.], [0.5]]),
                 mask=np.array([[1., 1., 1.], [1., 0., 1.]]))
    sh = attribution.modality_shares(res, batch)
    # row 0: |1*2| + |-1*1| = 3, |0.5*2| + 0 + |-2*1| = 3, |1*-1| = 1;  row 1: 2, 0, 2
    assert sh.shape == (2, 3) and np.allclose(sh, [[3 / 7, 3 / 7, 1 / 7], [0.5, 0.0, 0.5]]) and np.allclose(sh.sum(1), 1)
    assert np.allclose(attribution.modality_shares(dict(ct=None, rna=res["rna"], clinical=None), batch), [[0, 1, 0], [0, 0, 0]])
    # the cohort's key names are accepted too
    assert np.allclose(attribution.modality_shares(res, dict(image=batch["ct"], rnaseq=batch["rna"], clinical=batch["clinical"])), sh)
    g = attribution.gene_scores(res, batch, names=["A", "B", "C"], top=2)         # row 1 has no RNA: the mean is over row 0 alone
    assert g == [("C", 2.0), ("A", 0.5)]
    g = attribution.gene_scores(res, dict(rna=batch["rna"]), top=50)               # no mask: both rows; default names; top beyond the count
    assert g == [("g2", 1.0), ("g0", 0.25), ("g1", 0.0)]
    with pytest.raises(ValueError):
        attribution.gene_scores(res, batch, names=["A"])
    with pytest.raises(ValueError):
        attribution.gene_scores(dict(rna=None), batch)
    with pytest.raises(ValueError):
        attribution.saliency(None, batch, kind="integrated")


def test_attribution_is_exported_lazily():
    import multimodal_survival_prediction_amd as pkg
    assert "attribution" in pkg.__all__ and hasattr(pkg.attribution, "saliency") and hasattr(pkg.attribution, "gene_scores")
