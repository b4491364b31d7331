"""The ensemble entry points (mms_dn121_input_grad_group, mms_fb3_input_grad_group, mms_ensemble_reduce) are declared in
include/mmsurv.h, exported by the library, and refuse bad arguments on the host before any launch.  No GPU: every pointer is a non-NULL
dummy and the stream is NULL, so a call that got past its checks would fail differently (-2) or crash."""
import ctypes
import os

import pytest

from multimodal_survival_prediction_amd import _lib

EXPECTED = {"mms_dn121_input_grad_group": 14, "mms_fb3_input_grad_group": 15, "mms_ensemble_reduce": 2}
P = ctypes.c_void_p
D = 0x1000


def test_header_declares_the_entry_points():
    protos = _lib.protos()
    for name, nargs in EXPECTED.items():
        assert name in protos, name
        assert len(protos[name]) == nargs, (name, protos[name])
        assert protos[name][-1].strip() == "hipStream_t"
    # the single drivers' arguments plus ng
    assert len(protos["mms_dn121_input_grad_group"]) == len(protos["mms_dn121_input_grad"]) + 1
    assert len(protos["mms_fb3_input_grad_group"]) == len(protos["mms_fb3_input_grad"]) + 1
    assert "MmsDnOpts" in protos["mms_dn121_input_grad_group"][-2] and "EnsP" in protos["mms_ensemble_reduce"][0]


def test_structs():
    S = _lib.structs()
    assert [f[0] for f in S["EnsP"]._fields_] == ["x", "K", "n", "mean", "spread"]
    assert ctypes.sizeof(S["EnsP"]) == 10 * 8 + 8 + 8 + 8 + 8
    # ten members by value in the 4 KB kernel-argument segment: the regrouped head kernel, the 3-conv kernels (the conv kernel carries
    # each member's output BatchNorm beside its block)
    assert 10 * ctypes.sizeof(S["HeadBwdP"]) + 8 <= 4096
    assert 10 * ctypes.sizeof(S["FbPoolP"]) + 8 <= 4096
    assert 10 * (ctypes.sizeof(S["FbConvP"]) + ctypes.sizeof(S["BnSrc"])) + 8 <= 4096


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.lib_path()):
        pytest.fail("libmmsurv_hip.so is not built")
    return _lib.load_library()


def test_library_exports_and_sizes(lib):
    for name in EXPECTED:
        assert hasattr(lib, name), name
    assert lib.mms_abi_sizeof(b"EnsP") == ctypes.sizeof(_lib.structs()["EnsP"])


def _ens(K=3, n=100, mean=D, spread=D, x=None):
    p = _lib.structs()["EnsP"]()
    for g in range(10):
        p.x[g] = D if g < K else None
    for g, v in (x or {}).items():
        p.x[g] = v
    p.K, p.n, p.mean, p.spread = K, n, mean, spread
    return p


def test_ensemble_reduce_checks_arguments_on_the_host(lib):
    bad = dict(K0=_ens(K=0), K11=_ens(K=11), Kneg=_ens(K=-1), n0=_ens(n=0), no_mean=_ens(mean=None), null_member=_ens(x={1: None}),
               null_last=_ens(K=10, x={9: None}), mis_mean=_ens(mean=D + 4), mis_spread=_ens(spread=D + 8), mis_member=_ens(x={2: D + 4}),
               mis_mean_no_spread=_ens(mean=D + 12, spread=None))
    for what, p in bad.items():
        assert lib.mms_ensemble_reduce(ctypes.byref(p), None) == -1, what
    assert lib.mms_ensemble_reduce(None, None) == -1


def _tabs(ng, n):
    """ng real tables of n dummy pointers and the array of their addresses"""
    tabs = [(P * n)(*([D] * n)) for _ in range(ng)]
    return tabs, (P * 10)(*([ctypes.addressof(t) for t in tabs] + [None] * (10 - ng)))


def _vec(ng, hole=None):
    return (P * 10)(*[(D if (g < ng and g != hole) else None) for g in range(10)])


def test_dn121_input_grad_group_checks_arguments_on_the_host(lib):
    ng = 3
    keep, prm = _tabs(ng, 512)
    keep2, buf = _tabs(ng, 512)
    f = lib.mms_dn121_input_grad_group
    call = lambda **kw: f(kw.get("ng", ng), kw.get("ws", _vec(ng)), kw.get("B", 2), kw.get("D", 32), kw.get("H", 32), kw.get("W", 32),
                          kw.get("x", _vec(ng)), kw.get("prm", prm), kw.get("buf", buf), kw.get("dout", _vec(ng)), kw.get("ld", 128),
                          kw.get("dx", _vec(ng)), None, None)
    for kw in (dict(ng=0), dict(ng=11), dict(ng=-1), dict(ws=None), dict(x=None), dict(prm=None), dict(buf=None), dict(dout=None), dict(dx=None),
               dict(ws=_vec(ng, 1)), dict(x=_vec(ng, 2)), dict(dout=_vec(ng, 0)), dict(dx=_vec(ng, 2)),
               dict(prm=(P * 10)(ctypes.addressof(keep[0]), None, ctypes.addressof(keep[2]))),
               dict(buf=(P * 10)(ctypes.addressof(keep2[0]), ctypes.addressof(keep2[1]), None)),
               dict(B=0), dict(D=48), dict(W=16), dict(H=4096), dict(ld=64)):
        assert call(**kw) == -1, kw


def test_fb3_input_grad_group_checks_arguments_on_the_host(lib):
    ng = 2
    keep, prm = _tabs(ng, 12)
    keep2, buf = _tabs(ng, 9)
    w = (ctypes.c_int * 3)(32, 64, 128)
    n = ctypes.c_size_t(0)
    assert lib.mms_fb3_workspace_bytes(w, 2, 16, 16, 8, ctypes.byref(n)) == 0
    f = lib.mms_fb3_input_grad_group
    call = lambda **kw: f(kw.get("ng", ng), kw.get("ws", _vec(ng)), kw.get("nb", n.value), kw.get("w", w), kw.get("B", 2), 16, 16, 8,
                          kw.get("x", _vec(ng)), kw.get("prm", prm), kw.get("buf", buf), kw.get("dout", _vec(ng)), kw.get("ld", 128),
                          kw.get("dx", _vec(ng)), None)
    hole_p = (P * 12)(*([D] * 11 + [None]))
    hole_b = (P * 9)(*([D] * 8 + [None]))
    for kw in (dict(ng=0), dict(ng=11), dict(ws=None), dict(x=None), dict(prm=None), dict(buf=None), dict(dout=None), dict(dx=None),
               dict(ws=_vec(ng, 1)), dict(x=_vec(ng, 1)), dict(dout=_vec(ng, 0)), dict(dx=_vec(ng, 1)),
               dict(prm=(P * 10)(ctypes.addressof(keep[0]), None)), dict(buf=(P * 10)(None, ctypes.addressof(keep2[1]))),
               dict(prm=(P * 10)(ctypes.addressof(keep[0]), ctypes.addressof(hole_p))),
               dict(buf=(P * 10)(ctypes.addressof(hole_b), ctypes.addressof(keep2[1]))),
               dict(nb=n.value + 256), dict(B=0), dict(ld=64), dict(w=None), dict(w=(ctypes.c_int * 3)(8, 64, 128)),
               dict(w=(ctypes.c_int * 3)(48, 64, 128))):
        assert call(**kw) == -1, kw
