"""The fine-tuning entry points (mms_*_tuned[_group], mms_tune_check, mms_dn121_backward[_group]_from) are declared in include/mmsurv.h,
exported by the library, and refuse bad arguments on the host before any launch.  No GPU: every pointer is a non-NULL dummy and the
stream is NULL, so a call that got past its checks would fail differently (-2) or crash."""
import ctypes
import os

import pytest

from multimodal_survival_prediction_amd import _lib

D = 0x1000
TUNE_FIELDS = ["a", "bounds", "lr_mult", "wd_mult", "l2sp", "nseg", "anchor"]


def test_header_declares_the_entry_points():
    protos = _lib.protos()
    for name in ("mms_grad_sumsq_tuned", "mms_clip_adam_tuned"):
        a = [x.strip() for x in protos[name]]
        assert len(a) == 2 and "TuneP" in a[0] and a[1] == "hipStream_t"
        a = [x.strip() for x in protos[name + "_group"]]
        assert len(a) == 3 and "TuneP" in a[0] and a[1] == "int" and a[2] == "hipStream_t"
    assert len(protos["mms_tune_check"]) == 1
    # the _from drivers: the plain drivers' arguments with `int block_lo` before the options
    for plain, frm in (("mms_dn121_backward", "mms_dn121_backward_from"), ("mms_dn121_backward_group", "mms_dn121_backward_group_from")):
        a, b = [x.strip() for x in protos[plain]], [x.strip() for x in protos[frm]]
        assert b[:-3] + b[-2:] == a and b[-3] == "int"
    assert _lib.defines("MMS_TUNE_")["MAX_SEG"] == 512


def test_struct():
    S = _lib.structs()
    T = S["TuneP"]
    assert [f[0] for f in T._fields_] == TUNE_FIELDS
    assert T._fields_[0][1] is S["AdamP"]                 # AdamP itself is unchanged and embedded by value
    assert ctypes.sizeof(S["AdamP"]) == 152
    # a 152 | bounds lr_mult wd_mult l2sp 32 | nseg + pad 8 | anchor 8
    assert ctypes.sizeof(T) == 200 and T.bounds.offset == 152 and T.nseg.offset == 184 and T.anchor.offset == 192


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.lib_path()):
        pytest.fail("libmmsurv_hip.so is not built")
    return _lib.load_library()


def test_library_exports_and_size(lib):
    for name in ("mms_grad_sumsq_tuned", "mms_clip_adam_tuned", "mms_grad_sumsq_tuned_group", "mms_clip_adam_tuned_group", "mms_tune_check",
                 "mms_dn121_backward_from", "mms_dn121_backward_group_from"):
        assert hasattr(lib, name), name
    assert lib.mms_abi_sizeof(b"TuneP") == ctypes.sizeof(_lib.structs()["TuneP"])


def _t(adam=None, **kw):
    S = _lib.structs()
    a = dict(p=D, g=D, m=D, v=D, n=1000, hyper=D, sumsq=D, step=D)
    a.update(adam or {})
    t = S["TuneP"]()
    for k, v in a.items():
        setattr(t.a, k, v)
    v = dict(bounds=D, lr_mult=D, wd_mult=D, l2sp=D, nseg=3, anchor=None)
    v.update(kw)
    for k, x in v.items():
        setattr(t, k, x)
    return t


def _all(lib, t, ng=1):
    arr = (_lib.structs()["TuneP"] * len(t))(*t) if isinstance(t, list) else t
    ref = arr if isinstance(t, list) else ctypes.byref(t)
    return lib.mms_grad_sumsq_tuned_group(ref, ng, None), lib.mms_clip_adam_tuned_group(ref, ng, None)


def test_checks_arguments_on_the_host(lib):
    bad = dict(nseg0=_t(nseg=0), nseg_big=_t(nseg=513), nseg_neg=_t(nseg=-1), no_bounds=_t(bounds=None), no_lr=_t(lr_mult=None),
               no_wd=_t(wd_mult=None), no_l2=_t(l2sp=None), anchor_misaligned=_t(anchor=D + 4), n0=_t(adam=dict(n=0)),
               n_big=_t(adam=dict(n=1 << 33)), p_misaligned=_t(adam=dict(p=D + 4)), g_misaligned=_t(adam=dict(g=D + 8)),
               no_m=_t(adam=dict(m=None)), no_hyper=_t(adam=dict(hyper=None)), no_sumsq=_t(adam=dict(sumsq=None)),
               no_step=_t(adam=dict(step=None)), w2_without_tables=_t(adam=dict(n_w2=2)), w2_too_many=_t(adam=dict(n_w2=65, w2_off=D, w2_pack_b=D)))
    for what, t in bad.items():
        assert _all(lib, t) == (-1, -1), what
        assert lib.mms_tune_check(ctypes.byref(t)) == -1, what
        assert lib.mms_grad_sumsq_tuned(ctypes.byref(t), None) == -1 and lib.mms_clip_adam_tuned(ctypes.byref(t), None) == -1, what
    assert _all(lib, _t(), ng=0) == (-1, -1) and _all(lib, [_t()] * 11, ng=11) == (-1, -1)
    assert lib.mms_grad_sumsq_tuned_group(None, 1, None) == -1 and lib.mms_clip_adam_tuned_group(None, 1, None) == -1
    assert lib.mms_tune_check(None) == -1
    # a group shares ONE segment table and one shape
    assert _all(lib, [_t(), _t(bounds=D + 64)], ng=2) == (-1, -1)
    assert _all(lib, [_t(), _t(l2sp=D + 64)], ng=2) == (-1, -1)
    assert _all(lib, [_t(), _t(nseg=4)], ng=2) == (-1, -1)
    assert _all(lib, [_t(), _t(adam=dict(n=1004))], ng=2) == (-1, -1)


def test_backward_from_refuses_a_block_outside_the_net(lib):
    P = ctypes.c_void_p
    tab = (P * 364)(*([D] * 364))
    for lo in (-1, 4, 7):
        assert lib.mms_dn121_backward_from(D, 2, 32, 32, 32, D, tab, D, 128, tab, lo, None, None) == -1, lo
        ws, x, pp, gg = (P * 1)(D), (P * 1)(D), (P * 1)(ctypes.addressof(tab)), (P * 1)(ctypes.addressof(tab))
        assert lib.mms_dn121_backward_group_from(1, ws, 2, 32, 32, 32, x, pp, x, 128, gg, lo, None, None) == -1, lo
    assert lib.mms_dn121_backward_group_from(0, None, 2, 32, 32, 32, None, None, None, 128, None, 1, None, None) == -1
