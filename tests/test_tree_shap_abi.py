"""mms_tree_shap is declared in include/mmsurv.h, exported by the library, and refuses bad arguments on the host before any launch.  No
GPU: every pointer is a non-NULL dummy and the stream is NULL, so a call that got past its checks would fail differently (-2) or crash."""
import ctypes
import os

import pytest

from multimodal_survival_prediction_amd import _lib

D = 0x1000
FIELDS = ["R", "ldx", "p", "T", "nn", "G", "U", "ldr", "ldu", "pad_", "x", "feat", "thr", "value", "cover", "goff", "slot", "use", "phi", "base"]
SIZE = 120                 # 10 ints 40 | 10 pointers 80
LIM = _lib.defines("MMS_SHAP_")


def test_header_declares_the_entry_point_and_struct():
    protos = _lib.protos()
    assert len(protos["mms_tree_shap"]) == 2 and "TreeShapP" in protos["mms_tree_shap"][0] and protos["mms_tree_shap"][1].strip() == "hipStream_t"
    assert [f[0] for f in _lib.structs()["TreeShapP"]._fields_] == FIELDS
    assert ctypes.sizeof(_lib.structs()["TreeShapP"]) == SIZE
    assert LIM["MAX_DEPTH"] == 12 == _lib.defines("MMS_RSF_")["MAX_DEPTH"] >= _lib.defines("MMS_GBM_")["MAX_DEPTH"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.lib_path()):
        pytest.fail("libmmsurv_hip.so is not built")
    return _lib.load_library()


def test_library_exports_and_size(lib):
    assert hasattr(lib, "mms_tree_shap")
    assert lib.mms_abi_sizeof(b"TreeShapP") == SIZE


def _p(**kw):
    v = dict(dict(R=120, ldx=5005, p=5005, T=1500, nn=15, G=5, U=900, ldr=120, ldu=120, pad_=0, x=D, feat=D, thr=D, value=D, cover=D, goff=D,
                  slot=D, use=D, phi=D, base=D), **kw)
    s = _lib.structs()["TreeShapP"]()
    for k in FIELDS:
        setattr(s, k, v[k])
    return s


def test_checks_arguments_on_the_host(lib):
    bad = {"no_" + k: _p(**{k: None}) for k in ("x", "feat", "thr", "value", "cover", "goff", "slot", "phi", "base")}
    bad.update(R_neg=_p(R=-1), ldx_small=_p(ldx=5004), p0=_p(p=0, ldx=0), T_neg=_p(T=-1), G_neg=_p(G=-1), U0=_p(U=0), nn0=_p(nn=0),
               nn_big=_p(nn=2 << LIM["MAX_DEPTH"]), ldr_small=_p(ldr=119), ldu_small=_p(ldu=119))
    bad.update({k + "_misaligned": _p(**{k: D + 2}) for k in ("x", "feat", "thr", "cover", "goff", "slot")})
    bad.update({k + "_misaligned": _p(**{k: D + 4}) for k in ("value", "phi", "base")})
    for what, p in bad.items():
        assert lib.mms_tree_shap(ctypes.byref(p), None) == -1, what
    assert lib.mms_tree_shap(None, None) == -1


def test_empty_problems_are_valid_and_launch_nothing(lib):
    """R = 0 or G = 0 returns MMS_OK without a launch (a launch would need a GPU: there is none here and the pointers are dummies), with
    and without the use mask, at the largest table and with a use pitch that only matters with a mask"""
    assert lib.mms_tree_shap(ctypes.byref(_p(R=0)), None) == 0
    assert lib.mms_tree_shap(ctypes.byref(_p(G=0)), None) == 0
    assert lib.mms_tree_shap(ctypes.byref(_p(R=0, use=None, ldu=0, ldr=0)), None) == 0
    assert lib.mms_tree_shap(ctypes.byref(_p(G=0, use=None, ldu=0)), None) == 0
    assert lib.mms_tree_shap(ctypes.byref(_p(G=0, T=0, nn=(2 << LIM["MAX_DEPTH"]) - 1)), None) == 0
