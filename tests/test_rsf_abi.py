"""mms_rsf_split / mms_rsf_leaves / mms_rsf_predict are declared in include/mmsurv.h, exported by the library, and refuse bad arguments on
the host before any launch.  No GPU: every pointer is a non-NULL dummy and the stream is NULL, so a call that got past its checks would
fail differently (-2) or crash."""
import ctypes
import os
import re

import pytest

from multimodal_survival_prediction_amd import _lib

D = 0x1000
FIELDS = {
    "RsfSplitP": ["n", "ld", "p", "T", "level", "nn", "mtry", "nsplit", "min_leaf", "seed", "xt", "mult", "event", "tgroup", "tree_id", "node",
                  "feat", "thr", "stat", "n_node", "d_node", "U", "V", "n_left", "d_left", "ldo"],
    "RsfLeavesP": ["n", "ld", "T", "nn", "nh", "F", "mult", "event", "tgroup", "node", "feat", "n_node", "weight", "wset", "hpos", "mort", "H"],
    "RsfPredictP": ["R", "ldx", "p", "T", "nn", "nh", "x", "feat", "thr", "mort", "H", "use", "ldu", "out_mort", "out_H", "count"],
}
# 4-byte ints, 8-byte pointers: 10 ints 40 | 15 pointers 120 | ldo + pad 8;  6 ints 24 | 11 pointers 88;  6 ints 24 | 6 pointers 48 | ldu + pad 8 | 3 pointers 24
SIZES = {"RsfSplitP": 168, "RsfLeavesP": 112, "RsfPredictP": 104}
ENTRY = {"RsfSplitP": "mms_rsf_split", "RsfLeavesP": "mms_rsf_leaves", "RsfPredictP": "mms_rsf_predict"}


def _limit(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(_lib.HEADER).read()).group(1))


@pytest.mark.parametrize("S", sorted(FIELDS))
def test_header_declares_the_entry_points_and_structs(S):
    protos = _lib.protos()
    assert len(protos[ENTRY[S]]) == 2 and S in protos[ENTRY[S]][0] and protos[ENTRY[S]][1].strip() == "hipStream_t"
    assert [f[0] for f in _lib.structs()[S]._fields_] == FIELDS[S]
    assert ctypes.sizeof(_lib.structs()[S]) == SIZES[S]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.lib_path()):
        pytest.fail("libmmsurv_hip.so is not built")
    return _lib.load_library()


def test_library_exports_and_sizes(lib):
    for S, fn in ENTRY.items():
        assert hasattr(lib, fn)
        assert lib.mms_abi_sizeof(S.encode()) == ctypes.sizeof(_lib.structs()[S])


def _make(S, base, kw):
    v = dict(base, **kw)
    p = _lib.structs()[S]()
    for k in FIELDS[S]:
        setattr(p, k, v[k])
    return p


def _split(**kw):
    return _make("RsfSplitP", dict(n=608, ld=608, p=5005, T=2500, level=3, nn=2047, mtry=71, nsplit=10, min_leaf=15, seed=7, xt=D, mult=D,
                                   event=D, tgroup=D, tree_id=D, node=D, feat=D, thr=D, stat=D, n_node=D, d_node=D, U=D, V=D, n_left=D,
                                   d_left=D, ldo=710), kw)


def _leaves(**kw):
    return _make("RsfLeavesP", dict(n=608, ld=608, T=2500, nn=2047, nh=3, F=5, mult=D, event=D, tgroup=D, node=D, feat=D, n_node=D, weight=D,
                                    wset=D, hpos=D, mort=D, H=D), kw)


def _predict(**kw):
    return _make("RsfPredictP", dict(R=608, ldx=5005, p=5005, T=2500, nn=2047, nh=3, x=D, feat=D, thr=D, mort=D, H=D, use=D, ldu=608,
                                     out_mort=D, out_H=D, count=D), kw)


NO_TABLES = dict(U=None, V=None, n_left=None, d_left=None, ldo=0)


def test_split_checks_arguments_on_the_host(lib):
    bad = {"no_" + k: _split(**{k: None}) for k in ("xt", "mult", "event", "tgroup", "node", "feat", "thr", "stat", "n_node", "d_node")}
    bad.update(n0=_split(n=0), n_big=_split(n=_limit("MMS_RSF_MAX_N") + 1, ld=1 << 20), ld_small=_split(ld=607), p0=_split(p=0),
               T_neg=_split(T=-1), T_big=_split(T=_limit("MMS_RSF_MAX_T") + 1), level_neg=_split(level=-1),
               level_big=_split(level=_limit("MMS_RSF_MAX_DEPTH"), nn=(1 << 20)), nn_small=_split(nn=30), nn_big=_split(nn=2 << 13),
               mtry0=_split(mtry=0), nsplit0=_split(nsplit=0), min_leaf0=_split(min_leaf=0),
               C_big=_split(mtry=6554, nsplit=10, ldo=1 << 20), C_overflow=_split(mtry=1 << 20, nsplit=1 << 12, **NO_TABLES),
               only_U=_split(V=None, n_left=None, d_left=None), no_V=_split(V=None), no_n_left=_split(n_left=None),
               no_d_left=_split(d_left=None), ldo_small=_split(ldo=709))
    bad.update({k + "_misaligned": _split(**{k: D + 2}) for k in ("xt", "event", "tgroup", "tree_id", "node", "feat", "thr", "n_node",
                                                                 "d_node", "n_left", "d_left")})
    bad.update({k + "_misaligned": _split(**{k: D + 4}) for k in ("stat", "U", "V")})
    for what, p in bad.items():
        assert lib.mms_rsf_split(ctypes.byref(p), None) == -1, what
    assert lib.mms_rsf_split(None, None) == -1


def test_leaves_checks_arguments_on_the_host(lib):
    bad = {"no_" + k: _leaves(**{k: None}) for k in ("mult", "event", "tgroup", "node", "feat", "n_node", "weight", "hpos", "mort", "H")}
    bad.update(n0=_leaves(n=0), n_big=_leaves(n=_limit("MMS_RSF_MAX_N") + 1, ld=1 << 20), ld_small=_leaves(ld=607), T_neg=_leaves(T=-1),
               T_big=_leaves(T=_limit("MMS_RSF_MAX_T") + 1), nn0=_leaves(nn=0), nn_big=_leaves(nn=2 << 13), nh_neg=_leaves(nh=-1),
               nh_big=_leaves(nh=_limit("MMS_RSF_MAX_H") + 1), F0=_leaves(F=0))
    bad.update({k + "_misaligned": _leaves(**{k: D + 2}) for k in ("event", "tgroup", "node", "feat", "n_node", "wset", "hpos")})
    bad.update({k + "_misaligned": _leaves(**{k: D + 4}) for k in ("weight", "mort", "H")})
    for what, p in bad.items():
        assert lib.mms_rsf_leaves(ctypes.byref(p), None) == -1, what
    assert lib.mms_rsf_leaves(None, None) == -1


def test_predict_checks_arguments_on_the_host(lib):
    bad = {"no_" + k: _predict(**{k: None}) for k in ("x", "feat", "thr", "mort", "H", "out_mort", "out_H", "count")}
    bad.update(R_neg=_predict(R=-1), p0=_predict(p=0), ldx_small=_predict(ldx=5004), T_neg=_predict(T=-1),
               T_big=_predict(T=_limit("MMS_RSF_MAX_T") + 1), nn0=_predict(nn=0), nn_big=_predict(nn=2 << 13), nh_neg=_predict(nh=-1),
               nh_big=_predict(nh=_limit("MMS_RSF_MAX_H") + 1), ldu_small=_predict(ldu=607))
    bad.update({k + "_misaligned": _predict(**{k: D + 2}) for k in ("x", "feat", "thr", "count")})
    bad.update({k + "_misaligned": _predict(**{k: D + 4}) for k in ("mort", "H", "out_mort", "out_H")})
    for what, p in bad.items():
        assert lib.mms_rsf_predict(ctypes.byref(p), None) == -1, what
    assert lib.mms_rsf_predict(None, None) == -1


def test_empty_problems_are_valid_and_launch_nothing(lib):
    """T = 0 (R = 0 for predict) returns MMS_OK without a launch (a launch would need a GPU: there is none here and the pointers are
    dummies), with and without the optional pointers, at the limits"""
    assert lib.mms_rsf_split(ctypes.byref(_split(T=0)), None) == 0
    assert lib.mms_rsf_split(ctypes.byref(_split(T=0, tree_id=None, **NO_TABLES)), None) == 0
    assert lib.mms_rsf_split(ctypes.byref(_split(T=0, n=_limit("MMS_RSF_MAX_N"), ld=4096, level=_limit("MMS_RSF_MAX_DEPTH") - 1,
                                                 nn=(2 << _limit("MMS_RSF_MAX_DEPTH")) - 1, mtry=6553, nsplit=10, ldo=65530)), None) == 0
    assert lib.mms_rsf_leaves(ctypes.byref(_leaves(T=0)), None) == 0
    assert lib.mms_rsf_leaves(ctypes.byref(_leaves(T=0, wset=None, nh=0, hpos=None)), None) == 0
    assert lib.mms_rsf_predict(ctypes.byref(_predict(R=0)), None) == 0
    assert lib.mms_rsf_predict(ctypes.byref(_predict(R=0, use=None, ldu=0, nh=0, T=0)), None) == 0


def test_limits_in_the_header():
    """the member list of a node is 28 bytes of LDS a member; the deepest level's grid stays below 2^31 workgroups"""
    assert 28 * _limit("MMS_RSF_MAX_N") + 4096 <= 65536 and _limit("MMS_RSF_MAX_N") <= 65535
    assert _limit("MMS_RSF_MAX_DEPTH") == 12 and _limit("MMS_RSF_MAX_C") == 65535 and _limit("MMS_RSF_MAX_H") == 32
    assert _limit("MMS_RSF_MAX_T") << (_limit("MMS_RSF_MAX_DEPTH") - 1) < 2 ** 31 and 5 * 500 <= _limit("MMS_RSF_MAX_T")
