"""mms_gsea_scores and mms_gsea_es are declared in include/mmsurv.h, exported by the library, and refuse bad arguments on the host before
any launch.  No GPU: every pointer is a non-NULL dummy and the stream is NULL, so a call that got past its checks would fail differently
(-2) or crash."""
import ctypes
import os
import re

import pytest

from multimodal_survival_prediction_amd import _lib

D = 0x1000
SCORE_FIELDS = ["n", "N", "ld", "G", "R1", "ldz", "x", "row", "m", "perm", "scale", "Z"]
ES_FIELDS = ["G", "S", "R1", "weight", "ldz", "lde", "Z", "gperm", "set_off", "set_gene", "es", "peak"]
SIZE = 72                       # 4-byte ints, 8-byte pointers: 6 ints 24 | 6 pointers 48 (both blocks)


def _limit(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(_lib.HEADER).read()).group(1))


def test_header_declares_the_entry_points_and_structs():
    protos = _lib.protos()
    for fn, st, fields in (("mms_gsea_scores", "GseaScoreP", SCORE_FIELDS), ("mms_gsea_es", "GseaEsP", ES_FIELDS)):
        assert len(protos[fn]) == 2 and st in protos[fn][0] and protos[fn][1].strip() == "hipStream_t"
        assert [f[0] for f in _lib.structs()[st]._fields_] == fields
        assert ctypes.sizeof(_lib.structs()[st]) == SIZE
    assert _limit("MMS_GSEA_MAX_G") >= 8192
    assert 16 * _limit("MMS_GSEA_MAX_G") <= 160 * 1024              # 16 bytes of LDS a gene against the 160 KiB a workgroup may declare
    assert _limit("MMS_GSEA_MAX_G") & (_limit("MMS_GSEA_MAX_G") - 1) == 0      # the sort's padded size never exceeds it


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.lib_path()):
        pytest.fail("libmmsurv_hip.so is not built")
    return _lib.load_library()


def test_library_exports_and_sizes(lib):
    for fn, st in (("mms_gsea_scores", "GseaScoreP"), ("mms_gsea_es", "GseaEsP")):
        assert hasattr(lib, fn)
        assert lib.mms_abi_sizeof(st.encode()) == ctypes.sizeof(_lib.structs()[st]) == SIZE


def _block(struct, fields, base, kw):
    v = dict(base, **{k: D for k in fields[6:]})
    v.update(kw)
    p = _lib.structs()[struct]()
    for k in fields:
        setattr(p, k, v[k])
    return p


def _score(**kw):
    return _block("GseaScoreP", SCORE_FIELDS, dict(n=427, N=608, ld=5008, G=5005, R1=1001, ldz=5005), kw)


def _es(**kw):
    return _block("GseaEsP", ES_FIELDS, dict(G=5005, S=50, R1=1001, weight=1, ldz=5005, lde=50), kw)


def test_scores_checks_arguments_on_the_host(lib):
    bad = {"no_" + k: _score(**{k: None}) for k in SCORE_FIELDS[6:]}
    bad.update(n1=_score(n=1), n_neg=_score(n=-3), N0=_score(N=0), G0=_score(G=0, ld=0, ldz=0), G_big=_score(G=_limit("MMS_GSEA_MAX_G") + 1,
               ld=1 << 20, ldz=1 << 20), ld_small=_score(ld=5004), ldz_small=_score(ldz=5004), R1_neg=_score(R1=-1),
               R1_big=_score(R1=_limit("MMS_GSEA_MAX_R1") + 1))
    bad.update({k + "_misaligned": _score(**{k: D + 2}) for k in ("x", "row", "perm")})
    bad.update({k + "_misaligned": _score(**{k: D + 4}) for k in ("m", "scale", "Z")})
    for what, p in bad.items():
        assert lib.mms_gsea_scores(ctypes.byref(p), None) == -1, what
    assert lib.mms_gsea_scores(None, None) == -1


def test_es_checks_arguments_on_the_host(lib):
    bad = {"no_" + k: _es(**{k: None}) for k in ("Z", "set_off", "set_gene", "es")}
    bad.update(G1=_es(G=1), G_big=_es(G=_limit("MMS_GSEA_MAX_G") + 1, ldz=1 << 20), S_neg=_es(S=-1), R1_neg=_es(R1=-1),
               R1_big=_es(R1=_limit("MMS_GSEA_MAX_R1") + 1), weight2=_es(weight=2), weight_neg=_es(weight=-1), ldz_small=_es(ldz=5004),
               lde_small=_es(lde=49))
    bad.update({k + "_misaligned": _es(**{k: D + 2}) for k in ("gperm", "set_off", "set_gene", "peak")})
    bad.update({k + "_misaligned": _es(**{k: D + 4}) for k in ("Z", "es")})
    for what, p in bad.items():
        assert lib.mms_gsea_es(ctypes.byref(p), None) == -1, what
    assert lib.mms_gsea_es(None, None) == -1


def test_empty_problems_are_valid_and_launch_nothing(lib):
    """R1 = 0 or S = 0 returns MMS_OK without a launch (a launch would need a GPU: there is none here and the pointers are dummies), with
    and without the optional pointers, at the limits"""
    assert lib.mms_gsea_scores(ctypes.byref(_score(R1=0)), None) == 0
    assert lib.mms_gsea_scores(ctypes.byref(_score(R1=0, n=2, G=_limit("MMS_GSEA_MAX_G"), ld=8192, ldz=8192)), None) == 0
    assert lib.mms_gsea_es(ctypes.byref(_es(R1=0)), None) == 0
    assert lib.mms_gsea_es(ctypes.byref(_es(S=0, lde=0)), None) == 0
    assert lib.mms_gsea_es(ctypes.byref(_es(S=0, gperm=None, peak=None)), None) == 0
    assert lib.mms_gsea_es(ctypes.byref(_es(R1=0, G=_limit("MMS_GSEA_MAX_G"), ldz=8192, weight=0, S=1 << 20, lde=1 << 20)), None) == 0
