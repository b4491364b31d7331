"""mms_ct_preprocess_raw_batch is declared in include/mmsurv.h, exported by the library, and refuses bad arguments on the host before any
launch.  No GPU: every pointer is a non-NULL dummy and the stream is NULL, so a call that got past its checks would fail differently (-2)
or crash."""
import ctypes
import os
import re

import pytest

from multimodal_survival_prediction_amd import _lib

D = 0x1000
VOL_FIELDS = ["offset", "D", "H", "W", "dtype", "swap", "out_row", "slope", "inter"]
P_FIELDS = ["base", "base_bytes", "vols", "V", "n_rows", "out", "oD", "oH", "oW", "passes", "scratch"]
CODES = dict(MMS_CT_U8=2, MMS_CT_I16=4, MMS_CT_I32=8, MMS_CT_F32=16, MMS_CT_F64=64, MMS_CT_I8=256, MMS_CT_U16=512, MMS_CT_U32=768)


def _limit(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(_lib.HEADER).read()).group(1))


def test_header_declares_the_entry_point_and_the_codes():
    protos = _lib.protos()
    assert "mms_ct_preprocess_raw_batch" in protos and len(protos["mms_ct_preprocess_raw_batch"]) == 2
    assert "CtRawBatchP" in protos["mms_ct_preprocess_raw_batch"][0] and protos["mms_ct_preprocess_raw_batch"][1].strip() == "hipStream_t"
    for name, code in CODES.items():                        # the dtype codes are the NIfTI-1 datatype codes
        assert _limit(name) == code
    from multimodal_survival_prediction_amd import nifti
    assert sorted(nifti.DTYPES) == sorted(CODES.values())


def test_structs():
    V, P = _lib.structs()["CtRawVol"], _lib.structs()["CtRawBatchP"]
    assert [f[0] for f in V._fields_] == VOL_FIELDS and [f[0] for f in P._fields_] == P_FIELDS
    assert ctypes.sizeof(V) == 40                           # 8 | 6 x 4 | 2 x 4
    assert ctypes.sizeof(P) == 64                           # base 8, base_bytes 8, vols 8, V n_rows 8, out 8, oD oH oW passes 16, scratch 8


def test_limits_in_the_header():
    chunk, parts = _limit("MMS_CT_RAW_CHUNK"), _limit("MMS_CT_RAW_PARTS")
    assert _limit("MMS_CT_RAW_SCRATCH_FLOATS") == 2 * parts * chunk
    assert chunk * 48 + 64 <= 4096                          # a chunk's descriptors by value fit the kernarg segment
    assert _limit("MMS_CT_RAW_MAX_VOXELS") == 2 ** 31 - 1 and _limit("MMS_CT_RAW_MAX_VOLS") >= chunk


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.lib_path()):
        pytest.fail("libmmsurv_hip.so is not built")
    return _lib.load_library()


def test_library_exports_and_sizes(lib):
    assert hasattr(lib, "mms_ct_preprocess_raw_batch")
    for name in ("CtRawVol", "CtRawBatchP"):
        assert lib.mms_abi_sizeof(name.encode()) == ctypes.sizeof(_lib.structs()[name])


def _vol(**kw):
    v = dict(offset=0, D=3, H=5, W=7, dtype=4, swap=0, out_row=0, slope=1.0, inter=0.0)
    v.update(kw)
    return _lib.structs()["CtRawVol"](**v)


def _call(lib, descs, **kw):
    arr = (_lib.structs()["CtRawVol"] * max(1, len(descs)))(*descs)
    v = dict(base=D, base_bytes=1 << 20, vols=ctypes.cast(arr, ctypes.c_void_p), V=len(descs), n_rows=9, out=D, oD=8, oH=8, oW=4, scratch=D)
    v.update(kw)
    return lib.mms_ct_preprocess_raw_batch(ctypes.byref(_lib.structs()["CtRawBatchP"](**v)), None)


def test_checks_arguments_on_the_host(lib):
    ok = [_vol()]
    bad = dict(
        no_base=_call(lib, ok, base=None), no_out=_call(lib, ok, out=None), no_scratch=_call(lib, ok, scratch=None),
        no_vols=_call(lib, ok, vols=None), base_misaligned=_call(lib, ok, base=D + 8), out_misaligned=_call(lib, ok, out=D + 2),
        scratch_misaligned=_call(lib, ok, scratch=D + 1),
        V_neg=_call(lib, ok, V=-1), V_big=_call(lib, ok, V=_limit("MMS_CT_RAW_MAX_VOLS") + 1), base_bytes_neg=_call(lib, ok, base_bytes=-1),
        n_rows0=_call(lib, ok, n_rows=0), oD0=_call(lib, ok, oD=0), oH_neg=_call(lib, ok, oH=-1), oW0=_call(lib, ok, oW=0),
        out_big=_call(lib, ok, oD=2048, oH=2048, oW=512),
        offset_misaligned=_call(lib, [_vol(offset=8)]), offset_neg=_call(lib, [_vol(offset=-16)]),
        past_the_end=_call(lib, ok, base_bytes=2 * 105 - 1), past_the_end_offset=_call(lib, [_vol(offset=1 << 20)]),
        second_past_the_end=_call(lib, [_vol(), _vol(offset=224, out_row=1)], base_bytes=224 + 209),
        dtype_unknown=_call(lib, [_vol(dtype=128)]), dtype0=_call(lib, [_vol(dtype=0)]), dtype_i64=_call(lib, [_vol(dtype=1024)]),
        D0=_call(lib, [_vol(D=0)]), H_neg=_call(lib, [_vol(H=-5)]), W0=_call(lib, [_vol(W=0)]),
        voxels_2_31=_call(lib, [_vol(D=2048, H=2048, W=512, dtype=2)], base_bytes=1 << 40),
        row_neg=_call(lib, [_vol(out_row=-1)]), row_n=_call(lib, [_vol(out_row=9)]),
        row_twice=_call(lib, [_vol(), _vol(offset=224, out_row=3), _vol(offset=448, out_row=0)]),
        passes_neg=_call(lib, ok, passes=-1), passes_3=_call(lib, ok, passes=3),
        pass_alone_beyond_a_chunk=_call(lib, [_vol(offset=224 * j, out_row=j) for j in range(33)], n_rows=33, passes=1),
        slope_nan=_call(lib, [_vol(slope=float("nan"))]), inter_inf=_call(lib, [_vol(inter=float("inf"))]),
    )
    for what, rc in bad.items():
        assert rc == -1, what
    assert lib.mms_ct_preprocess_raw_batch(None, None) == -1
    assert len(bad) == 35


def test_no_volumes_is_valid_and_launches_nothing(lib):
    """V = 0 returns MMS_OK without a launch (a launch would need a GPU: there is none here and the pointers are dummies)"""
    assert _call(lib, []) == 0
    assert _call(lib, [], vols=None, base_bytes=0) == 0 and _call(lib, [], passes=2) == 0
