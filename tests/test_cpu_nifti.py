"""nifti.py (the NIfTI-1 reader / writer) against files built and parsed by tests/nifti_ref.py straight from the specification's byte
offsets: every datatype, both byte orders, .nii and .nii.gz, extensions, the three affine sources, every refusal, the writer, and the
saliency-map affine rule.  No GPU."""
import itertools

import numpy as np
import pytest

import nifti_ref as NR
from multimodal_survival_prediction_amd import nifti

SHAPE = (3, 5, 7)            # (nz, ny, nx)


@pytest.mark.parametrize("datatype,endian,ext", [(d, e, x) for d, e, x in itertools.product(sorted(NR.TYPES), "<>", (".nii", ".nii.gz"))])
def test_round_trip(tmp_path, datatype, endian, ext):
    vals = NR.ct_values(SHAPE, datatype, seed=datatype)
    path = NR.save(tmp_path / ("v" + ext), NR.build(vals, datatype, endian=endian, slope=2.5, inter=-1024.0))
    h, raw = nifti.read_nifti(path)
    assert raw.shape == SHAPE and h["shape"] == SHAPE and h["datatype"] == datatype and h["dim"][:4] == (3, 7, 5, 3)
    assert raw.dtype.itemsize == NR.TYPES[datatype][1] // 8 and raw.dtype.kind == NR.TYPES[datatype][0][0]
    # the stored bytes untouched (the device swaps), the values right once the byte order is read
    assert raw.tobytes() == NR.parse(path)["raw_bytes"]
    assert np.array_equal(raw.astype(raw.dtype.newbyteorder("=")), vals)
    import sys
    other = (endian == ">") != (sys.byteorder == "big")
    assert h["swap"] == (other and raw.dtype.itemsize > 1) and h["endian"] == endian
    assert (h["scl_slope"], h["scl_inter"]) == (2.5, -1024.0) and nifti.scaling(h) == (2.5, -1024.0)
    assert nifti.dtype_code(raw.dtype) == datatype
    assert nifti.read_header(path)["dim"] == h["dim"]


def test_array_order_is_z_y_x(tmp_path):
    """a ramp along x (the fastest file axis) varies along the LAST array axis: SimpleITK's GetArrayFromImage order"""
    ramp = np.broadcast_to(np.arange(7, dtype=np.int16), SHAPE)
    _, raw = nifti.read_nifti(NR.save(tmp_path / "r.nii", NR.build(ramp, 4)))
    assert np.array_equal(raw[0, 0], np.arange(7)) and (raw == raw[:1, :1]).all()
    zramp = np.broadcast_to(np.arange(3, dtype=np.int16)[:, None, None], SHAPE)
    blob = NR.build(zramp, 4)
    assert NR.parse(blob)["raw_bytes"][:2 * 35] == b"\0" * 70            # the first z-slab of the file is all zeros
    _, raw = nifti.read_nifti(NR.save(tmp_path / "z.nii", blob))
    assert np.array_equal(raw[:, 2, 3], np.arange(3))


@pytest.mark.parametrize("ext", [".nii", ".nii.gz"])
def test_vox_offset_and_extension(tmp_path, ext):
    vals = NR.ct_values(SHAPE, 4, seed=1)
    for off in (352, 400):
        h, raw = nifti.read_nifti(NR.save(tmp_path / ("o%d%s" % (off, ext)), NR.build(vals, 4, vox_offset=off)))
        assert h["vox_offset"] == off and np.array_equal(raw, vals)


def test_trailing_unit_dims_and_slope_zero(tmp_path):
    vals = NR.ct_values(SHAPE, 16, seed=2)
    h, raw = nifti.read_nifti(NR.save(tmp_path / "d4.nii.gz", NR.build(vals, 16, dim=(4, 7, 5, 3, 1, 0, 0, 0))))
    assert np.array_equal(raw, vals) and h["dim"][0] == 4
    assert nifti.scaling(h) == (1.0, 0.0)                                    # scl_slope 0: no scaling
    assert nifti.scaling(dict(h, scl_slope=0.0, scl_inter=7.0)) == (1.0, 0.0)
    assert nifti.read_header(NR.build(vals, 16))["shape"] == SHAPE           # bytes in, header out


def test_affine_sources():
    vals = np.zeros(SHAPE, np.int16)
    srow = [[0.7, 0.1, 0.0, -90.0], [0.0, 0.8, -0.2, 12.5], [0.05, 0.0, 3.0, 400.0]]
    A = nifti.affine_of(nifti.read_header(NR.build(vals, 4, sform=srow, qform=(0, 0, 0, 1, 2, 3, 1.0))))     # the sform wins
    assert np.array_equal(A[:3], np.array(srow, dtype=np.float32).astype(np.float64)) and np.array_equal(A[3], [0, 0, 0, 1])
    # qform: 90 degrees about z is the quaternion (a, b, c, d) = (cos 45, 0, 0, sin 45): x -> y, y -> -x; spacings 2, 3, 5
    s = float(np.sqrt(0.5))
    A = nifti.affine_of(nifti.read_header(NR.build(vals, 4, qform=(0.0, 0.0, s, 10.0, 20.0, 30.0, 1.0), pixdim=(2.0, 3.0, 5.0))))
    want = np.array([[0, -3, 0, 10], [2, 0, 0, 20], [0, 0, 5, 30], [0, 0, 0, 1]], dtype=np.float64)
    assert np.allclose(A, want, rtol=0, atol=1e-6)
    A = nifti.affine_of(nifti.read_header(NR.build(vals, 4, qform=(0.0, 0.0, s, 10.0, 20.0, 30.0, -1.0), pixdim=(2.0, 3.0, 5.0))))
    want[2, 2] = -5                                                          # qfac = pixdim[0] = -1 flips the third column
    assert np.allclose(A, want, rtol=0, atol=1e-6)
    A = nifti.affine_of(nifti.read_header(NR.build(vals, 4, pixdim=(0.5, 0.75, 2.5))))
    assert np.array_equal(A, np.diag([0.5, 0.75, 2.5, 1.0]))


def test_refusals_name_the_file_and_the_field(tmp_path):
    vals = NR.ct_values(SHAPE, 4, seed=3)
    cases = {
        "sizeof_hdr": dict(sizeof_hdr=540),                                   # NIfTI-2
        "magic": dict(magic=b"ni1\0"),                                        # two-file
        "datatype": dict(datatype=128, bitpix=24),                            # RGB
        "dim": dict(dim=(4, 7, 5, 3, 2, 1, 1, 1)),                            # 4-D
        "data": dict(data_bytes=2 * 105 - 1),                                 # one byte short
        "bitpix": dict(bitpix=32),
    }
    for field, kw in cases.items():
        kw = dict(kw)
        dt = kw.pop("datatype", 4)
        for ext in (".nii", ".nii.gz"):
            path = NR.save(tmp_path / ("bad_%s%s" % (field, ext)), NR.build(vals, dt, **kw))
            with pytest.raises(ValueError) as ei:
                nifti.read_nifti(path)
            assert field in str(ei.value) and path in str(ei.value), (field, str(ei.value))
    for dt, bits in ((32, 64), (1792, 128), (1536, 128), (2304, 32)):         # complex64, complex128, float128, RGBA
        with pytest.raises(ValueError, match="datatype"):
            nifti.read_header(NR.build(vals, dt, bitpix=bits))
    with pytest.raises(ValueError, match="magic"):
        nifti.read_header(NR.build(vals, 4, magic=b"\0\0\0\0"))               # Analyze 7.5: no magic
    with pytest.raises(ValueError, match="sizeof_hdr"):
        nifti.read_header(NR.build(vals, 4, sizeof_hdr=540, endian=">"))
    with pytest.raises(ValueError, match="sizeof_hdr"):
        nifti.read_header(b"\x1f\x8b" + bytes(400))
    with pytest.raises(ValueError, match=r"dim\[0\]"):
        nifti.read_header(NR.build(vals, 4, dim=(9, 7, 5, 3, 1, 1, 1, 1)))
    # a gzip stream cut in the middle of the data
    import gzip
    whole = gzip.compress(NR.build(NR.ct_values((20, 45, 24), 4, seed=4), 4))
    path = tmp_path / "cut.nii.gz"
    path.write_bytes(whole[:len(whole) // 2])
    with pytest.raises(ValueError, match="cut.nii.gz"):
        nifti.read_nifti(str(path))


@pytest.mark.parametrize("dtype,ext", [(np.float32, ".nii"), (np.float32, ".nii.gz"), (np.int16, ".nii.gz")])
def test_writer_against_the_test_side_parser(tmp_path, dtype, ext):
    vals = NR.ct_values((4, 6, 5), 4, seed=5).astype(dtype)
    A = np.array([[0.7, 0.1, 0.0, -90.0], [0.0, 0.8, -0.2, 12.5], [0.05, 0.0, 3.0, 400.0], [0, 0, 0, 1]])
    path = str(tmp_path / ("w" + ext))
    nifti.write_nifti(path, vals, affine=A)
    p = NR.parse(path)
    assert p["raw_bytes"] == vals.astype(np.dtype(dtype).newbyteorder("<")).tobytes() and p["vox_offset"] == 352 and p["endian"] == "<"
    assert p["dim"][:4] == (3, 5, 6, 4) and p["sform_code"] == 1 and p["datatype"] == {np.float32: 16, np.int16: 4}[dtype]
    assert np.array_equal(p["affine"], A.astype(np.float32).astype(np.float64))
    assert np.allclose(p["pixdim"][1:4], np.linalg.norm(A[:3, :3], axis=0), rtol=1e-6)
    h, raw = nifti.read_nifti(path)                                          # and our reader reads our writer
    assert np.array_equal(raw, vals) and np.array_equal(nifti.affine_of(h), p["affine"])
    nifti.write_nifti(str(tmp_path / "like.nii"), vals, like=h)              # geometry copied from a header
    assert np.array_equal(NR.parse(str(tmp_path / "like.nii"))["affine"], p["affine"])
    with pytest.raises(ValueError):
        nifti.write_nifti(path, vals.astype(np.float64))


def test_saliency_affine_rule():
    """native (nz, ny, nx) = (10, 12, 9) resampled to (tD, tH, tW) = (4, 4, 1): per axis (native - 1) / (target - 1), 1 where target is 1,
    applied in NIfTI index order (x, y, z) to the columns of the scan's matrix"""
    A = np.array([[0.5, 0, 0, -100.0], [0, 0.25, 0, 50.0], [0, 0, 2.0, 7.0], [0, 0, 0, 1]])
    got = nifti.saliency_affine(A, (10, 12, 9), (4, 4, 1))
    want = np.array([[0.5 * 1.0, 0, 0, -100.0], [0, 0.25 * 11 / 3, 0, 50.0], [0, 0, 2.0 * 3.0, 7.0], [0, 0, 0, 1]])
    assert np.allclose(got, want, rtol=1e-15, atol=0)
    # index 0 maps to index 0, the last target index to the last native index
    assert np.allclose(got @ [0, 3, 3, 1], A @ [0, 11, 9, 1]) and np.allclose(got @ [0, 0, 0, 1], A @ [0, 0, 0, 1])
    B = np.array([[0.0, -3, 0, 10], [2, 0, 0, 20], [0, 0, 5, 30], [0, 0, 0, 1.0]])     # a rotated scan: columns scale, not rows
    assert np.allclose(nifti.saliency_affine(B, (10, 12, 9), (4, 4, 1)), B @ np.diag([1.0, 11 / 3, 3.0, 1.0]))
    assert np.array_equal(nifti.saliency_affine(None, None, (4, 4, 1)), np.eye(4))


def test_write_cohort_nifti_mix(tmp_path):
    """write_cohort(volume_format="nii.gz"): the table points at NIfTI files the test-side parser reads; int16 by default, every third
    patient big-endian / float32 / uint16 with scl_inter; the values are the rounded HU-like values of the .npy form"""
    from multimodal_survival_prediction_amd import cohort_io, data
    c = data.make_cohort(n=14, dims=(8, 8, 4), rna_dim=6, seed=9, complete=False, counts=dict(n=14, imaging=12, rnaseq=10, clinical=12, survival=8))
    cohort_io.write_cohort(str(tmp_path / "n"), c, native_dims=(5, 6, 7), seed=3, volume_format="nii.gz")
    cohort_io.write_cohort(str(tmp_path / "p"), c, native_dims=(5, 6, 7), seed=3)
    mn, _ = cohort_io.read_tables(str(tmp_path / "n"))
    mp, _ = cohort_io.read_tables(str(tmp_path / "p"))
    kinds = set()
    for a, b in zip(mn["nifti_path"], mp["nifti_path"]):
        assert isinstance(a, str) == isinstance(b, str)
        if isinstance(a, str):
            assert a.endswith(".nii.gz") and b.endswith(".npy")
            p = NR.parse(a)
            kinds.add((p["datatype"], p["endian"]))
            assert p["data"].shape == (5, 6, 7) and np.array_equal(NR.scaled(p), np.rint(np.load(b).astype(np.float64)))
            assert p["sform_code"] == 1 and p["affine"][2, 2] > p["affine"][0, 0] > 0
    assert kinds == {(4, "<"), (4, ">"), (16, "<"), (512, "<")}
    with pytest.raises(ValueError):
        cohort_io.write_cohort(str(tmp_path / "x"), c, volume_format="dcm")
