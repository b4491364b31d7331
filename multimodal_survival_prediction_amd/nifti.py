"""Single-file NIfTI-1 (`n+1`) reader and writer on numpy and zlib alone (host only).

The reference's datasets read `.nii.gz` volumes with SimpleITK (partial_modality_training.py:91-109, simple_fusion.py:117-134,
flexible_multimodal.py:115-128) and take `D, H, W = img_np.shape` of GetArrayFromImage, i.e. the stored array with the index order
reversed: (nz, ny, nx), x fastest, no reorientation.  `read_nifti` returns exactly that array in its STORED dtype and byte order
(`header["swap"]` says whether the bytes are in the other order than the host's): the GPU loader (cohort_io, csrc/ct_ingest.hip)
converts, byte-swaps and scales on the device.

The format (NIfTI-1 specification, nifti1.h): a 348-byte header -- sizeof_hdr at 0, dim[8] at 40, datatype at 70, bitpix at 72,
pixdim[8] at 76, vox_offset at 108, scl_slope at 112, scl_inter at 116, qform_code at 252, sform_code at 254, quatern_b/c/d at 256,
qoffset_x/y/z at 268, srow_x/y/z at 280, magic at 344 -- four extension-flag bytes, optional extensions, then the raw array at
vox_offset; the whole file optionally gzipped.  The byte order is whichever makes sizeof_hdr read 348.

Not supported, refused with a ValueError naming the file and the field: NIfTI-2, two-file (`ni1`) and Analyze images, RGB / complex /
float128 / 64-bit integer datatypes, data of more than three non-trivial dimensions."""
import os
import struct
import sys
import zlib

import numpy as np

HEADER_BYTES = 348
DATA_OFFSET = 352                      # header + the four extension-flag bytes: the smallest vox_offset of an n+1 file
# NIfTI datatype code -> (numpy kind + size, bitpix); the codes are also the dtype codes of mms_ct_preprocess_raw_batch (MMS_CT_*)
DTYPES = {2: ("u1", 8), 4: ("i2", 16), 8: ("i4", 32), 16: ("f4", 32), 64: ("f8", 64), 256: ("i1", 8), 512: ("u2", 16), 768: ("u4", 32)}
CODE_OF = {np.dtype(k).newbyteorder("=").str[1:]: c for c, (k, _) in DTYPES.items()}
_UNSUPPORTED = {0: "unknown", 1: "binary", 32: "complex64", 128: "RGB24", 1024: "int64", 1280: "uint64", 1536: "float128",
                1792: "complex128", 2048: "complex256", 2304: "RGBA32"}
_NATIVE = "<" if sys.byteorder == "little" else ">"


def _is_gz(path):
    return str(path).lower().endswith(".gz")


def dtype_code(dtype):
    """numpy dtype (either byte order) -> NIfTI datatype code = MMS_CT_* code; KeyError for a type the format subset lacks."""
    return CODE_OF[np.dtype(dtype).str[1:]]


def parse_header(buf, name="<bytes>"):
    """The first 348 (or more) bytes of a file -> header dict.  Raises ValueError naming `name` and the offending field."""
    def bad(field, why):
        return ValueError("%s: %s: %s" % (name, field, why))
    if len(buf) < HEADER_BYTES:
        raise bad("sizeof_hdr", "file holds %d bytes, a NIfTI-1 header has 348" % len(buf))
    for e in "<>":
        size = struct.unpack_from(e + "i", buf, 0)[0]
        if size == 348:
            break
        if size == 540:
            raise bad("sizeof_hdr", "540 = NIfTI-2, not supported")
    else:
        raise bad("sizeof_hdr", "%d in neither byte order is 348: not a NIfTI-1 file" % struct.unpack_from("<i", buf, 0)[0])
    dim = struct.unpack_from(e + "8h", buf, 40)
    if not 1 <= dim[0] <= 7:
        raise bad("dim[0]", "%d is outside 1..7" % dim[0])
    magic = bytes(buf[344:348])
    if magic == b"ni1\0":
        raise bad("magic", "'ni1' = two-file image (.hdr/.img), not supported")
    if magic != b"n+1\0":
        raise bad("magic", "%r is not 'n+1' (Analyze 7.5 or not NIfTI)" % magic)
    datatype, bitpix = struct.unpack_from(e + "2h", buf, 70)
    if datatype not in DTYPES:
        raise bad("datatype", "%d (%s) is not supported" % (datatype, _UNSUPPORTED.get(datatype, "not a NIfTI-1 code")))
    if bitpix != DTYPES[datatype][1]:
        raise bad("bitpix", "%d disagrees with datatype %d (%d bits)" % (bitpix, datatype, DTYPES[datatype][1]))
    if dim[0] < 3:
        raise bad("dim[0]", "%d: a volume has three dimensions" % dim[0])
    if any(d < 1 for d in dim[1:4]):
        raise bad("dim", "%s: non-positive extent" % (dim[1:4],))
    if any(d != 1 for d in dim[4:dim[0] + 1]):
        raise bad("dim", "%s: data of more than three dimensions (4-D series) is not supported" % (dim[1:dim[0] + 1],))
    pixdim = struct.unpack_from(e + "8f", buf, 76)
    vox_offset, slope, inter = struct.unpack_from(e + "3f", buf, 108)
    if not (vox_offset >= DATA_OFFSET and vox_offset == int(vox_offset)):
        raise bad("vox_offset", "%r: the data of an n+1 file starts at byte 352 or later" % vox_offset)
    qform_code, sform_code = struct.unpack_from(e + "2h", buf, 252)
    dtype = np.dtype(e + DTYPES[datatype][0]) if DTYPES[datatype][1] > 8 else np.dtype(DTYPES[datatype][0])
    return dict(sizeof_hdr=348, endian=e, swap=(e != _NATIVE and bitpix > 8), dim=tuple(dim), datatype=datatype, bitpix=bitpix,
                dtype=dtype, shape=(dim[3], dim[2], dim[1]), pixdim=tuple(pixdim), vox_offset=int(vox_offset),
                scl_slope=slope, scl_inter=inter, qform_code=qform_code, sform_code=sform_code,
                quatern=struct.unpack_from(e + "3f", buf, 256), qoffset=struct.unpack_from(e + "3f", buf, 268),
                srow=np.array(struct.unpack_from(e + "12f", buf, 280), dtype=np.float64).reshape(3, 4), magic=magic)


def data_bytes(header):
    nz, ny, nx = header["shape"]
    return nz * ny * nx * header["bitpix"] // 8


def scaling(header):
    """-> (slope, inter) to apply to the stored values; scl_slope 0 (or a non-finite pair) means 'no scaling' (1, 0)."""
    s, i = float(header["scl_slope"]), float(header["scl_inter"])
    if s == 0.0 or not np.isfinite(s) or not np.isfinite(i):
        return 1.0, 0.0
    return s, i


def _inflate_prefix(comp, n, name):
    """the first n bytes of a gzip stream (fewer if it ends)"""
    try:
        return zlib.decompressobj(31).decompress(comp, n)
    except zlib.error as e:
        raise ValueError("%s: gzip stream: %s" % (name, e))


def read_header(path_or_bytes):
    """path of a .nii / .nii.gz file, or the (uncompressed) bytes of one -> header dict"""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return parse_header(bytes(path_or_bytes[:HEADER_BYTES]))
    path = os.fspath(path_or_bytes)
    with open(path, "rb") as f:
        head = _inflate_prefix(f.read(65536), HEADER_BYTES, path) if _is_gz(path) else f.read(HEADER_BYTES)
    return parse_header(head, path)


def read_into(path, header, dest):
    """The data section of `path` (whose header is `header`) into dest, a writable C-contiguous uint8 array of data_bytes(header)
    bytes -- e.g. a slot of a pinned staging buffer: gzip members are inflated piecewise straight into it (zlib releases the GIL), an
    uncompressed file is read into it.  ValueError if the file ends early."""
    need, skip = data_bytes(header), header["vox_offset"]
    assert dest.dtype == np.uint8 and dest.size == need
    got = 0
    with open(path, "rb") as f:
        if not _is_gz(path):
            f.seek(skip)
            got = f.readinto(memoryview(dest)) or 0
        else:
            comp = f.read()
            d = zlib.decompressobj(31)
            try:
                while got < need:
                    piece = d.decompress(comp, (skip if skip else min(need - got, 1 << 22)))
                    comp = d.unconsumed_tail
                    if skip:
                        skip -= len(piece)
                    elif piece:
                        dest[got:got + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
                        got += len(piece)
                    if d.eof:                                   # a further gzip member, if any, continues the file
                        comp = d.unused_data
                        if not comp:
                            break
                        d = zlib.decompressobj(31)
                    elif not piece and not comp:
                        break
            except zlib.error as e:
                raise ValueError("%s: gzip stream: %s" % (path, e))
    if got < need:
        raise ValueError("%s: data: %d bytes after vox_offset %d, dim %s x bitpix %d needs %d (truncated file)"
                         % (path, got, header["vox_offset"], header["dim"][1:4], header["bitpix"], need))


def read_nifti(path):
    """-> (header, raw): raw is the stored array as (nz, ny, nx) in the stored dtype and byte order (SimpleITK's GetArrayFromImage
    order; no reorientation, no scaling: see `scaling`)."""
    path = os.fspath(path)
    header = read_header(path)
    raw = np.empty(data_bytes(header), dtype=np.uint8)
    read_into(path, header, raw)
    return header, raw.view(header["dtype"]).reshape(header["shape"])


def affine_of(header):
    """4 x 4 index-to-world matrix of (i, j, k) = (x, y, z) indices: the sform when sform_code > 0, else the qform quaternion when
    qform_code > 0, else diag(pixdim)."""
    A = np.eye(4)
    pd = header["pixdim"]
    if header["sform_code"] > 0:
        A[:3, :] = header["srow"]
    elif header["qform_code"] > 0:
        b, c, d = (float(v) for v in header["quatern"])
        a = np.sqrt(max(0.0, 1.0 - (b * b + c * c + d * d)))
        R = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                      [2 * (b * c + a * d), a * a + c * c - b * b - d * d, 2 * (c * d - a * b)],
                      [2 * (b * d - a * c), 2 * (c * d + a * b), a * a + d * d - b * b - c * c]])
        qfac = -1.0 if pd[0] < 0 else 1.0
        A[:3, :3] = R * np.array([pd[1], pd[2], pd[3] * qfac], dtype=np.float64)
        A[:3, 3] = header["qoffset"]
    else:
        A[:3, :3] = np.diag([pd[1], pd[2], pd[3]])
    return A


def encode(array, affine=None, endian="<", slope=0.0, inter=0.0):
    """(nz, ny, nx) array of one of the eight supported dtypes -> the bytes of an uncompressed n+1 file in the given byte order."""
    a = np.asarray(array)
    if a.ndim != 3:
        raise ValueError("write_nifti: a volume has three dimensions, got shape %s" % (a.shape,))
    code = dtype_code(a.dtype)
    A = np.eye(4) if affine is None else np.asarray(affine, dtype=np.float64)
    if A.shape != (4, 4):
        raise ValueError("write_nifti: affine must be 4 x 4")
    nz, ny, nx = a.shape
    if max(a.shape) > 32767:
        raise ValueError("write_nifti: dim %s does not fit the header's int16" % (a.shape,))
    h = bytearray(DATA_OFFSET)
    e = endian
    struct.pack_into(e + "i", h, 0, 348)
    struct.pack_into(e + "8h", h, 40, 3, nx, ny, nz, 1, 1, 1, 1)
    struct.pack_into(e + "2h", h, 70, code, DTYPES[code][1])
    struct.pack_into(e + "8f", h, 76, 1.0, *np.linalg.norm(A[:3, :3], axis=0), 0.0, 0.0, 0.0, 0.0)
    struct.pack_into(e + "3f", h, 108, float(DATA_OFFSET), slope, inter)
    h[123] = 2                                                   # xyzt_units: millimetres
    struct.pack_into(e + "2h", h, 252, 0, 1)                     # qform_code 0, sform_code 1 (scanner anatomical)
    struct.pack_into(e + "12f", h, 280, *A[:3, :].reshape(-1))
    h[344:348] = b"n+1\0"
    return bytes(h) + np.ascontiguousarray(a, dtype=a.dtype.newbyteorder(e)).tobytes()


def dump(path, blob):
    if _is_gz(path):
        co = zlib.compressobj(6, zlib.DEFLATED, 31)
        blob = co.compress(blob) + co.flush()
    with open(path, "wb") as f:
        f.write(blob)


def write_nifti(path, array, affine=None, like=None):
    """Write a float32 or int16 (nz, ny, nx) volume as little-endian n+1 with vox_offset 352, sform_code 1 = affine and pixdim = the
    affine's column norms; gzipped when the path ends in .gz.  like: a header whose geometry (affine_of) is taken when affine is None."""
    a = np.asarray(array)
    if a.dtype.newbyteorder("=") not in (np.dtype(np.float32), np.dtype(np.int16)):
        raise ValueError("write_nifti writes float32 or int16 volumes, got %s" % a.dtype)
    if affine is None and like is not None:
        affine = affine_of(like)
    dump(os.fspath(path), encode(a, affine))


def saliency_affine(src_affine, native_dims, target_dims):
    """Index-to-world matrix of a volume on the network grid target_dims = (tD, tH, tW) that the loader's align-corners resample made
    from a scan of native_dims = (nz, ny, nx) with matrix src_affine: A_src . diag(sx, sy, sz, 1) in NIfTI index order (x, y, z), per axis
    s = (native - 1) / (target - 1), 1 where target == 1 -- target index 0 is native index 0 and the last is the last, so the map
    overlays the scan.  src_affine None: identity."""
    if src_affine is None or native_dims is None:
        return np.eye(4)
    s = [(n - 1) / (t - 1) if t > 1 else 1.0 for n, t in zip(native_dims, target_dims)]          # (z, y, x)
    return np.asarray(src_affine, dtype=np.float64) @ np.diag([s[2], s[1], s[0], 1.0])
