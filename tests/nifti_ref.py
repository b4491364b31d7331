"""Test-side NIfTI-1 files, written and parsed with struct at the byte offsets the specification (nifti1.h) publishes -- independent of
multimodal_survival_prediction_amd/nifti.py, with which this file shares no code.  Neither SimpleITK nor nibabel is available to the
suite, so the specification is the parity anchor of the format:
    sizeof_hdr int32 @0, dim[8] int16 @40, datatype int16 @70, bitpix int16 @72, pixdim[8] float32 @76, vox_offset float32 @108,
    scl_slope @112, scl_inter @116, qform_code int16 @252, sform_code int16 @254, quatern_b/c/d float32 @256/260/264,
    qoffset_x/y/z @268/272/276, srow_x/y/z 4 x float32 @280/296/312, magic @344; data at vox_offset, x fastest."""
import gzip
import struct

import numpy as np

# datatype code -> (struct / numpy letter, bits)
TYPES = {2: ("u1", 8), 4: ("i2", 16), 8: ("i4", 32), 16: ("f4", 32), 64: ("f8", 64), 256: ("i1", 8), 512: ("u2", 16), 768: ("u4", 32)}


def build(array, datatype, endian="<", vox_offset=352, slope=0.0, inter=0.0, dim=None, sizeof_hdr=348, magic=b"n+1\0", bitpix=None,
          sform=None, qform=None, pixdim=(1.0, 1.0, 1.0), data_bytes=None):
    """array: (nz, ny, nx) values -> bytes of an uncompressed file whose data are the values as `datatype` in byte order `endian`.
    dim: the 8 header entries (default: 3, nx, ny, nz, 1, 1, 1, 1).  sform: 3 x 4 rows (sform_code 1).  qform: (b, c, d, ox, oy, oz, qfac)
    (qform_code 1).  Bytes 348..vox_offset are an extension flag + filler.  data_bytes: cut the data section to that many bytes."""
    a = np.asarray(array)
    nz, ny, nx = a.shape
    h = bytearray(348)
    struct.pack_into(endian + "i", h, 0, sizeof_hdr)
    struct.pack_into(endian + "8h", h, 40, *(dim or (3, nx, ny, nz, 1, 1, 1, 1)))
    struct.pack_into(endian + "h", h, 70, datatype)
    struct.pack_into(endian + "h", h, 72, TYPES[datatype][1] if bitpix is None else bitpix)
    qfac = qform[6] if qform is not None else 1.0
    struct.pack_into(endian + "8f", h, 76, qfac, pixdim[0], pixdim[1], pixdim[2], 0, 0, 0, 0)
    struct.pack_into(endian + "f", h, 108, float(vox_offset))
    struct.pack_into(endian + "f", h, 112, slope)
    struct.pack_into(endian + "f", h, 116, inter)
    struct.pack_into(endian + "h", h, 252, 1 if qform is not None else 0)
    struct.pack_into(endian + "h", h, 254, 1 if sform is not None else 0)
    if qform is not None:
        struct.pack_into(endian + "3f", h, 256, *qform[:3])
        struct.pack_into(endian + "3f", h, 268, *qform[3:6])
    if sform is not None:
        for r in range(3):
            struct.pack_into(endian + "4f", h, 280 + 16 * r, *sform[r])
    h[344:348] = magic
    ext = bytearray(int(vox_offset) - 348)
    if len(ext) > 4:
        ext[0] = 1                                      # extension flag; the extension's bytes are filler that must be skipped
        ext[4:] = b"\xa5" * (len(ext) - 4)
    letter = TYPES.get(datatype, ("u1", 8))[0]
    data = a.astype(np.dtype(endian + letter) if letter[1] != "1" else np.dtype(letter)).tobytes()
    if data_bytes is not None:
        data = data[:data_bytes]
    return bytes(h) + bytes(ext) + data


def save(path, blob):
    """as is, or gzipped when the name ends in .gz"""
    if str(path).endswith(".gz"):
        blob = gzip.compress(blob, 1)
    with open(path, "wb") as f:
        f.write(blob)
    return str(path)


def parse(path_or_bytes):
    """-> dict(data (nz, ny, nx) in the host's byte order, datatype, slope, inter (as stored), affine (sform rows, if sform_code > 0),
    vox_offset, sform_code, pixdim, endian)"""
    if isinstance(path_or_bytes, bytes):
        blob = path_or_bytes
    else:
        with open(path_or_bytes, "rb") as f:
            blob = f.read()
        if str(path_or_bytes).endswith(".gz"):
            blob = gzip.decompress(blob)
    endian = "<" if struct.unpack_from("<i", blob, 0)[0] == 348 else ">"
    assert struct.unpack_from(endian + "i", blob, 0)[0] == 348 and blob[344:348] == b"n+1\0"
    dim = struct.unpack_from(endian + "8h", blob, 40)
    datatype, bitpix = struct.unpack_from(endian + "h", blob, 70)[0], struct.unpack_from(endian + "h", blob, 72)[0]
    letter, bits = TYPES[datatype]
    assert bits == bitpix
    off = int(struct.unpack_from(endian + "f", blob, 108)[0])
    n = dim[1] * dim[2] * dim[3]
    dt = np.dtype(endian + letter) if bits > 8 else np.dtype(letter)
    raw = blob[off:off + n * bits // 8]
    data = np.frombuffer(raw, dtype=dt).reshape(dim[3], dim[2], dim[1])
    affine = np.eye(4)
    sform_code = struct.unpack_from(endian + "h", blob, 254)[0]
    if sform_code > 0:
        for r in range(3):
            affine[r] = struct.unpack_from(endian + "4f", blob, 280 + 16 * r)
    return dict(data=data.astype(dt.newbyteorder("=")), raw_bytes=raw, datatype=datatype, endian=endian, vox_offset=off, dim=dim,
                slope=struct.unpack_from(endian + "f", blob, 112)[0], inter=struct.unpack_from(endian + "f", blob, 116)[0],
                sform_code=sform_code, affine=affine, pixdim=struct.unpack_from(endian + "8f", blob, 76))


def scaled(p):
    """the values a parsed file stands for, fp64: slope * stored + inter, slope 0 = no scaling"""
    s, i = (1.0, 0.0) if p["slope"] == 0 else (float(p["slope"]), float(p["inter"]))
    return s * p["data"].astype(np.float64) + i


def ct_values(shape, datatype, seed):
    """integer values of a CT-like range (-1024 .. 3071; shifted into range for the unsigned and 8-bit types) as the datatype's numpy type"""
    rng = np.random.default_rng(seed)
    letter = TYPES[datatype][0]
    if letter == "u1":
        v = rng.integers(0, 256, size=shape)
    elif letter == "i1":
        v = rng.integers(-128, 128, size=shape)
    elif letter[0] == "u":
        v = rng.integers(0, 4096, size=shape)
    else:
        v = rng.integers(-1024, 3072, size=shape)
    return v.astype(np.dtype(letter))


def full_range_values(shape, datatype, seed):
    """values that reach the ends of the stored type, so that its signedness and width matter, as the datatype's numpy type:
    u1 / i1 / i2 the whole range with both ends present; u2 [30000, 65535] with both ends (either side of 2^15); u4 2^31 + 256 k,
    |k| < 2^20 (either side of 2^31 and exact in fp32: below 2^32 its spacing is at most 256); i4 integers of [-2^24, 2^24] with both
    ends; f4 HU + U[0, 1) rounded to fp32, f8 the same fp32 values widened."""
    rng = np.random.default_rng(seed)
    letter = TYPES[datatype][0]
    ends = None
    if letter[0] == "f":
        v = (rng.integers(-1024, 3072, size=shape) + rng.random(shape)).astype(np.float32)
    elif letter == "u4":
        v = 2 ** 31 + 256 * rng.integers(-2 ** 20 + 1, 2 ** 20, size=shape)
        ends = (2 ** 31 - 256 * (2 ** 20 - 1), 2 ** 31 + 256 * (2 ** 20 - 1))
    else:
        ends = {"u1": (0, 255), "i1": (-128, 127), "u2": (30000, 65535), "i2": (-32768, 32767), "i4": (-2 ** 24, 2 ** 24)}[letter]
        v = rng.integers(ends[0], ends[1] + 1, size=shape)
    if ends is not None:
        lo, hi = rng.choice(v.size, size=2, replace=False)
        v.reshape(-1)[lo], v.reshape(-1)[hi] = ends
    return v.astype(np.dtype(letter))


def low_contrast_values(kind, shape, seed):
    """float32 volumes whose contrast is tiny next to their offset -- where normalising AFTER interpolating cancels:
    "two_level" {1000, 1001} (a mask-like scan), "sub_ulp" 1000 + U[0, 1e-3) rounded to fp32 (a few fp32 steps of 1000 apart),
    "four_level" -1024 + {0, 1, 2, 3}"""
    rng = np.random.default_rng(seed)
    if kind == "two_level":
        v = 1000.0 + rng.integers(0, 2, size=shape)
    elif kind == "sub_ulp":
        v = 1000.0 + rng.random(shape) * 1e-3
    elif kind == "four_level":
        v = -1024.0 + rng.integers(0, 4, size=shape)
    else:
        raise ValueError(kind)
    return v.astype(np.float32)


def scan_values(shape, letter, seed, min_at):
    """integer HU values of [-1000, 3000) with the only -1024 at flat index min_at and the only 3071 in the last element: a pass over the
    volume that drops a sweep or the tail gets an extreme wrong and with it every output voxel"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-1000, 3000, size=shape)
    flat = v.reshape(-1)
    assert 0 <= min_at < flat.size - 1
    flat[min_at], flat[-1] = -1024, 3071
    return v.astype(np.dtype(letter))
