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
