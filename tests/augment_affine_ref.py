"""float64 numpy restatement of the resampling-augmentation contract (include/mmsurv.h: AffRec) -- the reference
the tests compare mms_gather_affine_group against.  Written from the contract, not from the package: it imports nothing of it.

A row is (m, scale, offset, sigma, seed), m a 3 x 4 matrix:
  source coordinate  (cz, cy, cx) = m (z, y, x, 1) in voxel-index units;
  v = trilinear sample of src there: cell = floor(c), upper weight = c - floor(c), corners outside the volume count as 0;
  out = sigma * g(seed, i) + scale * v + offset,  i = (z H + y) W + x;
  g: h0 = mix(seed, 2i), h1 = mix(seed, 2i + 1) in uint32, mix(s, k) = hash(k * 0x9E3779B9 + hash(s)),
     hash(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16;
     S = sum of the eight bytes of h0, h1;  g = float32(S - 1020) * float32(1 / sqrt(43690)).
"""
import numpy as np

G_SCALE = np.float32(1.0 / np.sqrt(43690.0))
G_MAX = 1020.0 / np.sqrt(43690.0)            # 4.8799...


def _hash(x):
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def byte_sums(seed, n):
    """-> int64 [n]: S of voxel 0..n-1."""
    with np.errstate(over="ignore"):
        hs = _hash(np.array([seed & 0xFFFFFFFF], dtype=np.uint32))
        i = np.arange(n, dtype=np.uint32)
        S = np.zeros(n, dtype=np.int64)
        for k in (np.uint32(2) * i, np.uint32(2) * i + np.uint32(1)):
            h = _hash(k * np.uint32(0x9E3779B9) + hs)
            for sh in (0, 8, 16, 24):
                S += ((h >> np.uint32(sh)) & np.uint32(0xFF)).astype(np.int64)
    return S


def noise(seed, n):
    """-> float32 [n]: g(seed, i) bit for bit."""
    return (byte_sums(seed, n) - 1020).astype(np.float32) * G_SCALE


def coords(m, dims):
    """-> (cz, cy, cx), float64 [D, H, W] each."""
    D, H, W = dims
    m = np.asarray(m, dtype=np.float64).reshape(3, 4)
    z, y, x = np.meshgrid(np.arange(D, dtype=np.float64), np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return tuple(m[a, 0] * z + m[a, 1] * y + m[a, 2] * x + m[a, 3] for a in range(3))


def trilinear_zero(vol, cz, cy, cx):
    """Trilinear sample of vol [D, H, W] at the coordinate arrays, zero padding, float64.  A NaN coordinate samples air."""
    vol = np.asarray(vol, dtype=np.float64)
    D, H, W = vol.shape
    pad = np.zeros((D + 2, H + 2, W + 2))
    pad[1:-1, 1:-1, 1:-1] = vol
    ok = np.isfinite(cz) & np.isfinite(cy) & np.isfinite(cx)
    cl = lambda c, n: np.clip(np.where(ok, c, -2.0), -2.0, n + 1.0)           # beyond (-1, n) every corner is air anyway
    cz, cy, cx = cl(cz, D), cl(cy, H), cl(cx, W)
    fz, fy, fx = np.floor(cz), np.floor(cy), np.floor(cx)
    wz, wy, wx = cz - fz, cy - fy, cx - fx
    out = np.zeros(cz.shape)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                iz, iy, ix = fz.astype(np.int64) + dz, fy.astype(np.int64) + dy, fx.astype(np.int64) + dx
                inside = (iz >= 0) & (iz < D) & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
                v = pad[np.clip(iz + 1, 0, D + 1), np.clip(iy + 1, 0, H + 1), np.clip(ix + 1, 0, W + 1)]
                w = (wz if dz else 1 - wz) * (wy if dy else 1 - wy) * (wx if dx else 1 - wx)
                out += np.where(inside, w * v, 0.0)
    return out


def affine_volume(vol, m, scale=1.0, offset=0.0, sigma=0.0, seed=0):
    """vol [D, H, W] -> float64 [D, H, W]: the contract's output before its rounding to fp32.  scale / offset / sigma are taken at
    their fp32 values (the records hold fp32)."""
    vol = np.asarray(vol)
    v = trilinear_zero(vol, *coords(np.asarray(m, dtype=np.float32), vol.shape))
    out = float(np.float32(scale)) * v + float(np.float32(offset))
    if sigma != 0:
        out = out + float(np.float32(sigma)) * noise(seed, vol.size).astype(np.float64).reshape(vol.shape)
    return out
