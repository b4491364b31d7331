"""float64 numpy restatement of the elastic-deformation contract (include/mmsurv.h: ElaRec / ElaP) -- the reference
the tests compare mms_elastic_field and mms_gather_elastic_group against.  Written from the contract, not from the package: it imports
nothing of it (only the sibling reference of the affine contract, whose sampling it continues).

A row is (amp[3], seed) over a lattice of spacing s_a = 1 << l_a voxels along axis a of a volume of extents n = (D, H, W):
  K_a = ((n_a - 1) >> l_a) + 4 control planes, plane j at lattice position j - 1;
  control value of component a at (jz, jy, jx), k = 3 ((jz K_H + jy) K_W + jx) + a:
      c = float32(amp_a) * u(seed, k) rounded ONCE to fp32,  u = (int(h >> 8) - 8388608) * 2^-23,
      h = hash(k * 0x9E3779B9 + hash(seed ^ 0x85ebca6b)) in uint32 arithmetic, hash the mixer of augment_affine_ref;
  displacement at voxel p: k_a = p_a >> l_a, r_a = (p_a & (s_a - 1)) / s_a,
      d_a = sum_{i,j,m} B_i(r_z) B_j(r_y) B_m(r_x) c_a[k_z + i, k_y + j, k_x + m]   (uniform cubic B-spline basis), in float64;
  source coordinate = m (p + d, 1), then everything of the affine contract.
"""
import numpy as np

import augment_affine_ref as R

SALT = 0x85ebca6b


def u(seed, k):
    """-> float64 array of u(seed, k), k an integer array: multiples of 2^-23 in [-1, 1)."""
    with np.errstate(over="ignore"):
        hs = R._hash(np.array([(seed ^ SALT) & 0xFFFFFFFF], dtype=np.uint32))
        h = R._hash(np.asarray(k).astype(np.uint32) * np.uint32(0x9E3779B9) + hs)
    return ((h >> np.uint32(8)).astype(np.int64) - 8388608).astype(np.float64) * 2.0 ** -23


def lattice_shape(dims, l):
    return tuple(((int(n) - 1) >> int(la)) + 4 for n, la in zip(dims, l))


def lattice(dims, l, amp, seed):
    """-> c float64 [3, K_D, K_H, K_W]: the control values, each the fp32 product of the contract."""
    K = lattice_shape(dims, l)
    k = 3 * np.arange(K[0] * K[1] * K[2], dtype=np.int64).reshape(K)
    out = np.empty((3,) + K)
    for a in range(3):
        out[a] = (np.float32(amp[a]) * u(seed, k + a).astype(np.float32)).astype(np.float64)       # (u is exact in fp32)
    return out


def basis(r):
    """-> [..., 4]: B_0 .. B_3 at r."""
    r = np.asarray(r, dtype=np.float64)
    return np.stack([(1 - r) ** 3, 3 * r ** 3 - 6 * r ** 2 + 4, -3 * r ** 3 + 3 * r ** 2 + 3 * r + 1, r ** 3], -1) / 6.0


def basis_prime(r):
    """-> [..., 4]: dB_i / dr."""
    r = np.asarray(r, dtype=np.float64)
    return np.stack([-3 * (1 - r) ** 2, 9 * r ** 2 - 12 * r, -9 * r ** 2 + 6 * r + 3, 3 * r ** 2], -1) / 6.0


def _weights(n, K, la, prime=False):
    """-> W [n, K]: W[p, (p >> l) + i] = B_i(r_p)  (or dB_i/dp = B_i'(r_p) / s)."""
    s = 1 << la
    p = np.arange(n)
    r = (p & (s - 1)) / float(s)
    b = basis_prime(r) / s if prime else basis(r)
    W = np.zeros((n, K))
    for i in range(4):
        W[p, (p >> la) + i] = b[:, i]
    return W


def field(dims, l, amp, seed, c=None):
    """-> d float64 [3, D, H, W].  c: a lattice to use instead of the hashed one (worst-case lattices of the folding check)."""
    c = lattice(dims, l, amp, seed) if c is None else c
    Ws = [_weights(n, K, la) for n, K, la in zip(dims, c.shape[1:], l)]
    return np.einsum("zi,yj,xm,aijm->azyx", Ws[0], Ws[1], Ws[2], c)


def jacobian_det(dims, l, c):
    """det(I + dd/dp) of the map p -> p + d(p) at every voxel, from the analytic derivative of the spline -> [D, H, W]."""
    W = [_weights(n, K, la) for n, K, la in zip(dims, c.shape[1:], l)]
    Wp = [_weights(n, K, la, prime=True) for n, K, la in zip(dims, c.shape[1:], l)]
    J = np.zeros(tuple(dims) + (3, 3))
    for b in range(3):                       # derivative along axis b
        ws = [Wp[a] if a == b else W[a] for a in range(3)]
        J[..., :, b] = np.moveaxis(np.einsum("zi,yj,xm,aijm->azyx", ws[0], ws[1], ws[2], c), 0, -1)
    return np.linalg.det(J + np.eye(3))


def coords(m, dims, d):
    """The affine contract's source coordinates of the DEFORMED destination grid p + d -> (cz, cy, cx)."""
    D, H, W = dims
    m = np.asarray(m, dtype=np.float64).reshape(3, 4)
    z, y, x = np.meshgrid(np.arange(D, dtype=np.float64), np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    z, y, x = z + d[0], y + d[1], x + d[2]
    return tuple(m[a, 0] * z + m[a, 1] * y + m[a, 2] * x + m[a, 3] for a in range(3))


def elastic_volume(vol, m, l, amp, seed, scale=1.0, offset=0.0, sigma=0.0, noise_seed=0):
    """vol [D, H, W] -> float64 [D, H, W]: the contract's output before its rounding to fp32 (amp, scale, offset, sigma at their fp32
    values: the records hold fp32).  The noise is indexed by the destination voxel."""
    vol = np.asarray(vol)
    d = field(vol.shape, l, [float(np.float32(a)) for a in amp], seed)
    v = R.trilinear_zero(vol, *coords(np.asarray(m, dtype=np.float32), vol.shape, d))
    out = float(np.float32(scale)) * v + float(np.float32(offset))
    if sigma != 0:
        out = out + float(np.float32(sigma)) * R.noise(noise_seed, vol.size).astype(np.float64).reshape(vol.shape)
    return out
