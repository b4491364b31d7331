"""CPU: the rot / zoom / noise keys of the augmentation spec, their sampler and the host-side composition of the affine records, the
float64 test reference (augment_affine_ref) against independent implementations, the noise generator's statistics, and the C ABI of
mms_gather_affine_group (no GPU)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import augment_affine_ref as R
from augment_ref import aug_volume

from multimodal_survival_prediction_amd import _build, _lib, augment as A, data

FULL = "flip=0.5,shift=2:4:4,scale=0.9:1.1,offset=-0.05:0.05,moddrop=0.2"
NEW = ",rot=10,zoom=0.9:1.1,noise=0:0.03"


# ---- spec ---------------------------------------------------------------------------------------------------------------------------
def test_spec_parse_and_round_trip():
    s = A.AugmentSpec.parse(FULL + NEW)
    assert s.rot_max == (10.0, 10.0, 10.0) and s.zoom_range == (0.9, 1.1) and s.noise_range == (0.0, 0.03) and s.has_affine
    assert s.flip_p == (0.5, 0.5, 0.5) and s.max_shift == (2, 4, 4)
    assert A.AugmentSpec.parse(str(s)) == s
    t = A.AugmentSpec.parse("rot=10:0:0")
    assert t.rot_max == (10.0, 0.0, 0.0) and t.zoom_range == (1.0, 1.0) and t.has_affine and A.AugmentSpec.parse(str(t)) == t
    for text in ("zoom=0.8:0.8", "noise=0.01:0.01", "rot=0:0:5,seed=3"):
        u = A.AugmentSpec.parse(text)
        assert u.has_affine and A.AugmentSpec.parse(str(u)) == u
    old = A.AugmentSpec.parse(FULL)
    assert not old.has_affine and not A.AugmentSpec.parse("rot=0,zoom=1:1,noise=0:0").has_affine
    assert "rot" not in str(old) and "zoom" not in str(old) and "noise" not in str(old)      # prints as it always did


@pytest.mark.parametrize("bad", ["rot=-1", "rot=1:2", "rot=x", "zoom=1.1:0.9", "zoom=0:1", "zoom=-1:1", "zoom=1", "noise=-0.1:0.1",
                                 "noise=0.2:0.1", "noise=0.1", "rot=5,rot=5", "rot=nan", "zoom=1:inf"])
def test_spec_parse_errors(bad):
    with pytest.raises(ValueError):
        A.AugmentSpec.parse(bad)


def _cohort():
    return data.make_cohort(n=48, dims=(8, 8, 8), rna_dim=8, seed=3, complete=False)


def test_new_keys_leave_the_old_draws_alone():
    c = _cohort()
    old, new = A.AugmentSpec.parse(FULL), A.AugmentSpec.parse(FULL + NEW)
    g0, g1, g2 = (torch.Generator().manual_seed(5) for _ in range(3))
    r_old = A.sample_records(old, g0, c["mask"], c["dims"], "partial")
    r_new = A.sample_records(new, g1, c["mask"], c["dims"], "partial")
    assert torch.equal(r_old, r_new)                          # flip / shift / scale / offset / drop: the same draws
    recs, aff = A.sample(new, g2, c["mask"], c["dims"], "partial")
    assert aff.shape == (48, A.AFF_WORDS) and aff.dtype == torch.int32
    assert torch.equal(recs[:, A.SCALE:], r_old[:, A.SCALE:])
    assert not bool(recs[:, A.FLIP:A.DX + 1].any()) and bool(r_old[:, A.FLIP:A.DX + 1].any())      # handed on with flip / shift zeroed
    A.check_affine_records(aff, 48)
    f = aff.view(torch.float32)
    assert float(f[:, A.AFF_SIGMA].min()) >= 0 and float(f[:, A.AFF_SIGMA].max()) <= 0.03 + 1e-9
    assert len(set(aff[:, A.AFF_SEED].tolist())) > 40         # a seed per row
    # the matrices are A S with A = R^T / zoom: |det| = zoom^-3 within the zoom range
    det = np.abs(np.linalg.det(f[:, :12].double().numpy().reshape(-1, 3, 4)[:, :, :3]))
    assert det.min() >= 1.1 ** -3 - 1e-5 and det.max() <= 0.9 ** -3 + 1e-5


def test_a_spec_without_the_new_keys_draws_once():
    c = _cohort()
    g, h = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    recs, aff = A.sample(A.AugmentSpec.parse(FULL), g, c["mask"], c["dims"], "partial")
    torch.rand(48, 12, generator=h)
    assert aff is None and torch.equal(g.get_state(), h.get_state())
    A.sample(A.AugmentSpec.parse(FULL + NEW), g, c["mask"], c["dims"], "partial")
    torch.rand(48, 12, generator=h)
    assert not torch.equal(g.get_state(), h.get_state())
    torch.rand(48, 8, generator=h)                            # ... and the second call is 8 wide
    assert torch.equal(g.get_state(), h.get_state())


def test_loaders_carry_the_second_record():
    c = _cohort()
    mk = lambda spec: data.BatchLoader(c, torch.arange(48), 4, shuffle=True, seed=5, lazy=True, augment=spec, augment_style="partial")
    a, b = list(mk(FULL + NEW)), list(mk(FULL))
    assert all(x["augment"].aff is not None and x["augment"].aff.shape == (4, A.AFF_WORDS) for x in a)
    assert all(x["augment"].aff is None for x in b)
    assert [x["index"].tolist() for x in a] == [x["index"].tolist() for x in b]
    assert all(torch.equal(x["augment"].rec[:, A.SCALE:], y["augment"].rec[:, A.SCALE:]) for x, y in zip(a, b))
    assert "augment" not in next(iter(mk(FULL + NEW).without_augment()))


def test_check_affine_records():
    ok = A.affine_records(A.identity_records(3), dims=(4, 4, 4))
    A.check_affine_records(ok, 3)
    with pytest.raises(ValueError):
        A.check_affine_records(ok, 4)
    with pytest.raises(ValueError):
        A.check_affine_records(ok[:, :8])
    with pytest.raises(ValueError):
        A.check_affine_records(ok.float())
    for col, val in ((5, float("nan")), (0, float("inf")), (A.AFF_SIGMA, -0.1), (A.AFF_SIGMA, float("nan"))):
        bad = ok.clone()
        bad.view(torch.float32)[1, col] = val
        with pytest.raises(ValueError):
            A.check_affine_records(bad)


# ---- the reference against independent implementations -------------------------------------------------------------------------------
def _random_matrix(rng, dims):
    ang = rng.uniform(-30, 30, 3)
    A3 = A.rotation(ang[None])[0].T / rng.uniform(0.6, 1.5)
    c = (np.asarray(dims) - 1) / 2
    return np.concatenate([A3, (c - A3 @ c + rng.uniform(-3, 3, 3))[:, None]], 1)


def test_reference_reproduces_a_linear_ramp():
    """Trilinear interpolation reproduces linear functions: wherever the whole cell lies inside the volume the sample IS the ramp at
    the source coordinate."""
    dims = (6, 7, 9)
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dims], indexing="ij")
    a, b, c, d = 0.7, -1.3, 0.45, 2.0
    ramp = a * z + b * y + c * x + d
    rng = np.random.default_rng(0)
    n_in = 0
    for _ in range(6):
        m = _random_matrix(rng, dims)
        cz, cy, cx = R.coords(m, dims)
        got = R.trilinear_zero(ramp, cz, cy, cx)
        inside = (cz >= 0) & (cz <= dims[0] - 1) & (cy >= 0) & (cy <= dims[1] - 1) & (cx >= 0) & (cx <= dims[2] - 1)
        n_in += int(inside.sum())
        assert np.abs(got - (a * cz + b * cy + c * cx + d))[inside].max() <= 1e-12
        far = (cz <= -1) | (cz >= dims[0]) | (cy <= -1) | (cy >= dims[1]) | (cx <= -1) | (cx >= dims[2])
        assert not got[far].any()
    assert n_in > 300


def test_reference_matches_grid_sample_and_scipy():
    dims = (5, 7, 9)
    rng = np.random.default_rng(1)
    vol = rng.uniform(0, 1, dims)
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for _ in range(6):
        m = _random_matrix(rng, dims)
        cz, cy, cx = R.coords(m, dims)
        got = R.trilinear_zero(vol, cz, cy, cx)
        norm = lambda c, n: 2.0 * c / (n - 1) - 1.0
        grid = torch.from_numpy(np.stack([norm(cx, dims[2]), norm(cy, dims[1]), norm(cz, dims[0])], -1))[None]
        ref = torch.nn.functional.grid_sample(torch.from_numpy(vol)[None, None], grid, mode="bilinear", padding_mode="zeros",
                                              align_corners=True)[0, 0].numpy()
        assert np.abs(got - ref).max() <= 1e-12
        assert np.abs(got).max() > 0.1
        if ndimage is not None:
            sp = ndimage.affine_transform(vol, m[:, :3], offset=m[:, 3], order=1, mode="grid-constant", cval=0.0)
            assert np.abs(got - sp).max() <= 1e-12


# ---- composition --------------------------------------------------------------------------------------------------------------------
def _mat(aff, i=0):
    return aff.view(torch.float32)[i, :12].double().numpy().reshape(3, 4)


def test_no_rotation_no_zoom_is_the_integer_map():
    dims = (4, 5, 6)
    vol = torch.rand(dims, generator=torch.Generator().manual_seed(0))
    rows = [(f, s) for f in range(8) for s in ((0, 0, 0), (1, -2, 3), (-3, 4, -5), (3, 0, 0))]
    aff = A.affine_records(A.make_records(len(rows), [f for f, _ in rows], [s for _, s in rows]), dims=dims)
    for i, (f, s) in enumerate(rows):
        m = _mat(aff, i)
        assert np.array_equal(m, np.round(m))                 # integer entries
        got = R.affine_volume(vol.numpy(), m)
        assert np.array_equal(got, aug_volume(vol, f, s, 1.0, 0.0).double().numpy()), (f, s)
    assert np.array_equal(_mat(A.affine_records(A.identity_records(1), dims=dims)), np.eye(3, 4))


def test_quarter_turn_about_d_is_rot90():
    dims = (3, 6, 6)
    vol = torch.rand(dims, generator=torch.Generator().manual_seed(1))
    aff = A.affine_records(A.identity_records(2), angles=[[90.0, 0, 0], [-90.0, 0, 0]], dims=dims)
    assert np.array_equal(_mat(aff, 0), np.round(_mat(aff, 0)))
    assert np.array_equal(R.affine_volume(vol.numpy(), _mat(aff, 0)), torch.rot90(vol, 1, (1, 2)).double().numpy())
    assert np.array_equal(R.affine_volume(vol.numpy(), _mat(aff, 1)), torch.rot90(vol, -1, (1, 2)).double().numpy())


def test_zoom_keeps_the_centre_and_enlarges():
    dims = (5, 7, 9)
    m = _mat(A.affine_records(A.identity_records(1), zoom=2.0, dims=dims))
    c = (np.asarray(dims) - 1) / 2
    assert np.array_equal(m[:, :3] @ c + m[:, 3], c)          # the centre maps to the centre
    assert np.array_equal(m[:, :3], 0.5 * np.eye(3))          # zoom 2: neighbouring outputs are half a source voxel apart -- enlarged
    # the flip / shift act first: with a shift the centre of the SHIFTED grid is what stays
    m2 = _mat(A.affine_records(A.make_records(1, shift=(1, 0, -2)), zoom=2.0, dims=dims))
    assert np.array_equal(m2[:, :3] @ (c + np.array([1, 0, -2])) + m2[:, 3], c)


# ---- noise --------------------------------------------------------------------------------------------------------------------------
def test_noise_statistics():
    """N = 65536 values of unit variance: the sample mean has standard deviation 1/sqrt(N) = 1/256; the sample variance has standard
    deviation sqrt((mu4 - 1)/N) with mu4 = 3 - 1.2/8 = 2.85 for a sum of eight uniforms (excess kurtosis -1.2 each): 0.0053.  Five
    standard deviations each: |mean| <= 0.0196, |var - 1| <= 0.0266."""
    N = 65536
    S = R.byte_sums(1234, N)
    assert S.min() >= 0 and S.max() <= 2040
    g = R.noise(1234, N)
    assert g.dtype == np.float32
    mean, var = float(g.astype(np.float64).mean()), float(g.astype(np.float64).var())
    print("noise mean %.5f var %.5f max|g| %.3f" % (mean, var, float(np.abs(g).max())))
    assert abs(mean) <= 5.0 / 256.0
    assert abs(var - 1.0) <= 5.0 * np.sqrt(1.85 / N)
    assert float(np.abs(g).max()) <= 4.88 and R.G_MAX <= 4.88
    assert float(np.abs(g).max()) > 3.0                        # bell-shaped, not a clipped uniform: tails are reached
    h = R.noise(1235, N)
    assert not np.array_equal(g, h) and abs(float(np.corrcoef(g, h)[0, 1])) <= 5.0 / 256.0
    assert np.array_equal(R.noise(1234, 100), g[:100])        # g(seed, i) does not depend on how many voxels are asked for


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.lib_path()):
        _build.build()
    return _lib.load_library()


def test_abi_exports_the_affine_gather(lib):
    assert "mms_gather_affine_group" in _lib.protos() and hasattr(lib, "mms_gather_affine_group")
    S = _lib.structs()
    for name in ("AffRec", "AffP"):
        assert name in S and lib.mms_abi_sizeof(name.encode()) == ctypes.sizeof(S[name])
    assert ctypes.sizeof(S["AffRec"]) == 64 == 4 * A.AFF_WORDS
    r = A.affine_records(A.make_records(1, flip=4, shift=(1, 0, 0)), angles=[[0.0, 0.0, 20.0]], zoom=1.25, sigma=0.5, seed=0xDEADBEEF,
                         dims=(4, 6, 8))
    rec = S["AffRec"].from_buffer_copy(r.numpy().tobytes())
    assert list(rec.m) == r.view(torch.float32)[0, :12].tolist()
    assert (rec.sigma, rec.seed, list(rec.reserved)) == (0.5, 0xDEADBEEF, [0, 0])
    assert abs(rec.m[10] + 0.8) < 1e-6                        # W flipped, zoom 1.25, rotation about W leaves the x row alone
