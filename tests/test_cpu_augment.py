"""CPU: the augmentation spec, its sampler, the loaders' batch order, the test reference (augment_ref) on hand-checked values, and the
C ABI of mms_gather_aug_group (no GPU)."""
import ctypes
import itertools
import os

import pytest
import torch

from augment_ref import aug_volume

from multimodal_survival_prediction_amd import _build, _lib, augment as A, data

FULL = "flip=0.5,shift=2:4:4,scale=0.9:1.1,offset=-0.05:0.05,moddrop=0.2"


def test_spec_parse_and_round_trip():
    s = A.AugmentSpec.parse(FULL)
    assert s.flip_p == (0.5, 0.5, 0.5) and s.max_shift == (2, 4, 4) and s.scale_range == (0.9, 1.1)
    assert s.offset_range == (-0.05, 0.05) and s.modality_drop_p == 0.2 and s.seed == 0
    assert A.AugmentSpec.parse(str(s)) == s
    t = A.AugmentSpec.parse(" flip=0:0.25:1 , shift=3, seed=7 ")
    assert t.flip_p == (0.0, 0.25, 1.0) and t.max_shift == (3, 3, 3) and t.seed == 7 and t.scale_range == (1.0, 1.0)
    assert A.AugmentSpec.parse(str(t)) == t
    assert A.AugmentSpec.parse("") == A.AugmentSpec()


@pytest.mark.parametrize("bad", ["flip", "rotate=3", "flip=1.5", "shift=1:2", "shift=-1", "scale=1.1:0.9", "scale=1", "moddrop=x",
                                 "flip=0.5,flip=0.5", "moddrop=2"])
def test_spec_parse_errors(bad):
    with pytest.raises(ValueError):
        A.AugmentSpec.parse(bad)


def _cohort():
    return data.make_cohort(n=48, dims=(8, 8, 8), rna_dim=8, seed=3, complete=False)


def test_sampler_is_deterministic():
    c = _cohort()
    spec = A.AugmentSpec.parse(FULL)
    draw = lambda seed: A.sample_records(spec, torch.Generator().manual_seed(seed), c["mask"], c["dims"], "partial")
    assert torch.equal(draw(1), draw(1))
    assert not torch.equal(draw(1), draw(2))
    r = draw(1)
    assert r.shape == (48, A.REC_WORDS) and r.dtype == torch.int32
    assert int(r[:, A.DZ].abs().max()) <= 2 and int(r[:, A.DY].abs().max()) <= 4 and int(r[:, A.DX].abs().max()) <= 4
    f = r.view(torch.float32)
    assert float(f[:, A.SCALE].min()) >= 0.9 and float(f[:, A.SCALE].max()) <= 1.1
    assert float(f[:, A.OFFSET].min()) >= -0.05 and float(f[:, A.OFFSET].max()) <= 0.05
    # the loader's two epochs differ (the generator advances), two loaders with one seed agree
    mk = lambda: data.BatchLoader(c, torch.arange(48), 4, shuffle=True, seed=5, lazy=True, augment=spec, augment_style="partial")
    a, b = mk(), mk()
    e1 = torch.cat([x["augment"].rec for x in a])
    assert torch.equal(e1, torch.cat([x["augment"].rec for x in b]))
    assert not torch.equal(e1, torch.cat([x["augment"].rec for x in a]))


def test_batch_order_is_unchanged_by_a_spec():
    c = _cohort()
    order = lambda **kw: [x["index"].tolist() for _ in range(2) for x in data.BatchLoader(c, torch.arange(48), 4, shuffle=True, seed=11,
                                                                                          lazy=True, **kw)]
    assert order() == order(augment=FULL, augment_style="partial")


def test_sampler_constraints():
    c = _cohort()
    mask = c["mask"]
    spec = A.AugmentSpec(modality_drop_p=0.9, seed=0)
    r = A.sample_records(spec, torch.Generator().manual_seed(0), mask, c["dims"], "partial")
    drop = torch.stack([(r[:, A.DROP] >> j) & 1 for j in range(3)], 1).bool()
    has = mask != 0
    assert not bool((drop & ~has).any())                        # an absent modality is never "dropped"
    left = has & ~drop
    assert bool((left.any(1) == has.any(1)).all())              # nobody loses their last modality
    assert all(int(drop[:, j].sum()) >= 1 for j in range(3))    # the seed exercises every modality
    assert int(drop.all(1).sum()) == 0
    # flexible: the model sees image and rnaseq only
    rf = A.sample_records(spec, torch.Generator().manual_seed(0), mask, c["dims"], "flexible")
    df = torch.stack([(rf[:, A.DROP] >> j) & 1 for j in range(3)], 1).bool()
    assert not bool(df[:, 2].any()) and bool(((has[:, :2] & ~df[:, :2]).any(1) == has[:, :2].any(1)).all())


@pytest.mark.parametrize("style", ["final", "simple", "image", "rnaseq"])
def test_maskless_styles_refuse_moddrop(style):
    c = _cohort()
    with pytest.raises(ValueError, match=style):
        A.AugmentSpec.parse("moddrop=0.2").validate(style)
    with pytest.raises(ValueError, match=style):
        data.BatchLoader(c, torch.arange(8), 4, augment="moddrop=0.2", augment_style=style)
    A.AugmentSpec.parse("flip=0.5,shift=1").validate(style)      # geometry alone is fine


def test_oversized_shift_is_refused():
    c = _cohort()                                                # dims (8, 8, 8)
    with pytest.raises(ValueError, match="max_shift"):
        data.BatchLoader(c, torch.arange(8), 4, augment="shift=0:0:8")
    with pytest.raises(ValueError, match="max_shift"):
        A.sample_records(A.AugmentSpec(max_shift=(8, 0, 0)), torch.Generator(), c["mask"], c["dims"])
    data.BatchLoader(c, torch.arange(8), 4, lazy=True, augment="shift=7:7:7")
    with pytest.raises(ValueError):
        A.check_records(A.make_records(2, shift=(0, 0, -8)), c["dims"])
    with pytest.raises(ValueError):
        A.check_records(A.make_records(2, drop=1), c["dims"], has_mask=False)


def test_materialising_loader_needs_the_cohort_on_the_gpu():
    """A loader that materialises its batches augments them with the kernel: a host-resident cohort is refused when the loader is
    built, not at its first batch; a lazy loader only names batches and records."""
    c = _cohort()
    with pytest.raises(ValueError, match="lazy=True"):
        data.BatchLoader(c, torch.arange(8), 4, augment="flip=0.5")
    assert "augment" in next(iter(data.BatchLoader(c, torch.arange(8), 4, lazy=True, augment="flip=0.5")))


def test_reference_on_a_ramp_volume():
    """augment_ref.aug_volume, hand-checked on the 2 x 3 x 4 ramp v[z,y,x] = 12 z + 4 y + x."""
    v = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    P = -1.0                                                      # offset of the shift cases: padding comes out as P, a voxel v as v - 1
    ident = aug_volume(v, 0, (0, 0, 0), 1.0, 0.0)
    assert torch.equal(ident, v)
    assert aug_volume(v, 4, (0, 0, 0), 1.0, 0.0)[0, 0].tolist() == [3, 2, 1, 0]                  # flip W
    assert aug_volume(v, 2, (0, 0, 0), 1.0, 0.0)[0, :, 0].tolist() == [8, 4, 0]                  # flip H
    assert aug_volume(v, 1, (0, 0, 0), 1.0, 0.0)[:, 0, 0].tolist() == [12, 0]                    # flip D
    assert aug_volume(v, 7, (0, 0, 0), 1.0, 0.0)[0, 0].tolist() == [23, 22, 21, 20]
    pad = lambda s: aug_volume(v, 0, s, 1.0, P)
    assert pad((0, 0, 1))[0, 0].tolist() == [P, -1 + 0, -1 + 1, -1 + 2]                          # out[x] = src[x - 1]; padding = offset
    assert pad((0, 0, -1))[0, 0].tolist() == [0, 1, 2, P]                                        # out[x] = src[x + 1]
    assert pad((0, 1, 0))[0, :, 0].tolist() == [P, -1, 3]
    assert pad((0, -1, 0))[0, :, 0].tolist() == [3, 7, P]
    assert pad((1, 0, 0))[:, 0, 0].tolist() == [P, -1]
    assert pad((-1, 0, 0))[:, 0, 0].tolist() == [11, P]
    assert pad((0, 0, 1))[1, 2].tolist() == [P, 19, 20, 21]
    # flip first, then shift: out[x] = src[(W-1-x) - dx]
    assert aug_volume(v, 4, (0, 0, 1), 1.0, 0.0)[0, 0].tolist() == [2, 1, 0, 0]
    assert aug_volume(v, 4, (0, 0, -1), 1.0, 0.5)[0, 0].tolist() == [0.5, 3.5, 2.5, 1.5]
    assert aug_volume(v, 0, (0, 0, 0), 0.5, 0.25)[1, 2].tolist() == [10.25, 10.75, 11.25, 11.75]
    # every combination against the contract's formula, voxel by voxel
    for flip, dz, dy, dx in itertools.product(range(8), (-1, 0, 1), (-2, 0, 2), (-3, 0, 1)):
        got = aug_volume(v, flip, (dz, dy, dx), 2.0, 0.5)
        for z, y, x in itertools.product(range(2), range(3), range(4)):
            sz = (1 - z if flip & 1 else z) - dz
            sy = (2 - y if flip & 2 else y) - dy
            sx = (3 - x if flip & 4 else x) - dx
            src = float(v[sz, sy, sx]) if 0 <= sz < 2 and 0 <= sy < 3 and 0 <= sx < 4 else 0.0
            assert float(got[z, y, x]) == 2.0 * src + 0.5, (flip, dz, dy, dx, z, y, x)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.lib_path()):
        _build.build()
    return _lib.load_library()


def test_abi_exports_the_augmenting_gather(lib):
    assert "mms_gather_aug_group" in _lib.protos() and hasattr(lib, "mms_gather_aug_group")
    S = _lib.structs()
    for name in ("AugP", "AugRec"):
        assert name in S and lib.mms_abi_sizeof(name.encode()) == ctypes.sizeof(S[name])
    assert ctypes.sizeof(S["AugRec"]) == 4 * A.REC_WORDS       # a record row of augment.make_records IS an AugRec
    r = A.make_records(1, flip=5, shift=(1, -2, 3), scale=1.5, offset=-0.5, drop=6)
    rec = S["AugRec"].from_buffer_copy(r.numpy().tobytes())
    assert (rec.flip, rec.dz, rec.dy, rec.dx, rec.scale, rec.offset, rec.drop) == (5, 1, -2, 3, 1.5, -0.5, 6)
