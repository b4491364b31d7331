"""CPU: augment.Records, the bundle of record arrays that travels from the sampler to the gather launch -- its kind and key, slicing
and stacking, and the one host-side check in front of every launch (no GPU)."""
import pytest
import torch

from multimodal_survival_prediction_amd import augment as A, data

FULL = "flip=0.5,shift=2:4:4,scale=0.9:1.1,offset=-0.05:0.05,moddrop=0.2"
AFF = ",rot=10,zoom=0.9:1.1,noise=0:0.03"
ELA = ",elastic=0.5:3:8"
DIMS, N = (16, 16, 8), 8
SPECS = [(FULL, "mms_gather_aug_group", None), (FULL + AFF, "mms_gather_affine_group", None), (FULL + AFF + ELA, "mms_gather_elastic_group", 8)]


def _draw(text):
    spec = A.AugmentSpec.parse(text)
    mask = data.make_cohort(n=N, dims=DIMS, rna_dim=8, seed=3, complete=False)["mask"]
    arrays = A.sample_all(spec, torch.Generator().manual_seed(1), mask, DIMS, "partial")
    return arrays, A.Records(*arrays, spacing=spec.elastic_spacing)


def _same(a, b):
    return a is None and b is None or torch.equal(a, b)


@pytest.mark.parametrize("text,kind,spacing", SPECS)
def test_kind_key_slices_and_stack(text, kind, spacing):
    (rec, aff, ela), r = _draw(text)
    assert r.kind == kind and r.key == (kind, spacing)
    assert (r.aff is None) == (aff is None) and (r.ela is None) == (ela is None)
    for i in (0, 4):
        s = r[i:i + 4]
        assert s.key == r.key and torch.equal(s.rec, rec[i:i + 4])
        assert _same(s.aff, None if aff is None else aff[i:i + 4]) and _same(s.ela, None if ela is None else ela[i:i + 4])
    assert r[None].rec.shape == (1, N, A.REC_WORDS) and r[None].key == r.key
    st = A.Records.stack([r[0:4], r[4:8]])
    assert st.rec.shape == (2, 4, A.REC_WORDS) and st.key == r.key
    assert torch.equal(st[1].rec, r[4:8].rec) and _same(st[1].aff, r[4:8].aff) and _same(st[1].ela, r[4:8].ela)
    assert A.Records.of(r) is r
    bare = A.Records.of(rec)
    assert bare.aff is None and bare.ela is None and bare.kind == "mms_gather_aug_group" and torch.equal(bare.rec, rec)
    assert A.Records.of(rec.numpy()).aff is None


@pytest.mark.parametrize("text,kind,spacing", SPECS)
def test_check_returns_the_checkers_bounds(text, kind, spacing):
    (rec, aff, ela), r = _draw(text)
    want = (A.check_records(rec, DIMS), [0.0, 0.0, 0.0] if ela is None else A.check_elastic_records(ela, spacing=spacing))
    assert r.check((N,), DIMS, True) == want
    st = A.Records.stack([r[0:4], r[4:8]])
    assert st.check((2, 4), DIMS, True) == want
    assert r.check((N,), None, True) == want                       # (a model without an encoder: no extent to hold the shifts against)


@pytest.mark.parametrize("text,kind,spacing", SPECS)
def test_check_refuses(text, kind, spacing):
    (rec, aff, ela), r = _draw(text)
    mk = lambda **kw: A.Records(**{**dict(rec=rec, aff=aff, ela=ela, spacing=r.spacing), **kw})
    with pytest.raises(ValueError):
        r.check((N - 1,), DIMS, True)
    with pytest.raises(ValueError):
        r.check((2, 4), DIMS, True)
    for name, a in (("rec", rec), ("aff", aff), ("ela", ela)):       # a wrong leading shape on each array alone
        if a is not None:
            with pytest.raises(ValueError, match=name):
                mk(**{name: a[:N - 1]}).check((N,), DIMS, True)
    bad = rec.clone()
    bad[3, A.DY] = -DIMS[1]
    with pytest.raises(ValueError, match="extent"):
        mk(rec=bad).check((N,), DIMS, True)
    bad = rec.clone()
    bad[2, A.DROP] = 2
    mk(rec=bad).check((N,), DIMS, True)
    with pytest.raises(ValueError, match="no modality mask"):
        mk(rec=bad).check((N,), DIMS, False)
    if aff is not None:
        bad = aff.clone()
        bad.view(torch.float32)[5, 7] = float("inf")
        with pytest.raises(ValueError, match="not finite"):
            mk(aff=bad).check((N,), DIMS, True)
    if ela is not None:
        bad = ela.clone()
        bad.view(torch.float32)[1, 0] = 0.4 * spacing * 1.01
        with pytest.raises(ValueError, match="fold"):
            mk(ela=bad).check((N,), DIMS, True)
        with pytest.raises(ValueError, match="power of two"):
            mk(spacing=12).check((N,), DIMS, True)


def test_construction_and_stack_refuse_mixed_bundles():
    (rec, aff, ela), r = _draw(FULL + AFF + ELA)
    with pytest.raises(ValueError, match="8-word records"):
        A.Records(None, aff)
    with pytest.raises(ValueError, match="affine records"):
        A.Records(rec, None, ela, 8)
    with pytest.raises(ValueError, match="one kind"):
        A.Records.stack([r[0:4], A.Records(rec[4:8], aff[4:8])])
    with pytest.raises(ValueError, match="one kind"):
        A.Records.stack([r[0:4], A.Records(rec[4:8])])
    with pytest.raises(ValueError, match="spacing"):
        A.Records.stack([r[0:4], A.Records(rec[4:8], aff[4:8], ela[4:8], 4)])
