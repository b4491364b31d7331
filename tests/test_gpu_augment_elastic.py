"""GPU: mms_elastic_field and mms_gather_elastic_group (elastic deformation inside the batch gather) against
tests/augment_elastic_ref.py, the float64 restatement of the contract:
  1. the field and the kernel through the C ABI: the field within a derived bound, bounded by amp, independent of the launch;
     amp = 0 records == mms_gather_affine_group bit for bit, identity == mms_gather_rows_group; generic records (amp up to 0.4 spacing
     with rotation, zoom, intensity, noise) within a bound derived per record, EVERY voxel; staged == direct bit for bit; NaN / Inf /
     huge amplitudes stay inside the volume's range; bad arguments are refused.  Shapes (6, 12, 12) (16-byte path), (5, 7, 9) (scalar
     path) at spacings 2 and 4, (8, 24, 32) (several lattice cells per axis, two blocks per row) at 2, 4 and 8; B = 4, ng = 2 with
     different records per member, device and pinned-host cohorts, stage_floats 0 (the default: the direct form for rows that deform),
     8192 (staged) and 16 (direct), per-axis spacings through mms_elastic_field, rows without a CT and dropped rows;
  2. the step, the loaders, validation and one entry point.

The bounds (not tuned; if the GPU exceeds one that is a finding).  E = 2^-24, fp32's unit roundoff; A = amp_a.
  Field.  The kernel (gather_elastic.hip: ela_disp4) uses the basis numerators N_i = 6 B_i, exact in fp32 (r is a multiple of 2^-6:
  every term of the cubics has at most 18 fractional bits and is below 8), which sum to exactly 6, and reduces z first, then y, then
  x, each level a product and three fmaf, then multiplies once by fp32(1/216).  The control values are the same fp32 numbers on both
  sides, |c| <= A.  Level z: four roundings, each at most E times a partial sum of magnitude <= 6 A: 24 E A.  Level y: its inputs'
  errors weighted by numerators that sum to 6 (144 E A) plus four roundings on magnitudes <= 36 A (144 E A): 288 E A.  Level x:
  6 * 288 + 4 * 216 = 2592 E A.  Times 1/216: 12 E A, plus E A for the constant's own rounding and E A for the product's: 14 E A;
  the second-order terms ((1 + E)^12 - 1) are far below the remaining 2:
      |d_gpu - d_ref| <= 16 E amp_a,   and, the weights being non-negative with sum 1,   |d_gpu| <= amp_a (1 + 16 E).
  Generic records: the bound of tests/test_gpu_augment_affine.py with the coordinate error widened.  The deformed position p_a + d_a
  is one fp32 add: it differs from the reference's by the field's 16 E amp_a plus one rounding on at most n_a + amp_a, below
      dp_a = E (n_a + 18 amp_a)    (17 amp_a, and one more for the second-order terms).
  The chain's three fmaf now run on arguments of at most n_b + amp_b and see those argument errors through |m|:
      delta_axis <= 4 E (|m0| (D + amp_z) + |m1| (H + amp_y) + |m2| (W + amp_x) + |m3|) + (|m0| dp_z + |m1| dp_y + |m2| dp_x) (1 + 4 E).
  The value part -- L (delta_z + delta_y + delta_x) + 16 E (|scale| max|v| + |offset| + 5 sigma) -- is the affine test's, unchanged.
"""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_elastic_ref as ER
from gpu_util import DEV, GROUP_INDEPENDENT_OPTS as GI, rel_err
from test_gpu_augment_affine import (B, NG, SCALAR, VEC, _check_plain_sources, _cohort, _generic_rows, _launch as _launch_affine, _members,
                                     _patients, _placed, _records)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = 2.0 ** -24
BIG = (8, 24, 32)
CASES = [(VEC, 1), (VEC, 2), (SCALAR, 1), (SCALAR, 2), (BIG, 1), (BIG, 2), (BIG, 3)]         # (dims, log2 spacing)


# ---- 1. the kernel through the C ABI ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cpu(dims):
    return _cohort(dims)


@functools.lru_cache(maxsize=None)
def _on(dims, where):
    return _placed(_cpu(dims), where)


def _ela_blocks(A, S, ela_dev, l, max_amp, ng):
    out = []
    for g in range(ng):
        P = A.ela_block(ela_dev[g], 1 << l, max_amp)
        out.append(P)
    return (S["ElaP"] * ng)(*out)


def _launch(cohort, idx, recs, aff, ela, l, max_amp, stage=0, edit=None):
    """mms_gather_elastic_group over idx [ng][B] -> (rc, per member dict of destination tensors; NaN where nothing was written)."""
    from multimodal_survival_prediction_amd import _lib, augment as A, ops
    lib, S = _lib.load_library(), _lib.structs()
    ng, nb = idx.shape
    dims = tuple(cohort["image"].shape[-3:])
    vol = int(np.prod(dims))
    idx_dev = torch.as_tensor(idx, dtype=torch.int64).to(DEV)
    lab, mask = cohort["label"], cohort["mask"]
    srcs = [("image", cohort["image"].view(-1, vol), vol, mask, (A.ROLE_VOLUME, 0)),
            ("rnaseq", cohort["rnaseq"], cohort["rnaseq"].shape[1], mask[:, 1:], (A.ROLE_PLAIN, 1)),
            ("clinical", cohort["clinical"], 1, None, (A.ROLE_PLAIN, 2)),
            ("mask", mask, 3, None, (A.ROLE_MASK, -1)), ("time", lab, 1, None, (A.ROLE_PLAIN, -1)),
            ("valid", cohort["valid"].view(-1, 1), 1, None, (A.ROLE_PLAIN, -1))]
    outs, Gs = [], []
    for g in range(ng):
        o = {k: torch.full((nb, w), float("nan"), device=DEV) for k, _, w, _, _ in srcs}
        G = S["GatherP"]()
        G.idx, G.B, G.nsrc = idx_dev[g].data_ptr(), nb, len(srcs)
        for i, (k, a, w, flag, _) in enumerate(srcs):
            G.src[i], G.dst[i], G.src_ld[i], G.dst_ld[i], G.width[i] = a.data_ptr(), o[k].data_ptr(), a.stride(0), w, w
            if flag is not None:
                G.present[i], G.present_ld[i] = flag.data_ptr(), flag.stride(0)
        outs.append(o); Gs.append(G)
    Ga = (S["GatherP"] * ng)(*Gs)
    rec_dev, aff_dev, ela_dev = recs.to(DEV), aff.to(DEV), ela.to(DEV)
    stages = [stage] * ng if isinstance(stage, int) else list(stage)
    Aa = (S["AugP"] * ng)(*[A.aug_block(rec_dev[g], [r for *_, r in srcs], dims, (0, 0, 0)) for g in range(ng)])
    Fa = (S["AffP"] * ng)(*[A.aff_block(aff_dev[g], stages[g]) for g in range(ng)])
    Ea = _ela_blocks(A, S, ela_dev, l, max_amp, ng)
    if edit is not None:
        edit(Ga, Aa, Fa, Ea)
    rc = lib.mms_gather_elastic_group(Ga, Aa, Fa, Ea, ng, ops.stream())
    torch.cuda.synchronize()
    return rc, [{k: v.cpu() for k, v in o.items()} for o in outs]


def _field(ela, dims, l, max_amp, edit=None, B_=None):
    """mms_elastic_field -> (rc, [n, 3, D, H, W] host tensor)."""
    from multimodal_survival_prediction_amd import _lib, augment as A, ops
    lib = _lib.load_library()
    n = ela.shape[0]
    ela_dev = ela.to(DEV)
    out = torch.full((n, 3) + tuple(dims), float("nan"), device=DEV)
    P = A.ela_block(ela_dev, 1 << l, max_amp)
    args = [n if B_ is None else B_, dims[0], dims[1], dims[2], out.data_ptr()]
    if edit is not None:
        edit(P, args)
    import ctypes
    rc = lib.mms_elastic_field(ctypes.byref(P), *args, ops.stream())
    torch.cuda.synchronize()
    return rc, out.cpu()


def _amp32(amps):
    return np.asarray(amps, dtype=np.float32).astype(np.float64)


@pytest.mark.parametrize("dims,l", CASES)
def test_field_matches_the_reference_within_the_derived_bound(dims, l):
    from multimodal_survival_prediction_amd import augment as A
    s = 1 << l
    rng = np.random.default_rng(l)
    amps = np.concatenate([rng.uniform(0.1, 0.4, (5, 3)) * s, [[0.4 * s] * 3, [0.0, 0.4 * s, 0.0], [0.0, 0.0, 0.0]]])
    seeds = [1, 0xFFFFFFFF, 3, 4, 0, 77, 78, 79]
    ela = A.elastic_records(8, amps, seeds)
    mx = A.check_elastic_records(ela, 8, s)
    rc, got = _field(ela, dims, l, mx)
    assert rc == 0 and not bool(torch.isnan(got).any())
    a32 = _amp32(amps)
    worst = 0.0
    for i in range(8):
        ref = ER.field(dims, (l, l, l), a32[i], seeds[i])
        for a in range(3):
            err = float(np.abs(got[i, a].double().numpy() - ref[a]).max())
            tol = 16 * E * a32[i, a]
            worst = max(worst, err / tol) if tol else worst
            print("dims %s spacing %d row %d axis %d: err %.3e bound %.3e" % (dims, s, i, a, err, tol))
            assert err <= tol
            assert float(got[i, a].abs().max()) <= a32[i, a] * (1 + 16 * E)
    print("largest err / bound = %.3f" % worst)
    assert float(got[5].abs().max()) > 0.05 * s and not bool(got[7].any()) and not bool(got[6, 0].any()) and bool(got[6, 1].any())
    # a row's field does not depend on the launch: other batch size, other position, other neighbours, a larger declared bound
    perm = [5, 0, 6]
    rc, again = _field(ela[perm], dims, l, [0.4 * s + 1.0] * 3)
    assert rc == 0 and all(torch.equal(again[j], got[i]) for j, i in enumerate(perm))
    rc, one = _field(ela[3:4], dims, l, mx)
    assert rc == 0 and torch.equal(one[0], got[3])
    # max_amp clamps: a bound below the record's amplitude gives the field of the bound
    rc, low = _field(ela[5:6], dims, l, [0.1 * s] * 3)
    rc2, want = _field(A.elastic_records(1, 0.1 * s, seeds[5]), dims, l, [0.1 * s] * 3)
    assert rc == 0 and rc2 == 0 and torch.equal(low, want)


@pytest.mark.parametrize("dims,ll", [(BIG, (2, 1, 3)), (BIG, (3, 2, 1)), (SCALAR, (1, 2, 1)), (VEC, (2, 2, 1))])
def test_field_with_a_spacing_per_axis(dims, ll):
    """The C ABI takes a spacing per axis (the Python surface passes one): the field against the reference, which takes per-axis l too.
    (., ., 1) with coarser other axes is the five-column case of the x-reduction; (5, 7, 9) has lanes past the line's end."""
    from multimodal_survival_prediction_amd import augment as A
    amps = [[0.4 * (1 << la) for la in ll], [0.3, 0.7, 0.2], [0.0, 0.0, 0.8]]
    seeds = [11, 12, 0xFFFFFFFE]
    ela = A.elastic_records(3, amps, seeds)
    def per_axis(P, args):
        for a in range(3):
            P.log2_spacing[a] = ll[a]
    rc, got = _field(ela, dims, 1, [0.4 * (1 << max(ll))] * 3, edit=per_axis)
    assert rc == 0 and not bool(torch.isnan(got).any())
    a32 = _amp32(amps)
    for i in range(3):
        ref = ER.field(dims, ll, a32[i], seeds[i])
        for a in range(3):
            err, tol = float(np.abs(got[i, a].double().numpy() - ref[a]).max()), 16 * E * a32[i, a]
            print("dims %s spacings %s row %d axis %d: err %.3e bound %.3e" % (dims, ll, i, a, err, tol))
            assert err <= tol and float(got[i, a].abs().max()) <= a32[i, a] * (1 + 16 * E)
    assert bool(got[0].any()) and bool(got[2, 2].any()) and not bool(got[2, :2].any())


def _ela_rows(rows, l, rng, zero=False):
    """rows of _generic_rows -> rows + (amp[3], lattice seed): amplitudes in [0.2, 0.4] * spacing per axis, the first at the bound."""
    s = 1 << l
    out = []
    for k, r in enumerate(rows):
        amp = (0.0, 0.0, 0.0) if zero else tuple(0.4 * s for _ in range(3)) if k == 0 else tuple(rng.uniform(0.2, 0.4, 3) * s)
        out.append(r + (amp, int(rng.integers(0, 2 ** 32))))
    return out


def _ela_records(A, c):
    recs, aff = _records(A, c)
    return recs, aff, A.elastic_records(len(c), [r[7] for r in c], [r[8] for r in c])


@pytest.mark.parametrize("where", ["device", "pinned"])
def test_identity_records_equal_the_plain_gather(where):
    from multimodal_survival_prediction_amd import augment as A
    for dims in (VEC, SCALAR):
        cohort = _on(dims, where)
        idx = np.array([[0, 5, 5, 23], [7, 1, 12, 3]])
        recs = torch.stack([A.identity_records(B)] * NG)
        aff = torch.stack([A.affine_records(recs[g], dims=dims) for g in range(NG)])
        ela = torch.stack([A.elastic_records(B, 0.0, [1, 2, 3, 4])] * NG)
        rc, got = _launch(cohort, idx, recs, aff, ela, 1, [0.8] * 3)
        assert rc == 0
        _, plain = _launch_affine(cohort, idx)
        for g in range(NG):
            for k in plain[g]:
                assert torch.equal(got[g][k], plain[g][k]), k
                assert not bool(torch.isnan(got[g][k]).any())


@pytest.mark.parametrize("stage", [0, 16])
@pytest.mark.parametrize("dims,where", [(VEC, "device"), (VEC, "pinned"), (SCALAR, "device"), (BIG, "device")])
def test_zero_amplitude_equals_the_affine_gather(dims, where, stage):
    """Generic and noisy affine records: amp == 0 in the record (under a positive declared bound), and amp > 0 clamped to 0 by
    max_amp == 0 -- both the bits of mms_gather_affine_group."""
    from multimodal_survival_prediction_amd import augment as A
    cpu, cohort = _cpu(dims), _on(dims, where)
    rows = _ela_rows(_generic_rows(dims, cpu, np.random.default_rng(5)), 1, np.random.default_rng(6), zero=True)
    n = 0
    for members in _members(rows):
        idx = np.array([[r[0] for r in c] for c in members])
        ra = [_ela_records(A, c) for c in members]
        recs, aff, ela = (torch.stack([r[i] for r in ra]) for i in range(3))
        _, want = _launch_affine(cohort, idx, recs, aff, stage)
        rc, got = _launch(cohort, idx, recs, aff, ela, 1, [0.8] * 3, stage)
        loud = torch.stack([A.elastic_records(B, 0.8, [9, 8, 7, 6])] * NG)
        rc2, got2 = _launch(cohort, idx, recs, aff, loud, 1, [0.0] * 3, stage)
        assert rc == 0 and rc2 == 0
        for g in range(NG):
            for k in want[g]:
                assert torch.equal(got[g][k], want[g][k]) and torch.equal(got2[g][k], want[g][k]), (k, g)
            n += int(want[g]["image"].abs().sum() > 0)
    assert n >= 4


def _bound(vol, m32, amp, scale, offset, sigma):
    """The module docstring's bound for one record; vol float64 [D, H, W], m32 the fp32 matrix as float64, amp the fp32 amplitudes."""
    dims = np.asarray(vol.shape, dtype=np.float64)
    dp = E * (dims + 18 * amp)
    delta = [4 * E * (np.abs(m32[a, :3]) @ (dims + amp) + abs(m32[a, 3])) + (np.abs(m32[a, :3]) @ dp) * (1 + 4 * E) for a in range(3)]
    pad = np.pad(vol, 1)
    L = max(float(np.abs(np.diff(pad, axis=a)).max()) for a in range(3))
    return L * sum(delta) + 16 * E * (abs(scale) * float(np.abs(vol).max()) + abs(offset) + 5 * sigma)


@functools.lru_cache(maxsize=None)
def _generic_case(dims, l):
    """The generic rows of (dims, spacing) with their references and bounds, computed once: [(launch members)] and per row
    (ref float64 or None for a zero-filled row, tol).  The CONDITION is checked here, on the reference alone: the field moves every
    tested record's output by more than ten times its tolerance, so a kernel that ignored the field cannot pass."""
    cpu = _cpu(dims)
    rows = _ela_rows(_generic_rows(dims, cpu, np.random.default_rng(5)), l, np.random.default_rng(7 + l))
    info = {}
    for k, (p, m, scale, offset, sigma, seed, drop, amp, eseed) in enumerate(rows):
        if cpu["mask"][p, 0] == 0 or drop & 1:
            info[k] = (None, 0.0)
            continue
        vol = cpu["image"][p].reshape(dims).double().numpy()
        m32 = np.asarray(m, dtype=np.float32).astype(np.float64)
        s32, o32, g32, a32 = float(np.float32(scale)), float(np.float32(offset)), float(np.float32(sigma)), _amp32(amp)
        ref = ER.elastic_volume(vol, m32, (l, l, l), a32, eseed, s32, o32, g32, seed)
        tol = _bound(vol, m32, a32, s32, o32, g32)
        if a32.any():
            moved = float(np.abs(ref - ER.R.affine_volume(vol, m32, s32, o32, g32, seed)).max())
            assert moved > 10 * tol, (dims, l, k, moved, tol)
        info[k] = (ref, tol)
    launches = []
    for i, members in enumerate(_members(list(enumerate(rows)))):
        launches.append([[(k, r) for k, r in c] for c in members])
    return launches, info


@functools.lru_cache(maxsize=None)
def _generic_run(dims, where, l, stage):
    from multimodal_survival_prediction_amd import augment as A
    cohort = _on(dims, where)
    launches, _ = _generic_case(dims, l)
    outs = []
    for members in launches:
        idx = np.array([[r[0] for _, r in c] for c in members])
        ra = [_ela_records(A, [r for _, r in c]) for c in members]
        recs, aff, ela = (torch.stack([r[i] for r in ra]) for i in range(3))
        mx = A.check_elastic_records(ela, spacing=1 << l)
        rc, got = _launch(cohort, idx, recs, aff, ela, l, mx, stage)
        assert rc == 0
        outs.append((idx, got))
    return outs


GENERIC = [(VEC, "device", 1), (VEC, "pinned", 2), (VEC, "device", 2), (SCALAR, "device", 1), (SCALAR, "device", 2), (BIG, "device", 1),
           (BIG, "pinned", 2), (BIG, "device", 3)]


STAGED = 8192                # an explicit budget: deforming rows are staged too (0 is the default: direct for them)


@pytest.mark.parametrize("stage", [0, STAGED, 16])
@pytest.mark.parametrize("dims,where,l", GENERIC)
def test_generic_records_within_the_derived_bound(dims, where, l, stage):
    cpu = _cpu(dims)
    launches, info = _generic_case(dims, l)
    n = zeroed = 0
    worst = 0.0
    for members, (idx, got) in zip(launches, _generic_run(dims, where, l, stage)):
        for g, c in enumerate(members):
            _check_plain_sources(cpu, got[g], idx[g], [r[6] for _, r in c])
            for b, (k, r) in enumerate(c):
                gi = got[g]["image"][b].view(dims).double().numpy()
                ref, tol = info[k]
                if ref is None:
                    assert not gi.any()                       # zero-filled: neither offset nor noise
                    zeroed += 1
                    continue
                err = float(np.abs(gi - ref).max())           # every voxel
                worst = max(worst, err / tol)
                print("dims %s spacing %d stage %d patient %d: err %.3e bound %.3e" % (dims, 1 << l, stage, r[0], err, tol))
                assert err <= tol, (k, r[0], err, tol)
                n += 1
    print("largest err / bound = %.3f" % worst)
    assert n >= 13 and zeroed >= 2


@pytest.mark.parametrize("dims,where,l", GENERIC)
def test_staged_equals_direct_bit_for_bit(dims, where, l):
    """What catches a source box that is too small: every record of the generic test, every source."""
    for (_, a), (_, b), (_, c) in zip(_generic_run(dims, where, l, STAGED), _generic_run(dims, where, l, 16), _generic_run(dims, where, l, 0)):
        for g in range(NG):
            for k in a[g]:
                assert torch.equal(a[g][k], b[g][k]) and torch.equal(a[g][k], c[g][k]), (k, g)


def test_a_row_does_not_depend_on_its_launch():
    """ng = 1 against ng = 2, the member position swapped, other rows beside it: the same bits."""
    from multimodal_survival_prediction_amd import augment as A
    dims, l = VEC, 1
    launches, _ = _generic_case(dims, l)
    (idx, got), members = _generic_run(dims, "device", l, 0)[0], launches[0]
    ra = [_ela_records(A, [r for _, r in c]) for c in members]
    mx = A.check_elastic_records(torch.stack([r[2] for r in ra]), spacing=2)
    rc, solo = _launch(_on(dims, "device"), idx[1:2], ra[1][0][None], ra[1][1][None], ra[1][2][None], l, mx)
    assert rc == 0 and torch.equal(solo[0]["image"], got[1]["image"])
    sw = [ra[1], ra[0]]
    rc, swapped = _launch(_on(dims, "device"), idx[::-1].copy(), *(torch.stack([r[i] for r in sw]) for i in range(3)), l, mx)
    assert rc == 0 and torch.equal(swapped[0]["image"], got[1]["image"]) and torch.equal(swapped[1]["image"], got[0]["image"])


def test_non_finite_and_huge_amplitudes_stay_in_range():
    """The kernel clamps amp into [0, max_amp], NaN -> 0: whatever the record holds the launch completes, and with identity matrices,
    scale 1, offset 0, sigma 0 every output is a convex combination of voxels and air: finite, within [0, max of the volume].  Member 0
    takes the staged form, member 1 the direct one.  The host check refuses the same records."""
    from multimodal_survival_prediction_amd import augment as A
    cpu = _cpu(VEC)
    cohort = _on(VEC, "device")
    with_img, _, _ = _patients(cpu)
    nan, inf = float("nan"), float("inf")
    amps = [[nan, nan, nan], [inf, inf, inf], [1e30, -1e30, 3e38], [-inf, nan, 0.5]]
    ela = A.elastic_records(4, amps, [1, 2, 3, 4])
    with pytest.raises(ValueError):
        A.check_elastic_records(ela, 4, 2)
    for row in range(4):
        with pytest.raises(ValueError):
            A.check_elastic_records(ela[row:row + 1], 1, 2)
    recs = A.identity_records(4)
    aff = A.affine_records(recs, dims=VEC)
    idx = np.array([[with_img[0], with_img[1], with_img[0], with_img[1]]] * NG)
    rc, got = _launch(cohort, idx, torch.stack([recs] * NG), torch.stack([aff] * NG), torch.stack([ela] * NG), 1, [0.8] * 3, (STAGED, 16))
    assert rc == 0
    for g in range(NG):
        img = got[g]["image"]
        assert bool(torch.isfinite(img).all())
        for b in range(4):
            top = float(cpu["image"][idx[g][b]].max())
            assert float(img[b].min()) >= 0.0 and float(img[b].max()) <= top
        assert torch.equal(img[0], cpu["image"][idx[g][0]].view(-1))                  # NaN amplitudes: 0, the identity copy
        assert not torch.equal(img[1], cpu["image"][idx[g][1]].view(-1))              # Inf: clamped to max_amp, deformed
    assert torch.equal(got[0]["image"], got[1]["image"])
    rc, want = _launch(cohort, idx[:1], recs[None], aff[None], A.elastic_records(4, [[0, 0, 0], [0.8] * 3, [0.8, 0, 0.8], [0, 0, 0.5]], [1, 2, 3, 4])[None],
                       1, [0.8] * 3)
    assert rc == 0 and torch.equal(want[0]["image"], got[0]["image"])                 # ... exactly the records the clamp makes of them


def test_bad_arguments_are_refused():
    from multimodal_survival_prediction_amd import augment as A
    cohort = _on(VEC, "device")
    idx, recs = np.array([[0, 1, 2, 3], [4, 5, 6, 7]]), torch.stack([A.identity_records(4)] * 2)
    aff = torch.stack([A.affine_records(recs[0], dims=VEC)] * 2)
    ela = torch.stack([A.elastic_records(4, 0.5, 3)] * 2)
    nan, inf = float("nan"), float("inf")
    def no_elastic_records(G, Au, F, El): El[1].rec = None
    def spacing_zero(G, Au, F, El): El[0].log2_spacing[1] = 0; El[1].log2_spacing[1] = 0
    def spacing_seven(G, Au, F, El): El[0].log2_spacing[2] = 7; El[1].log2_spacing[2] = 7
    def bound_negative(G, Au, F, El): El[0].max_amp[0] = -0.5; El[1].max_amp[0] = -0.5
    def bound_nan(G, Au, F, El): El[0].max_amp[1] = nan; El[1].max_amp[1] = nan
    def bound_inf(G, Au, F, El): El[0].max_amp[2] = inf; El[1].max_amp[2] = inf
    def bound_above_64(G, Au, F, El): El[0].max_amp[0] = 64.5; El[1].max_amp[0] = 64.5
    def members_disagree_on_spacing(G, Au, F, El): El[1].log2_spacing[0] = 2
    def members_disagree_on_bound(G, Au, F, El): El[1].max_amp[0] = 0.25
    def no_affine_records(G, Au, F, El): F[0].rec = None
    def negative_budget(G, Au, F, El): F[1].stage_floats = -1
    def shift_bound_too_large(G, Au, F, El): Au[0].max_shift[0] = VEC[0]
    def wrong_width(G, Au, F, El): Au[0].W = 8
    def two_volumes(G, Au, F, El): Au[0].role[1] = A.ROLE_VOLUME
    def no_records(G, Au, F, El): Au[1].rec = None
    def no_index(G, Au, F, El): G[0].idx = None
    for edit in (no_elastic_records, spacing_zero, spacing_seven, bound_negative, bound_nan, bound_inf, bound_above_64,
                 members_disagree_on_spacing, members_disagree_on_bound, no_affine_records, negative_budget, shift_bound_too_large,
                 wrong_width, two_volumes, no_records, no_index):
        assert _launch(cohort, idx, recs, aff, ela, 1, [0.8] * 3, edit=edit)[0] == -1, edit.__name__
    assert _launch(cohort, idx, recs, aff, ela, 1, [0.8] * 3)[0] == 0
    def bound_64(G, Au, F, El): El[0].max_amp[0] = 64.0; El[1].max_amp[0] = 64.0
    def spacing_64(G, Au, F, El):
        for g in range(2):
            for a in range(3):
                El[g].log2_spacing[a] = 6
    assert _launch(cohort, idx, recs, aff, ela, 1, [0.8] * 3, edit=bound_64)[0] == 0
    assert _launch(cohort, idx, recs, aff, ela, 1, [0.8] * 3, edit=spacing_64)[0] == 0
    # a lattice above the LDS budget: (8, 32, 32) at spacing 2 takes 3 * 7 * 19 * 19 = 7581 floats; at spacing 4 it fits
    wide = _on((8, 32, 32), "device")
    aff_w = torch.stack([A.affine_records(recs[0], dims=(8, 32, 32))] * 2)
    assert _launch(wide, idx, recs, aff_w, ela, 1, [0.8] * 3)[0] == -1
    assert _launch(wide, idx, recs, aff_w, ela, 2, [0.8] * 3)[0] == 0
    # mms_elastic_field
    e1 = ela[0]
    def f_no_records(P, a): P.rec = None
    def f_spacing(P, a): P.log2_spacing[0] = 9
    def f_bound(P, a): P.max_amp[2] = nan
    def f_rows(P, a): a[0] = 0
    def f_extent(P, a): a[2] = 0
    def f_no_out(P, a): a[4] = None
    for edit in (f_no_records, f_spacing, f_bound, f_rows, f_extent, f_no_out):
        assert _field(e1, VEC, 1, [0.8] * 3, edit=edit)[0] == -1, edit.__name__
    assert _field(e1, (8, 32, 32), 1, [0.8] * 3)[0] == -1 and _field(e1, (8, 32, 32), 2, [0.8] * 3)[0] == 0
    assert _field(e1, VEC, 1, [0.8] * 3)[0] == 0


# ---- 2. step, loaders, validation, entry point ----------------------------------------------------------------------------------------
SPEC = "flip=0.5,shift=2:2:1,scale=0.9:1.1,offset=-0.05:0.05,rot=10,zoom=0.9:1.1,noise=0:0.02,seed=4,elastic=0.5:1.6:4"
DIMS, RNA = (16, 16, 8), 64


def _fallback_models(cls, G):
    from test_gpu_augment import _fallback_models as f
    return f(cls, G, RNA)


@pytest.mark.parametrize("cls,style", [("PartialModalityNet", "partial"), ("MultiModalSurvivalNet", "final")])
def test_indexed_augmented_step_equals_batch_step(cls, style):
    """train_step_indexed(cohort, idx, augment=Records with .aff and .ela) == train_step on the batches a materialising loader
    augmented beforehand (augment.apply: the same kernel over the same records; what is compared is the plumbing of the three record
    arrays through the fold group.  Tolerance of tests/test_gpu_fold_group.py::test_indexed_step_equals_batch_step).  The materialised
    CT is also held against the float64 reference, loosely (1e-5 on values in [-0.1, 1.3]): the loaders hand the kernel what they drew."""
    import copy
    from multimodal_survival_prediction_amd import augment as A, data, training as T
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    cpu = data.make_cohort(n=24, dims=DIMS, rna_dim=RNA, seed=3, complete=False)
    cohort = data.cohort_to(cpu, DEV)
    base = _fallback_models(cls, NG)
    Ae = FoldGroupEngine([copy.deepcopy(m).to(DEV).train() for m in base], dn_opts=GI)
    Be = FoldGroupEngine([copy.deepcopy(m).to(DEV).train() for m in base], dn_opts=GI)
    spec = SPEC + (",moddrop=0.3" if style == "partial" else "")
    folds = [torch.arange(0, 12), torch.arange(12, 24)]
    mk = lambda lazy: [data.BatchLoader(cohort, f, B, shuffle=True, seed=9 + g, style=style, lazy=lazy, with_valid=style == "partial",
                                        augment=spec, augment_style=style) for g, f in enumerate(folds)]
    skip = T._STYLES[style].skip_if_unusable
    for it, (mts, lzs) in enumerate(zip(zip(*mk(False)), zip(*mk(True)))):
        Ae.train_step([T._train_kwargs(style, mt) for mt in mts], skip_if_unusable=skip, use_graph=it > 0)
        Be.train_step_indexed(lzs[0]["gather"], torch.stack([lz["index"] for lz in lzs]), skip_if_unusable=skip, use_graph=it > 0,
                              augment=A.Records.stack([lz["augment"] for lz in lzs]))
        torch.cuda.synchronize()
        if it == 0:
            for g in range(NG):
                e = rel_err(Be.engines[g].gflat, Ae.engines[g].gflat)
                print(cls, "member", g, "rel_err(gflat) =", e, "max |gflat| =", float(Ae.engines[g].gflat.abs().max()))
                assert float(Ae.engines[g].gflat.abs().max()) > 0 and e <= 2e-5
            lz, mt = lzs[0], mts[0]
            f8, f16, f4 = lz["augment"].rec.view(torch.float32), lz["augment"].aff.view(torch.float32), lz["augment"].ela.view(torch.float32)
            seen = 0
            for b, p in enumerate(lz["index"].tolist()):
                if cpu["mask"][p, 0] == 0 or int(lz["augment"].rec[b, A.DROP]) & 1:
                    continue
                vol = cpu["image"][p].reshape(DIMS).double().numpy()
                m32 = f16[b, :12].double().numpy().reshape(3, 4)
                args = (float(f8[b, A.SCALE]), float(f8[b, A.OFFSET]), float(f16[b, A.AFF_SIGMA]), int(lz["augment"].aff[b, A.AFF_SEED]) & 0xFFFFFFFF)
                ref = ER.elastic_volume(vol, m32, (2, 2, 2), f4[b, :3].double().numpy(), int(lz["augment"].ela[b, A.ELA_SEED]) & 0xFFFFFFFF, *args)
                have = mt["image"][b].reshape(DIMS).double().cpu().numpy()
                assert float(np.abs(have - ref).max()) <= 1e-5
                assert float(np.abs(have - ER.R.affine_volume(vol, m32, *args)).max()) > 1e-3        # ... and the field is in there
                seen += 1
            assert seen > 0
    assert it == 2
    for a, b in zip(Ae.epoch_stats(), Be.epoch_stats()):
        assert a["n_batches"] == b["n_batches"] == 3 and a["n_usable"] == b["n_usable"]


@pytest.fixture(scope="module")
def partial_group():
    from multimodal_survival_prediction_amd import data
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    cohort = data.cohort_to(data.make_cohort(n=24, dims=DIMS, rna_dim=RNA, seed=3, complete=False), DEV)
    ge = FoldGroupEngine([m.to(DEV) for m in _fallback_models("PartialModalityNet", 2)], dn_opts=GI)
    return cohort, ge


def test_lazy_and_materialising_loaders_agree(partial_group):
    from multimodal_survival_prediction_amd import data
    cohort, ge = partial_group
    mk = lambda lazy: data.BatchLoader(cohort, torch.arange(24), 4, shuffle=True, seed=9, lazy=lazy, augment=SPEC + ",moddrop=0.3",
                                       augment_style="partial")
    GP = ge.plan(4, DIMS, (0,))
    P = GP.Ps[0]
    n = changed = 0
    for lz, mt in zip(mk(True), mk(False)):
        ge._gather_indexed(GP, lz["gather"], lz["index"][None], lz["augment"][None])
        torch.cuda.synchronize()
        assert torch.equal(P.ct.view(mt["image"].shape), mt["image"]) and torch.equal(P.buf["rna"], mt["rnaseq"])
        assert torch.equal(P.buf["clin"].view(mt["clinical"].shape), mt["clinical"]) and torch.equal(P.mask, mt["mask"])
        assert torch.equal(cohort["label"][lz["index"].to(DEV)], mt["label"])
        changed += int(not torch.equal(mt["image"], cohort["image"][lz["index"].to(DEV)]))
        n += 1
    assert n == 6 and changed > 0


def test_validation_ignores_the_spec(partial_group):
    from multimodal_survival_prediction_amd import data, training as T
    cohort, ge = partial_group
    lab = torch.nonzero(cohort["has_survival"]).view(-1).cpu()
    for lazy in (True, False):
        mk = lambda **kw: [data.BatchLoader(cohort, lab[f::2], 4, shuffle=False, lazy=lazy, **kw) for f in range(2)]
        plain = T.validate_lockstep(ge, mk(), "partial", DEV)
        withspec = T.validate_lockstep(ge, mk(augment=SPEC, augment_style="partial"), "partial", DEV)
        assert plain == withspec, (lazy, plain, withspec)


def test_an_elastic_spec_takes_the_elastic_gather_and_only_that(partial_group):
    from multimodal_survival_prediction_amd import data, training as T
    from test_gpu_augment import _Spy
    cohort, ge = partial_group
    mk = lambda spec: [data.BatchLoader(cohort, torch.arange(12 * f, 12 * f + 8), 4, shuffle=True, seed=f, lazy=True, augment=spec,
                                        augment_style="partial") for f in range(2)]
    real = ge.lib
    try:
        ge.lib = spy = _Spy(real)
        for spec, want in ((SPEC, "mms_gather_elastic_group"), ("flip=0.5,elastic=0.5:1.6:4", "mms_gather_elastic_group"),
                           (SPEC.replace(",elastic=0.5:1.6:4", ""), "mms_gather_affine_group"),      # without the key: what it launched
                           ("flip=0.5,scale=0.9:1.1", "mms_gather_aug_group")):
            del spy.calls[:]
            T.train_epoch_lockstep(ge, mk(spec), "partial")
            gathers = {c for c in spy.calls if c.startswith("mms_gather")}
            assert gathers == {want}, (spec, gathers)
    finally:
        ge.lib = real
        torch.cuda.synchronize()


def test_members_with_different_record_kinds_step_apart(partial_group):
    """Two members whose loaders carry records of different kinds cannot share a gather launch: train_epoch_lockstep groups the named
    batches by the records' key, so each position is two steps of one member each -- one launch of each kind's entry point, and
    nothing else; both members still see both of their batches."""
    from multimodal_survival_prediction_amd import data, training as T
    from test_gpu_augment import _Spy
    cohort, ge = partial_group
    loaders = [data.BatchLoader(cohort, torch.arange(12 * f, 12 * f + 8), 4, shuffle=True, seed=f, lazy=True, augment=spec, augment_style="partial")
               for f, spec in enumerate(("flip=0.5,scale=0.9:1.1", SPEC))]
    real = ge.lib
    try:
        ge.lib = spy = _Spy(real)
        stats = T.train_epoch_lockstep(ge, loaders, "partial")
        gathers = {c for c in spy.calls if c.startswith("mms_gather")}
        assert gathers == {"mms_gather_aug_group", "mms_gather_elastic_group"}, gathers
    finally:
        ge.lib = real
        torch.cuda.synchronize()
    assert len(stats) == 2
    assert [e.epoch_stats()["n_batches"] for e in ge.engines] == [2, 2]


def test_displacement_field_is_the_kernels_field():
    from multimodal_survival_prediction_amd import augment as A
    ela = A.elastic_records(2, [1.5, 0.0], [5, 6])
    d = A.displacement_field(ela, DIMS, 4)
    assert d.shape == (2, 3) + DIMS and d.is_cuda and not bool(d[1].any())
    assert float(np.abs(d[0].double().cpu().numpy() - ER.field(DIMS, (2, 2, 2), [1.5] * 3, 5)).max()) <= 16 * E * 1.5
    with pytest.raises(ValueError, match="fold"):
        A.displacement_field(A.elastic_records(1, 2.0, 1), DIMS, 4)


def test_entry_point_records_the_spec(tmp_path):
    from test_gpu_augment import _CHILD
    from multimodal_survival_prediction_amd.augment import AugmentSpec
    scripts = os.path.join(ROOT, "scripts", "training")
    code = _CHILD.format(root=ROOT, scripts=scripts, script=os.path.join(scripts, "partial_modality_training.py"))
    aug = "rot=10,zoom=0.9:1.1,elastic=0:1.6:4"
    env = dict(os.environ, MMS_PATIENTS="24", MMS_EPOCHS="2", MMS_FOLDS="2", MMS_BATCH_SIZE="3", MMS_VOLUME="16,16,8", MMS_AUGMENT=aug)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "-c", code], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    res = json.load(open(tmp_path / "results" / "partial_modality" / "cv_results.json"))
    spec = AugmentSpec.parse(res["hyperparameters"]["augment"])
    assert spec == AugmentSpec.parse(aug) and spec.has_elastic and spec.elastic_spacing == 4

    # the training log: "... epoch   1: train=(cox, entropy) val_loss=... C-index=..." per fold
    lines = [ln.split("train=", 1)[1] for ln in r.stdout.splitlines() if "train=" in ln and "val_loss=" in ln]
    assert len(lines) >= 2, r.stdout[-3000:]
    for ln in lines:
        vals = [float(x) for x in re.findall(r"[-+]?(?:\d+\.?\d*(?:[eE][-+]?\d+)?|nan|inf)", ln.split("C-index")[0])]
        assert len(vals) >= 2 and all(np.isfinite(v) for v in vals), ln
