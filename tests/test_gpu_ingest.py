"""CT ingest from the stored types (csrc/ct_ingest.hip: mms_ct_preprocess_raw_batch) and the NIfTI loading pipeline around it.

Yardstick: oracle.preproc.ct_preprocess(slope * raw.astype(float64) + inter, target) -- the reference's own numpy + scipy.zoom arithmetic on the
values the file stands for -- at 1e-5, the tolerance tests/test_gpu_preproc.py uses for the same arithmetic after the load.  The raw values
are integers of a CT-like range, so the int32 / uint32 / float64 cases are exact in fp32 as well.  Files come from tests/nifti_ref.py (the
specification's byte offsets), not from the implementation's writer.

Beyond that range: values at the ends of every stored type with a guard that the other signedness would fail (NR.full_range_values),
fractional float elements, the documented rounding of float64 elements to fp32, low contrast on an offset, and one volume of scan size
(pass 1 at its workgroup cap with a scalar tail, more than one sweep of pass 2's output loop, alone and next to small volumes)."""
import importlib.util
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nifti_ref as NR
from gpu_util import DEV, assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = "<" if sys.byteorder == "little" else ">"
OTHER = ">" if NATIVE == "<" else "<"
SHAPES = [((5, 7, 1), (8, 8, 4)),            # a unit axis
          ((3, 5, 7), (8, 8, 4)),            # 105 elements: a scalar tail at every vector width (16, 8, 4, 2 elements)
          ((20, 45, 24), (32, 32, 16)),      # more than one workgroup in both passes
          ((24, 45, 40), (8, 8, 4)),         # a downsample
          ((8, 8, 4), (8, 8, 4))]            # identity grid: min-max alone
_ORACLE = {}


def stored(vals, datatype, endian):
    """the values as the file would hold them: the datatype's numpy type in byte order `endian`"""
    letter = NR.TYPES[datatype][0]
    return vals.astype(np.dtype(endian + letter) if letter[1] != "1" else np.dtype(letter))


def oracle(key, vals, slope, inter, target):
    """computed once per case and shared; never modified"""
    from oracle import preproc as OP
    k = (key, slope, inter, target)
    if k not in _ORACLE:
        s, i = (1.0, 0.0) if slope == 0 else (slope, inter)
        w = OP.ct_preprocess(s * vals.astype(np.float64) + i, target)
        w.setflags(write=False)
        _ORACLE[k] = w
    return _ORACLE[k]


def run(vols, target, n_rows=None, rows=None, fill=None):
    """vols: [(stored array, slope, inter, swap)] -> the image store after ONE ct_preprocess_batch call"""
    from multimodal_survival_prediction_amd import cohort_io
    rows = list(range(len(vols))) if rows is None else rows
    out = torch.full((n_rows or len(vols), 1) + tuple(target), 0.0 if fill is None else fill, device=DEV)
    cohort_io.ct_preprocess_batch(vols, target, out, rows)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("datatype", sorted(NR.TYPES))
@pytest.mark.parametrize("native,target", SHAPES)
def test_one_volume_every_type_and_byte_order(native, target, datatype):
    vals = NR.ct_values(native, datatype, seed=sum(native) + datatype)
    want = torch.tensor(oracle((native, datatype), vals, 1.0, 0.0, target))
    got = {}
    for endian in (NATIVE, OTHER):
        got[endian] = run([(stored(vals, datatype, endian), 1.0, 0.0, endian != NATIVE)], target)[0, 0]
        assert got[endian].shape == tuple(target)
        assert_close(got[endian], want, 1e-5, "dtype %d %s %s->%s" % (datatype, endian, native, target))
    assert torch.equal(got[NATIVE], got[OTHER])                   # the byte order is a property of the file, not of the values
    assert float(got[NATIVE].min()) >= 0.0 and float(got[NATIVE].max()) <= 1.0 + 1e-6      # (an interpolated value may round an ulp up)
    if native == target:
        assert float(got[NATIVE].min()) == 0.0 and abs(float(got[NATIVE].max()) - 1.0) <= 1e-6


@pytest.mark.parametrize("native,target", [((3, 5, 7), (8, 8, 4)), ((24, 45, 40), (8, 8, 4))])
@pytest.mark.parametrize("datatype", [4, 512, 16, 64])
def test_slope_and_intercept(native, target, datatype):
    vals = NR.ct_values(native, datatype, seed=5 + datatype)
    raw = stored(vals, datatype, NATIVE)
    one, zero = run([(raw, 1.0, 0.0, False)], target), run([(raw, 0.0, 0.0, False)], target)
    assert torch.equal(one, zero)                                  # scl_slope 0 = no scaling, whatever scl_inter says
    assert torch.equal(one, run([(raw, 0.0, 55.0, False)], target))
    for slope, inter in ((2.5, -1024.0), (-1.0, 100.0)):           # a negative slope swaps the extremes
        got = run([(raw, slope, inter, False)], target)[0, 0]
        assert_close(got, torch.tensor(oracle((native, datatype, "s"), vals, slope, inter, target)), 1e-5, "slope %g inter %g" % (slope, inter))
    # min-max normalisation forgets a positive affine map of the values; a negative slope mirrors it
    assert_close(run([(raw, 2.5, -1024.0, False)], target), one, 1e-6, "positive slope")
    assert_close(run([(raw, -1.0, 100.0, False)], target), 1.0 - one, 1e-6, "negative slope")


@pytest.mark.parametrize("datatype", sorted(NR.TYPES))
def test_constant_volume_is_exactly_zero(datatype):
    vals = np.full((5, 6, 7), 100)
    for slope, inter in ((1.0, 0.0), (2.5, -1024.0), (-1.0, 100.0)):
        got = run([(stored(vals, datatype, OTHER), slope, inter, True)], (8, 8, 4), fill=-3.0)
        assert torch.equal(got, torch.zeros_like(got))


# the same bytes read with the other signedness: what a kernel that mixed up two MMS_CT_* cases would see
SIGN_TWIN = {512: "i2", 4: "u2", 768: "i4", 8: "u4"}


@pytest.mark.parametrize("datatype", sorted(NR.TYPES))
def test_full_range_values_every_type_and_byte_order(datatype):
    """values at the ends of the stored type (NR.full_range_values), fractional ones for the float types.  Guard, from the oracle alone:
    for the 16- and 32-bit integers the oracle of the same bytes under the other signedness is at least 100 tolerances away, so reading
    MMS_CT_U16 as int16 (or MMS_CT_U32 as int32, or the reverse) cannot pass"""
    native, target = (3, 5, 7), (8, 8, 4)
    vals = NR.full_range_values(native, datatype, seed=300 + datatype)
    want = torch.tensor(oracle(("full", datatype), vals, 1.0, 0.0, target))
    if datatype in SIGN_TWIN:
        twin = np.ascontiguousarray(vals).view(np.dtype(SIGN_TWIN[datatype]))
        assert twin.shape == vals.shape and not np.array_equal(twin.astype(np.float64), vals.astype(np.float64))
        wrong = torch.tensor(oracle(("full twin", datatype), twin, 1.0, 0.0, target))
        assert float((wrong - want).abs().max()) >= 100 * 1e-5
    else:
        assert datatype in (2, 256, 16, 64)
    if datatype in (16, 64):
        assert not np.array_equal(vals, np.rint(vals))              # fractional values
    got = {}
    for endian in (NATIVE, OTHER):
        got[endian] = run([(stored(vals, datatype, endian), 1.0, 0.0, endian != NATIVE)], target, fill=-3.0)[0, 0]
        assert_close(got[endian], want, 1e-5, "full range dtype %d %s" % (datatype, endian))
    assert torch.equal(got[NATIVE], got[OTHER])
    assert float(got[NATIVE].min()) >= 0.0 and float(got[NATIVE].max()) <= 1.0 + 1e-6


def test_float64_elements_round_to_float32_at_the_load():
    """The contract of csrc/ct_ingest.hip's header: a float64 element is rounded to the nearest fp32 at the load, as a host
    astype(float32) rounds it.  So the yardstick here is the oracle of vals.astype(float32) -- NOT the oracle of the float64 values, which
    is further than the tolerance away for 1000 + U[0, 1) (fp32 steps of 6e-5 on a range of 1): asserted below from the oracle alone"""
    native, target = (5, 6, 7), (8, 8, 4)
    vals = 1000.0 + np.random.default_rng(64).random(native)
    assert vals.dtype == np.float64 and not np.array_equal(vals, vals.astype(np.float32))
    want = torch.tensor(oracle("f8 rounded", vals.astype(np.float32), 1.0, 0.0, target))
    unrounded = torch.tensor(oracle("f8 as stored", vals, 1.0, 0.0, target))
    assert float((unrounded - want).abs().max()) > 1e-5
    for endian in (NATIVE, OTHER):
        got = run([(stored(vals, 64, endian), 1.0, 0.0, endian != NATIVE)], target, fill=-3.0)[0, 0]
        assert_close(got, want, 1e-5, "float64 %s" % endian)


@pytest.mark.parametrize("native,target", [((5, 6, 7), (8, 8, 4)), ((20, 45, 24), (32, 32, 16))])
def test_stored_float32_low_contrast_on_an_offset(native, target):
    """1000 + U[0, 1e-3): r - rmin is interpolated, so the error scales with the contrast and not with the offset"""
    vals = NR.low_contrast_values("sub_ulp", native, seed=sum(native))
    want = torch.tensor(oracle(("sub_ulp", native), vals, 1.0, 0.0, target))
    for endian in (NATIVE, OTHER):
        got = run([(stored(vals, 16, endian), 1.0, 0.0, endian != NATIVE)], target, fill=-3.0)[0, 0]
        assert_close(got, want, 1e-5, "low contrast %s" % endian)
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0 + 1e-6


# ---- scan size: pass 1 at its MMS_CT_RAW_PARTS cap, more than one sweep of the output loop of pass 2 ---------------------------------
SCAN_NATIVE = (129, 127, 129)                # 2,113,407 int16 elements = 4.23 MB > 256 x 16 KiB; odd: a 7-element scalar tail
SCAN_SWEEP = 256 * 256 * 8                   # int16 elements the capped grid of pass 1 reads in one sweep
_SCAN = {}


def scan_volume():
    """shared, never modified: the only minimum where a second sweep of pass 1 reads it, the only maximum in the last element (the tail)"""
    if not _SCAN:
        v = NR.scan_values(SCAN_NATIVE, "i2", seed=11, min_at=SCAN_SWEEP + 300001)
        assert v.size % 8 == 7 and v.nbytes > 256 * 16384 and int(v.argmin()) >= SCAN_SWEEP and int(v.argmax()) == v.size - 1
        v.setflags(write=False)
        _SCAN["v"] = v
    return _SCAN["v"]


@pytest.mark.parametrize("target", [(64, 64, 17), (64, 64, 32)])
def test_scan_size_volume(target):
    """(64, 64, 17) = 69,632 voxels: a ragged second sweep of the 256-workgroup output loop; (64, 64, 32): the production grid, two sweeps"""
    from test_ingest_abi import _limit
    assert _limit("MMS_CT_RAW_PARTS") == 256 and int(np.prod(target)) > 256 * 256
    vals = scan_volume()
    want = torch.tensor(oracle("scan", vals, 1.0, 0.0, target))
    got = {}
    for endian in (NATIVE, OTHER):
        got[endian] = run([(stored(vals, 4, endian), 1.0, 0.0, endian != NATIVE)], target, fill=-3.0)[0, 0]
        assert_close(got[endian], want, 1e-5, "scan %s->%s %s" % (SCAN_NATIVE, target, endian))
        assert float(got[endian].min()) >= 0.0 and float(got[endian].max()) <= 1.0 + 1e-6
    assert torch.equal(got[NATIVE], got[OTHER])


def test_scan_size_volume_next_to_small_ones_in_one_launch():
    """nb = 256 next to nb = 1 in one grid: the small volumes' workgroups b >= 1 of pass 1 return early.  Every row equals its own
    single-volume launch bit for bit"""
    target = (64, 64, 17)
    small = [NR.ct_values((3, 5, 7), dt, seed=400 + dt) for dt in (4, 16)]
    vols = [(stored(small[0], 4, OTHER), 1.0, 0.0, True), (stored(scan_volume(), 4, NATIVE), 1.0, 0.0, False),
            (stored(small[1], 16, NATIVE), 1.0, 0.0, False)]
    got = run(vols, target, n_rows=4, rows=[2, 0, 3], fill=-3.0)
    assert torch.equal(got[1], torch.full_like(got[1], -3.0))
    for vol, row in zip(vols, [2, 0, 3]):
        assert torch.equal(got[row], run([vol], target, fill=-3.0)[0]), "row %d depends on its launch" % row
    assert_close(got[0, 0], torch.tensor(oracle("scan", scan_volume(), 1.0, 0.0, target)), 1e-5, "scan volume in a mixed launch")


MIX = [((3, 5, 7), 4, NATIVE, 1.0, 0.0), ((20, 45, 24), 512, OTHER, 1.0, -1024.0), ((5, 7, 1), 16, OTHER, 0.0, 0.0),
       ((24, 45, 40), 2, NATIVE, 2.5, -1024.0), ((8, 8, 4), 64, OTHER, -1.0, 100.0), ((20, 45, 24), 8, NATIVE, 1.0, 0.0),
       ((3, 5, 7), 768, OTHER, 0.5, 3.0)]


def test_seven_mixed_volumes_in_one_launch():
    """mixed sizes, types and byte orders, out rows shuffled into a 9-row store: the two rows not named keep their bits, every volume
    equals its own single-volume call bit for bit (nothing depends on what shares the launch) and the oracle"""
    target = (8, 8, 4)
    vols, cases = [], []
    for j, (native, datatype, endian, slope, inter) in enumerate(MIX):
        vals = NR.ct_values(native, datatype, seed=100 + j)
        vols.append((stored(vals, datatype, endian), slope, inter, endian != NATIVE))
        cases.append((vals, slope, inter))
    rows = [6, 0, 8, 3, 1, 7, 4]
    sentinel = -7.25
    got = run(vols, target, n_rows=9, rows=rows, fill=sentinel)
    for r in (2, 5):
        assert torch.equal(got[r], torch.full_like(got[r], sentinel))
    for j, (vol, row) in enumerate(zip(vols, rows)):
        alone = run([vol], target)
        assert torch.equal(got[row], alone[0]), "volume %d depends on its launch" % j
        vals, slope, inter = cases[j]
        assert_close(got[row, 0], torch.tensor(oracle(("mix", j), vals, slope, inter, target)), 1e-5, "mixed volume %d" % j)


def test_more_volumes_than_one_chunk():
    """V = 40 > MMS_CT_RAW_CHUNK = 32 descriptors by value: two launch pairs in one call, every row right"""
    from test_ingest_abi import _limit
    assert _limit("MMS_CT_RAW_CHUNK") == 32
    target, native = (8, 8, 4), (3, 5, 7)
    types = sorted(NR.TYPES)
    vals = [NR.ct_values(native, types[j % 8], seed=200 + j) for j in range(40)]
    vols = [(stored(v, types[j % 8], OTHER if j % 3 else NATIVE), 1.0, 0.0, bool(j % 3)) for j, v in enumerate(vals)]
    rows = list(np.random.default_rng(0).permutation(40))
    got = run(vols, target, rows=[int(r) for r in rows])
    for j in range(40):
        assert_close(got[rows[j], 0], torch.tensor(oracle(("forty", j), vals[j], 1.0, 0.0, target)), 1e-5, "volume %d of 40" % j)


def test_bad_batches_are_refused():
    from multimodal_survival_prediction_amd import cohort_io, _lib
    raw = stored(NR.ct_values((3, 5, 7), 4, seed=1), 4, NATIVE)
    out = torch.zeros(2, 1, 8, 8, 4, device=DEV)
    with pytest.raises(_lib.MmsError):
        cohort_io.ct_preprocess_batch([(raw, 1.0, 0.0, False)] * 2, (8, 8, 4), out, [1, 1])          # one row twice
    with pytest.raises(_lib.MmsError):
        cohort_io.ct_preprocess_batch([(raw, 1.0, 0.0, False)], (8, 8, 4), out, [2])                # row outside the store
    with pytest.raises(ValueError):
        cohort_io.ct_preprocess_batch([(raw, 1.0, 0.0, False)], (8, 8, 8), out, [0])                # another grid than the store's
    with pytest.raises(RuntimeError):
        cohort_io.ct_preprocess_batch([(raw, 1.0, 0.0, False)], (8, 8, 4), out.cpu(), [0])          # no CPU fallback
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


# ---- pipeline -----------------------------------------------------------------------------------------------------------------------
DIMS = (32, 32, 16)


@pytest.fixture(scope="module")
def nifti_cohort(tmp_path_factory):
    """the 14-patient cohort of tests/test_gpu_preproc.py::test_cohort_roundtrip_through_disk, its volumes as .nii.gz at (20, 45, 24)"""
    from multimodal_survival_prediction_amd import cohort_io, data
    root = str(tmp_path_factory.mktemp("nifti_cohort"))
    c = data.make_cohort(n=14, dims=DIMS, rna_dim=40, seed=9, complete=False, counts=dict(n=14, imaging=9, rnaseq=10, clinical=12, survival=8))
    cohort_io.write_cohort(root, c, native_dims=(20, 45, 24), seed=3, volume_format="nii.gz")
    return root, c


def test_nifti_cohort_through_the_pipeline(nifti_cohort, tmp_path, monkeypatch):
    from multimodal_survival_prediction_amd import cohort_io
    root, c = nifti_cohort
    got = cohort_io.load_cohort(root, DEV, target_size=DIMS)
    torch.cuda.synchronize()
    assert got["n"] == 14 and got["rnaseq"].shape == (14, 40)
    assert torch.equal(got["mask"].cpu(), c["mask"]) and torch.equal(got["has_survival"].cpu(), c["has_survival"])
    assert_close(got["rnaseq"], c["rnaseq"], 1e-6, "rnaseq"); assert_close(got["clinical"], c["clinical"], 1e-6, "clinical")
    assert_close(got["label"], c["label"], 1e-6, "label")
    mt, _ = cohort_io.read_tables(root)
    kinds, n_img = set(), 0
    for i, p in enumerate(mt["nifti_path"]):
        if isinstance(p, str):
            f = NR.parse(p)
            kinds.add((f["datatype"], f["endian"]))
            n_img += 1
            from oracle import preproc as OP
            assert_close(got["image"][i, 0], torch.tensor(OP.ct_preprocess(NR.scaled(f), DIMS)), 1e-5, "image %d" % i)
            A, native = got["geometry"][i]
            assert np.array_equal(A, f["affine"]) and tuple(native) == (20, 45, 24)
        else:
            assert float(got["image"][i].abs().max()) == 0.0 and got["geometry"][i] is None
    assert n_img == 9 and len(kinds) >= 2                          # the synthetic cohort mixes stored types
    assert len(got["geometry"]) == 14
    # the store does not depend on the thread count or on how the volumes fall into batches
    for kw in (dict(threads=1), dict(threads=4), dict(stage_bytes=1 << 30), dict(stage_bytes=1), dict(threads=4, stage_bytes=100000)):
        again = cohort_io.load_cohort(root, DEV, target_size=DIMS, **kw)
        torch.cuda.synchronize()
        assert torch.equal(again["image"], got["image"]), kw
    # relative nifti_path entries are found under root from any working directory
    import pandas as pd
    import shutil
    moved = tmp_path / "moved"
    shutil.copytree(root, moved)
    t = pd.read_csv(moved / cohort_io.TABLE)
    t["nifti_path"] = [os.path.relpath(p, root) if isinstance(p, str) else p for p in t["nifti_path"]]
    t.to_csv(moved / cohort_io.TABLE, index=False)
    (tmp_path / "elsewhere").mkdir()
    monkeypatch.chdir(tmp_path / "elsewhere")
    rel = cohort_io.load_cohort(str(moved), DEV, target_size=DIMS)
    torch.cuda.synchronize()
    assert torch.equal(rel["image"], got["image"]) and torch.equal(rel["mask"], got["mask"])


def test_unreadable_volume_counts_as_missing(nifti_cohort, tmp_path):
    """a truncated .nii.gz among good files: mask 0, zeros, ONE warning naming it (the reference's `except: pass`); strict=True raises"""
    import shutil
    from multimodal_survival_prediction_amd import cohort_io
    root, c = nifti_cohort
    bad_root = tmp_path / "cut"
    shutil.copytree(root, bad_root)
    import pandas as pd
    t = pd.read_csv(bad_root / cohort_io.TABLE)
    t["nifti_path"] = [p.replace(root, str(bad_root)) if isinstance(p, str) else p for p in t["nifti_path"]]
    t.to_csv(bad_root / cohort_io.TABLE, index=False)
    have = [i for i, p in enumerate(t["nifti_path"]) if isinstance(p, str)]
    victim = have[3]
    blob = open(t["nifti_path"][victim], "rb").read()
    open(t["nifti_path"][victim], "wb").write(blob[:len(blob) // 2])
    good = cohort_io.load_cohort(root, DEV, target_size=DIMS)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = cohort_io.load_cohort(str(bad_root), DEV, target_size=DIMS, stage_bytes=200000)
    torch.cuda.synchronize()
    mine = [x for x in w if "could not be read" in str(x.message)]
    assert len(mine) == 1 and os.path.basename(t["nifti_path"][victim]) in str(mine[0].message)
    assert float(got["mask"][victim, 0]) == 0.0 and float(got["image"][victim].abs().max()) == 0.0 and got["geometry"][victim] is None
    keep = [i for i in range(14) if i != victim]
    assert torch.equal(got["image"][keep], good["image"][keep]) and torch.equal(got["mask"][keep], good["mask"][keep])
    with pytest.raises(ValueError, match=os.path.basename(t["nifti_path"][victim])):
        cohort_io.load_cohort(str(bad_root), DEV, target_size=DIMS, strict=True)


def test_attribution_maps_as_nifti(tmp_path, monkeypatch):
    """evaluate_model.py --predict ... --attribute --attribute-format nii on a tiny NIfTI cohort: the files parse (test-side parser), hold
    the .npy output of the same run configuration, and carry A_src . diag(sx, sy, sz, 1) of the loader's resample"""
    import image_only_ref as R
    from multimodal_survival_prediction_amd import cohort_io, data
    spec = importlib.util.spec_from_file_location("evaluate_model", os.path.join(ROOT, "scripts", "analysis", "evaluate_model.py"))
    em = importlib.util.module_from_spec(spec); spec.loader.exec_module(em)
    dims, native = (16, 16, 8), (12, 20, 9)
    c = data.make_cohort(n=48, dims=dims, rna_dim=8, seed=4, complete=False, counts=dict(n=48, imaging=40, rnaseq=24, clinical=40, survival=44))
    root = tmp_path / "cohort"
    cohort_io.write_cohort(str(root), c, native_dims=native, seed=1, volume_format="nii.gz")
    for k, v in dict(MMS_DATA_ROOT=str(root), MMS_VOLUME="16,16,8", MMS_FOLDS="2", MMS_BATCH_SIZE="4").items():
        monkeypatch.setenv(k, v)
    torch.manual_seed(3)
    torch.save(R.ImageOnlyModel().state_dict(), tmp_path / "fold_1_best.pth")
    base = ["--predict", str(tmp_path / "fold_1_best.pth"), "--model", "image_only", "--fold", "1", "--no-plots", "--attribute"]
    em.main(base + ["--predictions", str(tmp_path / "a" / "pred.csv"), "--outdir", str(tmp_path / "a")])
    em.main(base + ["--predictions", str(tmp_path / "b" / "pred.csv"), "--outdir", str(tmp_path / "b"), "--attribute-format", "nii"])
    assert open(tmp_path / "a" / "pred.csv", "rb").read() == open(tmp_path / "b" / "pred.csv", "rb").read()
    npys = sorted(os.listdir(tmp_path / "a" / "attribution"))
    niis = sorted(os.listdir(tmp_path / "b" / "attribution"))
    assert len(npys) >= 4 and all(f.endswith("_ct.npy") for f in npys) and niis == [f[:-4] + ".nii.gz" for f in npys]
    mt, _ = cohort_io.read_tables(str(root))
    src = {pid: p for pid, p in zip(mt["patient_id"], mt["nifti_path"])}
    for f_npy, f_nii in zip(npys, niis):
        want = np.load(tmp_path / "a" / "attribution" / f_npy)
        f = NR.parse(str(tmp_path / "b" / "attribution" / f_nii))
        assert f["datatype"] == 16 and f["data"].shape == dims and np.array_equal(f["data"], want) and np.abs(want).max() > 0
        A_src = NR.parse(src[f_npy[:-len("_ct.npy")]])["affine"]
        rule = A_src @ np.diag([(native[2] - 1) / (dims[2] - 1), (native[1] - 1) / (dims[1] - 1), (native[0] - 1) / (dims[0] - 1), 1.0])
        assert np.allclose(f["affine"], rule, rtol=1e-6, atol=1e-6) and f["sform_code"] == 1
