"""On-disk cohort contract of the reference + a GPU-side loader.

The reference's datasets read, relative to the cwd (partial_modality_training.py:60-158, simple_fusion.py:98-154,
flexible_multimodal.py:96-151, create_full_matching_table.py:124-134):
    data/processed/full_matching_table.csv    patient_id, nifti_path, has_imaging, has_rnaseq, has_clinical, age,
                                              survival_time, survival_status, has_survival
    data/processed/rnaseq_normalized_mapped.csv    patient-indexed, one column per gene (5005)
and, per item and on the CPU, look the patient's row up in a DataFrame, read the NIfTI volume, min-max normalise it and
scipy.zoom it (order 1) to 64x64x32 -- O(cohort) pandas work plus a resample per sample per epoch, with num_workers = 0.

`write_cohort` lays a synthetic cohort down in that contract; `load_cohort` reads the contract ONCE into an HBM-resident
tensor store (the dict `data.make_cohort` produces), doing the volume preprocessing on the GPU.
A `nifti_path` ending in .nii / .nii.gz is the reference's real file format, read by nifti.py (numpy + zlib): a thread pool inflates
the files into pinned staging buffers, the stored elements go to the device as they are and `mms_ct_preprocess_raw_batch`
(csrc/ct_ingest.hip) converts, min-max normalises and resamples a whole batch of volumes per launch pair.  A path ending in .npy is a
float volume saved with numpy and keeps the one-volume `mms_ct_preprocess` path.  Everything else is the reference's layout, so its own
CSV tooling reads these files.
"""
import ctypes
import os
import re
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib, nifti, ops

TABLE = os.path.join("data", "processed", "full_matching_table.csv")
RNASEQ = os.path.join("data", "processed", "rnaseq_normalized_mapped.csv")
COLUMNS = ["patient_id", "nifti_path", "has_imaging", "has_rnaseq", "has_clinical", "age", "survival_time", "survival_status",
           "has_survival"]


VOLUME_FORMATS = ("npy", "nii", "nii.gz")


def _write_nifti_volume(path, v, i, arng):
    """Volume i of a synthetic cohort as NIfTI: the HU-like values rounded to int16, with an anisotropic affine drawn from arng.  Every
    third patient is stored otherwise, in turn: big-endian int16, float32, uint16 with the offset in scl_inter -- one cohort has the mix."""
    hu = np.rint(v).astype(np.int16)
    A = np.eye(4)
    A[:3, :3] = np.diag(arng.uniform(0.6, 1.2, 3) * np.array([1.0, 1.0, 3.0]))         # (x, y, z) spacing: thick slices
    A[:3, 3] = arng.uniform(-200.0, 200.0, 3)
    kind = (i // 3) % 3 if i % 3 == 1 else -1
    if kind == 0:
        blob = nifti.encode(hu, A, endian=">")
    elif kind == 1:
        blob = nifti.encode(hu.astype(np.float32), A)
    elif kind == 2:
        blob = nifti.encode((hu.astype(np.int32) + 1024).astype(np.uint16), A, slope=1.0, inter=-1024.0)
    else:
        blob = nifti.encode(hu, A)
    nifti.dump(path, blob)


def write_cohort(root, cohort, native_dims=None, seed=0, volume_format="npy"):
    """cohort: CPU dict from data.make_cohort.  native_dims: store each volume resampled to this (D, H, W) -- i.e. at a
    'scanner' resolution different from the network grid -- so that loading exercises the resample; None = network grid.
    Raw intensities get a per-patient offset/scale (the loader's min-max must undo it).
    volume_format: "npy" (float32 arrays) or "nii" / "nii.gz" (NIfTI-1, _write_nifti_volume)."""
    if volume_format not in VOLUME_FORMATS:
        raise ValueError("volume_format must be one of %s" % (VOLUME_FORMATS,))
    import pandas as pd
    import torch.nn.functional as F
    n = cohort["n"]
    os.makedirs(os.path.join(root, "data", "processed"), exist_ok=True)
    os.makedirs(os.path.join(root, "data", "volumes"), exist_ok=True)
    rng = np.random.default_rng(seed)
    arng = np.random.default_rng([seed, 1])                  # the affines' own stream: the intensities do not depend on the format
    mask = cohort["mask"].numpy().astype(bool)
    has_surv = cohort["has_survival"].numpy().astype(bool)
    rows, rna_rows, rna_ids = [], [], []
    for i in range(n):
        pid = "TCGA-SYN-%04d" % i
        path = None
        if mask[i, 0]:
            v = cohort["image"][i:i + 1]
            if native_dims is not None:
                v = F.interpolate(v, size=tuple(native_dims), mode="trilinear", align_corners=True)
            v = v[0, 0].numpy() * float(rng.uniform(500, 3000)) + float(rng.uniform(-1000, 0))      # HU-like range
            path = os.path.join(root, "data", "volumes", pid + "." + volume_format)
            if volume_format == "npy":
                np.save(path, v.astype(np.float32))
            else:
                _write_nifti_volume(path, v, i, arng)
        if mask[i, 1]:
            rna_ids.append(pid); rna_rows.append(cohort["rnaseq"][i].numpy())
        lab = cohort["label"][i].numpy()
        rows.append([pid, path, bool(mask[i, 0]), bool(mask[i, 1]), bool(mask[i, 2]),
                     float(cohort["clinical"][i, 0]) * 100.0 if mask[i, 2] else np.nan,
                     float(lab[0]) if has_surv[i] else np.nan, int(lab[1]) if has_surv[i] else np.nan, bool(has_surv[i])])
    pd.DataFrame(rows, columns=COLUMNS).to_csv(os.path.join(root, TABLE), index=False)
    g = cohort["rnaseq"].shape[1]
    pd.DataFrame(np.stack(rna_rows) if rna_rows else np.zeros((0, g), np.float32), index=rna_ids,
                 columns=["ENSG%011d" % j for j in range(g)]).to_csv(os.path.join(root, RNASEQ), float_format="%.9g")
    return os.path.join(root, TABLE)


def ct_preprocess(vol_dev, target_size, out=None, scratch=None):
    """vol_dev: (D, H, W) fp32 device tensor at its native resolution -> (tD, tH, tW): min-max normalise + order-1 resample."""
    if not vol_dev.is_cuda:
        raise RuntimeError("ct_preprocess runs on the MI355X (no CPU fallback)")
    v = vol_dev.contiguous().float()
    if out is None:
        out = torch.empty(tuple(target_size), device=v.device)
    if scratch is None:
        scratch = torch.empty(512, device=v.device)
    _lib.check(_lib.load_library().mms_ct_preprocess(v.data_ptr(), v.shape[0], v.shape[1], v.shape[2], out.data_ptr(),
                                                    target_size[0], target_size[1], target_size[2], scratch.data_ptr(), ops.stream()),
               "mms_ct_preprocess")
    return out


def _align16(n):
    return (n + 15) & ~15


def _raw_descriptor(raw, slope, inter, swap, offset, row):
    nz, ny, nx = raw.shape
    return _lib.structs()["CtRawVol"](offset=offset, D=nz, H=ny, W=nx, dtype=nifti.dtype_code(raw.dtype), swap=int(bool(swap)),
                                      out_row=int(row), slope=float(slope), inter=float(inter))


def _launch_raw_batch(stage_dev, nbytes, descs, target_size, out, scratch, passes=0):
    S = _lib.structs()
    vols = (S["CtRawVol"] * max(1, len(descs)))(*descs)
    p = S["CtRawBatchP"](base=stage_dev.data_ptr(), base_bytes=nbytes, vols=ctypes.cast(vols, ctypes.c_void_p), V=len(descs),
                         n_rows=out.shape[0], out=out.data_ptr(), oD=target_size[0], oH=target_size[1], oW=target_size[2],
                         passes=passes, scratch=scratch.data_ptr())
    _lib.check(_lib.load_library().mms_ct_preprocess_raw_batch(ctypes.byref(p), ops.stream()), "mms_ct_preprocess_raw_batch")


def _check_store(out, target_size):
    if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()):
        raise RuntimeError("ct_preprocess_batch writes a contiguous fp32 image store on the MI355X (no CPU fallback)")
    if out.dim() < 4 or tuple(out.shape[-3:]) != tuple(target_size) or out[0].numel() != int(np.prod(target_size)):
        raise ValueError("image store %s is not [n, (1,) %d, %d, %d]" % ((tuple(out.shape),) + tuple(target_size)))


def _lib_limit(name):
    """a numeric #define of include/mmsurv.h (the limits of the C ABI are stated there only)"""
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(_lib.HEADER).read()).group(1))


def _raw_scratch(dev):
    return torch.empty(_lib_limit("MMS_CT_RAW_SCRATCH_FLOATS"), device=dev)


def ct_preprocess_batch(raws, target_size, out, rows):
    """raws: list of (raw, slope, inter, swap) -- raw a (nz, ny, nx) ndarray in its STORED dtype (one of nifti.DTYPES, either byte
    order), swap: its bytes are in the other order than the host's -- as nifti.read_nifti / nifti.scaling give them.  Each volume is
    min-max normalised and resampled (order 1) to target_size into row rows[k] of the image store `out` [n, 1, tD, tH, tW] (device,
    fp32) by ONE call of mms_ct_preprocess_raw_batch: the stored bytes are staged to the device as they are."""
    _check_store(out, target_size)
    if len(raws) != len(rows):
        raise ValueError("%d volumes for %d rows" % (len(raws), len(rows)))
    if not raws:
        return out
    offs, total = [], 0
    for raw, _, _, _ in raws:
        offs.append(total)
        total = _align16(total + raw.nbytes)
    host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    descs = []
    for (raw, slope, inter, swap), off, row in zip(raws, offs, rows):
        if raw.ndim != 3:
            raise ValueError("a volume has three dimensions, got shape %s" % (raw.shape,))
        hv[off:off + raw.nbytes] = np.ascontiguousarray(raw).reshape(-1).view(np.uint8)
        descs.append(_raw_descriptor(raw, slope, inter, swap, off, row))
    stage = torch.empty(total, dtype=torch.uint8, device=out.device)
    stage.copy_(host, non_blocking=True)
    _launch_raw_batch(stage, total, descs, target_size, out, _raw_scratch(out.device))
    return out


def _load_threads(threads):
    t = int(threads) if threads is not None else int(os.environ.get("MMS_LOAD_THREADS", "8"))
    return max(1, min(16, t))              # never sized by the machine's CPU count


def _ingest_nifti(jobs, image, target_size, threads, stage_bytes, strict):
    """jobs: [(row, path)] -> (geometry by row, loaded rows, failures [(path, reason)]).  Three stages: (1) the pool reads every header;
    the batches -- as many volumes as fit stage_bytes, a larger one alone -- and every volume's slot in them follow from the headers
    alone, so the image store does not depend on threads or stage_bytes; (2) the pool inflates batch k + 1 into one pinned buffer
    while (3) batch k, in the other, is copied to the device staging buffer and preprocessed by one call."""
    geometry, loaded, failures = {}, [], []

    def fail(path, e):
        if strict:
            raise ValueError("load_cohort(strict=True): cannot read %s: %s" % (path, e)) from e
        failures.append((path, "%s: %s" % (type(e).__name__, e)))

    def header_of(path):
        try:
            return nifti.read_header(path)
        except (ValueError, OSError, EOFError) as e:
            return e

    max_vols = _lib_limit("MMS_CT_RAW_MAX_VOLS")
    with ThreadPoolExecutor(max_workers=threads) as pool:
        batches, cur, cur_bytes = [], [], 0
        for (row, path), h in zip(jobs, pool.map(header_of, [p for _, p in jobs])):
            if isinstance(h, Exception):
                fail(path, h)
                continue
            nb = nifti.data_bytes(h)
            if nb >= 8 * 2 ** 31 or int(np.prod(h["shape"], dtype=np.int64)) >= 2 ** 31:
                fail(path, ValueError("dim: %s voxels, the loader takes fewer than 2^31" % (h["dim"][1:4],)))
                continue
            if cur and (cur_bytes + nb > stage_bytes or len(cur) >= max_vols):
                batches.append((cur, cur_bytes)); cur, cur_bytes = [], 0
            cur.append((row, path, h, cur_bytes))
            cur_bytes = _align16(cur_bytes + nb)
        if cur:
            batches.append((cur, cur_bytes))
        if not batches:
            return geometry, loaded, failures
        cap = max(b for _, b in batches)
        pinned = [torch.empty(cap, dtype=torch.uint8, pin_memory=True) for _ in range(min(2, len(batches)))]
        copied = [None] * len(pinned)                       # event behind the last host-to-device copy out of each pinned buffer
        stage = torch.empty(cap, dtype=torch.uint8, device=image.device)
        scratch = _raw_scratch(image.device)

        def inflate(args):
            (row, path, h, off), view = args
            try:
                nifti.read_into(path, h, view[off:off + nifti.data_bytes(h)])
            except (ValueError, OSError, EOFError) as e:
                return e
            return None

        def submit(k):
            b = k % len(pinned)
            if copied[b] is not None:
                copied[b].synchronize()                      # the buffer's previous batch has left for the device
            view = pinned[b].numpy()
            return [pool.submit(inflate, (vol, view)) for vol in batches[k][0]]

        pending = submit(0)
        for k, (vols, nbytes) in enumerate(batches):
            futures, b = pending, k % len(pinned)
            results = [f.result() for f in futures]
            stage[:nbytes].copy_(pinned[b][:nbytes], non_blocking=True)
            copied[b] = torch.cuda.Event()
            copied[b].record()
            if k + 1 < len(batches):
                pending = submit(k + 1)                      # inflates while this batch is copied and preprocessed
            descs = []
            for (row, path, h, off), err in zip(vols, results):
                if err is not None:
                    fail(path, err)
                    continue
                slope, inter = nifti.scaling(h)
                nz, ny, nx = h["shape"]
                descs.append(_lib.structs()["CtRawVol"](offset=off, D=nz, H=ny, W=nx, dtype=h["datatype"], swap=int(h["swap"]),
                                                        out_row=row, slope=slope, inter=inter))
                geometry[row] = (nifti.affine_of(h), h["shape"])
                loaded.append(row)
            _launch_raw_batch(stage, nbytes, descs, target_size, image, scratch)
    return geometry, loaded, failures


def rna_log_zscore(counts_dev):
    """counts_dev: (n, genes) fp32 device tensor of raw counts -> z-scored log2(count + 1) (preprocess_genomic.py:108-117)."""
    if not counts_dev.is_cuda:
        raise RuntimeError("rna_log_zscore runs on the MI355X (no CPU fallback)")
    c = counts_dev.contiguous().float()
    out = torch.empty_like(c)
    _lib.check(_lib.load_library().mms_rna_log_zscore(c.data_ptr(), out.data_ptr(), c.shape[0], c.shape[1], ops.stream()),
               "mms_rna_log_zscore")
    return out


def read_tables(root):
    """-> (matching table DataFrame, rnaseq DataFrame or None): the host side of the contract (CPU only)."""
    import pandas as pd
    mt = pd.read_csv(os.path.join(root, TABLE))
    missing = [c for c in COLUMNS if c not in mt.columns]
    if missing:
        raise ValueError("full_matching_table.csv lacks columns %s" % missing)
    rp = os.path.join(root, RNASEQ)
    rn = pd.read_csv(rp, index_col=0) if os.path.exists(rp) else None
    return mt, rn


def _is_nifti(path):
    return path.lower().endswith((".nii", ".nii.gz"))


def _find_volume(p, root):
    """nifti_path as the reference looks it up (relative to the cwd), then relative to root; None when there is no such file."""
    if not isinstance(p, str):
        return None
    if os.path.exists(p):
        return p
    if not os.path.isabs(p) and os.path.exists(os.path.join(root, p)):
        return os.path.join(root, p)
    return None


def load_cohort(root, device, target_size=(64, 64, 32), rna_dim=None, threads=None, stage_bytes=None, strict=False):
    """The reference datasets' __getitem__ for every patient, once: -> the HBM-resident cohort dict of data.make_cohort
    (image zeros / rnaseq zeros / clinical 0 where the modality is missing, mask, label, has_survival, patient_id) plus `geometry`, a
    host list with (4 x 4 index-to-world affine, native (nz, ny, nx)) of every patient whose volume is a NIfTI file, else None.
    .nii / .nii.gz volumes take the batched pipeline (_ingest_nifti): threads inflating workers (default MMS_LOAD_THREADS or 8, at most
    16), stage_bytes of staging per batch (default 1 GiB).  A volume that cannot be read is what the reference's `except: pass` makes of
    it -- no image: mask 0, zeros -- and ONE warning lists the files and reasons; strict=True raises instead."""
    import pandas as pd
    mt, rn = read_tables(root)
    n = len(mt)
    g = rn.shape[1] if rn is not None else (rna_dim or 5005)
    dev = torch.device(device)
    image = torch.zeros(n, 1, *target_size, device=dev)
    rna = torch.zeros(n, g)
    clin = torch.zeros(n, 1)
    label = torch.zeros(n, 2)
    mask = torch.zeros(n, 3)
    has_surv = torch.zeros(n, dtype=torch.bool)
    scratch = torch.empty(512, device=dev)
    rn_pos = {pid: i for i, pid in enumerate(rn.index)} if rn is not None else {}
    rn_vals = torch.from_numpy(rn.values.astype(np.float32)) if rn is not None else None
    nifti_jobs = []
    for i, row in enumerate(mt.itertuples(index=False)):
        p = _find_volume(row.nifti_path, root)                  # pd.notna(nifti_path) and os.path.exists (:92)
        if p is not None and _is_nifti(p):
            nifti_jobs.append((i, p))
        elif p is not None:
            vol = torch.from_numpy(np.load(p).astype(np.float32)).to(dev)
            ct_preprocess(vol, target_size, out=image[i, 0], scratch=scratch)
            mask[i, 0] = 1
        if row.patient_id in rn_pos:
            rna[i] = rn_vals[rn_pos[row.patient_id]]
            mask[i, 1] = 1
        if pd.notna(row.age):
            clin[i, 0] = row.age / 100.0
            mask[i, 2] = 1
        if pd.notna(row.survival_time):
            label[i, 0], label[i, 1] = float(row.survival_time), int(row.survival_status)
            has_surv[i] = True
    geometry = [None] * n
    if nifti_jobs:
        geo, loaded, failures = _ingest_nifti(nifti_jobs, image, tuple(int(t) for t in target_size), _load_threads(threads),
                                              int(stage_bytes) if stage_bytes is not None else 1 << 30, strict)
        for i in loaded:
            mask[i, 0] = 1
            geometry[i] = geo[i]
        if failures:
            warnings.warn("%d of %d volumes could not be read and count as missing (mask 0, zeros): %s"
                          % (len(failures), len(nifti_jobs), "; ".join("%s (%s)" % f for f in failures)))
    # real survival times repeat (days); the fused step's Cox loss then follows losses.USE_TORCHSURV (Efron, torchsurv's rule) -- with
    # the switch off it is the Breslow risk-set form, whereas the reference's in-file fallback is order-dependent under ties
    t_lab = label[has_surv, 0]
    n_dup = int(t_lab.numel() - torch.unique(t_lab).numel())
    if n_dup:
        from . import losses
        warnings.warn("cohort has %d repeated survival times among %d labelled patients: tie handling = %s (losses.USE_TORCHSURV = %s)"
                      % (n_dup, int(t_lab.numel()), losses.default_ties(), losses.USE_TORCHSURV))
    return dict(image=image, rnaseq=rna.to(dev), clinical=clin.to(dev), label=label.to(dev), mask=mask.to(dev),
                has_survival=has_surv.to(dev), n=n, dims=tuple(target_size), patient_id=list(mt["patient_id"]), tied_times=n_dup,
                geometry=geometry)
