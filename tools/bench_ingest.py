#!/usr/bin/env python
"""NIfTI ingest (nifti.py + cohort_io.load_cohort + csrc/ct_ingest.hip) on a synthetic cohort in a temporary directory: --volumes int16
volumes of --dims as .nii.gz, and the same values as float32 .npy (the one-volume path load_cohort has always had: the only comparison
basis).  In one process:

  load        wall time of load_cohort on the .nii.gz cohort at threads 1, 4 and 16 and on the .npy cohort, host clock around a call that
              ends in a device synchronise; the variants alternate, --load-reps rounds; median, min, max.  The files are in the page cache
              (they were just written): this is inflate + copy + kernels, not disk.
  passes      mms_ct_preprocess_raw_batch's two passes alone (CtRawBatchP.passes) on all volumes resident in one staging buffer, at most
              32 a call: HIP events around one call, --warmup calls first, --reps timed; per-volume time = call time / volumes.
  copy        a plain device-to-device copy of the same staging bytes, same events, same reps: pass 1 reads every byte once, the copy
              reads and writes every byte.  "pass1_read_gbps" is bytes over pass-1 time, "copy_traffic_gbps" twice the bytes over copy
              time, "pass1_over_copy_traffic" their ratio -- reported, not gated.

The image stores of every load variant are compared before anything is recorded (bit-identical among the NIfTI runs; 1e-5 against the
.npy path, which rounds nothing here either but divides in another order).  Writes --out as JSON and prints it."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), runs=len(xs))


def synth_volume(rng, dims):
    """CT-like int16: a smooth body of soft-tissue values in air, plus noise -- compresses about as a scan does"""
    import numpy as np
    z, y, x = (np.linspace(-1, 1, n, dtype=np.float32) for n in dims)
    r = np.sqrt((z[:, None, None] * 1.1) ** 2 + (y[None, :, None] + rng.uniform(-0.1, 0.1)) ** 2 + (x[None, None, :] * 1.2) ** 2)
    body = np.where(r < 0.8, 40.0 + 300.0 * np.cos(6 * r), -1000.0).astype(np.float32)
    return np.rint(body + rng.normal(0, 8.0, dims).astype(np.float32)).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=24)
    ap.add_argument("--dims", default="96,256,256", help="stored nz,ny,nx")
    ap.add_argument("--target", default="64,64,32")
    ap.add_argument("--load-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "ingest_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import pandas as pd
    import torch
    from multimodal_survival_prediction_amd import cohort_io, nifti

    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest measures on the MI355X: no device, no numbers")
    dev = torch.device("cuda:0")
    V, dims, target = args.volumes, tuple(int(v) for v in args.dims.split(",")), tuple(int(v) for v in args.target.split(","))
    rng = np.random.default_rng(96)
    with tempfile.TemporaryDirectory() as tmp:
        roots = {k: os.path.join(tmp, k) for k in ("nii", "npy")}
        for r in roots.values():
            os.makedirs(os.path.join(r, "data", "processed")); os.makedirs(os.path.join(r, "data", "volumes"))
        rows = {k: [] for k in roots}
        gz_bytes = 0
        t0 = time.perf_counter()
        for i in range(V):
            vol = synth_volume(rng, dims)
            pid = "TCGA-BEN-%04d" % i
            A = np.diag([0.8, 0.8, 2.5, 1.0])
            paths = dict(nii=os.path.join(roots["nii"], "data", "volumes", pid + ".nii.gz"), npy=os.path.join(roots["npy"], "data", "volumes", pid + ".npy"))
            nifti.write_nifti(paths["nii"], vol, affine=A)
            np.save(paths["npy"], vol.astype(np.float32))
            gz_bytes += os.path.getsize(paths["nii"])
            for k in roots:
                rows[k].append([pid, paths[k], True, True, True, 60.0, 100.0 + i, i % 2, True])
        for k, r in roots.items():
            pd.DataFrame(rows[k], columns=cohort_io.COLUMNS).to_csv(os.path.join(r, cohort_io.TABLE), index=False)
            pd.DataFrame(np.zeros((V, 8), np.float32), index=[x[0] for x in rows[k]], columns=["g%d" % j for j in range(8)]).to_csv(
                os.path.join(r, cohort_io.RNASEQ))
        write_s = time.perf_counter() - t0

        variants = [("nii_threads_1", "nii", dict(threads=1)), ("nii_threads_4", "nii", dict(threads=4)),
                    ("nii_threads_16", "nii", dict(threads=16)), ("npy", "npy", {})]
        cohort_io.load_cohort(roots["nii"], dev, target_size=target, threads=4)        # warm-up: code objects, pinned and device pools
        cohort_io.load_cohort(roots["npy"], dev, target_size=target)
        torch.cuda.synchronize()
        times, stores = {k: [] for k, _, _ in variants}, {}
        for _ in range(args.load_reps):
            for name, kind, kw in variants:                                            # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c = cohort_io.load_cohort(roots[kind], dev, target_size=target, **kw)
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
                stores[name] = c["image"]
        for name in ("nii_threads_4", "nii_threads_16"):
            assert torch.equal(stores[name], stores["nii_threads_1"]), name
        err = float((stores["npy"] - stores["nii_threads_1"]).abs().max())
        assert err <= 1e-5, err

        # the passes alone, volumes resident
        raws = [nifti.read_nifti(r[1]) for r in rows["nii"]]
        nb = raws[0][1].nbytes
        chunk = min(V, cohort_io._lib_limit("MMS_CT_RAW_CHUNK"))
        offs = [cohort_io._align16(nb) * j for j in range(chunk)]
        total = cohort_io._align16(nb) * chunk
        host = torch.empty(total, dtype=torch.uint8)
        for j in range(chunk):
            host.numpy()[offs[j]:offs[j] + nb] = raws[j][1].reshape(-1).view(np.uint8)
        stage = host.to(dev)
        descs = [cohort_io._raw_descriptor(raws[j][1], 1.0, 0.0, raws[j][0]["swap"], offs[j], j) for j in range(chunk)]
        out = torch.zeros(chunk, 1, *target, device=dev)
        scratch = cohort_io._raw_scratch(dev)
        dst = torch.empty_like(stage)

        def timed(fn):
            for _ in range(args.warmup):
                fn()
            ms = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); fn(); b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            return ms

        p1 = timed(lambda: cohort_io._launch_raw_batch(stage, total, descs, target, out, scratch, passes=1))
        p2 = timed(lambda: cohort_io._launch_raw_batch(stage, total, descs, target, out, scratch, passes=2))
        both = timed(lambda: cohort_io._launch_raw_batch(stage, total, descs, target, out, scratch))
        cp = timed(lambda: dst.copy_(stage))
        assert torch.equal(out[:, 0], stores["nii_threads_1"][:chunk, 0])
        data_bytes = nb * chunk
        m1, mc = statistics.median(p1), statistics.median(cp)
        res = dict(device=torch.cuda.get_device_name(0), volumes=V, dims=list(dims), target=list(target), stored_dtype="int16",
                   nii_gz_mb=round(gz_bytes / 2 ** 20, 1), raw_mb=round(V * nb / 2 ** 20, 1), npy_mb=round(2 * V * nb / 2 ** 20, 1),
                   write_cohort_s=round(write_s, 2), load_reps=args.load_reps, warmup=args.warmup, reps=args.reps,
                   load_cohort_s={k: stats(v) for k, v in times.items()},
                   npy_over_nii_threads_16=round(statistics.median(times["npy"]) / statistics.median(times["nii_threads_16"]), 3),
                   nii_vs_npy_max_abs_diff=err, volumes_per_call=chunk,
                   pass1_ms=stats(p1), pass2_ms=stats(p2), both_passes_ms=stats(both), d2d_copy_ms=stats(cp),
                   pass1_us_per_volume=round(1e3 * m1 / chunk, 2), pass2_us_per_volume=round(1e3 * statistics.median(p2) / chunk, 2),
                   pass1_read_gbps=round(data_bytes / m1 / 1e6, 1), copy_traffic_gbps=round(2 * total / mc / 1e6, 1),
                   pass1_over_copy_traffic=round((data_bytes / m1) / (2 * total / mc), 3),
                   pass1_time_over_copy_time=round(m1 / mc, 3))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
