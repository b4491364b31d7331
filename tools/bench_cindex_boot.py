#!/usr/bin/env python
"""mms_cindex_boot (bootstrap Harrell-C pair counts on the int8 matrix cores) at (n, R, M) = (348, 2000, 1), (1639, 2000, 2), (8192, 2000, 6),
beside the two routes a user had before it, in one process on the same box:

  kernel   ops.cindex_boot on device-resident ranks and weights (time-sorted, as cindex_bootstrap passes them): HIP events around one call,
           --warmup calls first, --reps timed calls; median, min, max.  The int8 MAC rate counts the (M + 1) R n^2 multiply-adds of the dense
           products W.S_m and W.P; the kernel skips the tiles in which no pair is comparable, so it is a rate of USEFUL work, not of issued
           MFMAs, and no share of peak.
  route a  a loop of losses.calculate_cindex over gathered resamples (one launch and one host sync per replicate and model), host clock ending
           in the sync, at R = --loop-reps replicates, reported per replicate and scaled to R
  route b  numpy float64 BLAS ((W @ S) * W).sum(1) per model and for P, threads as the environment sets them (16 on the measuring box), S and P
           built once and not timed; one timed run per shape (seconds each)
  end to end  bootstrap.cindex_bootstrap (draws, ranks, upload, kernel, statistics), host clock, 3 runs

The counts of the kernel and of route b are compared for equality before anything is recorded.  Writes --out as JSON and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="348x2000x1,1639x2000x2,8192x2000x6")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--loop-reps", type=int, default=200)
    ap.add_argument("--skip-blas-above", type=int, default=1 << 30, help="skip route b when n exceeds this")
    ap.add_argument("--out", default=os.path.join("profiles", "cindex_boot_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import cindex_boot_ref as REF
    from multimodal_survival_prediction_amd import bootstrap as B
    from multimodal_survival_prediction_amd import losses, ops

    dev = torch.device("cuda:0")
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
    res = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": args.reps, "loop_reps": args.loop_reps,
           "blas_threads": os.environ.get("OMP_NUM_THREADS", "unset"), "pair_rule": "lifelines", "shapes": []}
    for shape in args.shapes.split(","):
        n, R, M = (int(v) for v in shape.split("x"))
        c = REF.make_cohort(n, M, seed=n, n_times=max(2, n // 2), n_risks=max(2, n))
        w = B.bootstrap_weights(n, R, seed=n)
        order = np.argsort(c["time"], kind="stable")
        hr, tr, ev, wd = (up(B.dense_ranks(c["risk"])[:, order], torch.int32), up(B.dense_ranks(c["time"])[order], torch.int32),
                          up(c["event"][order], torch.int32), up(w[:, order], torch.int8))
        row = {"n": n, "R": R, "M": M, "max_multiplicity": int(w.max())}

        # kernel: HIP events around one call (its memset of `out`, padding copy of w when n % 64 != 0, and the launches)
        for _ in range(args.warmup):
            out = ops.cindex_boot(hr, tr, ev, wd, pair_rule=1)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = ops.cindex_boot(hr, tr, ev, wd, pair_rule=1)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        macs = (M + 1) * R * n * n
        row["kernel_ms"] = {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4)}
        row["kernel_us_per_replicate"] = round(med * 1e3 / R, 4)
        row["int8_dense_macs"] = macs
        row["int8_tera_macs_per_s_useful"] = round(macs / (med * 1e-3) / 1e12, 3)
        got = out.cpu().numpy()

        # route b: float64 BLAS
        if n <= args.skip_blas_above:
            Wf, ref, blas_s = w.astype(np.float64), [], 0.0
            for m in range(M):                          # one matrix at a time: n = 8192 would otherwise hold 7 x 0.5 GB twice
                S, P = REF.pair_matrices(c["risk"][m:m + 1], c["time"], c["event"], None, 1)
                for a in ([S[0]] if m < M - 1 else [S[0], P]):
                    a = a.astype(np.float64)
                    t0 = time.perf_counter()
                    ref.append(((Wf @ a) * Wf).sum(1))
                    blas_s += time.perf_counter() - t0
                del S, P, a
            ref = np.stack(ref)
            row["numpy_blas_ms"] = round(blas_s * 1e3, 2)
            assert ref.max() < 2.0 ** 53 and np.array_equal(got, ref.astype(np.int64)), "kernel and float64 BLAS counts differ"
            row["counts_equal_numpy"] = True
            row["numpy_blas_over_kernel"] = round(row["numpy_blas_ms"] / med, 1)
            del Wf, ref

        # route a: calculate_cindex over gathered resamples
        h = up(c["risk"], torch.float32)
        tt, ee = up(c["time"], torch.float32), up(c["event"], torch.float32)
        idx = torch.from_numpy(B.bootstrap_indices(n, args.loop_reps, seed=n)).to(dev)
        for r in range(3):
            losses.calculate_cindex(h[0][idx[r]], ee[idx[r]], tt[idx[r]])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for r in range(args.loop_reps):
            j = idx[r]
            for m in range(M):
                losses.calculate_cindex(h[m][j], ee[j], tt[j])
        torch.cuda.synchronize()
        loop_ms = (time.perf_counter() - t0) * 1e3
        row["loop_ms_per_replicate"] = round(loop_ms / args.loop_reps, 4)
        row["loop_ms_scaled_to_R"] = round(loop_ms / args.loop_reps * R, 2)
        row["loop_over_kernel"] = round(row["loop_ms_scaled_to_R"] / med, 1)

        # end to end
        e2e = []
        for _ in range(3):
            t0 = time.perf_counter()
            B.cindex_bootstrap(c["risk"], c["time"], c["event"], R=R, seed=n)
            e2e.append((time.perf_counter() - t0) * 1e3)
        row["cindex_bootstrap_ms"] = [round(v, 2) for v in e2e]
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)

    gate = [r for r in res["shapes"] if (r["n"], r["R"], r["M"]) == (1639, 2000, 2)]
    if gate:
        res["condition_kernel_faster_than_loop_at_1639x2000x2"] = bool(gate[0]["kernel_ms"]["median"] < gate[0]["loop_ms_scaled_to_R"])
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
