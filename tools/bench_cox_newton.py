#!/usr/bin/env python
"""mms_cox_newton (multivariable Cox fits by Newton-Raphson, csrc/cox_newton.hip) at the sizes multivariable.analyse is used at:
n in {348, 608} patients (two thirds events, times in whole days), p in {4, 16} covariates, the S = 6 nested models of a base model of
p - 2 covariates and two added ones, R = 10 000 bootstrap rows plus the all-ones row -- beside the test reference's numpy form on the
same host, in one process.  Per shape:

  kernel      the launch alone on device-resident inputs (ops.cox_newton(plan_only=True) uploads and checks once): HIP events around
              one call, --warmup calls first, --reps timed calls; median, min, max, spread.  "fits" = (R + 1) S; "evaluations" counts
              one (l, g, I) evaluation per fit for the start and one per accepted or rejected step (the all-ones row's iterations + 1
              stand for every row's: an estimate, marked as such); "us_per_fit" is the kernel time over the fits.
  numpy       tests/cox_newton_ref.py fit with evaluate_cumsum (float64, threads as the environment sets them, host clock) on the
              first --numpy-replicates weight rows x S models, in ms per fit, and scaled to all fits.
  end to end  multivariable.analyse (design, weight draw, upload, launch, download, statistics), host clock, 3 runs.

The kernel's coefficients of the timed rows are compared with numpy's (2e-9, converged fits) before anything is recorded.
Writes --out as JSON and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def one_shape(n, p, R, args):
    import numpy as np
    import torch
    import cox_newton_ref as REF
    from multimodal_survival_prediction_amd import multivariable as MV, ops
    from multimodal_survival_prediction_amd.bootstrap import bootstrap_weights

    rng = np.random.default_rng([n, p])
    raw = rng.normal(size=(n, p))
    raw[:, 0] = rng.integers(0, 2, n)
    coef = np.zeros(p)
    coef[[0, p - 2, p - 1]] = 0.5, 0.6, 0.3
    t = np.ceil(rng.exponential(900.0, n) * np.exp(-(raw @ coef)))
    e = (rng.random(n) < 0.67).astype(np.int64)
    names = ["x%d" % a for a in range(p)]
    columns = dict(zip(names, raw.T))
    base, add = names[:p - 2], names[p - 2:]
    models = MV.model_subsets(base, add)
    d = MV.design(columns)
    masks = MV.subset_masks([[names.index(k) for k in m[1]] for m in models], p)
    w = np.concatenate([np.ones((1, n), np.int8), bootstrap_weights(n, R, 0)])
    order, glast = MV.launch_order(t)
    P, keep, out = ops.cox_newton(np.ascontiguousarray(d.X[order]), t[order], e[order], glast, np.ascontiguousarray(w[:, order]), masks,
                                  plan_only=True)
    for _ in range(args.warmup):
        ops.call("mms_cox_newton", P)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.call("mms_cox_newton", P)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    fits = (R + 1) * len(masks)
    res = {"n": n, "p": p, "S": len(masks), "R": R, "events": int(e.sum()), "distinct_times": int(len(np.unique(t))), "fits": fits,
           "kernel_ms": {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4)},
           "us_per_fit": round(med * 1e3 / fits, 4), "iterations_mean": round(float(got["iters"].mean()), 3),
           "evaluations_estimated": int(got["iters"].sum() + fits),
           "status_counts": {int(k): int(v) for k, v in zip(*np.unique(got["status"], return_counts=True))}}
    nt = min(args.numpy_replicates, R + 1)
    t_np = 0.0
    for r in range(nt):
        for s, m in enumerate(masks):
            t0 = time.perf_counter()
            ref = REF.fit(d.X, t, e, w[r], REF.mask_columns(m, p), evaluate=REF.evaluate_cumsum)
            t_np += time.perf_counter() - t0
            if ref["status"] == 1 and got["status"][r, s] == 1:
                assert np.abs(got["beta"][r, s] - ref["beta"]).max() <= 2e-9, "kernel and numpy differ on replicate %d, model %d" % (r, s)
    res["numpy_ms_per_fit"] = round(t_np * 1e3 / (nt * len(masks)), 4)
    res["numpy_fits_timed"] = nt * len(masks)
    res["numpy_ms_scaled_to_all"] = round(t_np * 1e3 / (nt * len(masks)) * fits, 1)
    res["numpy_over_kernel"] = round(res["numpy_ms_scaled_to_all"] / med, 1)
    res["agrees_with_numpy"] = True
    del keep
    e2e = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        MV.analyse(columns, t, e, base, add, R=R, seed=0)
        e2e.append((time.perf_counter() - t0) * 1e3)
    res["analyse_ms"] = [round(v, 1) for v in e2e]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[348, 608])
    ap.add_argument("--p", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--replicates", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--numpy-replicates", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "cox_newton_bench.json"))
    args = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": args.reps,
           "numpy_threads": os.environ.get("OMP_NUM_THREADS", "unset"),
           "shapes": [one_shape(n, p, args.replicates, args) for n in args.n for p in args.p]}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
