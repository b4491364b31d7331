#!/usr/bin/env python
"""Elastic-net Cox baseline (csrc/coxnet.hip, coxnet.py) on the 608-patient cohort at G = 5005: nested cross-validation with K = 5 outer folds,
J = 5 inner folds and L = 30 penalties -- K (J + 1) L = 900 problems in lock-step -- beside the float64 numpy replica of the same solver
(tests/coxnet_ref.py) on ONE of those problems on the same host, in one process:

  end to end     coxnet.nested_cv (problems, scales, the lambda_max screen, upload, all fits, the evaluations, the criterion), host clock,
                 one warm-up run and --runs timed runs
  per iteration  one lock-step round of all 900 problems (four launches: eta, scan, x'r, update) on device-resident state: HIP events
                 around --batch rounds, --reps batches after the problems' first round; median, min, max per round.  Frozen problems still
                 pass through the products, so a round costs the same at any point of the fit.
  fit            iterations and status of the 900 problems from the device's own counters
  numpy          the replica's fit of one problem (outer fold 0, all its training patients, the middle of its path): total and per iteration

The fit of that problem is compared with the replica's (strong-convexity bound on beta) before anything is recorded.
Writes --out as JSON and prints it."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--n-lambda", type=int, default=30)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "coxnet_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import coxnet_ref as REF
    from multimodal_survival_prediction_amd import _lib, coxnet as CX, data, ops

    dev = torch.device("cuda:0")
    cpu = data.make_cohort(n=608, dims=(16, 16, 8), seed=608, complete=False)          # (the volumes are not read)
    folds = data.kfold_indices(608, args.folds, seed=42)
    cohort = data.cohort_to(cpu, dev)
    x = cohort["rnaseq"]
    G, L, J1 = int(x.shape[1]), args.n_lambda, args.inner + 1
    res = {"device": torch.cuda.get_device_name(0), "N": 608, "G": G, "outer_folds": args.folds, "inner_folds": args.inner, "n_lambda": L,
           "alpha": args.alpha, "tol": CX.TOL, "max_iter": CX.MAX_ITER, "numpy_threads": os.environ.get("OMP_NUM_THREADS", "unset")}

    e2e = []
    for i in range(args.runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = CX.nested_cv(cohort, folds, alpha=args.alpha, n_lambda=L, inner=args.inner, criterion="cindex", seed=0)
        if i:
            e2e.append((time.perf_counter() - t0) * 1e3)
    res["nested_cv_ms"] = [round(v, 1) for v in e2e]
    res["outer_c_index"] = [round(float(r["c_index"]), 4) for r in out]
    res["chosen_lambda_index"] = [int(r["lambda_index"]) for r in out]

    # the same problems, state kept on the device
    rr, mults, _ = CX.nested_problems(cpu, folds, args.inner, 0)
    m = mults.reshape(-1, len(rr))
    scale, _ = CX.problem_scales(x, rr, m)
    full = np.arange(args.folds) * J1 + args.inner
    _, lmax = CX.lambda_path(x, cohort, rr, m[full], args.alpha, L, 0.05, scale[full])
    lams = np.repeat(CX.log_path(lmax, L, 0.05), J1, axis=0).reshape(-1)
    mm, ss = np.repeat(m, L, axis=0), np.repeat(scale, L, axis=0)
    P = len(lams)
    res.update(P=P, rows=len(rr), rows_per_problem=[int(m.sum(1).min()), int(m.sum(1).max())])
    p, t = ops.coxnet_plan(x, rr.rows, rr.event, rr.glast, mm, lams, np.full(P, args.alpha), scale=ss, tol=CX.TOL, max_iter=CX.MAX_ITER)
    lib = _lib.load_library()
    it = lambda k: _lib.check(lib.mms_coxnet_iterate(ctypes.byref(p), k, ops.stream()), "mms_coxnet_iterate")
    it(1 + args.batch)                                             # the problems' first round and a warm-up batch
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        it(args.batch)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / args.batch)
    med = statistics.median(ms)
    res["round_ms"] = {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4),
                       "rounds_per_batch": args.batch, "batches": args.reps}
    res["round_us_per_problem"] = round(med * 1e3 / P, 3)
    res["round_gflop_f64"] = round(2 * 2.0 * P * len(rr) * G / 1e9, 2)          # the two products
    res["round_tflops_f64"] = round(res["round_gflop_f64"] / med, 2)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = ops.coxnet_fit(x, rr.rows, rr.event, rr.glast, mm, lams, np.full(P, args.alpha), scale=ss, tol=CX.TOL, max_iter=CX.MAX_ITER)
    res["fit_all_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["fit_ms_per_path"] = round(res["fit_all_ms"] / (P // L), 2)
    res["iterations"] = {"max": int(fit["iters"].max()), "mean": round(float(fit["iters"].mean()), 1)}
    res["status"] = {"converged": int((fit["status"] == 1).sum()), "max_iter": int((fit["status"] == 2).sum())}

    q = (0 * J1 + args.inner) * L + L // 2                          # outer fold 0, all its training patients, the middle of the path
    X = cpu["rnaseq"].numpy().astype(np.float64)[rr.rows] / ss[q][None, :]
    t0 = time.perf_counter()
    ref = REF.solve(X, rr.time, rr.event, mm[q], float(lams[q]), args.alpha, tol=CX.TOL, max_iter=CX.MAX_ITER)
    dt = (time.perf_counter() - t0) * 1e3
    at = REF.evaluate(X, rr.time, rr.event, mm[q], float(lams[q]), args.alpha, fit["beta"][q])
    bound = (at["kkt"] + ref["kkt"]) / (float(lams[q]) * (1.0 - args.alpha))
    diff = float(np.abs(fit["beta"][q] - ref["beta"]).max())
    assert ref["status"] == 1 and fit["status"][q] == 1 and diff <= bound, "the fit and the numpy replica differ: %g > %g" % (diff, bound)
    res["numpy_one_problem"] = {"problem": int(q), "lambda": float(lams[q]), "ms": round(dt, 1), "iterations": int(ref["iters"]),
                                "ms_per_iteration": round(dt / max(ref["iters"], 1), 3), "gpu_iterations": int(fit["iters"][q]),
                                "max_abs_beta_difference": diff, "strong_convexity_bound": bound}
    res["numpy_ms_scaled_to_P"] = round(res["numpy_one_problem"]["ms_per_iteration"] * float(fit["iters"].sum()), 0)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
