#!/usr/bin/env python
"""mms_gene_screen (univariate Cox score screen, csrc/gene_screen.hip) on the 608-patient cohort at G = 5005, beside the numpy closed form
on the same host, in one process:

  5-fold screen    P = 5: each fold's eligible training patients (RNA-seq and a survival label)
  stability run    P = 505: the same plus R = 100 bootstrap resamples per fold (gene_select.fold_problems)

  kernel   the launch alone on device-resident inputs (ops.gene_screen(plan_only=True) uploads and checks once): HIP events around one
           call, --warmup calls first, --reps timed calls; median, min, max.  "gb_per_s_requested" counts the x elements the launch
           asks for (sum over problems of rows x G x 4 bytes) -- most of them are served by L2, so it is no HBM rate and no share of peak;
           "unique_mb" is the matrix itself.
  numpy    the same closed form in float64 (fancy-index gather of the problem's rows, cumulative sum, three weighted column sums), threads
           as the environment sets them, host clock; the first --numpy-problems problems of each case are timed and scaled to P.
  end to end  gene_select.select_genes (coefficients, upload, launch, download, ranking), host clock, 3 runs

The kernel's U and V are compared with numpy's on the timed problems (1e-10 of the sums' magnitudes) before anything is recorded.
Writes --out as JSON and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def numpy_closed_form(x64, rows, coef):
    X = x64[rows]
    S1 = np.cumsum(X, 0)
    a, b, q = coef[:, 0:1], coef[:, 1:2], coef[:, 2:3]
    return (a * X).sum(0), (b * X * X).sum(0), (q * S1 * S1).sum(0), (np.abs(a) * np.abs(X)).sum(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resamples", type=int, default=100)
    ap.add_argument("--k", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--numpy-problems", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "gene_screen_bench.json"))
    args = ap.parse_args()

    global np
    import numpy as np
    import torch
    from multimodal_survival_prediction_amd import data, gene_select as GS, ops

    dev = torch.device("cuda:0")
    cpu = data.make_cohort(n=608, dims=(16, 16, 8), seed=608, complete=False)          # (the volumes are not read)
    folds = [tr for tr, _ in data.kfold_indices(608, 5, seed=42)]
    cohort = data.cohort_to(cpu, dev)
    x, x64 = cohort["rnaseq"], cpu["rnaseq"].numpy().astype(np.float64)
    lab = cpu["label"].numpy()
    res = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": args.reps, "N": 608, "G": int(x.shape[1]),
           "numpy_threads": os.environ.get("OMP_NUM_THREADS", "unset"), "cases": []}
    for name, R in (("5-fold screen", 0), ("stability run", args.resamples)):
        problems, rows_f = GS.fold_problems(cpu, folds, stability=R, seed=0)
        off, rows, coefs = [0], [], []
        for lst in problems:
            order, a, b, q = GS.score_coefficients(lab[:, 0], lab[:, 1], lst)
            rows.append(lst[order]); coefs.append(np.stack([a, b, q], 1)); off.append(off[-1] + len(lst))
        p, keep, U, V = ops.gene_screen(x, off, np.concatenate(rows), np.concatenate(coefs), plan_only=True)
        for _ in range(args.warmup):
            ops.call("mms_gene_screen", p)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.call("mms_gene_screen", p)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        G, P = int(x.shape[1]), len(problems)
        req = off[-1] * G * 4
        row = {"case": name, "P": P, "resamples_per_fold": R, "rows_per_fold": [len(r) for r in rows_f], "rows_total": off[-1],
               "kernel_ms": {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4)},
               "kernel_us_per_problem": round(med * 1e3 / P, 3), "requested_mb": round(req / 1e6, 1), "unique_mb": round(608 * G * 4 / 1e6, 1),
               "gb_per_s_requested": round(req / (med * 1e-3) / 1e9, 1)}
        Ud, Vd = U.cpu().numpy(), V.cpu().numpy()
        nt = min(args.numpy_problems, P)
        t_np = 0.0
        for i in range(nt):
            t0 = time.perf_counter()
            u, vb, vq, bu = numpy_closed_form(x64, rows[i], coefs[i])
            t_np += time.perf_counter() - t0
            assert (np.abs(Ud[i] - u) <= 1e-10 * bu + 1e-300).all() and (np.abs(Vd[i] - (vb - vq)) <= 1e-10 * (vb + vq) + 1e-300).all(), \
                "kernel and numpy closed form differ on problem %d" % i
        row["numpy_ms_per_problem"] = round(t_np * 1e3 / nt, 2)
        row["numpy_problems_timed"] = nt
        row["numpy_ms_scaled_to_P"] = round(t_np * 1e3 / nt * P, 1)
        row["numpy_over_kernel"] = round(row["numpy_ms_scaled_to_P"] / med, 1)
        row["agrees_with_numpy"] = True
        e2e = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            GS.select_genes(cohort, folds, args.k, stability=R, seed=0)
            e2e.append((time.perf_counter() - t0) * 1e3)
        row["select_genes_ms"] = [round(v, 1) for v in e2e]
        res["cases"].append(row)
        print(json.dumps(row), flush=True)
        del keep
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
