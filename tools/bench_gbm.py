#!/usr/bin/env python
"""Gradient-boosted Cox trees (csrc/gbm.hip, boosting.py) at the size the baseline runs at: 608 patients x 5005 genes, a third censored,
K = 5 outer x J = 5 inner folds (30 boosters in lock-step), 300 rounds, depth 3, 32 bins -- and one point with a 3 x 2 grid (180
boosters) -- beside the numpy replica (tests/gbm_ref.py) on the same host, in one process:

  launches     --timed-rounds rounds of the 30 boosters with HIP events around every launch (fit(timings=); it synchronises after each,
               so the sums are not the end-to-end time), once per histogram form of mms_gbm_split, the forms ALTERNATING --form-reps
               times; per launch name the median, min and max over all timed rounds, and a round = the sum of the medians.  The two
               forms' tables are compared (they must be byte-equal) before anything is recorded.
  fit          boosting.fit of the 30 boosters for all rounds (default form), host clock around a device synchronise; --warmup runs
               first, --reps timed runs; median, min, max.
  nested_cv    boosting.nested_cv end to end (fold tables on the host, binning, upload, every launch, selection, the prediction launch,
               C-indices), once for the single grid point and once for the 3 x 2 grid (learning rate 0.05 / 0.1 / 0.2 x depth 2 / 3).
  numpy        gbm_ref.boost of ONE round of ONE of the boosters on the same binned matrix (host clock), and that time scaled to all
               boosters and rounds -- the scaled figure is an extrapolation and is named so.  The replica's round-0 tree is compared
               with the GPU's.
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


def spread(v):
    med = statistics.median(v)
    return {"median": round(med, 4), "min": round(min(v), 4), "max": round(max(v), 4), "spread": round((max(v) - min(v)) / med, 4) if med else 0.0,
            "samples": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patients", type=int, default=608)
    ap.add_argument("--genes", type=int, default=5005)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--timed-rounds", type=int, default=20)
    ap.add_argument("--form-reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-grid", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "gbm_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import gbm_cases as CASES
    import gbm_ref as REF
    from multimodal_survival_prediction_amd import _lib, boosting, coxnet, data

    dev = torch.device("cuda:0")
    N, p, K, J, M, D, B = args.patients, args.genes, args.folds, args.inner, args.rounds, args.depth, args.bins
    rng = np.random.default_rng(608)
    X = rng.normal(size=(N, p)).astype(np.float32)
    t = np.ceil(rng.exponential(900.0, N) * np.exp(-0.5 * X[:, 0] - 0.8 * (np.abs(X[:, 1]) - 0.8)))
    e = (rng.random(N) < 0.67).astype(np.float64)
    cohort = dict(rnaseq=torch.from_numpy(X).to(dev), label=torch.from_numpy(np.stack([t, e], 1)), has_survival=torch.ones(N, dtype=torch.bool), n=N)
    folds = data.kfold_indices(N, K, seed=42)
    rr, mults, plan = coxnet.nested_problems(cohort, folds, J, 0)
    m = mults.reshape(-1, len(rr))
    P = len(m)
    xe = cohort["rnaseq"][torch.as_tensor(rr.rows, device=dev)].contiguous()
    masks = m == 0
    kw = dict(learning_rate=0.1, max_depth=D, min_leaf=10, l2=1.0, bins=B, seed=0, eval_masks=masks)
    lim = _lib.defines("MMS_GBM_")

    # per-launch times, the two histogram forms alternating
    boosting.fit(xe, rr.time, rr.event, m, rounds=2, form=1, **kw); boosting.fit(xe, rr.time, rr.event, m, rounds=2, form=2, **kw)      # warm
    per = {1: {}, 2: {}}
    tabs = {}
    for rep in range(args.form_reps):
        for form in (1, 2):
            tm = []
            b = boosting.fit(xe, rr.time, rr.event, m, rounds=args.timed_rounds, form=form, timings=tm, **kw)
            tabs[form] = {k: v.cpu().numpy().tobytes() for k, v in b.tables.items()}
            for name, ms in tm:
                per[form].setdefault(name, []).append(ms)
    if tabs[1] != tabs[2]:
        raise SystemExit("the two histogram forms disagree: nothing recorded")
    launches = {("members" if f == 1 else "private"): {name: spread(v) for name, v in per[f].items()} for f in (1, 2)}
    round_ms = {name: round(sum(launches[name][k]["median"] for k in launches[name]), 4) for name in launches}
    split_ms = {name: round(sum(v["median"] for k, v in launches[name].items() if k.startswith("split_level_")), 4) for name in launches}

    # fit, all rounds, default form
    fit_ms, bst = [], None
    for i in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bst = boosting.fit(xe, rr.time, rr.event, m, rounds=M, **kw)
        torch.cuda.synchronize()
        if i >= args.warmup:
            fit_ms.append((time.perf_counter() - t0) * 1e3)

    def nested(grid):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = boosting.nested_cv(cohort, folds, inner=J, rounds=M, grid=grid, seed=0, bins=B)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    one = boosting.default_grid((0.1,), (D,))
    nested(one)                                                     # warm
    cv_ms, cv_res = zip(*[nested(one) for _ in range(args.reps)])
    grid_ms = grid_res = None
    if not args.skip_grid:
        grid_ms, grid_res = nested(boosting.default_grid((0.05, 0.1, 0.2), (2, D)))

    # the replica: one round of booster 0 on the same bins
    edges = bst.edges.cpu().numpy()
    order, gid = REF.positions(rr.time)
    xb = CASES.bins_of(xe.cpu().numpy()[order], edges)
    t0 = time.perf_counter()
    ref = REF.boost(xb, edges, rr.event[order].astype(np.int64), gid, order, m[0][order].astype(np.int64), B, 1, lr=0.1, depth=D, min_leaf=10, l2=1.0,
                    min_gain=0.0, subsample=0xFFFFFFFF, colsample=0xFFFFFFFF, pid=0, seed=0, nn=(2 << D) - 1)
    np_ms = (time.perf_counter() - t0) * 1e3
    feat0 = bst.tables["feat"][0, 0].cpu().numpy()
    nodes = bst.tables["feat"].cpu().numpy() >= 0

    res = {"device": torch.cuda.get_device_name(0), "patients": N, "eligible": len(rr), "genes": p, "outer_folds": K, "inner_folds": J, "boosters": P,
           "rounds": M, "max_depth": D, "bins": B, "min_leaf": 10, "l2": 1.0, "learning_rate": 0.1, "events": int(e.sum()),
           "gene_tile": lim["TILE"], "lds_cells": lim["LDS_CELLS"], "timed_rounds": args.timed_rounds, "form_reps": args.form_reps,
           "launch_ms": launches, "round_ms_sum_of_medians": round_ms, "split_ms_per_round": split_ms,
           "private_over_members_split": round(split_ms["private"] / split_ms["members"], 3), "default_form": "members",
           "forms_byte_equal": True, "warmup": args.warmup, "reps": args.reps, "fit_ms": spread(fit_ms),
           "fit_ms_per_round": round(statistics.median(fit_ms) / M, 4), "nested_cv_ms": spread(list(cv_ms)),
           "nested_cv_chosen": [[r["grid_index"], r["rounds"]] for r in cv_res[-1]], "nested_cv_c_index": [round(r["c_index"], 4) for r in cv_res[-1]],
           "splits_per_tree_mean": round(float(nodes.sum()) / (P * M), 2),
           "numpy_threads": os.environ.get("OMP_NUM_THREADS", "unset"), "numpy_ms_per_round_one_booster": round(np_ms, 1),
           "numpy_ms_all_boosters_all_rounds_EXTRAPOLATED": round(np_ms * P * M, 0),
           "numpy_round0_tree_equal": bool(np.array_equal(ref["trees"][0]["feat"], feat0))}
    if grid_ms is not None:
        res.update(grid_3x2={"boosters": P * 6, "nested_cv_ms_one_run": round(grid_ms, 1), "chosen": [[r["grid_index"], r["rounds"]] for r in grid_res],
                             "c_index": [round(r["c_index"], 4) for r in grid_res]})
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
