#!/usr/bin/env python
"""Random survival forest (csrc/rsf.hip, survival_forest.py) at the size the baseline runs at: 608 patients x 5005 genes, two thirds
events, K = 5 folds x T = 500 trees, mtry = ceil(sqrt(5005)) = 71, nsplit = 10, min_leaf = 15, max_depth = 10 -- beside the numpy replica
(tests/rsf_ref.py) on the same host, in one process:

  end to end   survival_forest.cross_validate (bootstrap draws on the host, upload, the feature-major copy, every launch, the validation and
               out-of-bag predictions, download, C-indices), host clock; --warmup runs first, --reps timed runs; median, min, max.
  launches     one more growth of the same K T trees with HIP events around every launch (fit(timings=); it synchronises after each, so
               the sum is not the end-to-end time): milliseconds per level, for the leaves and for one prediction launch over all rows,
               and each one's share of their sum.  "live_nodes" is the number of nodes of the level that tried to split.
  numpy        rsf_ref.grow + leaves of --numpy-trees of the same trees (float64, threads as the environment sets them, host clock),
               per tree and scaled to all.  The replica's candidate scoring is vectorised over a node's candidates.

The GPU's trees of the timed replica trees are compared with the replica's (split features) before anything is recorded; a tree that
differs is counted, not hidden (near-ties between candidates may legitimately go either way: tests/rsf_ref.node_margin).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patients", type=int, default=608)
    ap.add_argument("--genes", type=int, default=5005)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--trees", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-trees", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "rsf_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import rsf_ref as REF
    from multimodal_survival_prediction_amd import coxnet, data, survival_forest as SF

    dev = torch.device("cuda:0")
    N, p, K, T = args.patients, args.genes, args.folds, args.trees
    rng = np.random.default_rng(608)
    X = rng.normal(size=(N, p)).astype(np.float32)
    t = np.ceil(rng.exponential(900.0, N) * np.exp(-0.5 * X[:, 0] - 0.8 * (np.abs(X[:, 1]) - 0.8)))
    e = (rng.random(N) < 0.67).astype(np.float64)
    cohort = dict(rnaseq=torch.from_numpy(X).to(dev), label=torch.from_numpy(np.stack([t, e], 1)), has_survival=torch.ones(N, dtype=torch.bool), n=N)
    folds = data.kfold_indices(N, K, seed=42)
    kw = dict(nsplit=10, min_leaf=15, max_depth=10, seed=0)

    e2e, res_cv = [], None
    for i in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res_cv = SF.cross_validate(cohort, folds, n_trees=T, **kw)
        torch.cuda.synchronize()
        if i >= args.warmup:
            e2e.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(e2e)

    rr = coxnet.risk_rows(cohort)
    pos = [rr.positions(tr, N) for tr, _ in folds]
    t0 = time.perf_counter()
    mults = SF.bootstrap_mults(pos, N, T, kw["seed"])
    draw_ms = (time.perf_counter() - t0) * 1e3
    masks = np.zeros((K, N), bool)
    for f, tr in enumerate(pos):
        masks[f, tr] = True
    wset = np.repeat(np.arange(K), T)
    hz = SF.default_horizons(rr.time, rr.event)
    xe = cohort["rnaseq"][torch.as_tensor(rr.rows, device=dev)].contiguous()
    SF.fit(xe, rr.time, rr.event, mults, train_sets=(masks, wset), horizons=hz, **kw)            # warm
    timings = []
    forest = SF.fit(xe, rr.time, rr.event, mults, train_sets=(masks, wset), horizons=hz, timings=timings, **kw)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    forest.predict(xe)
    e0.record(); forest.predict(xe); e1.record(); e1.synchronize()
    timings.append(("predict_all_rows", e0.elapsed_time(e1)))
    total = sum(ms for _, ms in timings)
    feat, n_node = forest.feat.cpu().numpy(), forest.n_node.cpu().numpy()
    live = {}
    for name, _ in timings:
        if name.startswith("split_level_"):
            L = int(name.rsplit("_", 1)[1])
            lo = (1 << L) - 1
            live[name] = int((n_node[:, lo:2 * lo + 1] >= 2 * kw["min_leaf"]).sum())

    nt = min(args.numpy_trees, K * T)
    pick = np.linspace(0, K * T - 1, nt).astype(np.int64)
    Xp = xe.cpu().numpy()
    gid = REF.positions(rr.time)[1]
    ev = rr.event.astype(np.int64)
    t_np, differ = 0.0, 0
    for q in pick:
        t0 = time.perf_counter()
        tree = REF.grow(Xp, ev, gid, mults[q].astype(np.int64), int(q), kw["seed"], forest.hyper["mtry"], kw["nsplit"], kw["min_leaf"], kw["max_depth"])
        REF.leaves(rr.time, ev, mults[q].astype(np.int64), tree, masks[wset[q]], hz)
        t_np += time.perf_counter() - t0
        differ += int(not np.array_equal(tree["feat"], feat[q]))

    res = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": args.reps, "patients": N, "genes": p, "folds": K,
           "trees_per_fold": T, "trees": K * T, "events": int(e.sum()), "distinct_times": int(len(np.unique(t))), **forest.hyper,
           "candidates_per_node": forest.hyper["mtry"] * kw["nsplit"], "horizons": [float(h) for h in hz],
           "numpy_threads": os.environ.get("OMP_NUM_THREADS", "unset"),
           "cross_validate_ms": {"median": round(med, 1), "min": round(min(e2e), 1), "max": round(max(e2e), 1),
                                 "spread": round((max(e2e) - min(e2e)) / med, 4)},
           "bootstrap_draws_host_ms": round(draw_ms, 1),
           "launch_ms": {name: round(ms, 3) for name, ms in timings},
           "launch_share": {name: round(ms / total, 4) for name, ms in timings}, "launch_sum_ms": round(total, 2),
           "live_nodes": live, "split_nodes": int((feat >= 0).sum()), "leaves": int(((feat < 0) & (n_node > 0)).sum()),
           "val_c_index": [round(r["c_index"], 4) for r in res_cv], "oob_c_index": [round(r["oob_c_index"], 4) for r in res_cv],
           "numpy_trees_timed": nt, "numpy_ms_per_tree": round(t_np * 1e3 / nt, 1), "numpy_ms_scaled_to_all": round(t_np * 1e3 / nt * K * T, 0),
           "numpy_trees_that_differ": differ}
    res["numpy_growth_over_launch_sum"] = round(res["numpy_ms_scaled_to_all"] / total, 1)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
