#!/usr/bin/env python
"""TreeSHAP of the two tree baselines (csrc/tree_shap.hip: mms_tree_shap; Booster.shap, Forest.shap) at the size the baselines run at:
608 patients x 5005 genes, K = 5 folds, each fold's model explained on its own ~120 validation patients, in one process:

  booster      5 boosters (one per fold, trained on the fold's training patients) x --rounds (300) rounds of depth --depth (3); a pass
               is the 5 Booster.shap calls nested_cv(shap=True) makes.
  forest       K x --trees (500) trees of depth 10 (tools/bench_rsf.py's forest); a pass is the 5 Forest.shap(trees=) calls
               cross_validate(shap=True) makes, each over the fold's own trees.
  launch       the mms_tree_shap launches of a pass, HIP events, summed over the 5 folds; median, min and max of --reps passes.
  end to end   the pass on the host clock with a synchronise: gathering the tables, the slots, the host checks, the launch, the download
               and the reshaping.
  numpy        tests/tree_shap_ref.py's replica (vectorised over the rows) on the first --numpy-trees trees of fold 0's model and all of
               that fold's validation rows, per tree and scaled to every tree of the 5 folds; its values are compared with the device's
               within the tests' bound before anything is recorded.
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
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--trees", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--numpy-trees", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "tree_shap_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import tree_shap_ref as REF
    from multimodal_survival_prediction_amd import boosting, coxnet, data, survival_forest as SF

    dev = torch.device("cuda:0")
    N, p, K = args.patients, args.genes, args.folds
    rng = np.random.default_rng(608)
    X = rng.normal(size=(N, p)).astype(np.float32)
    t = np.ceil(rng.exponential(900.0, N) * np.exp(-0.5 * X[:, 0] - 0.8 * (np.abs(X[:, 1]) - 0.8)))
    e = (rng.random(N) < 0.67).astype(np.float64)
    cohort = dict(rnaseq=torch.from_numpy(X).to(dev), label=torch.from_numpy(np.stack([t, e], 1)), has_survival=torch.ones(N, dtype=torch.bool), n=N)
    folds = data.kfold_indices(N, K, seed=42)
    rr = coxnet.risk_rows(cohort)
    pos = [(rr.positions(tr, N), rr.positions(va, N)) for tr, va in folds]
    xe = cohort["rnaseq"][torch.as_tensor(rr.rows, device=dev)].contiguous()
    xv = [xe[torch.as_tensor(va, device=dev)].contiguous() for _, va in pos]
    stat = lambda v: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}

    def passes(call):
        """call(fold, timings) -> ShapValues; -> (launch ms and end-to-end ms of every pass after the warm-up, the last pass's values)"""
        launch, total, last = [], [], None
        for i in range(args.warmup + args.reps):
            tm = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = [call(f, tm) for f in range(K)]
            torch.cuda.synchronize()
            if i >= args.warmup:
                launch.append(sum(ms for _, ms in tm)); total.append((time.perf_counter() - t0) * 1e3)
        return launch, total, last

    def replica(tab, xrows, sv, n_trees):
        """the replica on the model's first n_trees trees and all rows -> (ms per tree, max |difference| / bound against the device)"""
        tab = [a[:n_trees].cpu().numpy() for a in tab]
        t0 = time.perf_counter()
        rphi, rbase = REF.shap(xrows.cpu().numpy(), *tab, [0, n_trees])
        ms = (time.perf_counter() - t0) * 1e3 / n_trees
        tol = REF.tolerance(tab[0], tab[2], [0, n_trees])[0]
        return ms, float(max(np.abs(sv.dense(0, p) - rphi[0]).max(), np.abs(sv.base[0] - rbase[0]).max()) / tol)

    res = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": args.reps, "patients": N, "genes": p, "folds": K,
           "validation_rows": [int(len(va)) for _, va in pos], "numpy_threads": os.environ.get("OMP_NUM_THREADS", "unset")}

    # ---- the boosters ----
    mults = np.zeros((K, N), np.int64)
    for f, (tr, _) in enumerate(pos):
        mults[f, tr] = 1
    M, nt = args.rounds, args.numpy_trees
    bst = boosting.fit(xe, rr.time, rr.event, mults, rounds=M, max_depth=args.depth, seed=0)
    launch, total, last = passes(lambda f, tm: bst.shap(xv[f], problems=[f], rounds=M, timings=tm))
    feat = bst.tables["feat"].cpu().numpy()
    tab0 = [bst.tables[k][0] for k in ("feat", "thr", "value", "n_node")]
    np_ms, np_err = replica(tab0, xv[0], bst.shap(xv[0], problems=[0], rounds=nt), nt)
    F = bst.predict(xv[0])[0]
    res["booster"] = {"rounds": M, "max_depth": args.depth, "nn": int(feat.shape[2]), "trees": K * M, "split_nodes": int((feat >= 0).sum()),
                      "genes_per_fold": [int(len(s.genes[0])) for s in last], "launch_ms": stat(launch), "end_to_end_ms": stat(total),
                      "local_accuracy_max_abs": float(np.abs(last[0].base[0] + last[0].phi[0].sum(1) - F).max()),
                      "numpy_trees_timed": nt, "numpy_rows": int(len(pos[0][1])), "numpy_ms_per_tree": round(np_ms, 2),
                      "numpy_max_diff_over_bound": np_err, "numpy_ms_scaled": round(np_ms * K * M, 0)}
    res["booster"]["numpy_over_launch"] = round(res["booster"]["numpy_ms_scaled"] / res["booster"]["launch_ms"]["median"], 0)

    # ---- the forest ----
    T = args.trees
    kw = dict(nsplit=10, min_leaf=15, max_depth=10, seed=0)
    bm = SF.bootstrap_mults([tr for tr, _ in pos], N, T, kw["seed"])
    masks = np.zeros((K, N), bool)
    for f, (tr, _) in enumerate(pos):
        masks[f, tr] = True
    sets = np.repeat(np.arange(K), T)
    forest = SF.fit(xe, rr.time, rr.event, bm, train_sets=(masks, sets), **kw)
    fold_trees = [np.arange(f * T, (f + 1) * T) for f in range(K)]
    launch, total, last = passes(lambda f, tm: forest.shap(xv[f], trees=fold_trees[f], timings=tm))
    sv = forest.shap(xv[0], trees=np.arange(nt))
    sv.phi[0], sv.base[0] = sv.phi[0] * nt, sv.base[0] * nt         # back to the launch's sums: the replica does not divide
    np_ms, np_err = replica([forest.feat, forest.thr, forest.mort, forest.n_node], xv[0], sv, nt)
    only0 = np.zeros((K * T, len(pos[0][1])), np.uint8)
    only0[:T] = 1
    m = forest.predict(xv[0], use=only0)["mortality"]
    feat = forest.feat.cpu().numpy()
    res["forest"] = {"trees_per_fold": T, **forest.hyper, "nn": int(feat.shape[1]), "trees": K * T, "split_nodes": int((feat >= 0).sum()),
                     "genes_per_fold": [int(len(s.genes[0])) for s in last], "launch_ms": stat(launch), "end_to_end_ms": stat(total),
                     "local_accuracy_max_abs": float(np.abs(last[0].base[0] + last[0].phi[0].sum(1) - m).max()),
                     "numpy_trees_timed": nt, "numpy_rows": int(len(pos[0][1])), "numpy_ms_per_tree": round(np_ms, 2),
                     "numpy_max_diff_over_bound": np_err, "numpy_ms_scaled": round(np_ms * K * T, 0)}
    res["forest"]["numpy_over_launch"] = round(res["forest"]["numpy_ms_scaled"] / res["forest"]["launch_ms"]["median"], 0)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
