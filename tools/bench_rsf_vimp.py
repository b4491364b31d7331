#!/usr/bin/env python
"""Out-of-bag permutation importance of the survival forest (csrc/rsf.hip: mms_rsf_vimp; Forest.vimp) at the size the baseline runs at:
608 patients x 5005 genes, K = 5 folds x T = 500 trees (tools/bench_rsf.py's cohort and forest), R = 1 and R = 5 repeats, in one process:

  launch       the ONE mms_rsf_vimp launch over all (fold, gene, repeat) problems, HIP events; median of --reps.
  tables       the problem table and the donor tables, built on the device with torch (unique / stable sorts), host clock with a
               synchronise; Forest.vimp end to end (the K base predictions, tables, launch, download, the VIMP arithmetic) beside it.
  end to end   survival_forest.cross_validate(vimp=R) against vimp=0, host clock, median of --reps after --warmup.
  numpy        tests/rsf_vimp_ref.py's delta sum + pair count of --numpy-problems problems (one repeat), per problem and scaled to all;
               its counts are compared with the launch's before anything is recorded.
  naive        the form DESIGN.md section 7 used to describe: per permuted gene one Forest.predict over the fold's out-of-bag mask plus a
               host C-index, timed on --naive-genes genes of fold 0 and scaled to all problems x repeats.
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
    ap.add_argument("--repeats", default="1,5")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-problems", type=int, default=6)
    ap.add_argument("--naive-genes", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "rsf_vimp_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import rsf_vimp_ref as VREF
    from multimodal_survival_prediction_amd import coxnet, data, survival_forest as SF
    from multimodal_survival_prediction_amd.survival_stats import concordance_index

    dev = torch.device("cuda:0")
    N, p, K, T = args.patients, args.genes, args.folds, args.trees
    rng = np.random.default_rng(608)
    X = rng.normal(size=(N, p)).astype(np.float32)
    t = np.ceil(rng.exponential(900.0, N) * np.exp(-0.5 * X[:, 0] - 0.8 * (np.abs(X[:, 1]) - 0.8)))
    e = (rng.random(N) < 0.67).astype(np.float64)
    cohort = dict(rnaseq=torch.from_numpy(X).to(dev), label=torch.from_numpy(np.stack([t, e], 1)), has_survival=torch.ones(N, dtype=torch.bool), n=N)
    folds = data.kfold_indices(N, K, seed=42)
    kw = dict(nsplit=10, min_leaf=15, max_depth=10, seed=0)
    med = statistics.median

    def cv_ms(R):
        ms = []
        for i in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = SF.cross_validate(cohort, folds, n_trees=T, vimp=R, **kw)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return {"median": round(med(ms), 1), "min": round(min(ms), 1), "max": round(max(ms), 1)}, out

    rr = coxnet.risk_rows(cohort)
    pos = [rr.positions(tr, N) for tr, _ in folds]
    mults = SF.bootstrap_mults(pos, N, T, kw["seed"])
    masks = np.zeros((K, N), bool)
    for f, tr in enumerate(pos):
        masks[f, tr] = True
    sets = np.repeat(np.arange(K), T)
    xe = cohort["rnaseq"][torch.as_tensor(rr.rows, device=dev)].contiguous()
    forest = SF.fit(xe, rr.time, rr.event, mults, train_sets=(masks, sets), **kw)
    use = (mults == 0) & masks[sets]
    ev = rr.event.astype(np.int64)

    res = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": args.reps, "patients": N, "genes": p, "folds": K,
           "trees_per_fold": T, **forest.hyper, "split_nodes": int((forest.feat >= 0).sum()), "numpy_threads": os.environ.get("OMP_NUM_THREADS", "unset")}
    res["cross_validate_ms"] = {"vimp_0": cv_ms(0)[0]}
    last = None
    for R in [int(v) for v in args.repeats.split(",")]:
        runs = []
        for i in range(args.warmup + args.reps):
            tm = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = forest.vimp(xe, rr.time, ev, use, sets=sets, nperm=R, timings=tm)
            torch.cuda.synchronize()
            if i >= args.warmup:
                runs.append(dict(tm, total=(time.perf_counter() - t0) * 1e3))
        P = len(last["problems"]["set"])
        cv, out = cv_ms(R)
        res["cross_validate_ms"]["vimp_%d" % R] = cv
        res["repeats_%d" % R] = {"problems": P, "workgroups": (P + K) * R, "launch_ms": round(med(r["launch"] for r in runs), 3),
                                 "tables_ms": round(med(r["tables"] for r in runs), 2), "forest_vimp_ms": round(med(r["total"] for r in runs), 1),
                                 "launch_us_per_problem_repeat": round(med(r["launch"] for r in runs) * 1e3 / ((P + K) * R), 3),
                                 "top_gene_per_fold": [int(np.argmax(r["vimp"])) for r in out],
                                 "top_vimp_per_fold": [round(float(np.max(r["vimp"])), 4) for r in out]}
    prob = last["problems"]
    P = len(prob["set"])
    res["trees_per_problem"] = {"mean": round(float(np.diff(prob["off"]).mean()), 2), "max": int(np.diff(prob["off"]).max())}
    res["c_base"] = [round(float(c), 4) for c in last["c_base"]]

    # the numpy replica on a few problems of the last run (repeat 0), from the device's tables, M0 and counts
    feat, thr, mort = (getattr(forest, k).cpu().numpy() for k in ("feat", "thr", "mort"))
    M0 = np.stack([forest.predict(xe, use=(use & (sets == f)[:, None]).astype(np.uint8))["mortality"] for f in range(K)])
    cnt = np.stack([(use & (sets == f)[:, None]).sum(0) for f in range(K)])
    Xh = xe.cpu().numpy()
    pick = np.linspace(0, P - 1, min(args.numpy_problems, P)).astype(np.int64)
    t_np, differ = 0.0, 0
    for q in pick:
        f, g = int(prob["set"][q]), int(prob["gene"][q])
        trees = [int(v) for v in prob["tree"][prob["off"][q]:prob["off"][q + 1]]]
        t0 = time.perf_counter()
        don = {tr: VREF.donors(kw["seed"], int(forest.tree_id[tr]), 0, use[tr]) for tr in trees}
        D = VREF.delta(Xh, feat, thr, mort, use, don, trees, g, cnt[f])
        rows = cnt[f] > 0
        M = M0[f].copy()
        M[rows] = M0[f][rows] + D[rows] / cnt[f][rows].astype(np.float64)
        got = VREF.pair_counts(rr.time, ev, M, rows)
        t_np += time.perf_counter() - t0
        differ += int(got != (int(last["conc2"][q, 0]), int(last["comparable"][q, 0])))
    res.update(numpy_problems_timed=len(pick), numpy_ms_per_problem=round(t_np * 1e3 / len(pick), 1), numpy_problems_that_differ=differ)

    # the naive form: one prediction launch and a host C-index per permuted gene
    f0 = np.nonzero(prob["set"] == 0)[0]
    genes = prob["gene"][f0[np.linspace(0, len(f0) - 1, min(args.naive_genes, len(f0))).astype(np.int64)]]
    use0 = torch.from_numpy((use & (sets == 0)[:, None]).astype(np.uint8)).to(dev)
    tr0 = pos[0]
    prng = np.random.default_rng(1)
    xp = xe.clone()
    forest.predict(xp, use=use0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for g in genes:
        col = xe[:, int(g)].clone()
        xp[:, int(g)] = col[torch.from_numpy(prng.permutation(N)).to(dev)]
        m = forest.predict(xp, use=use0)["mortality"][tr0]
        ok = ~np.isnan(m)
        concordance_index(rr.time[tr0][ok], -m[ok], rr.event[tr0][ok])
        xp[:, int(g)] = col
    torch.cuda.synchronize()
    naive = (time.perf_counter() - t0) * 1e3 / len(genes)
    res.update(naive_genes_timed=int(len(genes)), naive_ms_per_problem_repeat=round(naive, 2))
    for R in [int(v) for v in args.repeats.split(",")]:
        r = res["repeats_%d" % R]
        r["numpy_ms_scaled"] = round(res["numpy_ms_per_problem"] * r["problems"] * R, 0)
        r["naive_ms_scaled"] = round(naive * r["problems"] * R, 0)
        r["naive_over_forest_vimp"] = round(r["naive_ms_scaled"] / r["forest_vimp_ms"], 1)
        r["numpy_over_launch"] = round(r["numpy_ms_scaled"] / r["launch_ms"], 0)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
