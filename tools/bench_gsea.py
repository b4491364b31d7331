#!/usr/bin/env python
"""Gene-set enrichment (mms_gsea_scores / mms_gsea_es, csrc/gsea.hip) at the cohort's size -- n = 427 analysed patients, G = 5005 genes -- for
R = 1000 and 10 000 relabellings and collections of S = 50 and S = 5000 sets (sizes drawn uniformly from 15 .. 500), in one process:

  launches  each entry point alone on device-resident inputs (ops.gsea_scores / ops.gsea_es with plan_only=True upload and check once): HIP
            events around one call, --warmup calls first, --reps timed calls; median, min, max, spread = (max - min) / median.  The scores
            entry point is two launches (scale, product); "product_gflops" counts 2 R1 n G over its time (the scale pass is inside it).
            "es_sort_ms" is the ES entry point with ONE set of 15 genes: load, sort and one walk -- what the ranking costs before any set is
            walked; the set walk's share of the full launch is 1 - es_sort_ms / es_ms.
  enrich    enrichment.enrich end to end (residuals, permutations, upload, both entry points, download, the numpy summaries), host clock
            around a call that ends with the results on the host, 3 runs.  Not run for R = 10 000 x S = 5000 (its [R1, S] summaries need
            several GB on the host; the launches are timed).
  numpy     the replica of tests/gsea_ref.py on the same host, threads as the environment sets them: --numpy-replicates replicates and at
            most --numpy-sets sets are timed, and the time is EXTRAPOLATED linearly to R1 replicates and S sets ("numpy_s_extrapolated").

The kernels' Z and es are compared with the replica on the timed replicates before anything is recorded.  Writes --out as JSON and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(torch, ops, name, p, warmup, reps):
    for _ in range(warmup):
        ops.call(name, p)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.call(name, p)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    return {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--numpy-replicates", type=int, default=2)
    ap.add_argument("--numpy-sets", type=int, default=50)
    ap.add_argument("--R", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--S", type=int, nargs="+", default=[50, 5000])
    ap.add_argument("--out", default=os.path.join("profiles", "gsea_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import gsea_ref as REF
    from multimodal_survival_prediction_amd import data, enrichment as E, ops, transfer

    dev = torch.device("cuda:0")
    n, G = 427, 5005
    cpu = data.make_cohort(n=n, dims=(16, 16, 8), seed=427, complete=True)             # (the volumes are not read)
    cohort = data.cohort_to(cpu, dev)
    x, lab = cohort["rnaseq"], cpu["label"].numpy()
    assert x.shape == (n, G)
    rows = np.arange(n)
    m = E.null_residuals(lab[:, 0], lab[:, 1], rows)
    names = transfer.default_gene_names(G)
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": args.reps, "n": n, "G": G,
           "numpy_threads": os.environ.get("OMP_NUM_THREADS", "unset"), "cases": []}
    for S in args.S:
        sizes = rng.integers(15, 501, S)
        off = np.concatenate([[0], np.cumsum(sizes)])
        gene = np.concatenate([np.sort(rng.choice(G, k, replace=False)) for k in sizes])
        sets = {"set_%04d" % j: [names[g] for g in gene[off[j]:off[j + 1]]] for j in range(S)}
        for R in args.R:
            perm = E.permutation_table(n, R, seed=0)
            ps, keep_s, scale, Z = ops.gsea_scores(x, rows, m, perm, plan_only=True)
            row = {"S": S, "R": R, "set_members": int(off[-1]), "scores_ms": timed(torch, ops, "mms_gsea_scores", ps, args.warmup, args.reps)}
            row["product_gflops"] = round(2.0 * (R + 1) * n * G / (row["scores_ms"]["median"] * 1e-3) / 1e9, 1)
            pe, keep_e, es, peak = ops.gsea_es(Z, off, gene, plan_only=True)
            row["es_ms"] = timed(torch, ops, "mms_gsea_es", pe, args.warmup, args.reps)
            p1, keep_1, _, _ = ops.gsea_es(Z, np.array([0, 15]), gene[:15], plan_only=True)           # (every set has >= 15 genes)
            row["es_sort_ms"] = timed(torch, ops, "mms_gsea_es", p1, args.warmup, args.reps)
            row["es_walk_share"] = round(1.0 - row["es_sort_ms"]["median"] / row["es_ms"]["median"], 3)
            ops.call("mms_gsea_es", pe)
            torch.cuda.synchronize()
            nr, ns = min(args.numpy_replicates, R + 1), min(args.numpy_sets, S)
            t0 = time.perf_counter()
            _, Zr = REF.scores(cpu["rnaseq"].numpy(), rows, m, perm[:nr])
            t_sc = time.perf_counter() - t0
            t0 = time.perf_counter()
            er, pr, gap = REF.es_all(Zr, off[:ns + 1], gene[:off[ns]], 1)
            t_es = time.perf_counter() - t0
            Zd, ed, pd_ = Z[:nr].cpu().numpy(), es[:nr, :ns].cpu().numpy(), peak[:nr, :ns].cpu().numpy()
            assert np.abs(Zd - Zr).max() <= 1e-10 * max(1.0, np.abs(Zr).max()), "kernel and replica Z differ"
            eh, ph, gh = REF.es_all(Zd, off[:ns + 1], gene[:off[ns]], 1)                     # the walk on the device's own Z
            assert np.abs(ed - eh).max() <= 4 * G * 2.0 ** -53 and (pd_ == ph)[gh > 1e-9].all(), "kernel and replica es differ"
            row.update(numpy_replicates_timed=nr, numpy_sets_timed=ns, numpy_scores_ms_per_replicate=round(t_sc * 1e3 / nr, 2),
                       numpy_es_ms_per_replicate_and_set=round(t_es * 1e3 / (nr * ns), 3),
                       numpy_s_extrapolated=round((t_sc / nr + t_es / (nr * ns) * S) * (R + 1), 1), agrees_with_numpy=True)
            row["numpy_over_launches"] = round(row["numpy_s_extrapolated"] * 1e3 / (row["scores_ms"]["median"] + row["es_ms"]["median"]), 1)
            del keep_s, keep_e, keep_1, es, peak, Z
            if R * S <= 10_000_000:
                e2e = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    E.enrich(cohort, sets, R=R, seed=0)
                    e2e.append((time.perf_counter() - t0) * 1e3)
                row["enrich_ms"] = [round(v, 1) for v in e2e]
            res["cases"].append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
