#!/usr/bin/env python3
"""Gene-set enrichment of the cohort's Cox scores: which pathways?

    python scripts/analysis/gene_set_enrichment.py --gmt sets.gmt [--R 1000] [--seed 0] [--min-size 15] [--max-size 500] [--weight 1]
    python scripts/analysis/gene_set_enrichment.py --gmt sets.gmt --scores results/attribution/gene_scores.csv
    python scripts/analysis/gene_set_enrichment.py --gmt sets.gmt --scores results/rsf_baseline/fold_1_vimp.csv --score-column vimp

Default (no --scores): the LABEL-PERMUTATION analysis (multimodal_survival_prediction_amd/enrichment.py: enrich).  The cohort is the one
cox_baseline.py reads -- data/processed/* under the cwd or MMS_DATA_ROOT when present, else the seeded synthetic cohort of MMS_PATIENTS
patients -- and every patient with RNA-seq and a survival label is analysed.  The gene statistic is the Cox score at beta = 0
standardised by its exact permutation variance; the null relabels the PATIENTS R times, so gene-gene correlation is kept.  All of it
runs on the MI355X (no CPU fallback).

--scores CSV: the PRERANKED analysis of one score per gene (columns gene, score; evaluate_model.py --attribute's gene_scores.csv is read by
its mean_abs_grad column; any other file by the column named with --score-column, e.g. rsf_baseline.py's fold_k_vimp.csv).  Its null shuffles GENE labels: it ignores
gene-gene correlation and is anti-conservative.  Use it only for scores that have no labels behind them; whenever labels exist the
label-permutation form above is the default and the one to report.

The gene-set file is yours (tab-separated .gmt: name, description, genes; e.g. an MSigDB collection in gene symbols); none ships with
the package.  Names are matched exactly against the cohort's gene names (gene_00000 ... for a cohort without names).

Writes --out (results/enrichment): enrichment.csv (set, size, es, nes, p, fdr, fwer, peak, leading_edge_size; by p, then |nes|),
enrichment_summary.json (settings, the dropped sets and unmatched genes, every set's numbers) and leading_edge.json ({set: [genes]})."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts", "training"))


def read_scores(path, column):
    import pandas as pd
    df = pd.read_csv(path)
    if column is None:                                  # "score", else gene_scores.csv's own column
        column = next((c for c in ("score", "mean_abs_grad") if c in df.columns), "score")
    if "gene" not in df.columns or column not in df.columns:
        raise SystemExit("%s must have the columns gene and %s (has %s)" % (path, column, list(df.columns)))
    if df["gene"].duplicated().any():
        raise SystemExit("%s lists a gene twice" % path)
    return [str(g) for g in df["gene"]], df[column].to_numpy(dtype=np.float64)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Gene-set enrichment of Cox scores.  Default: label-permutation null (relabels patients, keeps "
                                 "gene-gene correlation).  --scores: preranked null (shuffles gene labels, IGNORES gene-gene correlation, "
                                 "anti-conservative) -- only for scores without labels behind them.")
    ap.add_argument("--gmt", required=True, help="gene sets, tab-separated: name, description, genes (user-supplied; none ships)")
    ap.add_argument("--R", type=int, default=1000, help="permutations (default 1000)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--min-size", type=int, default=15, help="smallest set after matching (default 15)")
    ap.add_argument("--max-size", type=int, default=500, help="largest set after matching (default 500)")
    ap.add_argument("--weight", type=int, choices=(0, 1), default=1, help="1: hits weigh |score| (default); 0: classic Kolmogorov-Smirnov")
    ap.add_argument("--scores", metavar="CSV", help="preranked mode: columns gene,score.  This null ignores gene-gene correlation; the "
                    "label-permutation form (no --scores) is the default whenever labels exist")
    ap.add_argument("--score-column", default=None, help="the score column of --scores (default: score, else gene_scores.csv's mean_abs_grad)")
    ap.add_argument("--out", default="results/enrichment")
    a = ap.parse_args(argv)

    from _common import env_int, load_or_make_cohort, setup_device
    from multimodal_survival_prediction_amd import enrichment
    _, rank, device = setup_device()
    if rank != 0:
        return
    os.makedirs(a.out, exist_ok=True)
    t0 = time.perf_counter()
    kw = dict(R=a.R, seed=a.seed, weight=a.weight, min_size=a.min_size, max_size=a.max_size)
    if a.scores:
        genes, z = read_scores(a.scores, a.score_column)
        res = enrichment.enrich_preranked(z, genes, a.gmt, **kw)
    else:
        cohort = load_or_make_cohort(device, n=env_int("MMS_PATIENTS", 240), dims=(32, 32, 32), seed=427, complete=True)   # volumes unused
        res = enrichment.enrich(cohort, a.gmt, **kw)
    dt = time.perf_counter() - t0
    df = res.to_frame()
    df = df.assign(_a=-df["nes"].abs().fillna(0.0)).sort_values(["p", "_a"], kind="stable").drop(columns="_a")
    df.to_csv(os.path.join(a.out, "enrichment.csv"), index=False)
    res.save(os.path.join(a.out, "enrichment_summary.json"))
    with open(os.path.join(a.out, "leading_edge.json"), "w") as f:
        json.dump(dict(zip(res.names, res.leading_edge)), f, indent=2)
    print(f"{res.mode}: {len(res.names)} sets ({len(res.report['dropped'])} dropped), {len(res.z)} genes, "
          f"{res.n if res.n else 'no'} patients, R = {res.R}, {dt:.2f} s; saved {a.out}/enrichment.csv")
    for _, r in df.head(10).iterrows():
        print(f"  {r['set']:<40s} size {int(r['size']):4d}  ES {r['es']:+.3f}  NES {r['nes']:+.2f}  p {r['p']:.4f}  fdr {r['fdr']:.3f}  fwer {r['fwer']:.3f}")


if __name__ == "__main__":
    main()
