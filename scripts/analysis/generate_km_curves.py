#!/usr/bin/env python3
"""Kaplan-Meier curves of the models' risk groups -- what the reference's scripts/analysis/generate_km_curves.py announces and leaves
unimplemented ("load each model's best-fold checkpoint, predict, draw the KM curves"; it stops at the model definitions).

    python scripts/analysis/generate_km_curves.py --model final simmim            # best fold of each, scored on the MI355X
    python scripts/analysis/generate_km_curves.py --predictions final=a.csv cox=results/cox_baseline/fold_1_predictions.csv
    python scripts/analysis/generate_km_curves.py --model final --stratify 10000 --min-prop 0.1 --seed 0 --cut best

--model NAME: reads results/NAME/cv_results.json, takes the fold with the largest best_c_index and scores that fold's held-out split
with models/NAME/fold_k_best.pth through evaluate_model.py's --predict path (the HIP eval forward; no CPU fallback).
--predictions NAME=FILE.csv: ready predictions (columns survival_time, event, risk_score[, patient_id]).

Every model is split at the median of its risk score (survival_stats.risk_groups) -- or, with --cut best, at the cut with the largest
log-rank statistic -- and reported with the cut-point scan of multimodal_survival_prediction_amd/risk_strata.py: the median split's
asymptotic and permutation p, the best cut with the ADJUSTED p of the maximally selected statistic, Peto hazard ratios.  Models scored on
the same patients (same survival_time / event columns) go through ONE stratify call, so they see the same relabellings.

Writes <outdir>/km_summary.json, <outdir>/NAME_km.csv (both groups' Kaplan-Meier tables with Greenwood variance and log-log bands) and,
when matplotlib is importable, <outdir>/km_curves.png.  <outdir> defaults to results/km_curves."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multimodal_survival_prediction_amd import risk_strata as RS  # noqa: E402


def _evaluate_model():
    spec = importlib.util.spec_from_file_location("evaluate_model", os.path.join(os.path.dirname(os.path.abspath(__file__)), "evaluate_model.py"))
    em = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(em)
    return em


def best_fold(cv):
    """-> (fold number, its best_c_index, the number of folds) of a cv_results.json dictionary; the first fold wins a tie"""
    folds = cv["fold_results"]
    best = max(folds, key=lambda f: (f["best_c_index"], -int(f["fold"])))
    return int(best["fold"]), float(best["best_c_index"]), int(cv.get("hyperparameters", {}).get("n_folds", cv.get("n_folds", len(folds))))


def predict_best_fold(name, results_dir, models_dir, outdir):
    em = _evaluate_model()
    if name not in em.MODELS:
        raise SystemExit(f"--model {name}: evaluate_model.py knows {sorted(em.MODELS)}")
    with open(os.path.join(results_dir, name, "cv_results.json")) as f:
        fold, c, n_folds = best_fold(json.load(f))
    ckpt = os.path.join(models_dir, name, f"fold_{fold}_best.pth")
    genes = os.path.join(models_dir, name, f"fold_{fold}_genes.json")
    df = em.predict(ckpt, name, fold, n_folds, 0, os.path.join(outdir, f"{name}_predictions.csv"), genes=genes if os.path.exists(genes) else None)
    return df, dict(fold=fold, best_c_index=c, checkpoint=ckpt)


def _groups_of_same_patients(frames):
    """names grouped by identical (survival_time, event) columns, in first-seen order"""
    keys, groups = [], []
    for name, df in frames.items():
        k = (df["survival_time"].to_numpy(float).tobytes(), df["event"].to_numpy(int).tobytes())
        if k in keys:
            groups[keys.index(k)].append(name)
        else:
            keys.append(k)
            groups.append([name])
    return groups


def km_curves(frames, outdir, replicates=10000, seed=0, min_prop=0.1, cut="median", alpha=0.05, plots=True, sources=None):
    """frames: {name: predictions DataFrame} -> the km_summary.json dictionary (written with the per-model CSVs and the figure)."""
    os.makedirs(outdir, exist_ok=True)
    summary = dict(replicates=int(replicates), seed=int(seed), min_prop=float(min_prop), alpha=float(alpha), cut=cut, models={})
    curves = {}
    for names in _groups_of_same_patients(frames):
        first = frames[names[0]]
        t, e = first["survival_time"].to_numpy(float), first["event"].to_numpy(int)
        risk = np.stack([frames[k]["risk_score"].to_numpy(float) for k in names])
        res = RS.stratify(risk, t, e, R=replicates, seed=seed, min_prop=min_prop, alpha=alpha)
        for k, r, m in zip(names, risk, res.models):
            cs = RS.km_groups(t, e, m.high(r, cut), alpha)
            curves[k] = (cs, m)
            pd.DataFrame([row for c in cs for row in c.rows()]).to_csv(os.path.join(outdir, f"{k}_km.csv"), index=False)
            entry = dict(patients=int(len(t)), deaths=int((e != 0).sum()), **m.summary())
            entry["km"] = {c.group: dict(patients=int(c.at_risk[0]), median=c.median, median_low=c.median_low, median_high=c.median_high) for c in cs}
            if sources and k in sources:
                entry["source"] = sources[k]
            summary["models"][k] = entry
    summary["models"] = {k: summary["models"][k] for k in frames}                # the order given
    with open(os.path.join(outdir, "km_summary.json"), "w") as f:
        json.dump(summary, f, indent=2)
    if plots:
        _plot(curves, [k for k in frames], cut, os.path.join(outdir, "km_curves.png"))
    return summary


def _plot(curves, names, cut, path):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        print("matplotlib not available: figure skipped")
        return
    fig, axes = plt.subplots(1, len(names), figsize=(6 * len(names), 4.5), squeeze=False)
    for ax, k in zip(axes[0], names):
        cs, m = curves[k]
        for c in cs:
            colour = "tab:red" if c.group == "High Risk" else "tab:blue"
            ax.step(c.time, c.survival, where="post", color=colour, label=f"{c.group} (n = {int(c.at_risk[0])})")
            ax.fill_between(c.time, c.low, c.high, step="post", alpha=0.15, color=colour, linewidth=0)
        p = m.median_p_permutation if cut == "median" else m.p_adjusted
        ax.set_title(f"{k}: {'median split, permutation' if cut == 'median' else 'best cut, adjusted'} p = {p:.3g}")
        ax.set_xlabel("Time (days)"); ax.set_ylabel("Survival Probability"); ax.set_ylim(0, 1.02); ax.grid(True, alpha=0.3); ax.legend(loc="best")
    fig.tight_layout(); fig.savefig(path, dpi=150); plt.close(fig)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", nargs="+", default=[], metavar="NAME", help="score the best fold of results/NAME/cv_results.json")
    ap.add_argument("--predictions", nargs="+", default=[], metavar="NAME=FILE.csv", help="ready predictions instead of a checkpoint")
    ap.add_argument("--results-dir", default="results")
    ap.add_argument("--models-dir", default="models")
    ap.add_argument("--outdir", default=os.path.join("results", "km_curves"))
    ap.add_argument("--stratify", type=int, default=10000, metavar="R", help="random relabellings of the cut-point scan")
    ap.add_argument("--min-prop", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cut", choices=("median", "best"), default="median", help="the split the curves are drawn for")
    ap.add_argument("--no-plots", action="store_true")
    a = ap.parse_args(argv)
    if not a.model and not a.predictions:
        ap.error("give --model NAME ... and / or --predictions NAME=FILE.csv ...")
    if a.stratify < 0 or not 0.0 <= a.min_prop <= 0.5:
        ap.error("--stratify needs R >= 0 and --min-prop a share in [0, 0.5]")
    os.makedirs(a.outdir, exist_ok=True)
    frames, sources = {}, {}
    for name in a.model:
        frames[name], sources[name] = predict_best_fold(name, a.results_dir, a.models_dir, a.outdir)
    for item in a.predictions:
        name, sep, path = item.partition("=")
        if not sep or not name or name in frames:
            ap.error(f"--predictions {item}: expected NAME=FILE.csv with a name not used twice")
        frames[name], sources[name] = pd.read_csv(path), dict(predictions=path)
    s = km_curves(frames, a.outdir, a.stratify, a.seed, a.min_prop, a.cut, plots=not a.no_plots, sources=sources)
    for k, m in s["models"].items():
        print(f"{k}: {m['patients']} patients; median split chi2 {m['median']['chi2']:.3f} (p {m['median']['p_asymptotic']:.3g} asymptotic, "
              f"{m['median']['p_permutation']:.3g} permutation), HR {m['median']['hazard_ratio']:.2f}; best of {m['n_cuts']} cuts: risk > "
              f"{m['best']['threshold']:.4f}, chi2 {m['best']['chi2']:.3f}, adjusted p {m['best']['p_adjusted']:.3g}")
    print(f"saved {os.path.join(a.outdir, 'km_summary.json')}, one NAME_km.csv per model" + ("" if a.no_plots else ", km_curves.png"))
    return s


if __name__ == "__main__":
    main()
