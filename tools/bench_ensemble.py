#!/usr/bin/env python
"""K = 5 PartialModalityNet (DenseNet121-3D encoder) at 64x64x32 as one ensemble, B in {4, 16, 32}, in patients/s:
  lock-step legs   FoldEnsemble.predict / FoldEnsemble.attribute (one launch sequence for the five members, one copy of the volumes,
                   mms_ensemble_reduce over the members)
  sequential legs  five SurvivalEngine.forward_eval / SurvivalEngine.attribute calls one after another: what the code offered before the
                   ensemble existed, on code this feature does not change
The legs are interleaved round by round in one process on the same batch; round 0 warms every shape (plans, graph capture) and is not
recorded.  Writes the per-round times, medians, patients/s and run-to-run spreads to --out as JSON and prints the same line.

  --sequential-only   the sequential legs alone: needs nothing of the ensemble, so the same file runs on an older checkout
  --parent-json FILE  a --sequential-only result measured on the parent commit in the same session: recorded under "parent_sequential"
  --reduce-only       mms_ensemble_reduce alone on K members of 32 x 64x64x32 floats -- under `rocprofv3 --kernel-trace --stats --` the
                      kernel's time against its (K + 2) n 4-byte traffic
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 16, 32])
    ap.add_argument("--steps", type=int, default=5, help="calls per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--volume", type=int, nargs=3, default=[64, 64, 32])
    ap.add_argument("--sequential-only", action="store_true")
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--reduce-only", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "ensemble_bench.json"))
    args = ap.parse_args()

    import torch
    from multimodal_survival_prediction_amd import models
    from multimodal_survival_prediction_amd.engine import engine_of

    dev = torch.device("cuda:0")
    K, dims = args.k, tuple(args.volume)

    if args.reduce_only:
        from multimodal_survival_prediction_amd.ensemble import ensemble_reduce
        n = 32 * dims[0] * dims[1] * dims[2]
        xs = [torch.randn(n, device=dev) for _ in range(K)]
        mean, spread = torch.empty(n, device=dev), torch.empty(n, device=dev)
        for _ in range(3):
            ensemble_reduce(xs, mean, spread)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(50):
            ensemble_reduce(xs, mean, spread)
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) / 50 * 1e6
        nbytes = (K + 2) * n * 4
        print(json.dumps({"K": K, "n": n, "bytes": nbytes, "us_per_call_host_timed": round(us, 2), "GB_per_s_host_timed": round(nbytes / us / 1e3, 1)}))
        return

    def make_models():
        ms = []
        for g in range(K):
            torch.manual_seed(42 + g)
            ms.append(models.PartialModalityNet(rna_dim=5005).to(dev).eval())
        return ms

    seq = [engine_of(m) for m in make_models()]
    ens = None
    if not args.sequential_only:
        from multimodal_survival_prediction_amd.ensemble import FoldEnsemble
        ens = FoldEnsemble(make_models())

    batches = {}
    for B in args.batches:
        g = torch.Generator().manual_seed(7 + B)
        batches[B] = dict(ct=torch.rand(B, 1, *dims, generator=g).to(dev), rna=torch.randn(B, 5005, generator=g).to(dev),
                          clinical=torch.randn(B, 1, generator=g).to(dev), mask=torch.ones(B, 3, device=dev))

    def seq_predict(b):
        return [e.forward_eval(b["ct"], b["rna"], b["clinical"], mask=b["mask"])[0].clone() for e in seq]

    def seq_attribute(b):
        return [e.attribute(b["ct"], b["rna"], b["clinical"], mask=b["mask"]) for e in seq]

    legs = {"sequential_predict": seq_predict, "sequential_attribute": seq_attribute}
    if ens is not None:
        legs["ensemble_predict"] = lambda b: ens.predict(b)
        legs["ensemble_attribute"] = lambda b: ens.attribute(b)

    ms = {name: {B: [] for B in args.batches} for name in legs}
    for r in range(args.rounds + 1):                # round 0: warm-up of every shape, not recorded
        for B in args.batches:
            for name, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    fn(batches[B])
                torch.cuda.synchronize()
                if r:
                    ms[name][B].append((time.perf_counter() - t0) / args.steps * 1e3)
    for e in seq:
        e.check_b4()
    med = {name: {B: statistics.median(v) for B, v in d.items()} for name, d in ms.items()}
    res = {"config": "%d x PartialModalityNet (DenseNet121-3D), %dx%dx%d, rna_dim 5005; a call scores / explains B patients with all %d members"
                     % (K, dims[0], dims[1], dims[2], K),
           "device": torch.cuda.get_device_name(0), "steps_per_round": args.steps, "rounds": args.rounds, "batches": args.batches,
           "ms_per_call": {name: {str(B): [round(x, 3) for x in v] for B, v in d.items()} for name, d in ms.items()},
           "ms_per_call_median": {name: {str(B): round(v, 3) for B, v in d.items()} for name, d in med.items()},
           "patients_per_s": {name: {str(B): round(B / v * 1e3, 1) for B, v in d.items()} for name, d in med.items()},
           "spread": {name: {str(B): round((max(v) - min(v)) / med[name][B], 4) for B, v in d.items()} for name, d in ms.items()}}
    if ens is not None:
        res["ensemble_over_sequential"] = {what: {str(B): round(med["sequential_" + what][B] / med["ensemble_" + what][B], 3) for B in args.batches}
                                           for what in ("predict", "attribute")}
    if args.parent_json:
        with open(args.parent_json) as fh:
            parent = json.load(fh)
        res["parent_sequential"] = {k: {n: v for n, v in parent[k].items() if n.startswith("sequential_")}
                                    for k in ("ms_per_call", "ms_per_call_median", "patients_per_s", "spread")}
        if ens is not None:
            res["ensemble_over_parent_sequential"] = {
                what: {str(B): round(parent["ms_per_call_median"]["sequential_" + what][str(B)] / med["ensemble_" + what][B], 3) for B in args.batches}
                for what in ("predict", "attribute")}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
