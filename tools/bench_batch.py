#!/usr/bin/env python
"""Batch-size scaling of ONE model's fused-graph training step (SurvivalEngine.train_step, graph replay).

Two models, each alone on the chip:
  partial_densenet   PartialModalityNet, DenseNet121-3D CT encoder, 64x64x32 volumes, RNA-seq 5005, modality masks, gate entropy
  image_only         ImageOnlyModel (3-conv encoder at 16 / 32 / 64 channels + two Linear layers), 64x64x32 volumes
at B in {4, 8, 16, 32, 64, 128}.  B <= 32 runs the small-batch head kernels (and B <= 16 the one-workgroup-row mms_head_fwd), larger
batches the MFMA Linear chain, the row-tiled gate backward and the sample-chunked mms_head_fwd.  Per (model, B): the first steps build
the plan and capture the graph (not recorded), a probe round sizes the timed window to ~0.5 s, then --rounds windows are timed with a host
clock around work that ends in a device synchronise.  Writes ms per step (median, all rounds, spread) and patients/s per B to --out as
JSON and prints the same line.  A batch size the build cannot run is recorded with its error text instead of a time."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 8, 16, 32, 64, 128])
    ap.add_argument("--models", nargs="+", default=["partial_densenet", "image_only"], choices=["partial_densenet", "image_only"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of work per timed round")
    ap.add_argument("--volume", type=int, nargs=3, default=[64, 64, 32])
    ap.add_argument("--rna-dim", type=int, default=5005)
    ap.add_argument("--out", default=os.path.join("profiles", "batch_scaling.json"))
    args = ap.parse_args()

    import torch
    from multimodal_survival_prediction_amd import _lib, data, models
    from multimodal_survival_prediction_amd.training import FusedOptimizer

    dev = torch.device("cuda:0")
    dims = tuple(args.volume)
    res = {"config": "one model, fused-graph train_step, %dx%dx%d volumes, rna %d" % (dims + (args.rna_dim,)),
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "models": {}}
    for name in args.models:
        torch.manual_seed(42)
        net = (models.PartialModalityNet(rna_dim=args.rna_dim) if name == "partial_densenet" else models.ImageOnlyModel()).to(dev).train()
        eng = FusedOptimizer(net, lr=1e-4, weight_decay=1e-4).engine
        rows = {}
        for B in args.batches:
            c = data.cohort_to(data.make_cohort(n=B, dims=dims, rna_dim=args.rna_dim if name == "partial_densenet" else 8, seed=B,
                                                complete=True), dev)
            mask = torch.tensor([[1, 1, 1], [0, 1, 1], [1, 0, 1], [1, 1, 0], [0, 1, 0], [1, 1, 1], [0, 0, 1], [1, 0, 0]],
                                dtype=torch.float32, device=dev).repeat((B + 7) // 8, 1)[:B].contiguous()
            t, e = c["label"][:, 0].contiguous(), c["label"][:, 1].contiguous()
            e[0] = 1.0                          # at least one event: every step is a usable Cox batch

            def step():
                if name == "partial_densenet":
                    eng.train_step(c["image"], c["rnaseq"], c["clinical"], mask=mask, time=t, event=e, skip_if_unusable=False)
                else:
                    eng.train_step(c["image"], time=t, event=e, skip_if_unusable=True)

            def timed(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    step()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / n
            try:
                for _ in range(3):              # plan, warm-up step, graph capture, first replays
                    step()
                n = max(5, min(2000, int(math.ceil(args.window / max(timed(5), 1e-5)))))
                ms = [timed(n) * 1e3 for _ in range(args.rounds)]
                eng.epoch_stats()               # (checks the in-launch hand-off time-out word of the DenseNet kernels)
            except RuntimeError as err:         # a batch size this build refuses (a limit's RuntimeError / MmsError): recorded, not timed
                if type(err) not in (RuntimeError, _lib.MmsError) or "HIP error" in str(err):
                    raise                       # a device error is not a refused shape: stop here
                rows[str(B)] = {"error": str(err)[:200]}
                print("%s B=%d: %s" % (name, B, rows[str(B)]["error"]), flush=True)
                continue
            med = statistics.median(ms)
            rows[str(B)] = {"steps_per_round": n, "ms_per_step": [round(x, 4) for x in ms], "ms_per_step_median": round(med, 4),
                            "spread": round((max(ms) - min(ms)) / med, 4), "patients_per_s": round(B / med * 1e3, 1)}
            print("%s B=%d: %.3f ms/step, %.1f patients/s" % (name, B, med, B / med * 1e3), flush=True)
            eng.plans.clear()                   # release this batch size's workspace and graphs before the next plan
            del c
            torch.cuda.empty_cache()
        res["models"][name] = rows
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
