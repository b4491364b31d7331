#!/usr/bin/env python
"""Input-gradient attribution of one PartialModalityNet (DenseNet121-3D encoder) at batch 4, 64x64x32: patients/s of
SurvivalEngine.attribute (eval forward in the per-layer forms + heads' backward + mms_dn121_input_grad + the result's device copies)
against patients/s of forward_eval alone (the captured eval graph, default forms) at the same size.  The two legs are interleaved round by
round in one process on the same batch.  Writes both, their ratio and the per-round times to --out as JSON and prints the same line.
Under `rocprofv3 --kernel-trace --stats -- python tools/bench_attribution.py --rounds 2` the kernel table shows conv0_bwd_data_kernel
beside conv0_fwd_box_kernel (the same 360 M MACs per sample) -- profiles/attribution_kernels.txt."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="calls per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--volume", type=int, nargs=3, default=[64, 64, 32])
    ap.add_argument("--train-leg", action="store_true", help="also run train_step rounds (puts conv0_bwd_weight into a kernel trace)")
    ap.add_argument("--out", default=os.path.join("profiles", "attribution_bench.json"))
    args = ap.parse_args()

    import torch
    from multimodal_survival_prediction_amd import models
    from multimodal_survival_prediction_amd.engine import engine_of

    dev = torch.device("cuda:0")
    B, dims = args.batch, tuple(args.volume)
    torch.manual_seed(42)
    model = models.PartialModalityNet(rna_dim=5005).to(dev)
    eng = engine_of(model)
    g = torch.Generator().manual_seed(7)
    ct = torch.rand(B, 1, *dims, generator=g).to(dev)
    rna = torch.randn(B, 5005, generator=g).to(dev)
    clin = torch.randn(B, 1, generator=g).to(dev)
    mask = torch.ones(B, 3, device=dev)
    time_, event = torch.arange(1, B + 1, dtype=torch.float32, device=dev), torch.ones(B, device=dev)

    def leg_attribute():
        for _ in range(args.steps):
            eng.attribute(ct, rna, clin, mask=mask)

    def leg_forward():
        for _ in range(args.steps):
            eng.forward_eval(ct, rna, clin, mask=mask)

    def leg_train():
        model.train()
        for _ in range(args.steps):
            eng.train_step(ct, rna, clin, mask=mask, time=time_, event=event)
        model.eval()

    legs = {"forward_eval": leg_forward, "attribute": leg_attribute}
    if args.train_leg:
        legs["train_step"] = leg_train
    model.eval()
    ms = {k: [] for k in legs}
    for r in range(args.rounds + 1):                # round 0: warm-up (plans, graph capture), not recorded
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    eng.check_b4()
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"config": "PartialModalityNet (DenseNet121-3D), batch %d, %dx%dx%d, rna_dim 5005" % (B, dims[0], dims[1], dims[2]),
           "device": torch.cuda.get_device_name(0), "steps_per_round": args.steps, "rounds": args.rounds,
           "ms_per_call": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "ms_per_call_median": {k: round(v, 4) for k, v in med.items()},
           "patients_per_s": {k: round(B / v * 1e3, 1) for k, v in med.items()},
           "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
           "attribute_over_forward": round(med["attribute"] / med["forward_eval"], 3)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
