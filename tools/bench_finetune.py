#!/usr/bin/env python
"""What fine-tuning plans cost and save (multimodal_survival_prediction_amd.transfer; csrc/finetune.hip).

PartialModalityNet on the DenseNet121-3D encoder, 64x64x32 volumes, batch 4, one engine and the 5-fold lock-step group; one process,
device events, every variant warmed (plan, graph capture, first replays) before anything is timed, variants alternated inside each of
--repeats rounds so that drift hits all of them alike.

  step     ms per fused-graph training step: plain (no plan), the trivial plan (one segment, all multipliers 1 -- the price of the segment
           lookup), freeze_stages = 1..4 (the backward stops above the frozen stages; 4: no encoder backward), and 4 with encoder_eval.
  kernels  us of the optimiser pair alone: mms_grad_sumsq + mms_clip_adam against their tuned forms under the trivial plan and with the
           whole encoder frozen; achieved bytes/s from the segment sizes: 4 bytes per trainable element for the norm, 28 for the update
           (p, g, m, v read; p, m, v written) and 8 per trainable packed conv2 element for the two derived packs.

Writes --out as JSON and prints the same line; keys of an existing --out file that the tool does not produce are kept (`bench_py`: three
runs each of `python bench.py --gpus 1 --steps 20 --warmup 5` on the parent commit's tree and on this one, alternated, recorded by hand)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = [("plain", None), ("trivial", ""), ("freeze1", "freeze=1"), ("freeze2", "freeze=2"), ("freeze3", "freeze=3"), ("freeze4", "freeze=4"),
            ("freeze4_enceval", "freeze=4,enceval=1")]
W2N = 32 * 27 * 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30, help="steps per timed window")
    ap.add_argument("--group", type=int, default=5)
    ap.add_argument("--volume", type=int, nargs=3, default=[64, 64, 32])
    ap.add_argument("--rna-dim", type=int, default=5005)
    ap.add_argument("--out", default=os.path.join("profiles", "finetune_bench.json"))
    args = ap.parse_args()

    import torch
    from multimodal_survival_prediction_amd import _lib, data, models, ops
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    from multimodal_survival_prediction_amd.training import FusedOptimizer
    from multimodal_survival_prediction_amd.transfer import FineTunePlan

    dev, dims, B = torch.device("cuda:0"), tuple(args.volume), 4
    lib = _lib.load_library()
    c = data.cohort_to(data.make_cohort(n=B * args.group, dims=dims, rna_dim=args.rna_dim, seed=7, complete=True), dev)
    mask = torch.tensor([[1, 1, 1], [0, 1, 1], [1, 0, 1], [1, 1, 0]], dtype=torch.float32, device=dev)
    t, e = c["label"][:, 0].contiguous(), c["label"][:, 1].contiguous()
    e[::B] = 1.0                                # an event in every batch: every step is usable

    def batch(g):
        j = slice(g * B, (g + 1) * B)
        return dict(ct=c["image"][j], rna=c["rnaseq"][j], clinical=c["clinical"][j], mask=mask, time=t[j], event=e[j])

    def new_model(seed):
        torch.manual_seed(seed)
        return models.PartialModalityNet(rna_dim=args.rna_dim).to(dev).train()

    def plan_of(spec):
        return None if spec is None else FineTunePlan.parse(spec)

    def window(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    def series(fns, n):
        out = {k: [] for k in fns}
        for _ in range(args.repeats):           # variants alternated inside every round
            for k, fn in fns.items():
                out[k].append(window(fn, n))
        return {k: dict(ms=[round(x, 4) for x in v], median_ms=round(statistics.median(v), 4), spread_ms=round(max(v) - min(v), 4))
                for k, v in out.items()}

    res = {"config": "PartialModalityNet, DenseNet121-3D, %dx%dx%d, batch %d, rna %d" % (dims + (B, args.rna_dim)),
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "steps_per_window": args.steps}

    # ---- one engine ----
    engines, fns = {}, {}
    for name, spec in VARIANTS:
        kw = {} if spec is None else dict(finetune=plan_of(spec))
        eng = FusedOptimizer(new_model(1), lr=1e-4, weight_decay=1e-4, **kw).engine
        b0 = batch(0)
        step = (lambda eng=eng, b0=b0: eng.train_step(b0["ct"], b0["rna"], b0["clinical"], mask=b0["mask"], time=b0["time"], event=b0["event"],
                                                       skip_if_unusable=False))
        for _ in range(3):
            step()
        engines[name], fns[name] = eng, step
    torch.cuda.synchronize()
    res["step_single"] = series(fns, args.steps)
    print("single engine:", {k: v["median_ms"] for k, v in res["step_single"].items()}, flush=True)

    # ---- optimiser pair alone ----
    def pair(eng, tuned):
        P = next(iter(eng.plans.values()))
        st = ops.stream()
        if tuned:
            blk = ctypes.byref(P.tune)
            return lambda: (eng.sumsq.zero_(), lib.mms_grad_sumsq_tuned(blk, st), lib.mms_clip_adam_tuned(blk, st))
        blk = ctypes.byref(P.adam)
        return lambda: (eng.sumsq.zero_(), lib.mms_grad_sumsq(blk, st), lib.mms_clip_adam(blk, st))

    kf = {"plain": pair(engines["plain"], False), "trivial": pair(engines["trivial"], True), "encoder_frozen": pair(engines["freeze4"], True)}
    for fn in kf.values():
        fn()
    kern = series(kf, 50)
    n_all = engines["plain"].flat.numel()
    seg = engines["freeze4"].segments
    n_train = int(sum(int(seg.bounds[s + 1] - seg.bounds[s]) for s in range(len(seg.lr_mult)) if float(seg.lr_mult[s]) > 0))
    n_w2 = len(engines["plain"].w2_offsets) * W2N
    for k, (elems, packed) in {"plain": (n_all, n_w2), "trivial": (n_all, n_w2), "encoder_frozen": (n_train, 0)}.items():
        nbytes = 32 * elems + 8 * packed
        kern[k].update(trainable_elements=elems, bytes=nbytes, tbytes_per_s=round(nbytes / (kern[k]["median_ms"] * 1e-3) / 1e12, 3))
    res["optimiser_pair"] = kern
    print("optimiser pair (ms incl. the 8-byte memset):", {k: (v["median_ms"], v["tbytes_per_s"]) for k, v in kern.items()}, flush=True)
    del engines, fns, kf
    torch.cuda.empty_cache()

    # ---- the fold group ----
    fns = {}
    for name, spec in VARIANTS:
        kw = {} if spec is None else dict(finetune=plan_of(spec))
        grp = FoldGroupEngine([new_model(10 + g) for g in range(args.group)], lr=1e-4, weight_decay=1e-4, **kw)
        bs = [batch(g) for g in range(args.group)]
        step = lambda grp=grp, bs=bs: grp.train_step(bs, skip_if_unusable=False)
        for _ in range(3):
            step()
        fns[name] = step
    torch.cuda.synchronize()
    res["step_group%d" % args.group] = series(fns, max(5, args.steps // 2))
    print("group of %d:" % args.group, {k: v["median_ms"] for k, v in res["step_group%d" % args.group].items()}, flush=True)

    if os.path.exists(args.out):                # series recorded beside the tool's own (bench_py: the headline bench, parent against this change)
        try:
            old = json.load(open(args.out))
            res.update({k: v for k, v in old.items() if k not in res})
        except ValueError:
            pass
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
