#!/usr/bin/env python
"""GPU batch augmentation: what it costs (profiles/augment_bench.json; with --affine the rotation / zoom / noise leg,
profiles/augment_affine_bench.json; with --elastic the elastic-deformation leg, profiles/augment_elastic_bench.json).

The headline layout: 608-patient masked cohort, PartialModalityNet (DenseNet121-3D encoder), 5 folds in lock-step, batch 4, 64x64x32
volumes, batches named by index (one gather launch per step), sub-groups on three streams -- one training epoch per sample.

  epoch    one process = one tree (--root: this checkout, or a checkout of the parent commit built next to it): a warm-up epoch, then
           --epochs timed epochs per leg.  Legs: off (no spec: the plain gather -- the only leg a parent tree knows), on_device /
           on_pinned (every record-only transform enabled; cohort in HBM / in pinned host memory), off_pinned, and aff_device /
           aff_pinned (rot, zoom and noise on top: the resampling launch mms_gather_affine_group), ela_device / ela_pinned (elastic
           deformation on top of those: mms_gather_elastic_group).  Prints one JSON line.
  compare  --parent-root DIR: fresh child processes `epoch --legs off` of the parent tree and of this tree, alternated --rounds
           times, each under its own time limit; stops at the first child that fails.  Then one child of this tree with every leg.
           Condition checked: mean(off, this tree) - mean(off, parent) <= max(spread parent, spread this tree), spread = max - min.
           --affine: the last child also runs the aff_* legs and the result goes to profiles/augment_affine_bench.json.
           --elastic: ... the aff_* and the ela_* legs, profiles/augment_elastic_bench.json.  --leg LEG: the leg that parent and this
           tree are compared on (default off; aff_device: the affine-only spec, which the parent knows too), stored under its name
           (LEG_parent_vs_this; the all-legs child under same_process, or same_process_LEG for a leg other than off).
  kernel   the two gather kernels alone on the SAME batches (run under `rocprofv3 --kernel-trace --stats`): per lock-step position
           one mms_gather_rows_group and one mms_gather_aug_group launch; prints the bytes each launch moves (from the shapes: rows
           read + rows written).  --affine-form staged | direct: a mms_gather_affine_group launch per position as well, in that form
           (both forms are one kernel name: one profiler run each); its bytes are the rows it must read and write, plus the records.
           --elastic: a mms_gather_elastic_group launch per position too, same rows, same matrices, in the same form.
  merge    --stats-csv: kernel-stats CSV of that run -> per-launch time of both kernels, achieved bytes/s and its share of the HBM
           peak, merged into --out.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
SPEC = "flip=0.5,shift=2:4:4,scale=0.9:1.1,offset=-0.05:0.05,moddrop=0.2"
SPEC_AFF = SPEC + ",rot=10,zoom=0.9:1.1,noise=0:0.03"
SPEC_ELA = SPEC_AFF + ",elastic=0:3:16"
DIRECT_STAGE = 16          # AffP.stage_floats that no source box fits: the direct form everywhere
STAGED_STAGE = 8192        # ... the library's whole budget, given explicitly: the staged form also for rows that deform (whose default, 0, is direct)
HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E specification (6.29e12 measured with a float4 copy)
B, K, DIMS, RNA = 4, 5, (64, 64, 32), 5005


def _setup(root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from multimodal_survival_prediction_amd import data
    cpu = data.make_cohort(n=608, dims=DIMS, rna_dim=RNA, seed=608, complete=False)
    has = cpu["has_survival"].numpy()
    survival, non_survival = np.nonzero(has)[0], np.nonzero(~has)[0]
    folds = data.kfold_indices(len(survival), K, seed=42)
    return torch, data, cpu, [np.concatenate([survival[f[0]], non_survival]) for f in folds]


def cmd_epoch(args):
    torch, data, cpu, train_sets = _setup(args.root)
    from multimodal_survival_prediction_amd import models
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    from multimodal_survival_prediction_amd.training import train_epoch_lockstep
    dev = torch.device("cuda:0")
    cohorts = {"device": data.cohort_to(cpu, dev)}
    legs = args.legs.split(",")
    if any(leg.endswith("pinned") for leg in legs):
        cohorts["pinned"] = data.cohort_pin(cpu)
    ms = []
    for k in range(K):
        torch.manual_seed(42 + k)
        ms.append(models.PartialModalityNet(rna_dim=RNA).to(dev).train())
    group = FoldGroupEngine(ms, lr=1e-4, weight_decay=1e-4, adamw=False, gate_entropy_weight=0.01)

    def loaders(leg):
        c = cohorts["pinned" if leg.endswith("pinned") else "device"]
        spec = {"on": SPEC, "af": SPEC_AFF, "el": SPEC_ELA}.get(leg[:2])
        kw = dict(augment=spec, augment_style="partial") if spec else {}
        return [data.BatchLoader(c, t, B, shuffle=True, seed=42 + k, lazy=True, with_valid=True, **kw) for k, t in enumerate(train_sets)]

    ld = {leg: loaders(leg) for leg in legs}
    out = {leg: [] for leg in legs}
    for r in range(args.epochs + 1):                # epoch 0: warm-up (plans, graph capture), not recorded
        for leg in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            train_epoch_lockstep(group, ld[leg], "partial", concurrent=3)
            torch.cuda.synchronize()
            if r:
                out[leg].append(round(time.perf_counter() - t0, 5))
    print(json.dumps({"root": os.path.abspath(args.root), "device": torch.cuda.get_device_name(0), "epoch_s": out,
                      "patients_per_epoch": int(sum(len(t) for t in train_sets))}), flush=True)


def _child(root, legs, epochs, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "epoch", "--root", root, "--legs", legs, "--epochs", str(epochs)],
                       capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("child `epoch --root %s` ended with %d: nothing more is started" % (root, r.returncode))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def cmd_compare(args):
    this = os.path.dirname(HERE)
    off = {"parent": [], "this": []}
    dev = None
    affine = args.affine or args.elastic
    same = "same_process" if args.leg == "off" else "same_process_" + args.leg      # (a second compare on another leg keeps the first's block)
    for _ in range(args.rounds):
        for name, root in (("parent", args.parent_root), ("this", this)):
            res = _child(root, args.leg, args.epochs, args.limit)
            off[name] += res["epoch_s"][args.leg]
            dev = res["device"]
            print(name, res["epoch_s"][args.leg], flush=True)
    full = _child(this, "off,on_device,off_pinned,on_pinned" + (",aff_device,aff_pinned" if affine else "") +
                  (",ela_device,ela_pinned" if args.elastic else ""), args.epochs, args.limit)
    mean = {k: statistics.mean(v) for k, v in off.items()}
    spread = {k: max(v) - min(v) for k, v in off.items()}
    res = {"config": "608 masked patients, PartialModalityNet (DenseNet121-3D), %d folds lock-step, batch %d, %dx%dx%d, rna_dim %d, "
                     "batches named by index, 3 streams; one training epoch per sample" % ((K, B) + DIMS + (RNA,)),
           "device": dev, "spec": SPEC, **({"spec_affine": SPEC_AFF} if affine else {}), **({"spec_elastic": SPEC_ELA} if args.elastic else {}),
           "patients_per_epoch": full["patients_per_epoch"],
           args.leg + "_parent_vs_this": {"order": "parent, this alternated; %d processes each, %d timed epochs per process after a warm-up epoch"
                                           % (args.rounds, args.epochs),
                                  "epoch_s": off, "mean_s": {k: round(v, 5) for k, v in mean.items()},
                                  "spread_s": {k: round(v, 5) for k, v in spread.items()},
                                  "excess_s": round(mean["this"] - mean["parent"], 5), "allowed_s": round(max(spread.values()), 5),
                                  "condition_met": bool(mean["this"] - mean["parent"] <= max(spread.values()))},
           same: {"epoch_s": full["epoch_s"], "mean_s": {k: round(statistics.mean(v), 5) for k, v in full["epoch_s"].items()}}}
    m = res[same]["mean_s"]
    res[same]["on_over_off"] = {"device": round(m["on_device"] / m["off"], 4), "pinned": round(m["on_pinned"] / m["off_pinned"], 4)}
    if affine:
        res[same]["affine_over_off"] = {"device": round(m["aff_device"] / m["off"], 4),
                                                  "pinned": round(m["aff_pinned"] / m["off_pinned"], 4)}
    if args.elastic:
        sp = {k: max(v) - min(v) for k, v in full["epoch_s"].items()}
        res[same]["elastic_over_affine"] = {"device": round(m["ela_device"] / m["aff_device"], 4),
                                                      "pinned": round(m["ela_pinned"] / m["aff_pinned"], 4)}
        res[same]["elastic_minus_affine_s"] = {
            w: {"difference": round(m["ela_" + w] - m["aff_" + w], 5), "spread": round(max(sp["ela_" + w], sp["aff_" + w]), 5)}
            for w in ("device", "pinned")}
    _merge(args.out, res)
    print(json.dumps(res), flush=True)
    if not res[args.leg + "_parent_vs_this"]["condition_met"]:
        raise SystemExit("leg %s is slower than the parent by more than the run-to-run spread" % args.leg)


def _merge(path, res):
    old = {}
    if os.path.exists(path):
        with open(path) as fh:
            old = json.load(fh)
    old.update(res)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(json.dumps(old, indent=1) + "\n")


def _kernel_key(args):
    return "kernel_" + args.where + ("" if args.affine_form == "none" else "_" + args.affine_form)


KERNELS = ("gather_rows_kernel", "gather_aug_kernel", "gather_affine_kernel", "gather_elastic_kernel")


def cmd_kernel(args):
    torch, data, cpu, train_sets = _setup(os.path.dirname(HERE))
    from multimodal_survival_prediction_amd import _lib, augment as A, ops
    lib, S = _lib.load_library(), _lib.structs()
    dev = torch.device("cuda:0")
    c = data.cohort_to(cpu, dev) if args.where == "device" else data.cohort_pin(cpu)
    valid = cpu["has_survival"].float()
    valid = valid.to(dev) if args.where == "device" else valid.pin_memory()
    vol = DIMS[0] * DIMS[1] * DIMS[2]
    lab, mask = c["label"], c["mask"]
    srcs = [(c["rnaseq"], RNA, mask[:, 1:], (A.ROLE_PLAIN, 1)), (c["image"].view(-1, vol), vol, mask, (A.ROLE_VOLUME, 0)),
            (c["clinical"], 1, None, (A.ROLE_PLAIN, 2)), (mask, 3, None, (A.ROLE_MASK, -1)), (lab, 1, None, (A.ROLE_PLAIN, -1)),
            (lab[:, 1:], 1, None, (A.ROLE_PLAIN, -1)), (valid.view(-1, 1), 1, None, (A.ROLE_PLAIN, -1))]
    idx_dev = torch.zeros(K, B, dtype=torch.int64, device=dev)
    rec_dev = torch.zeros(K, B, A.REC_WORDS, dtype=torch.int32, device=dev)
    aff_dev = torch.zeros(K, B, A.AFF_WORDS, dtype=torch.int32, device=dev)
    ela_dev = torch.zeros(K, B, A.ELA_WORDS, dtype=torch.int32, device=dev)
    form = args.affine_form
    if args.elastic and form == "none":
        raise SystemExit("--elastic times the elastic launch beside the affine one: give --affine-form staged or direct")
    ela_spec = A.AugmentSpec.parse(SPEC_ELA)
    keep, Gs, As = [], [], []
    for g in range(K):
        outs = [torch.zeros(B, w, device=dev) for _, w, _, _ in srcs]
        keep += outs
        Gs.append(ops.gather_params(idx_dev[g], B, [(a, o, w, flag) for (a, w, flag, _), o in zip(srcs, outs)]))
        As.append(A.aug_block(rec_dev[g], [r for *_, r in srcs], DIMS, (2, 4, 4)))
    Ga, Aa = (S["GatherP"] * K)(*Gs), (S["AugP"] * K)(*As)
    Fa = (S["AffP"] * K)(*[A.aff_block(aff_dev[g], DIRECT_STAGE if form == "direct" else STAGED_STAGE if args.elastic else 0) for g in range(K)])
    ld = [data.BatchLoader(c, t, B, shuffle=True, seed=42 + k, lazy=True, with_valid=True, augment=SPEC, augment_style="partial")
          for k, t in enumerate(train_sets)]
    # the affine records of the same rows: a second loader with the same seeds (the first draw, hence drop bits and bytes, is the same)
    ld_aff = [data.BatchLoader(c, t, B, shuffle=True, seed=42 + k, lazy=True, with_valid=True, augment=SPEC_AFF, augment_style="partial")
              for k, t in enumerate(train_sets)] if form != "none" else ld
    # ... and the elastic records: a third loader, same seeds (its first two draws are the second loader's)
    ld_ela = [data.BatchLoader(c, t, B, shuffle=True, seed=42 + k, lazy=True, with_valid=True, augment=SPEC_ELA, augment_style="partial")
              for k, t in enumerate(train_sets)] if args.elastic else ld
    Ea = (S["ElaP"] * K)(*[A.ela_block(ela_dev[g], ela_spec.elastic_spacing, [ela_spec.elastic_range[1]] * 3) for g in range(K)])
    n = 0
    bytes_plain = bytes_aug = 0
    widths = torch.tensor([float(RNA), float(vol), 1.0])
    for pos, pos_aff, pos_ela in zip(zip(*ld), zip(*ld_aff), zip(*ld_ela)):
        if any(len(b["index"]) != B for b in pos):
            break
        idx = torch.stack([b["index"] for b in pos])
        rec = torch.stack([b["augment"].rec for b in pos])
        has = cpu["mask"][idx][..., [1, 0, 2]] != 0                                        # rna, image, clinical rows that exist
        drop = torch.stack([(rec[..., A.DROP] >> j) & 1 for j in (1, 0, 2)], -1) != 0
        written = K * B * (RNA + vol + 1 + 3 + 3) * 4
        has[..., 2] = True                                                                 # (clinical rows are always read)
        bytes_plain += written + int((has * widths).sum()) * 4 + K * B * 6 * 4
        bytes_aug += written + int(((has & ~drop) * widths).sum()) * 4 + K * B * 6 * 4
        idx_dev.copy_(idx)
        rec_dev.copy_(rec)
        if form != "none":
            aff_dev.copy_(torch.stack([b["augment"].aff for b in pos_aff]))
        if args.elastic:
            assert all(torch.equal(a["augment"].aff, e["augment"].aff) for a, e in zip(pos_aff, pos_ela))      # the same matrices
            ela_dev.copy_(torch.stack([b["augment"].ela for b in pos_ela]))
        for _ in range(args.repeat):     # one launch per kind: the plain gather, then one more block array at a time
            A.launch_gather(lib, Ga, ng=K)
            A.launch_gather(lib, Ga, Aa, ng=K)
            if form != "none":      # (the 8-word records keep their flip / shift: this entry point does not read them)
                A.launch_gather(lib, Ga, Aa, Fa, ng=K)
            if args.elastic:
                A.launch_gather(lib, Ga, Aa, Fa, Ea, ng=K)
        torch.cuda.synchronize()
        n += 1
    per = {"gather_rows_kernel": bytes_plain // n, "gather_aug_kernel": bytes_aug // n}
    if form != "none":
        per["gather_affine_kernel"] = bytes_aug // n + K * B * 4 * A.AFF_WORDS
    if args.elastic:
        per["gather_elastic_kernel"] = per["gather_affine_kernel"] + K * B * 4 * A.ELA_WORDS
    res = {_kernel_key(args): {"positions": n, "launches_per_kernel": n * args.repeat, "members": K, "batch": B, "bytes_per_launch": per}}
    if form != "none":
        res[_kernel_key(args)]["affine_form"] = form
    _merge(args.out, res)
    print(json.dumps(res), flush=True)


def cmd_merge(args):
    import csv
    with open(args.out) as fh:
        res = json.load(fh)
    key = _kernel_key(args)
    t = {}
    with open(args.stats_csv) as fh:
        for row in csv.DictReader(fh):
            for name in KERNELS:
                if row["Name"].startswith(name):
                    t[name] = {"calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 3),
                               "min_us": round(float(row["MinNs"]) / 1e3, 3), "max_us": round(float(row["MaxNs"]) / 1e3, 3)}
    for name, v in t.items():
        v["bytes_per_s"] = round(res[key]["bytes_per_launch"][name] / (v["mean_us"] * 1e-6), 1)
        v["share_of_hbm_peak"] = round(v["bytes_per_s"] / HBM_PEAK, 5)
    res[key]["rocprofv3_kernel_stats"] = t
    res[key]["aug_over_plain"] = round(t["gather_aug_kernel"]["mean_us"] / t["gather_rows_kernel"]["mean_us"], 3)
    if "gather_affine_kernel" in t:
        res[key]["affine_over_plain"] = round(t["gather_affine_kernel"]["mean_us"] / t["gather_rows_kernel"]["mean_us"], 3)
        res[key]["affine_over_aug"] = round(t["gather_affine_kernel"]["mean_us"] / t["gather_aug_kernel"]["mean_us"], 3)
    if "gather_elastic_kernel" in t:
        res[key]["elastic_over_plain"] = round(t["gather_elastic_kernel"]["mean_us"] / t["gather_rows_kernel"]["mean_us"], 3)
        res[key]["elastic_over_affine"] = round(t["gather_elastic_kernel"]["mean_us"] / t["gather_affine_kernel"]["mean_us"], 3)
    res["hbm_peak_bytes_per_s"] = HBM_PEAK
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res[key]), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("epoch"); p.add_argument("--root", default=os.path.dirname(HERE)); p.add_argument("--legs", default="off")
    p.add_argument("--epochs", type=int, default=3); p.set_defaults(fn=cmd_epoch)
    p = sub.add_parser("compare"); p.add_argument("--parent-root", required=True); p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--epochs", type=int, default=3); p.add_argument("--limit", type=int, default=300, help="seconds per child process")
    p.add_argument("--affine", action="store_true"); p.add_argument("--elastic", action="store_true")
    p.add_argument("--leg", default="off", help="the leg compared between the two trees"); p.add_argument("--out"); p.set_defaults(fn=cmd_compare)
    p = sub.add_parser("kernel"); p.add_argument("--where", choices=["device", "pinned"], default="device")
    p.add_argument("--repeat", type=int, default=1); p.add_argument("--affine-form", choices=["none", "staged", "direct"], default="none")
    p.add_argument("--elastic", action="store_true"); p.add_argument("--out"); p.set_defaults(fn=cmd_kernel)
    p = sub.add_parser("merge"); p.add_argument("--stats-csv", required=True); p.add_argument("--where", choices=["device", "pinned"], default="device")
    p.add_argument("--affine-form", choices=["none", "staged", "direct"], default="none"); p.add_argument("--elastic", action="store_true")
    p.add_argument("--out"); p.set_defaults(fn=cmd_merge)
    args = ap.parse_args()
    if getattr(args, "out", "") is None:
        affine = getattr(args, "affine", False) or getattr(args, "affine_form", "none") != "none"
        name = "augment_elastic_bench.json" if getattr(args, "elastic", False) else "augment_affine_bench.json" if affine else "augment_bench.json"
        args.out = os.path.join(os.path.dirname(HERE), "profiles", name)
    args.fn(args)


if __name__ == "__main__":
    main()
