#!/usr/bin/env python3
"""Generate tests/golden/g8_image_only.npz by executing the REFERENCE's own ImageOnlyModel definition.

scripts/analysis/generate_km_curves.py runs its whole pipeline on import, so the class block (lines 28-54) is exec'd by line range into
a scratch namespace.  Only data is stored: seeds, inputs, outputs, running statistics, gradients, parameter names and weight checksums;
no reference text.  Two cases: "a" = 8 patients, 16x16x8 volumes; "b" = 3 patients, 9x10x7 volumes (odd grids: 5x5x4 -> 3x3x2 -> 2x2x1).

Usage:  python tests/golden/generate_image_only_golden.py <path of a reference checkout>   (from the repository root)
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 83
CASES = {"a": (8, (16, 16, 8)), "b": (3, (9, 10, 7))}


def harvest(ref_root):
    path = os.path.join(ref_root, "scripts", "analysis", "generate_km_curves.py")
    lines = open(path, encoding="utf-8").read().split("\n")
    src = "\n" * 27 + "\n".join(lines[27:54])          # keep the original line numbers for tracebacks
    ns = {"torch": torch, "nn": nn, "np": np}
    exec(compile(src, path, "exec"), ns)
    return ns


def inputs(tag):
    B, vol = CASES[tag]
    rng = np.random.default_rng(SEED + ord(tag))
    return rng.random((B, 1) + vol, dtype=np.float32), rng.normal(0, 1, B).astype(np.float32)


def main(ref_root):
    ns = harvest(ref_root)
    out = {}
    for tag in CASES:
        torch.manual_seed(SEED)
        model = ns["ImageOnlyModel"]()
        if tag == "a":
            out["param_names"] = np.array([k for k, _ in model.named_parameters()])
            out["init_sum"] = np.array([float(p.detach().double().sum()) for _, p in model.named_parameters()])
            out["init_abs"] = np.array([float(p.detach().double().abs().sum()) for _, p in model.named_parameters()])
            out["state_keys"] = np.array(list(model.state_dict().keys()))
        ct, coef = inputs(tag)
        out[tag + ".ct"], out[tag + ".coef"] = ct, coef
        model.train()
        risk = model(torch.tensor(ct))
        out[tag + ".train_risk"] = risk.detach().numpy()
        (torch.tensor(coef) * risk).sum().backward()          # a fixed linear functional of the risks
        for k, p in model.named_parameters():
            out[tag + ".grad." + k] = p.grad.numpy().copy()
        for k, b in model.named_buffers():
            out[tag + ".buf." + k] = b.numpy().copy()
        model.eval()
        with torch.no_grad():                                  # eval after the train forward: the moved running statistics
            out[tag + ".eval_risk"] = model(torch.tensor(ct)).numpy()
    path = os.path.join(OUT, "g8_image_only.npz")
    np.savez_compressed(path, **out)
    print("wrote g8_image_only.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
