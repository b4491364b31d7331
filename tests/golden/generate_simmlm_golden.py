#!/usr/bin/env python3
"""Generate tests/golden/g7_simmlm.npz by executing the REFERENCE's own SimMLM_SurvivalNet definition.

scripts/analysis/generate_km_curves.py imports SimpleITK (absent in the build container) after its model classes, so the class
block (lines 158-281: ModalityExpert, GatingNetwork, SimMLM_SurvivalNet) is exec'd by line range into a scratch namespace with
USE_MONAI = False -- the branch an install without MONAI takes.  Only data is stored: seeds, inputs, outputs, running statistics,
gradients and weight checksums; no reference text.

Usage:  python tests/golden/generate_simmlm_golden.py <path of a reference checkout>   (from the repository root)
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch
import torch.nn as nn

OUT = os.path.dirname(os.path.abspath(__file__))
SEED, B, RNA, VOL = 71, 8, 256, (16, 16, 8)
BIG, SUB = 100000, 7        # gradients of more than BIG elements are stored subsampled (1 MiB fixture limit)


def harvest(ref_root):
    path = os.path.join(ref_root, "scripts", "analysis", "generate_km_curves.py")
    lines = open(path, encoding="utf-8").read().split("\n")
    src = "\n" * 157 + "\n".join(lines[157:281])          # keep the original line numbers for tracebacks
    ns = {"torch": torch, "nn": nn, "np": np, "USE_MONAI": False}
    with contextlib.redirect_stdout(io.StringIO()):
        exec(compile(src, path, "exec"), ns)
    return ns


def inputs():
    rng = np.random.default_rng(SEED)
    ct = rng.random((B, 1) + VOL, dtype=np.float32)
    rna = rng.normal(0, 1, (B, RNA)).astype(np.float32)
    clin = rng.normal(0, 1, (B, 1)).astype(np.float32)
    # image-only, RNA-only, clinical-only, image+RNA, RNA+clinical, image+clinical, full, full
    mask = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1], [1, 1, 1]], np.float32)
    ct[mask[:, 0] == 0] = 0
    rna[mask[:, 1] == 0] = 0
    coef = rng.normal(0, 1, (5, B)).astype(np.float32)          # linear functional: ensemble, 3 experts, gate (B x 3 -> flattened below)
    gcoef = rng.normal(0, 1, (B, 3)).astype(np.float32)
    return ct, rna, clin, mask, coef, gcoef


def main(ref_root):
    ns = harvest(ref_root)
    torch.manual_seed(SEED)
    model = ns["SimMLM_SurvivalNet"](rna_dim=RNA, clinical_dim=1, feature_dim=128)
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
    out = {}
    sd = model.state_dict()
    out["param_names"] = np.array([k for k, _ in model.named_parameters()])
    out["init_sum"] = np.array([float(p.detach().double().sum()) for _, p in model.named_parameters()])
    out["init_abs"] = np.array([float(p.detach().double().abs().sum()) for _, p in model.named_parameters()])
    out["state_keys"] = np.array(list(sd.keys()))
    ct, rna, clin, mask, coef, gcoef = inputs()
    out.update(ct=ct, rna=rna, clin=clin, mask=mask, coef=coef, gcoef=gcoef)
    model.train()
    t = [torch.tensor(a) for a in (ct, rna, clin, mask)]
    ens, hz, g = model(*t)
    outs = [ens, hz['image'], hz['rnaseq'], hz['clinical']]
    for k, v in zip(("out_ens", "out_img", "out_rna", "out_clin"), outs):
        out[k] = v.detach().numpy()
    out["out_gate"] = g.detach().numpy()
    L = sum((torch.tensor(coef[i]) * outs[i]).sum() for i in range(4)) + (torch.tensor(gcoef) * g).sum()
    L.backward()
    for k, p in model.named_parameters():       # the two largest gradients (fallback conv3, RNA Linear 1) as every SUB-th element
        g = p.grad.numpy().reshape(-1)
        out["grad." + k] = g[::SUB].copy() if g.size > BIG else g.copy()
    for k, b in model.named_buffers():
        if not k.endswith("num_batches_tracked"):
            out["buf." + k] = b.numpy().copy()
    # an all-zero-mask row: NaN gate weights and ensemble hazard in the forward
    mask_z = mask.copy(); mask_z[5] = 0
    ct_z, rna_z = ct.copy(), rna.copy(); ct_z[5] = 0; rna_z[5] = 0
    with torch.no_grad():
        m2 = ns["SimMLM_SurvivalNet"](rna_dim=RNA, clinical_dim=1, feature_dim=128)
        m2.load_state_dict(model.state_dict())       # (post-step running statistics: the restatement loads the same)
        for m in m2.modules():
            if isinstance(m, nn.Dropout):
                m.p = 0.0
        m2.train()
        e2, h2, g2 = m2(torch.tensor(ct_z), torch.tensor(rna_z), torch.tensor(clin), torch.tensor(mask_z))
    out.update(zero_row=np.array(5), zero_ens=e2.numpy(), zero_gate=g2.numpy(),
               zero_img=h2['image'].numpy(), zero_rnah=h2['rnaseq'].numpy(), zero_clin=h2['clinical'].numpy())
    np.savez_compressed(os.path.join(OUT, "g7_simmlm.npz"), **out)
    print("wrote g7_simmlm.npz:", os.path.getsize(os.path.join(OUT, "g7_simmlm.npz")), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
