#!/usr/bin/env python3
"""Generate golden input/output vectors by executing the REFERENCE's own definitions.

Runs only in the build container (needs /root/reference); the fixtures it writes
(`tests/golden/*.npz`) are data only -- seeds, inputs, expected outputs -- and are what
travels to the GPU box.  No reference source is copied into the repo: the reference
scripts are read as text from /root/reference at generation time and executed in a
scratch namespace / scratch cwd.

How each reference file is harvested:
  * scripts/training/final_multimodal.py   exec'd whole; stops with FileNotFoundError at
    its first CSV read (:205) AFTER MultiModalSurvivalNet (:59), custom cox_loss (:171)
    and calculate_cindex (:188) exist; train_epoch/validate (:238-305) are then exec'd by line range
    into that namespace.  MONAI/torchsurv are absent here, so the fallback
    3-conv encoder and the custom Cox loss are what is defined.
  * scripts/training/train_rnaseq_only.py  exec'd whole; stops at :217.  Gives fallback
    neg_partial_log_likelihood (:40) and the O(n^2) ConcordanceIndex (:55).
  * scripts/training/partial_modality_training.py / simple_fusion.py import SimpleITK
    before any class is defined, so the class blocks are exec'd by line range
    (partial :165-331 -> PartialModalityNet, cox_loss, gate_entropy_loss;
     simple  :46-73,160-236 -> fallback NPLL, ConcordanceIndex, SimpleFusionModel)
    with USE_MONAI = USE_TORCHSURV = False, exactly the branch an install without
    MONAI/torchsurv would take.

  * the epoch loops of partial_modality_training.py (:382-485), simple_fusion.py (:242-333) and flexible_multimodal.py
    (:262-351, with its fallback loss / metric :42-67) sit after the data access or the SimpleITK import: exec'd by line range
    into the namespaces above, with GATE_ENTROPY_WEIGHT = 0.01 (partial :369) and tqdm = an identity function of this harness.

Usage:  python tests/golden/generate_golden.py          (from the repo root) writes g9_loops.npz and g10_cindex_ties.npz
        python tests/golden/generate_golden.py --all    also rewrites g1 ... g6 (same arrays; the zip members carry new time stamps)
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn as nn

REF = "/root/reference/scripts/training"
OUT = os.path.dirname(os.path.abspath(__file__))


def _exec_until_data(path):
    """exec a reference script in a scratch cwd; return its namespace at the first data access."""
    src = open(path, encoding="utf-8").read()
    ns = {"__name__": "__ref__", "__file__": path}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                exec(compile(src, path, "exec"), ns)
        except FileNotFoundError:
            pass
        finally:
            os.chdir(cwd)
    return ns


def _exec_lines(path, ranges, ns):
    lines = open(path, encoding="utf-8").read().split("\n")
    for lo, hi in ranges:
        # keep original line numbers for tracebacks
        src = "\n" * (lo - 1) + "\n".join(lines[lo - 1:hi])
        with contextlib.redirect_stdout(io.StringIO()):
            exec(compile(src, path, "exec"), ns)
    return ns


def harvest():
    fm = _exec_until_data(f"{REF}/final_multimodal.py")
    # train_epoch/validate sit after the CSV read (:238-305): exec'd by line range into the same namespace
    _exec_lines(f"{REF}/final_multimodal.py", [(238, 305)], fm)
    rn = _exec_until_data(f"{REF}/train_rnaseq_only.py")
    # train_rnaseq_only.py defines its model and train_epoch/validate before the data access: rn holds RNASeqSurvivalModel too
    base = {"torch": torch, "nn": nn, "np": np, "USE_MONAI": False, "USE_TORCHSURV": False, "tqdm": _tqdm}
    pm = _exec_lines(f"{REF}/partial_modality_training.py", [(165, 331)], dict(base))
    sf = _exec_lines(f"{REF}/simple_fusion.py", [(46, 73), (160, 236)], dict(base))
    # the epoch loops: partial :382-485 (reads GATE_ENTROPY_WEIGHT, :369), simple :242-333
    pm["GATE_ENTROPY_WEIGHT"] = 0.01
    _exec_lines(f"{REF}/partial_modality_training.py", [(382, 485)], pm)
    _exec_lines(f"{REF}/simple_fusion.py", [(242, 333)], sf)
    return fm, rn, pm, sf


def _tqdm(it, **kw):
    return it


def harvest_flexible():
    """flexible_multimodal.py: fallback loss / metric (:42-67), FlexibleMultimodalModel (:157-256), train_epoch / validate (:262-351)."""
    base = {"torch": torch, "nn": nn, "np": np, "USE_MONAI": False, "USE_TORCHSURV": False, "tqdm": _tqdm}
    return _exec_lines(f"{REF}/flexible_multimodal.py", [(42, 67), (157, 256), (262, 351)], base)


# ----------------------------------------------------------------------------------------------
# synthetic inputs (all from numpy default_rng so the tests can regenerate them without torch RNG)
# ----------------------------------------------------------------------------------------------

def surv_batch(rng, n, mode):
    """distinct survival times (no ties) + event pattern `mode`."""
    t = rng.exponential(1000.0, size=n) + np.arange(n) * 1e-3 + 1.0
    t = t.astype(np.float32)
    assert len(np.unique(t)) == n
    if mode == "all":
        e = np.ones(n, np.float32)
    elif mode == "none":
        e = np.zeros(n, np.float32)
    elif mode == "one":
        e = np.zeros(n, np.float32)
        e[rng.integers(n)] = 1
    elif mode == "maxtime":  # the single event sits at the largest time
        e = np.zeros(n, np.float32)
        e[np.argmax(t)] = 1
    else:
        e = (rng.random(n) < 0.57).astype(np.float32)
        if e.sum() == 0:
            e[0] = 1
    h = rng.normal(0, 1.0, size=n).astype(np.float32)
    return h, e, t


def gen_cox(fm, rn, sf):
    out = {}
    rng = np.random.default_rng(1234)
    cases = []
    for n in (1, 2, 3, 4, 8, 16, 64, 2048):
        for mode in ("all", "mixed", "one", "none", "maxtime"):
            if n == 1 and mode != "all":
                continue
            cases.append((n, mode))
    for ci, (n, mode) in enumerate(cases):
        h, e, t = surv_batch(rng, n, mode)
        key = f"c{ci:02d}_n{n}_{mode}"
        ht = torch.tensor(h, requires_grad=True)
        loss = fm["cox_loss"](ht, torch.tensor(e), torch.tensor(t))
        if loss.grad_fn is not None:
            loss.backward()
            g = ht.grad.numpy()
        else:  # degenerate batch: fresh leaf, no graph (final_multimodal.py:173-176)
            g = np.zeros_like(h)
        out[key + "_h"], out[key + "_e"], out[key + "_t"] = h, e, t
        out[key + "_loss"] = np.float32(loss.item())
        out[key + "_grad"] = g.astype(np.float32)
        # the two other in-file formulations must agree on these no-tie batches
        if e.sum() > 0 and n >= 2:
            l2 = rn["neg_partial_log_likelihood"](torch.tensor(h), torch.tensor(e), torch.tensor(t)).item()
            l3 = sf["neg_partial_log_likelihood"](torch.tensor(h), torch.tensor(e), torch.tensor(t)).item()
            assert abs(l2 - loss.item()) <= 2e-5 * max(1, abs(l2)), (key, l2, loss.item())
            assert abs(l3 - loss.item()) <= 2e-5 * max(1, abs(l3)), (key, l3, loss.item())
    np.savez_compressed(f"{OUT}/g1_cox.npz", **out)
    print("g1_cox:", len(cases), "cases")


def gen_cindex(rn, sf):
    out = {}
    rng = np.random.default_rng(4321)
    for n in (4, 23, 116, 1639):
        h, e, t = surv_batch(rng, n, "mixed")
        c = rn["ConcordanceIndex"]()(torch.tensor(h), torch.tensor(e), torch.tensor(t)).item()
        if n <= 116:
            c2 = sf["ConcordanceIndex"]()(torch.tensor(h), torch.tensor(e), torch.tensor(t)).item()
            assert c == c2
        out[f"n{n}_h"], out[f"n{n}_e"], out[f"n{n}_t"] = h, e, t
        out[f"n{n}_cindex"] = np.float64(c)
    # no permissible pair -> 0.5 (train_rnaseq_only.py:70)
    h, e, t = surv_batch(rng, 5, "none")
    out["n5none_h"], out["n5none_e"], out["n5none_t"] = h, e, t
    out["n5none_cindex"] = np.float64(rn["ConcordanceIndex"]()(torch.tensor(h), torch.tensor(e), torch.tensor(t)).item())
    np.savez_compressed(f"{OUT}/g2_cindex.npz", **out)
    print("g2_cindex done")


def _zero_dropout(m):
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0


def model_inputs(rng, B, rna_dim, vol):
    ct = rng.random((B, 1) + vol, dtype=np.float32)
    rna = rng.normal(0, 1, (B, rna_dim)).astype(np.float32)
    clin = (np.clip(rng.normal(60, 11, (B, 1)), 30, 90) / 100.0).astype(np.float32)
    return ct, rna, clin


def _grads(model):
    return {k: p.grad.detach().numpy().copy() for k, p in model.named_parameters()}


def gen_models(fm, pm, sf):
    """G3: the three classes with the reference's fallback CT encoder.

    small variant (rna_dim=96, volume 16x16x8): inputs + outputs + per-parameter grad norms for all three;
    full state_dict + all grads for MultiModalSurvivalNet, head grads for the other two (weights of those
    come from torch.manual_seed(seed) construction, as in the full variant).
    full variant (rna_dim=5005, volume 64x64x32): weights come from torch.manual_seed(seed) construction,
    only inputs' seed, outputs and per-parameter grad norms are stored.
    """
    out = {}
    for tag, rna_dim, vol, B, seed in (("small", 96, (16, 16, 8), 4, 7), ("full", 5005, (64, 64, 32), 4, 11)):
        rng = np.random.default_rng(100 + seed)
        ct, rna, clin = model_inputs(rng, B, rna_dim, vol)
        h0, e, t = surv_batch(rng, B, "mixed")
        mask = np.array([[1, 1, 1], [0, 1, 1], [1, 0, 1], [0, 1, 0]], np.float32)[:B]
        out[f"{tag}_e"], out[f"{tag}_t"], out[f"{tag}_mask"] = e, t, mask
        if tag == "small":
            out["small_ct"], out["small_rna"], out["small_clin"] = ct, rna, clin
        tct, trna, tclin = torch.tensor(ct), torch.tensor(rna), torch.tensor(clin)
        te, tt, tmask = torch.tensor(e), torch.tensor(t), torch.tensor(mask)

        # ---- MultiModalSurvivalNet (final_multimodal.py:59) ----
        torch.manual_seed(seed)
        m = fm["MultiModalSurvivalNet"](rna_dim=rna_dim)
        _zero_dropout(m)
        sd0 = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
        m.eval()
        with torch.no_grad():
            out[f"{tag}_mm_eval_hazard"] = m(tct, trna, tclin).numpy()
        m.train()
        hz = m(tct, trna, tclin)
        loss = fm["cox_loss"](hz, te, tt)
        loss.backward()
        out[f"{tag}_mm_train_hazard"] = hz.detach().numpy()
        out[f"{tag}_mm_train_loss"] = np.float32(loss.item())
        g = _grads(m)
        sd1 = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
        for k in g:
            out[f"{tag}_mm_gnorm/{k}"] = np.float64(np.linalg.norm(g[k].astype(np.float64)))
        if tag == "small":
            for k in sd0:
                out[f"small_mm_sd/{k}"] = sd0[k]
            for k in g:
                out[f"small_mm_grad/{k}"] = g[k]
            for k in sd1:  # BN running stats after the one train-mode forward
                if "running" in k:
                    out[f"small_mm_sd_after/{k}"] = sd1[k]

        # ---- PartialModalityNet (partial_modality_training.py:165) ----
        torch.manual_seed(seed)
        m = pm["PartialModalityNet"](rna_dim=rna_dim)
        _zero_dropout(m)
        sd0 = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
        m.eval()
        with torch.no_grad():
            hz, gw = m(tct, trna, tclin, tmask)
            out[f"{tag}_pm_eval_hazard"], out[f"{tag}_pm_eval_gate"] = hz.numpy(), gw.numpy()
        m.train()
        hz, gw = m(tct, trna, tclin, tmask)
        c_loss = pm["cox_loss"](hz, te, tt)
        e_loss = pm["gate_entropy_loss"](gw)
        loss = c_loss + 0.01 * e_loss  # partial_modality_training.py:422
        loss.backward()
        out[f"{tag}_pm_train_hazard"], out[f"{tag}_pm_train_gate"] = hz.detach().numpy(), gw.detach().numpy()
        out[f"{tag}_pm_cox"], out[f"{tag}_pm_entropy"] = np.float32(c_loss.item()), np.float32(e_loss.item())
        g = _grads(m)
        for k in g:
            out[f"{tag}_pm_gnorm/{k}"] = np.float64(np.linalg.norm(g[k].astype(np.float64)))
        if tag == "small":  # heads only (encoder weights are pinned by the mm variant + seed construction)
            for k in g:
                if not k.startswith("ct_encoder") and not k.startswith("rna_encoder.0"):
                    out[f"small_pm_grad/{k}"] = g[k]

        # ---- SimpleFusionModel (simple_fusion.py:160) ----
        torch.manual_seed(seed)
        m = sf["SimpleFusionModel"](rna_dim=rna_dim)
        _zero_dropout(m)
        sd0 = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
        m.eval()
        with torch.no_grad():
            out[f"{tag}_sf_eval_hazard"] = m(tct, trna).numpy()
        m.train()
        hz = m(tct, trna)
        loss = sf["neg_partial_log_likelihood"](hz, te, tt)
        loss.backward()
        out[f"{tag}_sf_train_hazard"] = hz.detach().numpy()
        out[f"{tag}_sf_train_loss"] = np.float32(loss.item())
        g = _grads(m)
        for k in g:
            out[f"{tag}_sf_gnorm/{k}"] = np.float64(np.linalg.norm(g[k].astype(np.float64)))
        if tag == "small":
            for k in g:
                if k.startswith("fusion"):
                    out[f"small_sf_grad/{k}"] = g[k]
    np.savez_compressed(f"{OUT}/g3_models.npz", **out)
    print("g3_models done:", len(out), "arrays")


def gen_extra_models(rn):
    """g6: RNASeqSurvivalModel (train_rnaseq_only.py:126-151, harvested whole) and FlexibleMultimodalModel
    (flexible_multimodal.py:157-256, class block exec'd by line range with USE_MONAI = False: SimpleITK is imported at :38,
    before any class exists).  Dropout forced to 0; weights from torch.manual_seed construction; small variants store the
    full state_dict and gradients, default-width variants only outputs and gradient norms."""
    out = {}
    fx = harvest_flexible()
    for tag, seed, B, rna_dim, vol in (("small", 21, 6, 40, (16, 16, 8)), ("full", 22, 16, 5005, (32, 32, 16))):
        rng = np.random.default_rng(300 + seed)
        ct = rng.random((B, 1) + vol, dtype=np.float32)
        rna = rng.normal(0, 1, (B, rna_dim)).astype(np.float32)
        h0, e, t = surv_batch(rng, B, "mixed")
        mask = (rng.random((B, 2)) < 0.6).astype(np.float32)
        mask[0] = (1, 1); mask[1] = (0, 1); mask[2] = (1, 0); mask[3] = (0, 0)
        out[f"{tag}_e"], out[f"{tag}_t"], out[f"{tag}_mask2"] = e, t, mask
        if tag == "small":
            out["small_ct"], out["small_rna"] = ct, rna
        tct, trna, te, tt, tmask = torch.tensor(ct), torch.tensor(rna), torch.tensor(e), torch.tensor(t), torch.tensor(mask)
        # ---- RNASeqSurvivalModel ----
        torch.manual_seed(seed)
        m = rn["RNASeqSurvivalModel"](input_dim=rna_dim) if tag == "full" else rn["RNASeqSurvivalModel"](input_dim=rna_dim, hidden_dims=[48, 32, 16])
        _zero_dropout(m)
        sd0 = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
        m.eval()
        with torch.no_grad():
            out[f"{tag}_rs_eval"] = m(trna).squeeze().numpy()
        m.train()
        hz = m(trna).squeeze()
        loss = rn["neg_partial_log_likelihood"](hz, te.long(), tt)
        loss.backward()
        out[f"{tag}_rs_train"], out[f"{tag}_rs_loss"] = hz.detach().numpy(), np.float32(loss.item())
        g = _grads(m)
        for k in g:
            out[f"{tag}_rs_gnorm/{k}"] = np.float64(np.linalg.norm(g[k].astype(np.float64)))
        if tag == "small":
            for k in sd0:
                out[f"small_rs_sd/{k}"] = sd0[k]
            for k in g:
                out[f"small_rs_grad/{k}"] = g[k]
        # ---- FlexibleMultimodalModel (fallback encoder branch) ----
        torch.manual_seed(seed)
        m = fx["FlexibleMultimodalModel"](rna_dim=rna_dim)
        _zero_dropout(m)
        sd0 = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
        m.eval()
        with torch.no_grad():
            out[f"{tag}_fx_eval"] = m(tct, trna, tmask).numpy()
        m.train()
        hz = m(tct, trna, tmask)
        loss = rn["neg_partial_log_likelihood"](hz, te.long(), tt)
        loss.backward()
        out[f"{tag}_fx_train"], out[f"{tag}_fx_loss"] = hz.detach().numpy(), np.float32(loss.item())
        g = _grads(m)
        for k in g:
            out[f"{tag}_fx_gnorm/{k}"] = np.float64(np.linalg.norm(g[k].astype(np.float64)))
        if tag == "small":     # a few whole tensors (creation-order / RNG pin + element-wise gradients); the rest as norms above
            keep = [k for k in sd0 if k.startswith("missing_") or k.startswith("fusion.7") or k.startswith("rna_encoder.8.bias")
                    or k.startswith("image_encoder.0.")]
            for k in keep:
                out[f"small_fx_sd/{k}"] = sd0[k]
                if k in g:
                    out[f"small_fx_grad/{k}"] = g[k]
    # one epoch of the reference's own train_epoch (train_rnaseq_only.py:157-176: no clipping, loss / len(loader))
    rng = np.random.default_rng(77)
    n, B, rna_dim = 40, 8, 24
    rna = rng.normal(0, 1, (n, rna_dim)).astype(np.float32)
    t = (rng.exponential(1000.0, n) + 1 + np.arange(n) * 1e-3).astype(np.float32)
    e = (rng.random(n) < 0.6).astype(np.int64)
    torch.manual_seed(5)
    m = rn["RNASeqSurvivalModel"](input_dim=rna_dim, hidden_dims=[32, 16])
    _zero_dropout(m)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-3)
    loader = [dict(rnaseq=torch.tensor(rna[i:i + B]), time=torch.tensor(t[i:i + B]).view(-1, 1),
                   event=torch.tensor(e[i:i + B]).view(-1, 1)) for i in range(0, n, B)]
    losses = [rn["train_epoch"](m, loader, opt, torch.device("cpu")) for _ in range(3)]
    vl, vc = rn["validate"](m, loader, torch.device("cpu"))
    out["ep_rna"], out["ep_t"], out["ep_e"] = rna, t, e.astype(np.float32)
    out["ep_losses"], out["ep_val"] = np.array(losses, np.float64), np.array([vl, vc], np.float64)
    np.savez_compressed(f"{OUT}/g6_extra_models.npz", **out)
    print("g6_extra_models done:", len(out), "arrays")


def gen_epoch(fm):
    """G5: one epoch of the reference's own train_epoch/validate (final_multimodal.py:238-305) on a seeded
    synthetic 88-patient cohort, config-1 style (small volume so it runs in seconds; dropout ACTIVE, so the
    trajectory also pins RNG consumption order of the restated model)."""
    rng = np.random.default_rng(88)
    N, rna_dim, vol, B = 88, 96, (16, 16, 8), 4
    ct, rna, clin = model_inputs(rng, N, rna_dim, vol)
    _, e, t = surv_batch(rng, N, "mixed")
    label = np.stack([t, e], 1).astype(np.float32)
    batches = [dict(image=torch.tensor(ct[i:i + B]), rnaseq=torch.tensor(rna[i:i + B]),
                    clinical=torch.tensor(clin[i:i + B]), label=torch.tensor(label[i:i + B]))
               for i in range(0, N, B)]
    torch.manual_seed(5)
    m = fm["MultiModalSurvivalNet"](rna_dim=rna_dim)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4, weight_decay=1e-4)  # final_multimodal.py:350
    losses = []
    for ep in range(2):
        losses.append(fm["train_epoch"](m, batches, opt, torch.device("cpu")))
    val_loss, _ = fm["validate"](m, batches[:6], torch.device("cpu"))
    m.eval()
    with torch.no_grad():
        hz = m(batches[0]["image"], batches[0]["rnaseq"], batches[0]["clinical"]).numpy()
    np.savez_compressed(f"{OUT}/g5_epoch.npz", train_losses=np.array(losses, np.float64),
                        val_loss=np.float64(val_loss), final_hazard_b0=hz,
                        cohort_seed=np.int64(88), model_seed=np.int64(5))
    print("g5_epoch:", losses, val_loss)


# ----------------------------------------------------------------------------------------------
# g9: the partial / simple / flexible epoch loops on ONE special-batch cohort
# ----------------------------------------------------------------------------------------------

LOOP_VOL, LOOP_RNA, LOOP_B, LOOP_NTRAIN = (16, 16, 8), 96, 4, 22
LOOP_SGD = (1e-2, 0.9)          # lr, momentum of the optimizer handed to the loops


def special_cohort(seed=2024, vol=LOOP_VOL, rna_dim=LOOP_RNA):
    """36 patients (numpy only; tests/test_oracle_golden.py and tests/test_gpu_flexible_epoch.py restate this function and are
    pinned to it by the arrays stored in g9_loops.npz).  Training split = patients 0..21 in batches of 4:
      batch 0  all labelled, events present            batch 3  2 labelled (1 event) + 2 unlabelled
      batch 1  all labelled, NO event                  batch 4  all labelled
      batch 2  ONE labelled patient + 3 unlabelled     batch 5  ragged tail of 2
    validation split = patients 22..35: batch A ordinary, batch B without events, batch C three labelled + one unlabelled patient,
    batch D (tail of 2) one unlabelled + one labelled patient.
    Rows of absent modalities (mask column 0) are zero, unlabelled patients carry time = event = 0."""
    rng = np.random.default_rng(seed)
    n, v = 36, LOOP_NTRAIN
    ct = rng.random((n, 1) + tuple(vol), dtype=np.float32)
    rna = rng.normal(0, 1, (n, rna_dim)).astype(np.float32)
    age = (np.clip(rng.normal(60, 11, n), 30, 90) / 100.0).astype(np.float32)
    time = (rng.exponential(1000.0, n) + 1.0 + np.arange(n) * 1e-2).astype(np.float32)
    event = (rng.random(n) < 0.6).astype(np.float32)
    has = np.ones(n, bool)
    event[0], event[3] = 1, 0
    event[4:8] = 0
    has[9:12] = False; event[8] = 1
    has[14:16] = False; event[12], event[13] = 1, 0
    event[16] = 1
    event[20], event[21] = 1, 0
    event[v] = 1
    event[v + 4:v + 8] = 0
    event[v + 8] = 1; has[v + 9] = False
    has[v + 12] = False; event[v + 13] = 1
    mask = np.ones((n, 3), np.float32)          # [has_image, has_rnaseq, has_clinical]
    mask[1, 0] = 0; mask[5, 1] = 0; mask[10, 0] = 0; mask[13, 2] = 0; mask[17, 0] = 0; mask[18, 1] = 0; mask[19, :2] = 0
    mask[v + 1, 0] = 0; mask[v + 2, 1] = 0
    ct[mask[:, 0] == 0] = 0.0
    rna[mask[:, 1] == 0] = 0.0
    clin = (age * mask[:, 2]).astype(np.float32).reshape(n, 1)
    time = np.where(has, time, 0.0).astype(np.float32)
    event = np.where(has, event, 0.0).astype(np.float32)
    assert len(np.unique(time[has])) == int(has.sum())
    return dict(image=ct, rnaseq=rna, clinical=clin, time=time, event=event, has_survival=has, mask=mask, n=n)


def loop_batches(c, idx, style, B=LOOP_B):
    """Plain dicts in the key layout each reference loop reads (partial: label / mask (B, 3) / clinical; simple and flexible: time (B, 1)
    float, event (B, 1) long; flexible: mask (B, 2)); has_survival is a list of bools."""
    out = []
    for i in range(0, len(idx), B):
        j = np.asarray(idx[i:i + B])
        b = dict(image=torch.tensor(c["image"][j]), rnaseq=torch.tensor(c["rnaseq"][j]), has_survival=[bool(x) for x in c["has_survival"][j]])
        if style == "partial":
            b["clinical"] = torch.tensor(c["clinical"][j])
            b["label"] = torch.tensor(np.stack([c["time"][j], c["event"][j]], 1))
            b["mask"] = torch.tensor(c["mask"][j])
        else:
            b["time"] = torch.tensor(c["time"][j]).view(-1, 1)
            b["event"] = torch.tensor(c["event"][j]).long().view(-1, 1)
            if style == "flexible":
                b["mask"] = torch.tensor(c["mask"][j][:, :2])
        out.append(b)
    return out


class _Recorder:
    """Harness code: records what a loop hands to its C-index (hazards, events, times), then calls the original."""

    def __init__(self):
        self.calls = []

    def function(self, fn):
        def wrapped(hazard, event, time):
            self.calls.append(tuple(np.asarray(torch.as_tensor(a).numpy()).copy() for a in (hazard, event, time)))
            return fn(hazard, event, time)
        return wrapped

    def metric_class(self, cls):
        rec = self

        class Recording:
            def __call__(self, log_hazard, event, time):
                return rec.function(cls())(log_hazard, event, time)
        return Recording


def gen_loops(pm, sf, fx):
    try:
        import lifelines  # noqa: F401
        have_lifelines = True
    except ImportError:
        have_lifelines = False
    c = special_cohort()
    out = dict(cohort_seed=np.int64(2024), time=c["time"], event=c["event"], has_survival=c["has_survival"], mask=c["mask"],
               image_sum=np.float64(c["image"].astype(np.float64).sum()), rnaseq_sum=np.float64(c["rnaseq"].astype(np.float64).sum()),
               lifelines=np.bool_(have_lifelines))
    tr, va = np.arange(LOOP_NTRAIN), np.arange(LOOP_NTRAIN, c["n"])
    cpu = torch.device("cpu")
    # The optimizer is the caller's argument, not part of the loop text: plain SGD.  Under the scripts' Adam the parameters whose true
    # gradient is exactly zero (every bias that feeds a training-mode BatchNorm) move by +-lr per step along the SIGN of rounding
    # noise, which depends on the host's thread count -- measured between 1 and 8 threads: running means apart by 4.5e-3 of their
    # maximum after two epochs.  SGD moves them by the noise itself, and a step taken or left out is as visible as under Adam.
    mkopt = lambda p: torch.optim.SGD(p, lr=LOOP_SGD[0], momentum=LOOP_SGD[1])
    # (tag, namespace, model, model seed, C-index entry point that is recorded)
    specs = (("partial", pm, "PartialModalityNet", 31, "calculate_cindex"),
             ("simple", sf, "SimpleFusionModel", 32, "ConcordanceIndex"),
             ("flexible", fx, "FlexibleMultimodalModel", 33, "ConcordanceIndex"))
    out["sgd_lr_momentum"] = np.array(LOOP_SGD, np.float64)
    for tag, ns, cls, seed, metric in specs:
        trb, vab = loop_batches(c, tr, tag), loop_batches(c, va, tag)
        torch.manual_seed(seed)                       # construction, then dropout ACTIVE: the loops draw from the same generator
        m = ns[cls](rna_dim=LOOP_RNA)
        opt = mkopt(m.parameters())
        rets = [ns["train_epoch"](m, trb, opt, cpu) for _ in range(2)]
        rec, orig = _Recorder(), ns[metric]
        ns[metric] = rec.function(orig) if metric == "calculate_cindex" else rec.metric_class(orig)
        try:
            val = ns["validate"](m, vab, cpu)
        finally:
            ns[metric] = orig
        assert len(rec.calls) == 1, (tag, len(rec.calls))
        m.eval()
        with torch.no_grad():
            b0 = trb[0]
            hz = (m(b0["image"], b0["rnaseq"], b0["clinical"], b0["mask"])[0] if tag == "partial" else
                  m(b0["image"], b0["rnaseq"]) if tag == "simple" else m(b0["image"], b0["rnaseq"], b0["mask"]))
        out[f"{tag}_model_seed"] = np.int64(seed)
        out[f"{tag}_train"] = np.array(rets, np.float64)                 # partial: (avg_cox, avg_entropy) per epoch
        out[f"{tag}_val"] = np.array(val, np.float64)                    # (avg_loss, c_index)
        out[f"{tag}_hazard_b0"] = hz.numpy()
        out[f"{tag}_cindex_h"], out[f"{tag}_cindex_e"], out[f"{tag}_cindex_t"] = (a.astype(np.float32) for a in rec.calls[0])
        for k, b in m.named_buffers():
            out[f"{tag}_buf/{k}"] = b.numpy().copy()
        assert np.all(np.array(rets, np.float64).reshape(2, -1)[:, 0] > 0), (tag, rets)
        if tag == "partial" and not have_lifelines:
            assert val[1] == 0.5                      # the bare `except` of calculate_cindex (:318-319)
        print("g9", tag, rets, val, len(rec.calls[0][0]), "samples in the C-index")
    np.savez_compressed(f"{OUT}/g9_loops.npz", **out)
    print("g9_loops done:", len(out), "arrays")


# ----------------------------------------------------------------------------------------------
# g10: C-index on tied risk scores and tied times
# ----------------------------------------------------------------------------------------------

def tied_case(rng, n, pattern):
    """hazards from 3 to 7 distinct float32 values, times from ceil(n / 3) distinct values (every value used), events by `pattern`
    ("mixed" | "all" | "none" | "maxtime").  A mixed case with n >= 4 is given one permissible pair of equal scores by construction."""
    kh, kt = int(rng.integers(3, 8)), -(-n // 3)
    hv = np.unique(rng.normal(0, 1, 16).astype(np.float32))[:kh]
    tv = (np.sort(rng.exponential(1000.0, kt)) + 1.0 + np.arange(kt)).astype(np.float32)
    h = hv[rng.integers(len(hv), size=n)]
    t = tv[rng.permutation(np.concatenate([np.arange(kt), rng.integers(kt, size=n - kt)]))]
    if pattern == "all":
        e = np.ones(n, np.float32)
    elif pattern == "none":
        e = np.zeros(n, np.float32)
    elif pattern == "maxtime":
        e = np.zeros(n, np.float32)
        e[np.argmax(t)] = 1
    else:
        e = (rng.random(n) < 0.57).astype(np.float32)
        if n >= 4:
            i, j = int(np.argmin(t)), int(np.argmax(t))
            e[i] = 1
            h[j] = h[i]
    return h.astype(np.float32), e, t


def gen_cindex_ties(rn, sf, fx):
    out = {}
    rng = np.random.default_rng(9876)
    for n in (4, 23, 116):
        h, e, t = tied_case(rng, n, "mixed")
        args = (torch.tensor(h), torch.tensor(e), torch.tensor(t))
        cs = [ns["ConcordanceIndex"]()(*args).item() for ns in (rn, sf, fx)]     # train_rnaseq_only.py:55, simple_fusion.py:59, flexible_multimodal.py:54
        assert cs[0] == cs[1] == cs[2], (n, cs)
        perm = (t[None, :] > t[:, None]) & (e[:, None] == 1)
        assert (perm & (h[:, None] == h[None, :])).sum() > 0 and len(np.unique(t)) < n
        out[f"n{n}_h"], out[f"n{n}_e"], out[f"n{n}_t"] = h, e, t
        out[f"n{n}_cindex"] = np.float64(cs[0])
    np.savez_compressed(f"{OUT}/g10_cindex_ties.npz", **out)
    print("g10_cindex_ties done")


if __name__ == "__main__":
    torch.set_num_threads(8)
    fm, rn, pm, sf = harvest()
    fx = harvest_flexible()
    for name, ns, keys in (("final_multimodal", fm, ["MultiModalSurvivalNet", "cox_loss", "calculate_cindex", "train_epoch", "validate"]),
                           ("train_rnaseq_only", rn, ["neg_partial_log_likelihood", "ConcordanceIndex", "RNASeqSurvivalModel", "train_epoch", "validate"]),
                           ("partial_modality_training", pm, ["PartialModalityNet", "cox_loss", "gate_entropy_loss"]),
                           ("simple_fusion", sf, ["SimpleFusionModel", "neg_partial_log_likelihood", "ConcordanceIndex"])):
        missing = [k for k in keys if k not in ns]
        assert not missing, (name, missing)
    for name, ns in (("partial_modality_training", pm), ("simple_fusion", sf), ("flexible_multimodal", fx)):
        assert "train_epoch" in ns and "validate" in ns, name
    if "--all" in sys.argv[1:]:
        gen_cox(fm, rn, sf)
        gen_cindex(rn, sf)
        gen_models(fm, pm, sf)
        gen_extra_models(rn)
        gen_epoch(fm)
    gen_loops(pm, sf, fx)
    gen_cindex_ties(rn, sf, fx)
