"""The K fold models of a cross-validation run as ONE predictor (the reference's analyze_all_results.py:396-400 lists "Ensemble methods
(combining the fold models)" as a next step): one risk score from all of them, how much they disagree, and one saliency map that does
not depend on which fold's model was picked.

A FoldEnsemble owns a FoldGroupEngine: every launch of the eval forward and of the input-gradient backward is issued once for all K
members (FoldGroupEngine.forward_eval_shared / attribute_lockstep), on one copy of the batch's CT volumes; the members' results are
combined by mms_ensemble_reduce (csrc/ensemble.hip: mean and population standard deviation over the members, straight from their
gradient buffers).

A `batch` is a dict with any of the keys ct (or image) [B, 1, D, H, W], rna (or rnaseq) [B, rna_dim], clinical [B, clinical_dim],
mask [B, 3], as in `attribution`.

On the cohort the members were trained on, an ensemble's score is optimistic: each patient was seen in training by K - 1 members.
Out-of-fold evaluation is training.validate_lockstep; this module is for new patients and external cohorts.
"""
import ctypes

import numpy as np
import torch

from . import _lib, ops
from .attribution import _get

MAX_MODELS = 10         # MMS_MAX_GROUP


def midranks(v):
    """1-based ranks of a 1-D array, ties sharing the mean of the ranks they span (scipy.stats.rankdata's 'average')."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    order = np.argsort(v, kind="stable")
    r = np.empty(len(v), dtype=np.float64)
    s = v[order]
    i = 0
    while i < len(s):
        j = i
        while j + 1 < len(s) and s[j + 1] == s[i]:
            j += 1
        r[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    return r


def combine_rank(hazards):
    """hazards [K, N] -> [N]: the mean over members of each member's midranks over the N predicted patients, divided by N (in (0, 1],
    larger = higher risk).  A Cox log-hazard is defined only up to a per-model shift, so ranks are the scale-free way to combine folds."""
    h = np.asarray(hazards, dtype=np.float64)
    if h.ndim != 2 or h.shape[1] == 0:
        raise ValueError("combine_rank: hazards must be [K, N] with N > 0")
    return np.stack([midranks(row) for row in h]).mean(0) / h.shape[1]


def check_models(models):
    """The constructor's refusals that need no GPU."""
    models = list(models)
    if not 1 <= len(models) <= MAX_MODELS:
        raise ValueError("FoldEnsemble takes 1..%d models (the fold-group launches carry at most %d members by value), got %d"
                         % (MAX_MODELS, MAX_MODELS, len(models)))
    kinds = sorted({type(m).__name__ for m in models})
    if len(kinds) != 1:
        raise ValueError("FoldEnsemble: the members must be of one class (they run as one launch sequence), got %s" % kinds)
    for g, m in enumerate(models):
        if m.training:
            raise RuntimeError("FoldEnsemble: model %d is in train mode -- an ensemble predicts with frozen BatchNorm statistics and no "
                               "dropout; call model.eval() on every member first" % g)
    return models


def ensemble_reduce(xs, mean, spread=None):
    """mms_ensemble_reduce: xs = K contiguous float32 device tensors of one size -> mean (and spread) written, tensors of that size."""
    S = _lib.structs()
    p = S["EnsP"]()
    n = xs[0].numel()
    for g, x in enumerate(xs):
        if x.numel() != n or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("ensemble_reduce: members must be contiguous float32 tensors of one size")
        p.x[g] = x.data_ptr()
    for t in (mean, spread):
        if t is not None and (t.numel() != n or t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("ensemble_reduce: outputs must be contiguous float32 tensors of the members' size")
    p.K, p.n, p.mean, p.spread = len(xs), n, mean.data_ptr(), (spread.data_ptr() if spread is not None else None)
    _lib.check(_lib.load_library().mms_ensemble_reduce(ctypes.byref(p), ops.stream()), "mms_ensemble_reduce")


def _class_batch(kind, batch):
    """load_batch's keywords for a model class (as attribution.attribute / evaluate_model.predict hand them to one model)."""
    ct, rna, clin, mask = _get(batch, "ct"), _get(batch, "rna"), _get(batch, "clinical"), _get(batch, "mask")
    if kind == "RNASeqSurvivalModel":
        return dict(rna=rna)
    if kind == "ImageOnlyModel":
        return dict(ct=ct)
    if kind == "SimpleFusionModel":
        return dict(ct=ct, rna=rna)
    if kind == "FlexibleMultimodalModel":
        return dict(ct=ct, rna=rna, mask=None if mask is None else mask[:, :2])
    if kind == "MultiModalSurvivalNet":
        return dict(ct=ct, rna=rna, clinical=clin)
    return dict(ct=ct, rna=rna, clinical=clin, mask=mask)            # PartialModalityNet, SimMLM_SurvivalNet


class FoldEnsemble:
    def __init__(self, models, **group_kw):
        """models: 1..10 eval-mode modules of one class and shape, on the GPU and not yet bound to an engine."""
        from .fold_group import FoldGroupEngine
        self.models = check_models(models)
        self.kind = type(self.models[0]).__name__
        self.group = FoldGroupEngine(self.models, **group_kw)
        self.device = self.group.device

    @classmethod
    def from_checkpoints(cls, paths, make_model, device="cuda"):
        """paths: state_dicts written by a training entry point (models/<name>/fold_k_best.pth); make_model() -> a fresh module."""
        paths = list(paths)
        if not 1 <= len(paths) <= MAX_MODELS:
            raise ValueError("FoldEnsemble takes 1..%d models (the fold-group launches carry at most %d members by value), got %d"
                             % (MAX_MODELS, MAX_MODELS, len(paths)))
        ms = []
        for p in paths:
            m = make_model()
            m.load_state_dict(torch.load(p, map_location="cpu"))
            ms.append(m.to(device).eval())
        return cls(ms)

    def __len__(self):
        return len(self.models)

    # ---- helpers --------------------------------------------------------------------------------------------
    def _chunks(self, batch):
        kb = _class_batch(self.kind, batch)
        ref = kb["rna"] if kb.get("rna") is not None else kb["ct"]
        B = ref.shape[0]
        for b0 in range(0, B, 32):
            b1 = min(B, b0 + 32)
            yield b0, b1, {k: (None if v is None else v[b0:b1]) for k, v in kb.items()}

    def _rows(self, batch):
        kb = _class_batch(self.kind, batch)
        return (kb["rna"] if kb.get("rna") is not None else kb["ct"]).shape[0]

    def _check_train(self):
        for g, m in enumerate(self.models):
            if m.training:
                raise RuntimeError("FoldEnsemble: model %d is in train mode -- an ensemble predicts with frozen BatchNorm statistics and "
                                   "no dropout; call model.eval() on every member first" % g)

    def _reduce_hazards(self, hazards):
        """hazards [K, B] -> (mean [B], std [B]) by mms_ensemble_reduce (rows re-pitched to 16 bytes: a copy of K x B floats)."""
        K, B = hazards.shape
        pitch = B + (-B) % 4
        buf = torch.zeros(K + 2, pitch, device=hazards.device)
        buf[:K, :B] = hazards
        ensemble_reduce([buf[g] for g in range(K)], buf[K], buf[K + 1])
        return buf[K, :B].clone(), buf[K + 1, :B].clone()

    # ---- public ---------------------------------------------------------------------------------------------
    def predict(self, batch, combine="mean"):
        """-> dict(hazard [B], hazard_std [B], hazards [K, B], gate [K, B, 3] | None).  hazard: the members' mean log-hazard
        (combine = "mean") or their mean midrank over the batch divided by B ("rank"); hazard_std: the population standard deviation of
        the members' log-hazards.  Any B: chunks of <= 32 rows, a ragged tail on its own plan.  Ends with the members' check_b4()."""
        if combine not in ("mean", "rank"):
            raise ValueError("predict: combine is 'mean' or 'rank', got %r" % (combine,))
        self._check_train()
        K, B = len(self), self._rows(batch)
        hazards = torch.empty(K, B, device=self.device)
        gates = None
        for b0, b1, kb in self._chunks(batch):
            res = self.group.forward_eval_shared(kb)
            for g, (hz, gate) in enumerate(res):
                hazards[g, b0:b1] = hz
                if gate is not None:
                    if gates is None:
                        gates = torch.empty(K, B, gate.shape[1], device=self.device)
                    gates[g, b0:b1] = gate
        for e in self.group.engines:
            e.check_b4()
        mean, std = self._reduce_hazards(hazards)
        if combine == "rank":
            mean = torch.as_tensor(combine_rank(hazards.cpu().numpy()), dtype=torch.float32, device=self.device)
        return dict(hazard=mean, hazard_std=std, hazards=hazards, gate=gates)

    def predict_cohort(self, cohort, indices, batch_size=32, combine="mean"):
        """predict over the patients `indices` of a cohort dict (data.make_cohort / cohort_io: image, rnaseq, clinical, mask) in batches
        of batch_size -> predict's dict over all of them; "rank": the midranks are taken over the whole predicted set (host arithmetic
        on N x K numbers)."""
        if combine not in ("mean", "rank"):
            raise ValueError("predict_cohort: combine is 'mean' or 'rank', got %r" % (combine,))
        if "rnaseq_folds" in cohort:
            raise NotImplementedError("predict_cohort: ensembles of selected-gene models are not supported -- the members share ONE batch, "
                                      "and per-fold gene selection (gene_select.GeneSelection.apply) gives every member its own columns")
        idx =torch.as_tensor(np.asarray(indices), dtype=torch.int64)
        parts = []
        for s in range(0, len(idx), max(1, int(batch_size))):
            j = idx[s:s + batch_size].to(cohort["image"].device)
            b = {k: cohort[k][j] for k in ("image", "rnaseq", "clinical", "mask") if cohort.get(k) is not None}
            parts.append(self.predict(b, combine="mean"))
        out = {k: torch.cat([p[k] for p in parts], 0 if k in ("hazard", "hazard_std") else 1) if parts[0][k] is not None else None
               for k in ("hazard", "hazard_std", "hazards", "gate")}
        if combine == "rank":
            out["hazard"] = torch.as_tensor(combine_rank(out["hazards"].cpu().numpy()), dtype=torch.float32, device=self.device)
        return out

    def attribute(self, batch, wrt=("ct", "rna", "clinical"), members_out=False):
        """Input-gradient attribution of the ensemble: -> dict(hazard, hazard_std [B], ct, ct_std [B, 1, D, H, W], rna, rna_std
        [B, rna_dim], clinical, clinical_std [B, clinical_dim]): the mean over members of d hazard_g[b] / d input[b] and its population
        standard deviation (None for an input the class does not have or that is not in wrt).  members_out: also `members`, the
        per-member dicts of SurvivalEngine.attribute.  The members run in lock-step (FoldGroupEngine.attribute_lockstep) and
        mms_ensemble_reduce reads their gradient buffers in place.  Any B in chunks of <= 32.  The dict is accepted by
        attribution.gene_scores / modality_shares like a single model's."""
        G = self.group
        G._check_attribute(wrt)
        K, B = len(self), self._rows(batch)
        out = dict(hazard=None, hazard_std=None)
        hazards = torch.empty(K, B, device=self.device)
        keys = (("ct", "dct"), ("rna", "drna"), ("clinical", "dclin"))
        mem = [dict(hazard=[], gate=[], ct=[], rna=[], clinical=[]) for _ in range(K)] if members_out else None
        for b0, b1, kb in self._chunks(batch):
            GP, AG = G._attribute_lockstep_run(kb)
            for g, P in enumerate(GP.Ps):
                hazards[g, b0:b1] = P.buf["hz"][:, 0]
            for k, ak in keys:
                bufs = [A.get(ak) for A in AG["members"]]
                if bufs[0] is None or k not in wrt:
                    out.setdefault(k, None); out.setdefault(k + "_std", None)
                    continue
                if out.get(k) is None:
                    shape = (B,) + tuple(bufs[0].shape[1:])
                    out[k], out[k + "_std"] = torch.empty(shape, device=self.device), torch.empty(shape, device=self.device)
                ensemble_reduce(bufs, out[k][b0:b1], out[k + "_std"][b0:b1])
            if members_out:
                for g, (P, A) in enumerate(zip(GP.Ps, AG["members"])):
                    mem[g]["hazard"].append(P.buf["hz"][:, 0].clone())
                    mem[g]["gate"].append(P.gatew.clone() if P.gate is not None else None)
                    for k, ak in keys:
                        mem[g][k].append(A[ak].clone() if (A.get(ak) is not None and k in wrt) else None)
        out["hazard"], out["hazard_std"] = self._reduce_hazards(hazards)
        if members_out:
            cat = lambda v: None if v[0] is None else (v[0] if len(v) == 1 else torch.cat(v, 0))
            out["members"] = [{k: cat(v) for k, v in m.items()} for m in mem]
        return out
