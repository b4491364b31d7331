"""Host-side execution engine for the three survival networks.

One `SurvivalEngine` per model instance.  It
  * re-points every parameter (and creates every gradient) as a view into ONE flat fp32 buffer, so the
    gradient zeroing, the global-norm reduction and the Adam update are single launches over 14-17 M floats;
  * keeps, per batch size, a *plan*: static input buffers, the DenseNet workspace, the head activation buffers
    and the prebuilt C-ABI parameter blocks (ctypes structs holding raw device pointers) for every launch;
  * runs a plan either eagerly (autograd-compatible path used by the nn.Module's forward/backward) or as a
    captured HIP graph of the WHOLE training step (zero-grad -> forward -> Cox -> backward -> clip -> Adam),
    which is what `training.train_epoch_*` (one loop, `training._train_epoch`, over the per-style table there) and bench.py
    replay once per batch.

The state roll-back around graph capture exists once, for this engine and for fold_group.FoldGroupEngine:
`SurvivalEngine.snapshot` / `restore`, used by `capture`.

PyTorch supplies device memory, streams and graph capture only; every numeric op is a kernel behind
include/mmsurv.h.  Nothing here falls back to torch math.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib, ops

_S = _lib.structs


def check_train_batch(B, bn_world=1):
    """A training-mode forward on ONE patient: torch's BatchNorm1d (every head of the reference's models has one) raises
    `ValueError: Expected more than 1 value per channel when training` -- e.g. a DataLoader tail of 1 in the reference's loops.
    Same error here, instead of the kernels' bare MMS_ERR_ARG."""
    if B * max(int(bn_world), 1) <= 1:
        raise ValueError("Expected more than 1 value per channel when training: a batch of 1 patient cannot be normalised by the "
                         "heads' BatchNorm1d layers (torch raises the same in the reference's train_epoch; choose a batch size / "
                         "fold split without a tail of 1)")

class _Lin:
    """One nn.Linear application with the neighbouring BN1d/ReLU/Dropout folded in (see InProlog in mmsurv.h)."""

    def __init__(self, lin, src, dst, out_relu, pro_bn=None, pro_drop=None, need_dx=True):
        self.lin, self.src, self.dst, self.out_relu = lin, src, dst, out_relu
        self.pro_bn, self.pro_drop, self.need_dx = pro_bn, pro_drop, need_dx


def head_program(model):
    """-> dict(kind, width, ct_cols, lins=[...], gate=(l1, l2) | None, bufs={name: width}, encoder).
    Buffer/column wiring restates the reference forward()s: final_multimodal.py:122-150,
    partial_modality_training.py:234-277, simple_fusion.py:217-236."""
    kind = type(model).__name__
    if kind in ("MultiModalSurvivalNet", "PartialModalityNet"):
        r, c, f = model.rna_encoder, model.clinical_encoder, model.fusion
        rna_dim = r[0].in_features
        lins = [
            _Lin(r[0], ("rna", 0), ("r1", 0), False, need_dx=False),
            _Lin(r[4], ("r1", 0), ("feats", 128), True, pro_bn=r[1], pro_drop=r[3]),
            _Lin(c[0], ("clin", 0), ("feats", 256), True, need_dx=False),
            _Lin(f[0], ("fused" if kind == "PartialModalityNet" else "feats", 0), ("f1", 0), False),
            _Lin(f[4], ("f1", 0), ("f2", 0), True, pro_bn=f[1], pro_drop=f[3]),
            _Lin(model.cox_head, ("f2", 0), ("hz", 0), False),
        ]
        bufs = dict(rna=rna_dim, clin=c[0].in_features, r1=512, feats=288, f1=256, f2=128, hz=1)
        gate = None
        if kind == "PartialModalityNet":
            bufs["fused"] = 288
            gate = (model.gate[0], model.gate[2])
        return dict(kind=kind, width=288, ct_cols=0, lins=lins, gate=gate, bufs=bufs, encoder=model.ct_encoder,
                    n_pre=3)
    if kind == "SimpleFusionModel":
        r, f = model.rna_encoder, model.fusion
        lins = [
            _Lin(r[0], ("rna", 0), ("r1", 0), False, need_dx=False),
            _Lin(r[4], ("r1", 0), ("r2", 0), False, pro_bn=r[1], pro_drop=r[3]),
            _Lin(r[8], ("r2", 0), ("feats", 0), True, pro_bn=r[5], pro_drop=r[7]),
            _Lin(f[0], ("feats", 0), ("f1", 0), False),
            _Lin(f[4], ("f1", 0), ("f2", 0), True, pro_bn=f[1], pro_drop=f[3]),
            _Lin(f[7], ("f2", 0), ("hz", 0), False, pro_drop=f[6]),
        ]
        rd = r[8].out_features                      # rna_feature_dim (simple_fusion.py:163); the encoder's img_feature_dim columns follow
        idim = f[0].in_features - rd
        bufs = dict(rna=r[0].in_features, r1=1024, r2=512, feats=rd + idim, f1=256, f2=128, hz=1)
        return dict(kind=kind, width=rd + idim, ct_cols=rd, lins=lins, gate=None, bufs=bufs, encoder=model.image_encoder,
                    n_pre=3, enc_width=idim)
    if kind == "FlexibleMultimodalModel":      # flexible_multimodal.py:157-256: simple-fusion heads, [image | rna] order, missing bias
        r, f = model.rna_encoder, model.fusion
        lins = [
            _Lin(r[0], ("rna", 0), ("r1", 0), False, need_dx=False),
            _Lin(r[4], ("r1", 0), ("r2", 0), False, pro_bn=r[1], pro_drop=r[3]),
            _Lin(r[8], ("r2", 0), ("feats", model.missing_image_bias.numel()), True, pro_bn=r[5], pro_drop=r[7]),
            _Lin(f[0], ("feats", 0), ("f1", 0), False),
            _Lin(f[4], ("f1", 0), ("f2", 0), True, pro_bn=f[1], pro_drop=f[3]),
            _Lin(f[7], ("f2", 0), ("hz", 0), False, pro_drop=f[6]),
        ]
        rd, idim = r[8].out_features, model.missing_image_bias.numel()
        bufs = dict(rna=r[0].in_features, r1=1024, r2=512, feats=idim + rd, f1=256, f2=128, hz=1)
        return dict(kind=kind, width=idim + rd, ct_cols=0, lins=lins, gate=None, bufs=bufs, encoder=model.image_encoder, n_pre=3,
                    mix=dict(biases=[model.missing_image_bias, model.missing_rna_bias], segs=[(0, idim), (idim, rd)]), enc_width=idim)
    if kind == "RNASeqSurvivalModel":          # train_rnaseq_only.py:126-151: [Linear, BN1d, ReLU, Dropout] x n + Linear(., 1)
        mods = list(model.mlp)
        lin_idx = [i for i, m in enumerate(mods) if isinstance(m, nn.Linear)]
        lins, bufs = [], dict(rna=mods[0].in_features)
        for n, i in enumerate(lin_idx):
            src = ("rna", 0) if n == 0 else ("h%d" % n, 0)
            last = n == len(lin_idx) - 1
            dst = ("hz", 0) if last else ("h%d" % (n + 1), 0)
            if not last:
                bufs["h%d" % (n + 1)] = mods[i].out_features
            pro_bn = mods[lin_idx[n - 1] + 1] if n > 0 else None
            pro_drop = mods[lin_idx[n - 1] + 3] if n > 0 else None
            lins.append(_Lin(mods[i], src, dst, False, pro_bn=pro_bn, pro_drop=pro_drop, need_dx=n > 0))
        bufs["hz"] = 1
        return dict(kind=kind, width=0, ct_cols=0, lins=lins, gate=None, bufs=bufs, encoder=None, n_pre=0)
    if kind == "SimMLM_SurvivalNet":           # generate_km_curves.py:158-281: experts -> masked gate MLP -> mixture (MoeP, include/mmsurv.h)
        F = model.feature_dim
        r, c, g = model.expert_rnaseq.encoder, model.expert_clinical.encoder, model.gating.gate
        lins = [
            _Lin(r[0], ("rna", 0), ("r1", 0), False, need_dx=False),
            _Lin(r[4], ("r1", 0), ("feats", F), True, pro_bn=r[1], pro_drop=r[3]),
            _Lin(c[0], ("clin", 0), ("c1", 0), True, need_dx=False),
            _Lin(c[2], ("c1", 0), ("feats", 2 * F), True),
            _Lin(g[0], ("gin", 0), ("g1", 0), True),                   # (the first stage of mms_moe_fwd fills gin)
            _Lin(g[3], ("g1", 0), ("g2", 0), True, pro_drop=g[2]),     # g2 feeds the second stage (gate output layer, softmax, mixture)
        ]
        bufs = dict(rna=r[0].in_features, clin=c[0].in_features, r1=512, c1=64, feats=3 * F, gin=3 * F + 3, g1=128, g2=64, hz=4)
        experts = [model.expert_image.cox_head, model.expert_rnaseq.cox_head, model.expert_clinical.cox_head]
        return dict(kind=kind, width=3 * F, ct_cols=0, lins=lins, gate=None, bufs=bufs, encoder=model.expert_image.encoder, n_pre=4,
                    enc_width=F, moe=dict(F=F, out=g[5], experts=experts, ensemble=model.ensemble_cox))
    if kind == "ImageOnlyModel":               # generate_km_curves.py:28-54: 3-conv encoder (16, 32, 64) -> Linear(64, 32)+ReLU -> Linear(32, 1)
        w = model.fc[0].in_features
        lins = [
            _Lin(model.fc[0], ("feats", 0), ("f1", 0), True),
            _Lin(model.risk_head, ("f1", 0), ("hz", 0), False),
        ]
        bufs = dict(feats=w, f1=model.fc[0].out_features, hz=1)
        return dict(kind=kind, width=w, ct_cols=0, lins=lins, gate=None, bufs=bufs, encoder=model.encoder, n_pre=0, enc_width=w)
    raise TypeError("unsupported model %s" % kind)


def capture(engines, body):
    """-> HIP graph of body().  Warm-up on one fresh side stream (first-launch attribute calls, lazy module loads), roll the engines
    back, capture, roll back again (capture does not execute, but keep state exact regardless)."""
    snaps = [e.snapshot() for e in engines]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for e, snap in zip(engines, snaps):
        e.restore(snap)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    for e, snap in zip(engines, snaps):
        e.restore(snap)
    return g


def gate_out(P):
    """The gate weights [B, 3] a forward leaves on plan P, or None for a model without a gate."""
    return P.gatew if (P.gate is not None or P.moe is not None) else None


def check_attribute(engines, wrt):
    """The argument checks of SurvivalEngine.attribute / FoldGroupEngine.attribute_lockstep."""
    if engines[0].prog["kind"] == "SimMLM_SurvivalNet":
        raise RuntimeError("attribute: SimMLM_SurvivalNet is not supported -- its mixture-of-experts kernels (csrc/moe.hip) have no "
                           "input-gradient form; supported: the five imaging classes and RNASeqSurvivalModel")
    if any(e.model.training for e in engines):
        raise RuntimeError("attribute needs the model in eval mode (call model.eval()): input gradients are taken with frozen "
                           "BatchNorm statistics; train-mode (batch-statistic) input gradients are not computed")
    bad = [w for w in wrt if w not in ("ct", "rna", "clinical")]
    if bad:
        raise ValueError("attribute: wrt takes 'ct', 'rna', 'clinical'; got %r" % (bad,))


def fallback_widths(enc):
    """The three channel widths of a 3 x [Conv3d(k3, s2, p1) + BatchNorm3d + ReLU] + pool nn.Sequential, read from its Conv3d modules
    (what the mms_fb3_* drivers take); raises for what no driver computes.  What only ONE path cannot run is refused where that path is
    chosen, with the reason: scalar_widths_ok (SurvivalEngine's own launches), group_widths_ok (FoldGroupEngine.plan)."""
    convs = [m for m in enc if isinstance(m, nn.Conv3d)]
    bns = [m for m in enc if isinstance(m, nn.BatchNorm3d)]
    cin = 1
    if len(convs) != 3 or len(bns) != 3:
        raise TypeError("the 3-conv CT encoder has three Conv3d and three BatchNorm3d modules")
    for c, b in zip(convs, bns):
        if (c.in_channels != cin or c.kernel_size != (3, 3, 3) or c.stride != (2, 2, 2) or c.padding != (1, 1, 1) or c.bias is None
                or b.num_features != c.out_channels):
            raise TypeError("the 3-conv CT encoder is a chain of Conv3d(k=3, s=2, p=1, bias) + BatchNorm3d starting at 1 channel")
        if c.out_channels % 16 != 0 or not 16 <= c.out_channels <= 128:
            raise ValueError("3-conv CT encoder: channel widths must be multiples of 16 in 16..128, got %d" % c.out_channels)
        cin = c.out_channels
    return tuple(c.out_channels for c in convs)


def scalar_widths_ok(widths):
    """the single-model scalar kernels (csrc/fallback.hip): a thread per (voxel, channel) of a 256-thread workgroup"""
    return all(256 % w == 0 for w in widths)


def group_widths_ok(widths):
    """the fold-group kernels (csrc/fb_group.hip, fbg_conv_ok): every multiple of 16 except 48 + 64 n"""
    return all(w % 64 != 48 for w in widths)


def _weights_token(params, flat):
    """What torch knows about the last change of `params` (parameters whose .data are views of `flat`) and of `flat` itself: their
    version counters.  `p.data = view` gives the parameter a counter of its own, so an in-place change of p (p.mul_(), p.copy_(),
    load_state_dict, a torch optimiser's step) bumps p._version and NOT flat._version; a write to flat (restore) bumps flat's only.
    A write through p.data bumps neither.  Pure host code."""
    return tuple(p._version for p in params) + (flat._version,)


class _Plan:
    """Everything that depends on the batch size B (and the volume dims)."""
    pass


class SurvivalEngine:
    def __init__(self, model, adamw=None, lr=1e-4, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0,
                 gate_entropy_weight=0.01, cox_ties=None, dn_opts=None, expert_weight=0.1, finetune=None, _slots=None):
        """expert_weight: lambda of SimMLM_SurvivalNet's training objective (project-defined)
        L = cox(ensemble; has_survival) + lambda * sum_m cox(h_m; has_survival and mask_m); ignored by the other models.
        dn_opts: launch-shape options of the encoder drivers (dict of MmsDnOpts fields, include/mmsurv.h; None = defaults).
        finetune: None, a transfer.FineTunePlan or its string -- per-segment learning rates, frozen segments, L2-SP (the tuned optimiser
        launches, csrc/finetune.hip), a backward that stops above the frozen DenseNet121 stages, the encoder in eval mode.  Fixed for
        the engine's life.  None: the engine takes the launches it took before fine-tuning existed.
        _slots (used by FoldGroupEngine): dict(gflat=[n] fp32, sumsq=[1] fp64, entropy=[1] fp32) views of group-wide
        buffers, so the per-step zeroing of a whole fold group is three memsets; tune_tab = the group's one segment table."""
        self.lib = _lib.load_library()
        self.model = model
        self.prog = head_program(model)
        # MmsDnOpts of every encoder driver call of this engine (the width of class_layers.out rides in it)
        from .densenet import DenseNet121
        self.packed = isinstance(self.prog["encoder"], DenseNet121)      # conv2 weights in packed primary storage (MmsDnOpts.w2_packed)
        self.dn_opts = ops.dn_opts(dict(dn_opts or {}), out_features=self.prog.get("enc_width", 128), w2_packed=1 if self.packed else 0)
        p0 = next(model.parameters())
        if not p0.is_cuda:
            raise RuntimeError("SurvivalEngine: move the model to the GPU first (model.to('cuda')); no CPU fallback")
        self.device = p0.device
        self.params = list(model.parameters())
        # (torch's "more than 1 value per channel" error of a training batch of ONE patient comes from BatchNorm1d; a model without one,
        # like ImageOnlyModel, normalises over the voxels of that patient)
        self.has_bn1d = any(isinstance(m, nn.BatchNorm1d) for m in model.modules())
        self._slots = _slots or {}
        self._flatten()
        n = self.flat.numel()
        self.m = torch.zeros(n, device=self.device)
        self.v = torch.zeros(n, device=self.device)
        self.adamw = bool(adamw) if adamw is not None else self.prog["kind"] in ("SimpleFusionModel", "FlexibleMultimodalModel",
                                                                                 "RNASeqSurvivalModel")
        self.hyper = torch.tensor([lr, betas[0], betas[1], eps, weight_decay, max_norm], device=self.device)
        self.sumsq = self._slots["sumsq"] if "sumsq" in self._slots else torch.zeros(1, dtype=torch.float64, device=self.device)
        self.entropy = self._slots["entropy"] if "entropy" in self._slots else torch.zeros(1, device=self.device)
        self.step_count = torch.zeros(1, device=self.device)
        self.rng = torch.tensor([0x5EED, 0], dtype=torch.int32, device=self.device)
        self.ent_weight = gate_entropy_weight
        self.expert_weight = float(expert_weight)
        from . import losses
        self.tie_mode = ops.TIE_MODES[cox_ties or losses.default_ties()]    # CoxP.tie_mode of the fused step's loss
        self.sync_collectives = 0    # all-reduces issued by the SyncBN hook (distributed.DataParallel; bench.py --mode ddp --sync-bn reports them)
        self._dp = None              # distributed.DataParallel, created by the first data-parallel train_step
        self.plans = {}
        self.dropout_masks = {}      # parity mode: {lin index: [B, K] multiplicative mask}
        # device-side epoch accumulators: [sum loss*usable, n usable, sum entropy, n batches]
        self.acc = torch.zeros(4, device=self.device)
        self.acc_eval = torch.zeros(4, device=self.device)      # validation: [sum of batch losses, usable batches, -, batches]
        self._set_finetune(finetune)
        model._mms_engine = self

    # ---- parameters ------------------------------------------------------------------------------
    def _flatten(self):
        n = sum(p.numel() for p in self.params)
        pad = (-n) % 4
        self.flat = torch.zeros(n + pad, device=self.device)
        self.gflat = self._slots["gflat"] if "gflat" in self._slots else torch.zeros(n + pad, device=self.device)
        assert self.gflat.numel() == n + pad and self.gflat.is_contiguous()
        o = 0
        self.gviews = []
        # DenseNet121's 58 conv2 weights (_DenseLayer.layers.conv2, [32, 128, 3, 3, 3]) are stored [cout][tap][cin] -- the layout the
        # forward kernels read and the weight-gradient kernels flush -- as strided VIEWS with the torch shape: state_dict(),
        # load_state_dict(), .grad and torch optimisers see ordinary tensors (MmsDnOpts.w2_packed; csrc/heads.hip w2_adam_pack_kernel)
        w2ids = set()
        if self.packed:
            w2ids = {id(p) for k, p in self.prog["encoder"].named_parameters() if k.endswith("layers.conv2.weight")}
            assert len(w2ids) == 58
        self.w2_offsets = []
        self._w2_params = []              # the conv2 parameters, in the order of w2_offsets (sync_packs watches their version counters)

        def view(buf, o, p):
            if id(p) in w2ids:
                return buf.as_strided((32, 128, 3, 3, 3), (27 * 128, 1, 9 * 128, 3 * 128, 128), buf.storage_offset() + o)      # (the offset is absolute in the storage)
            return buf[o:o + p.numel()].view_as(p)
        with torch.no_grad():
            for p in self.params:
                if id(p) in w2ids:
                    assert tuple(p.shape) == (32, 128, 3, 3, 3) and o % 4 == 0
                    self.w2_offsets.append(o)
                    self._w2_params.append(p)
                v = view(self.flat, o, p)
                v.copy_(p.data)
                p.data = v
                self.gviews.append(view(self.gflat, o, p))
                o += p.numel()
        self._key = (self.params[0].data_ptr(), self.params[-1].data_ptr())
        self.w2 = None
        if self.w2_offsets:
            # the derived packs (backward-data pack; forward MFMA-fragment pack of the small-grid layers) and the device tables of AdamP.w2_*
            self.w2_packs = torch.zeros(len(self.w2_offsets), 2, 32 * 27 * 128, device=self.device)
            base, step = self.w2_packs.data_ptr(), 32 * 27 * 128 * 4
            self.w2 = dict(off=torch.tensor(self.w2_offsets, dtype=torch.int64, device=self.device),
                           pack_b=torch.tensor([base + 2 * i * step for i in range(len(self.w2_offsets))], dtype=torch.int64, device=self.device),
                           pack_f=torch.tensor([base + (2 * i + 1) * step for i in range(len(self.w2_offsets))], dtype=torch.int64, device=self.device),
                           fragmask=None)
            self._packs_version = None

    def _set_finetune(self, finetune):
        """The plan's consequences for the launches (transfer.FineTunePlan): the segment table of the tuned optimiser pair, the L2-SP
        anchor (a snapshot of the flat buffer, only where some trainable segment has l2sp > 0; constant, so not part of _state()),
        whether the encoder backward runs and from which dense block, whether the encoder forward runs in eval mode."""
        from . import transfer
        self.finetune = transfer.as_plan(finetune)
        self.tune_tab, self.anchor, self.enc_frozen, self.block_lo, self.enc_eval = None, None, False, 0, False
        if self.finetune is None:
            return
        plan = self.finetune
        seg = plan.resolve(self.model)
        assert int(seg.bounds[-1]) == self.flat.numel()
        self.segments = seg
        self.tune_tab = self._slots.get("tune_tab") or ops.tune_table(seg.bounds.tolist(), seg.lr_mult.tolist(), seg.wd_mult.tolist(),
                                                                      seg.l2sp.tolist(), self.device)
        if bool(((seg.l2sp > 0) & (seg.lr_mult > 0)).any()):
            self.anchor = self.flat.clone()          # (the weights at this moment; transfer.load_pretrained on a live engine calls reset_anchor)
        self.enc_frozen = plan.encoder_frozen(self.model)
        self.enc_eval = plan.encoder_eval
        if self.enc_eval and not self.enc_frozen:
            raise ValueError("encoder_eval: %s has no CT encoder to run in eval mode" % self.prog["kind"])
        if self.packed and not self.enc_frozen:
            self.block_lo = plan.freeze_stages

    def reset_anchor(self):
        """L2-SP pulls towards the weights as they are NOW (in place: the launches keep the anchor's address).  For weights loaded after the
        engine was built; no-op without an anchor."""
        if self.anchor is not None:
            self.anchor.copy_(self.flat)

    def _refuse_ddp(self):
        if self.finetune is not None:
            raise RuntimeError("fine-tuning plans are not implemented for the data-parallel steps (ddp_world > 1): their staged graphs "
                               "take the plain optimiser launches; fine-tune on one GPU or as a fold group")

    def _check_params(self):
        if (self.params[0].data_ptr(), self.params[-1].data_ptr()) != self._key:
            raise RuntimeError("model parameters were re-allocated (e.g. .to()/.load on another device) after the "
                               "engine was built; create a new SurvivalEngine")

    def sync_packs(self, force=False):
        """Packed primary conv2 storage: the derived packs are written by the fused optimiser step (mms_clip_adam); after ANY other
        change of the weights -- load_state_dict, a torch optimiser, an in-place edit of a parameter, the roll-back around graph
        capture -- they are rebuilt here (mms_w2_pack).  Detected through `_weights_token`: the version counters torch keeps for the 58
        conv2 parameters and for the flat buffer.  Host-side attribute reads only: no synchronisation, and no launch when nothing
        changed (so none inside a graph capture: every eager entry point calls this before it captures or replays).
        NOT detected: writes through `p.data` (`p.data.mul_()`, optimisers written in the old `.data` style) -- they bump no version
        counter at all.  After such a write call `sync_packs(force=True)`."""
        if self.w2 is None or self.w2["fragmask"] is None:
            return
        token = _weights_token(self._w2_params, self.flat)
        if force or self._packs_version != token:
            _lib.check(self.lib.mms_w2_pack(ctypes.byref(self._w2_adam), ops.stream()), "mms_w2_pack")
            self._packs_version = token

    def _state(self):
        """Every tensor a training or validation step changes: a state word added to the fused step is added here, nowhere else."""
        return [self.flat, self.m, self.v, self.step_count, self.rng, self.acc, self.acc_eval] + list(self.model.buffers())

    def snapshot(self):
        """Copy of the engine's state for the roll-back around graph capture (`capture`, `distributed.DataParallel.step`)."""
        return [t.clone() for t in self._state()]

    def restore(self, snap):
        with torch.no_grad():
            for t, t0 in zip(self._state(), snap):
                t.copy_(t0)
        self.sync_packs()          # (the roll-back changed the weights: rebuild the derived conv2 packs, outside any capture)

    def check_train_batch(self, B, dims=None, bn_world=1):
        """check_train_batch for THIS model: BatchNorm1d heads need more than one patient; a model without them (ImageOnlyModel) trains
        on one patient as long as its last BatchNorm3d sees more than one voxel (torch's rule for BatchNorm3d)."""
        if self.has_bn1d:
            check_train_batch(B, bn_world)
        elif dims is not None and isinstance(self.prog["encoder"], nn.Sequential):
            vox = 1
            for d in dims:
                vox *= (((int(d) + 1) // 2 + 1) // 2 + 1) // 2
            if B * vox <= 1:
                raise ValueError("Expected more than 1 value per channel when training: one patient whose volume shrinks to a single "
                                 "voxel cannot be normalised by the encoder's last BatchNorm3d")

    def set_lr(self, lr):
        self.hyper[0] = lr

    def get_lr(self):
        return float(self.hyper[0])

    def attach_grads(self):
        """Expose the flat gradient buffer as .grad views (what clip_grad_norm_/torch.optim would read)."""
        for p, g in zip(self.params, self.gviews):
            p.grad = g

    # ---- plans -----------------------------------------------------------------------------------
    def plan(self, B, dims, heads_only=False, bn_world=1):
        """heads_only: no encoder workspace (the replicated global-batch heads of the SyncBN data-parallel step: the encoder's
        128 feature columns are filled by an all-gather); bn_world: ranks the encoder's BatchNorm statistics span."""
        dims = tuple(dims) if dims is not None else ()
        key = (B,) + dims + (("heads",) if heads_only else ()) + ((("bnw", bn_world),) if bn_world > 1 else ())
        if key in self.plans:
            return self.plans[key]
        self._check_params()
        P = _Plan()
        P.B, P.dims = B, dims
        # which forward the plan's one workspace holds (stamped by every forward on it), and which of them a backward has consumed:
        # what the autograd path (models._Net) checks before it runs a backward
        P.fwd_serial = P.bwd_serial = 0
        dev = self.device
        prog = self.prog
        P.has_enc = prog["encoder"] is not None and not heads_only
        P.bn_world = bn_world
        D, H, W = dims if P.has_enc else (1, 1, 1)
        P.ct = torch.zeros(B, 1, D, H, W, device=dev)
        P.big = B > 32                 # rows beyond the one-lane-per-column head kernels: MFMA GEMM path (mms_linear_big_*)
        if P.big and prog.get("moe") is not None:
            raise RuntimeError("SimMLM_SurvivalNet: batches are limited to 32 rows (its mixture-of-experts kernels, csrc/moe.hip, hold one "
                               "model's rows in LDS arrays of 32); got %d -- train and evaluate it at a batch size of at most 32" % B)
        if P.big and heads_only:
            raise RuntimeError("the SyncBN data-parallel step replicates the heads on the GLOBAL batch with the small-batch head kernels, "
                               "limited to 32 rows; got %d global rows -- lower the per-rank batch or the number of ranks, or train "
                               "large batches on one GPU (SurvivalEngine.train_step)" % B)
        # row pitch padded to a multiple of 4 floats so that the 5005-wide RNA rows are 16-B aligned (float4 operand loads)
        P.buf = {k: torch.zeros(B, (w + 3) & ~3, device=dev)[:, :w] if P.big and w > 1 else torch.zeros(B, w, device=dev)
                 for k, w in prog["bufs"].items()}
        P.dbuf = {k: torch.zeros(B, w, device=dev) for k, w in prog["bufs"].items() if k not in ("rna", "clin")}
        P.mask = torch.ones(B, 3, device=dev)
        P.time = torch.zeros(B, device=dev)
        P.event = torch.zeros(B, device=dev)
        P.valid = torch.ones(B, device=dev)
        P.cox_out = torch.zeros(2, device=dev)
        P.lse = torch.zeros(B, device=dev)
        P.tie_frac = torch.zeros(B, device=dev)
        # encoder: DenseNet121-3D (MONAI topology) or the reference's 3-conv fallback
        enc = prog["encoder"]
        gmap = {id(p): g for p, g in zip(self.params, self.gviews)}
        P.fallback = isinstance(enc, nn.Sequential)
        if P.has_enc:
            eparams = list(enc.parameters())
            ebufs = list(enc.buffers())
            npar, nbuf = (12, 9) if P.fallback else (364, 363)
            assert len(eparams) == npar and len(ebufs) == nbuf
            if self.w2 is not None:
                mask = ctypes.c_uint64(0)
                _lib.check(self.lib.mms_dn121_w2_fragmask(B, D, H, W, ctypes.byref(self.dn_opts), ctypes.byref(mask)), "mms_dn121_w2_fragmask")
                if self.w2["fragmask"] is None:
                    self.w2["fragmask"] = mask.value
                    self._w2_adam = ops.adam_params(self.flat, self.gflat, self.m, self.v, self.hyper, self.sumsq, self.step_count, w2=self.w2)
                elif self.w2["fragmask"] != mask.value:
                    raise RuntimeError("this engine's conv2 packs were laid out for another volume size (fragment-order layers differ); "
                                       "use one volume size per model")
            nbytes = ctypes.c_size_t(0)
            if P.fallback:
                P.widths = (ctypes.c_int * 3)(*fallback_widths(enc))
                if P.widths[2] != prog.get("enc_width", 128):
                    raise ValueError("the CT encoder's last convolution has %d channels, the heads read %d" % (P.widths[2], prog.get("enc_width", 128)))
                _lib.check(self.lib.mms_fb3_workspace_bytes(P.widths, B, D, H, W, ctypes.byref(nbytes)), "workspace_bytes")
            else:
                _lib.check(self.lib.mms_dn121_workspace_bytes(B, D, H, W, ctypes.byref(nbytes)), "workspace_bytes")
            P.ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
            P.ws_bytes = nbytes.value
            ptrs = [p.data_ptr() for p in eparams]
            if self.w2 is not None:       # packed primary conv2 storage: + 116 pointers (layer l: backward-data pack, forward fragment pack)
                base, step = self.w2_packs.data_ptr(), 32 * 27 * 128 * 4
                ptrs += [base + j * step for j in range(2 * len(self.w2_offsets))]
            P.ptab = (ctypes.c_void_p * len(ptrs))(*ptrs)
            P.btab = (ctypes.c_void_p * nbuf)(*[b.data_ptr() for b in ebufs])
            P.gtab = (ctypes.c_void_p * npar)(*[gmap[id(p)].data_ptr() for p in eparams])
            if P.fallback:
                if bn_world > 1:
                    raise RuntimeError("SyncBN drives the DenseNet121-3D encoder only")
                _lib.check(self.lib.mms_fb3_init(P.ws.data_ptr(), P.ws_bytes, P.widths, B, D, H, W, P.btab, ops.stream()), "mms_fb3_init")
            else:
                _lib.check(self.lib.mms_dn121_init_sync(P.ws.data_ptr(), B, D, H, W, P.ptab, P.btab, bn_world, ctypes.byref(self.dn_opts),
                                                        ops.stream()), "mms_dn121_init_sync")
        # head launches (train / eval variants)
        P.lin_fwd = {True: [], False: []}
        P.lin_bwd = []
        if P.big:
            self._plan_big(P, gmap)
        for i, L in enumerate(() if P.big else prog["lins"]):
            xs, xo = L.src
            ys, yo = L.dst
            x = P.buf[xs][:, xo:]
            y = P.buf[ys][:, yo:]
            K, N = L.lin.in_features, L.lin.out_features
            for train in (True, False):
                pro = self._prolog(L, i, train)
                P.lin_fwd[train].append(_S()["LinearFwdP"](x.data_ptr(), x.stride(0), B, K, pro, L.lin.weight.data_ptr(),
                                                            L.lin.bias.data_ptr(), N, y.data_ptr(), y.stride(0),
                                                            1 if L.out_relu else 0))
            dy = P.dbuf[ys][:, yo:]
            dx = P.dbuf[xs][:, xo:] if L.need_dx else None
            pro = self._prolog(L, i, True)
            P.lin_bwd.append(_S()["LinearBwdP"](
                dy.data_ptr(), dy.stride(0), y.data_ptr(), y.stride(0), 1 if L.out_relu else 0,
                x.data_ptr(), x.stride(0), B, K, pro, L.lin.weight.data_ptr(), N,
                gmap[id(L.lin.weight)].data_ptr(), gmap[id(L.lin.bias)].data_ptr(),
                dx.data_ptr() if dx is not None else None, dx.stride(0) if dx is not None else 0,
                gmap[id(L.pro_bn.weight)].data_ptr() if L.pro_bn is not None else None,
                gmap[id(L.pro_bn.bias)].data_ptr() if L.pro_bn is not None else None))
        P.gate = None
        if prog["gate"] is not None:
            g1, g2 = prog["gate"]
            P.hidden = torch.zeros(B, 64, device=dev)
            P.gatew = torch.zeros(B, 3, device=dev)
            P.gate = ops.gate_params(P.buf["feats"], P.mask, g1.weight, g1.bias, g2.weight, g2.bias, P.hidden, P.gatew,
                                     P.buf["fused"], P.dbuf["fused"], self.ent_weight, P.dbuf["feats"],
                                     gmap[id(g1.weight)], gmap[id(g1.bias)], gmap[id(g2.weight)], gmap[id(g2.bias)],
                                     self.entropy)
        P.mix = None
        if prog.get("mix") is not None:            # learnable missing-modality bias between the encoders and the fusion MLP
            mx = prog["mix"]
            P.mask2 = torch.ones(B, len(mx["segs"]), device=dev)
            M = _S()["MixP"]()
            fe, dfe = P.buf["feats"], P.dbuf["feats"]
            M.feats, M.ld, M.M = fe.data_ptr(), fe.stride(0), B
            M.mask, M.ldm, M.nseg = P.mask2.data_ptr(), P.mask2.stride(0), len(mx["segs"])
            M.dfeats, M.ldd = dfe.data_ptr(), dfe.stride(0)
            for i, ((b0, w), bias) in enumerate(zip(mx["segs"], mx["biases"])):
                M.seg_begin[i], M.seg_width[i] = b0, w
                M.bias[i], M.dbias[i] = bias.data_ptr(), gmap[id(bias)].data_ptr()
            P.mix = M
        P.moe = None
        if prog.get("moe") is not None:
            self._plan_moe(P, gmap)
        hz = P.buf["hz"]
        # (SimMLM: the ensemble term's set leaves out rows without any modality, whose ensemble hazard is NaN)
        ens_valid = P.valid_x[0] if P.moe is not None else P.valid
        P.cox = _S()["CoxP"](hz.data_ptr(), hz.stride(0), P.time.data_ptr(), P.event.data_ptr(), ens_valid.data_ptr(), B, 1.0,
                             P.lse.data_ptr(), P.dbuf["hz"].data_ptr(), P.dbuf["hz"].stride(0), P.cox_out.data_ptr(), self.tie_mode,
                             P.tie_frac.data_ptr())
        # validation: the batch's Cox value only (no gradient), (loss | usable) kept per batch for validate_*'s bookkeeping
        P.cox_eval_out = torch.zeros(2, device=self.device)
        P.cox_eval = _S()["CoxP"](hz.data_ptr(), hz.stride(0), P.time.data_ptr(), P.event.data_ptr(), ens_valid.data_ptr(), B, 1.0,
                                  P.lse.data_ptr(), None, 1, P.cox_eval_out.data_ptr(), self.tie_mode, P.tie_frac.data_ptr())
        book = dict(acc=self.acc, cox_out=P.cox_out, entropy=self.entropy, rng=self.rng)   # per-step bookkeeping, in-kernel
        w2 = self.w2 if (self.w2 is not None and self.w2["fragmask"] is not None) else None
        if self.w2 is not None and w2 is None:        # (an encoder-less plan of an imaging model, e.g. the SyncBN heads plan, made first)
            raise RuntimeError("create the engine's first plan with the encoder (packed conv2 storage needs the volume size)")
        P.adam = ops.adam_params(self.flat, self.gflat, self.m, self.v, self.hyper, self.sumsq, self.step_count,
                                 None, self.adamw, w2=w2, **book)
        P.adam_skip = ops.adam_params(self.flat, self.gflat, self.m, self.v, self.hyper, self.sumsq, self.step_count,
                                      P.cox_out[1:], self.adamw, w2=w2, **book)
        if self.tune_tab is not None:
            P.tune = ops.tune_params(P.adam, self.tune_tab, self.anchor)
            P.tune_skip = ops.tune_params(P.adam_skip, self.tune_tab, self.anchor, check=False)
        P.graphs = {}
        self.plans[key] = P
        return P

    def _plan_moe(self, P, gmap):
        """MoeP blocks (include/mmsurv.h) of SimMLM_SurvivalNet: the two forward and two backward stages around the gate MLP, and the
        four Cox terms of the fused step (ensemble | image | rna | clinical) for ONE mms_cox_fwd_bwd_group launch."""
        mo, B, dev, S = self.prog["moe"], P.B, self.device, _S()
        F = mo["F"]
        P.gatew = torch.zeros(B, 3, device=dev)
        P.fused = torch.zeros(B, F, device=dev)
        P.valid_x = torch.ones(4, B, device=dev)          # Cox sets of the ensemble and the three experts (MoeP.valid_x)
        P.cox_outs = torch.zeros(4, 2, device=dev)
        P.lse4, P.frac4 = torch.zeros(4, B, device=dev), torch.zeros(4, B, device=dev)
        fe, dfe, hz, dhz = P.buf["feats"], P.dbuf["feats"], P.buf["hz"], P.dbuf["hz"]
        gin, dgin, h2, dh2 = P.buf["gin"], P.dbuf["gin"], P.buf["g2"], P.dbuf["g2"]
        out, ens = mo["out"], mo["ensemble"]

        def block(stage):
            q = S["MoeP"]()
            q.M, q.F, q.stage = B, F, stage
            q.feats, q.ldf, q.mask, q.ldm = fe.data_ptr(), fe.stride(0), P.mask.data_ptr(), P.mask.stride(0)
            q.valid, q.valid_x = P.valid.data_ptr(), P.valid_x.data_ptr()
            q.gin, q.ldg, q.h2, q.ldh2 = gin.data_ptr(), gin.stride(0), h2.data_ptr(), h2.stride(0)
            q.w3, q.b3 = out.weight.data_ptr(), out.bias.data_ptr()
            for e, L in enumerate(mo["experts"]):
                q.wx[e], q.bx[e] = L.weight.data_ptr(), L.bias.data_ptr()
                q.dwx[e], q.dbx[e] = gmap[id(L.weight)].data_ptr(), gmap[id(L.bias)].data_ptr()
            q.we, q.be = ens.weight.data_ptr(), ens.bias.data_ptr()
            q.hz, q.ldhz, q.gate, q.fused = hz.data_ptr(), hz.stride(0), P.gatew.data_ptr(), P.fused.data_ptr()
            q.dhz, q.lddhz, q.dh2, q.lddh2 = dhz.data_ptr(), dhz.stride(0), dh2.data_ptr(), dh2.stride(0)
            q.dgin, q.lddg, q.dfeats, q.lddf = dgin.data_ptr(), dgin.stride(0), dfe.data_ptr(), dfe.stride(0)
            q.dw3, q.db3 = gmap[id(out.weight)].data_ptr(), gmap[id(out.bias)].data_ptr()
            q.dwe, q.dbe = gmap[id(ens.weight)].data_ptr(), gmap[id(ens.bias)].data_ptr()
            # the objective's value for the step's bookkeeping (AdamP.cox_out): written by the backward's stage 1 (on the autograd path
            # too, where nothing reads it)
            q.cox_outs, q.expert_weight, q.loss_out = P.cox_outs.data_ptr(), self.expert_weight, P.cox_out.data_ptr()
            return q
        P.moe = [block(0), block(1)]
        P.moe_bwd = [block(0), block(1)]
        lam = self.expert_weight
        cox = (S["CoxP"] * 4)()
        for c in range(4):
            valid = P.valid_x[c]
            cox[c] = S["CoxP"](hz[:, c].data_ptr(), hz.stride(0), P.time.data_ptr(), P.event.data_ptr(), valid.data_ptr(), B,
                               1.0 if c == 0 else lam, P.lse4[c].data_ptr(), dhz[:, c].data_ptr(), dhz.stride(0), P.cox_outs[c].data_ptr(),
                               self.tie_mode, P.frac4[c].data_ptr())
        P.cox4 = cox

    def _cox_step(self, P):
        """The fused step's loss: one Cox term, or SimMLM's four (one launch; their sum is formed by the backward's mms_moe_bwd)."""
        if P.moe is not None:
            _lib.check(self.lib.mms_cox_fwd_bwd_group(P.cox4, 4, ops.stream()), "mms_cox_fwd_bwd_group")
        else:
            _lib.check(self.lib.mms_cox_fwd_bwd(ctypes.byref(P.cox), ops.stream()), "mms_cox_fwd_bwd")

    def _plan_big(self, P, gmap):
        """LinBigP blocks (include/mmsurv.h) of the large-batch Linear chain.  BatchNorm1d statistics of a buffer live in one
        fp64 array per plan: [sum | sumsq | s1 | s2] x columns, zeroed once per training step.  A layer's (buffer, column offset) source /
        destination is a pointer into the buffer with the buffer's pitch (the multimodal heads write [ct | rna | clinical] into `feats`)."""
        prog, B, dev = self.prog, P.B, self.device
        S, ptr = _S()["LinBigP"], ops.ptr
        # (keyed by (buffer, column offset): two layers that read different columns of one buffer get slots of their own)
        widths = {L.src: L.lin.in_features for L in prog["lins"] if L.pro_bn is not None}
        off, o = {}, 0
        for name, k in widths.items():
            off[name] = o
            o += 4 * k
        P.big_stats = torch.zeros(max(o, 1), dtype=torch.float64, device=dev)
        P.big_dbn = torch.zeros(B, max(list(widths.values()) + [4]), device=dev)
        st = lambda name, j: P.big_stats[off[name] + j * widths[name]:]
        P.big_lin = {True: [], False: []}
        for i, L in enumerate(prog["lins"]):
            (xs, xo), (ys, yo) = L.src, L.dst
            # column offsets are pointer offsets with the buffer's pitch; the float4 operand loads want 16-byte aligned rows
            for what, name, co in (("source", xs, xo), ("destination", ys, yo)):
                if co % 4 != 0 or (co and P.buf[name].stride(0) % 4 != 0):
                    raise RuntimeError("large-batch path: %s column offset %d of buffer '%s' (pitch %d floats) of layer %d is not 16-byte "
                                       "aligned; feature widths must be multiples of 4" % (what, co, name, P.buf[name].stride(0), i))
            x, y = P.buf[xs][:, xo:], P.buf[ys][:, yo:]
            K, N = L.lin.in_features, L.lin.out_features
            for train in (True, False):
                q = S()
                q.x, q.ldx, q.M, q.K = x.data_ptr(), x.stride(0), B, K
                q.w, q.bias, q.N = L.lin.weight.data_ptr(), L.lin.bias.data_ptr(), N
                q.y, q.ldy, q.out_relu = y.data_ptr(), y.stride(0), 1 if L.out_relu else 0
                q.train = 1 if train else 0
                q.drop_p = float(L.pro_drop.p) if L.pro_drop is not None else 0.0
                q.drop_mask, q.rng, q.stream_id = ptr(self.dropout_masks.get(i)), self.rng.data_ptr(), i + 1
                bn = L.pro_bn
                if bn is not None:
                    q.has_bn = 1
                    q.bn.sum, q.bn.sumsq = st(L.src, 0).data_ptr(), st(L.src, 1).data_ptr()
                    q.bn.rmean, q.bn.rvar = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
                    q.bn.gamma, q.bn.beta = bn.weight.data_ptr(), bn.bias.data_ptr()
                    q.bn.inv_count, q.bn.eps, q.bn.train, q.bn.nrep, q.bn.rep_stride = 1.0 / B, float(bn.eps), q.train, 1, 0
                    q.rmean, q.rvar, q.nbt = bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr()
                    q.momentum = float(bn.momentum)
                if train and L.dst in widths:        # a BatchNorm1d follows: the forward accumulates its batch statistics
                    q.osum, q.osumsq = st(L.dst, 0).data_ptr(), st(L.dst, 1).data_ptr()
                if train:
                    dy = P.dbuf[ys][:, yo:]
                    q.dy, q.lddy = dy.data_ptr(), dy.stride(0)
                    q.dw, q.dbias = gmap[id(L.lin.weight)].data_ptr(), gmap[id(L.lin.bias)].data_ptr()
                    tiles = ((N + 63) // 64) * ((K + 63) // 64)
                    q.msplit = max(1, min((512 + tiles - 1) // tiles, (B + 63) // 64))
                    if L.need_dx:
                        dx = P.dbuf[xs][:, xo:]
                        if bn is not None:
                            q.dbn, q.lddbn = P.big_dbn.data_ptr(), P.big_dbn.stride(0)
                            q.s1, q.s2 = st(L.src, 2).data_ptr(), st(L.src, 3).data_ptr()
                            q.dx, q.lddx = dx.data_ptr(), dx.stride(0)
                            q.dgamma, q.dbeta = gmap[id(bn.weight)].data_ptr(), gmap[id(bn.bias)].data_ptr()
                        else:
                            q.dbn, q.lddbn = dx.data_ptr(), dx.stride(0)
                P.big_lin[train].append(q)

    def _prolog(self, L, idx, train):
        p = float(L.pro_drop.p) if (L.pro_drop is not None) else 0.0
        mask = self.dropout_masks.get(idx)
        return ops.inprolog(L.pro_bn, train=train, drop_p=p, drop_mask=mask, rng=self.rng, stream_id=idx + 1)

    # ---- launches (all on torch's current stream; capturable) ---------------------------------------
    def _opts_arg(self, P):
        """`const MmsDnOpts*` of this engine's driver calls on plan P (ops.persistent_opts: the persistent per-block launches are taken
        only where their workgroups can all be co-resident; decided here, at launch = graph-capture time, and passed as an ARGUMENT)."""
        o = ops.persistent_opts(self.dn_opts, self.device, 1, P.B, P.dims)
        self._opts_live = o          # (keeps the block alive for the duration of the call)
        return ctypes.byref(o)

    def _zero_step(self):
        """The step's accumulators (flat gradient, sum of squares, gate entropy) zeroed by ONE launch (mms_zero_spans_group)."""
        if getattr(self, "_zspans", None) is None:
            self._zspans = ops.zero_spans([self.gflat, self.sumsq, self.entropy])
        _lib.check(self.lib.mms_zero_spans_group(self._zspans, len(self._zspans), ops.stream()), "mms_zero_spans_group")

    def _forward(self, P, train, enc_opts=None, entropy_zeroed=False):
        """enc_opts: `const MmsDnOpts*` of the DenseNet121 driver call instead of _opts_arg's (attribute: the per-layer forms);
        entropy_zeroed: the caller has zeroed the gate-entropy word on this stream (_zero_step)."""
        self.sync_packs()
        P.fwd_serial += 1
        st = ops.stream()
        lib, prog = self.lib, self.prog
        B, (D, H, W) = P.B, (P.dims if P.has_enc else (1, 1, 1))
        if P.has_enc:
            feats = P.buf["feats"]
            out = feats[:, prog["ct_cols"]:]
            enc_train = train and not self.enc_eval        # (FineTunePlan.encoder_eval: running statistics, not updated)
            if P.fallback:
                self._check_scalar_path(P)
                _lib.check(lib.mms_fb3_forward(P.ws.data_ptr(), P.ws_bytes, P.widths, B, D, H, W, P.ct.data_ptr(), P.ptab, P.btab, out.data_ptr(),
                                               feats.stride(0), 1 if enc_train else 0, st), "mms_fb3_forward")
            else:
                _lib.check(lib.mms_dn121_forward(P.ws.data_ptr(), B, D, H, W, P.ct.data_ptr(), P.ptab, P.btab, out.data_ptr(),
                                                 feats.stride(0), 1 if enc_train else 0, enc_opts if enc_opts is not None else self._opts_arg(P), st),
                           "mms_dn121_forward")
        if P.big:
            if train:
                P.big_stats.zero_()
            bl, n_pre = P.big_lin[train], prog["n_pre"]
            for q in bl[:n_pre]:
                _lib.check(lib.mms_linear_big_fwd(ctypes.byref(q), st), "mms_linear_big_fwd")
            if P.gate is not None:
                if not entropy_zeroed:
                    self.entropy.zero_()
                _lib.check(lib.mms_gate_fwd(ctypes.byref(P.gate), st), "mms_gate_fwd")
            if P.mix is not None:
                _lib.check(lib.mms_missing_mix_fwd(ctypes.byref(P.mix), st), "mms_missing_mix_fwd")
            for q in bl[n_pre:]:
                _lib.check(lib.mms_linear_big_fwd(ctypes.byref(q), st), "mms_linear_big_fwd")
            return
        lf = P.lin_fwd[train]
        n_pre = prog["n_pre"]
        for i in range(n_pre):
            _lib.check(lib.mms_linear_fwd(ctypes.byref(lf[i]), st), "mms_linear_fwd")
        if P.moe is not None:
            _lib.check(lib.mms_moe_fwd(ctypes.byref(P.moe[0]), st), "mms_moe_fwd")
        if P.gate is not None:
            if not entropy_zeroed:
                self.entropy.zero_()
            _lib.check(lib.mms_gate_fwd(ctypes.byref(P.gate), st), "mms_gate_fwd")
        if P.mix is not None:
            _lib.check(lib.mms_missing_mix_fwd(ctypes.byref(P.mix), st), "mms_missing_mix_fwd")
        for i in range(n_pre, len(lf)):
            _lib.check(lib.mms_linear_fwd(ctypes.byref(lf[i]), st), "mms_linear_fwd")
        if P.moe is not None:
            _lib.check(lib.mms_moe_fwd(ctypes.byref(P.moe[1]), st), "mms_moe_fwd")

    def _check_scalar_path(self, P):
        if not scalar_widths_ok(P.widths):
            raise ValueError("3-conv CT encoder widths %s: one model at a time runs the scalar kernels, which take widths that divide 256 "
                             "(16, 32, 64, 128); train and evaluate this model as a FoldGroupEngine (a group of one is fine)" % (tuple(P.widths),))

    def _backward_from_dhz(self, P):
        """dbuf['hz'] holds dL/dhazard; accumulates every parameter gradient into gflat."""
        self._backward_heads(P)
        self._backward_encoder(P)

    def _backward_heads(self, P):
        """Heads' backward: dbuf['hz'] -> every head parameter gradient and dbuf['feats'] (gradient wrt the encoder's output)."""
        st = ops.stream()
        lib, prog = self.lib, self.prog
        B, (D, H, W) = P.B, (P.dims if P.has_enc else (1, 1, 1))
        n_pre = prog["n_pre"]
        if P.big:
            def big_bwd(i):
                L, q = prog["lins"][i], P.big_lin[True][i]
                _lib.check(lib.mms_linear_big_bwd_w(ctypes.byref(q), st), "mms_linear_big_bwd_w")
                if L.need_dx:
                    _lib.check(lib.mms_linear_big_bwd_x(ctypes.byref(q), st), "mms_linear_big_bwd_x")
                    if L.pro_bn is not None:
                        _lib.check(lib.mms_bn1d_bwd_apply(ctypes.byref(q), st), "mms_bn1d_bwd_apply")
            for i in range(len(prog["lins"]) - 1, n_pre - 1, -1):
                big_bwd(i)
            if P.gate is not None:         # (mms_gate_bwd: the row-tiled form above 32 rows)
                _lib.check(lib.mms_gate_bwd(ctypes.byref(P.gate), st), "mms_gate_bwd")
            if P.mix is not None:
                _lib.check(lib.mms_missing_mix_bwd(ctypes.byref(P.mix), st), "mms_missing_mix_bwd")
            for i in range(n_pre - 1, -1, -1):
                big_bwd(i)
            return
        if P.moe is not None:
            _lib.check(lib.mms_moe_bwd(ctypes.byref(P.moe_bwd[1]), st), "mms_moe_bwd")
        for i in range(len(P.lin_bwd) - 1, n_pre - 1, -1):
            _lib.check(lib.mms_linear_bwd(ctypes.byref(P.lin_bwd[i]), st), "mms_linear_bwd")
        if P.gate is not None:
            _lib.check(lib.mms_gate_bwd(ctypes.byref(P.gate), st), "mms_gate_bwd")
        if P.mix is not None:
            _lib.check(lib.mms_missing_mix_bwd(ctypes.byref(P.mix), st), "mms_missing_mix_bwd")
        if P.moe is not None:
            _lib.check(lib.mms_moe_bwd(ctypes.byref(P.moe_bwd[0]), st), "mms_moe_bwd")
        for i in range(n_pre - 1, -1, -1):
            _lib.check(lib.mms_linear_bwd(ctypes.byref(P.lin_bwd[i]), st), "mms_linear_bwd")

    def _backward_encoder(self, P, stage=None, hook=None):
        """Encoder backward from dbuf['feats'].  stage = (block_hi, block_lo): one stage of the DenseNet121 backward
        (mms_dn121_backward_stage; the data-parallel step all-reduces each stage's gradient bucket while the next stage runs);
        hook: SyncBN statistics all-reduce (P.bn_world ranks)."""
        if not P.has_enc or self.enc_frozen:          # (a wholly frozen encoder: no gradient of it is wanted)
            return
        st = ops.stream()
        lib, prog = self.lib, self.prog
        B, (D, H, W) = P.B, P.dims
        dfe = P.dbuf["feats"]
        dct = dfe[:, prog["ct_cols"]:]
        # frozen lower stages: the backward stops above them.  Batches above 32 rows and SimMLM_SurvivalNet take the plan as an
        # optimiser-only feature: the full backward, whose frozen gradients nothing reads.
        if self.block_lo > 0 and not P.big and P.moe is None:
            if stage is not None or hook is not None or P.bn_world > 1:
                self._refuse_ddp()
            _lib.check(lib.mms_dn121_backward_from(P.ws.data_ptr(), B, D, H, W, P.ct.data_ptr(), P.ptab, dct.data_ptr(), dfe.stride(0),
                                                   P.gtab, self.block_lo, self._opts_arg(P), st), "mms_dn121_backward_from")
            return
        if P.fallback:
            _lib.check(lib.mms_fb3_backward(P.ws.data_ptr(), P.ws_bytes, P.widths, B, D, H, W, P.ct.data_ptr(), P.ptab, dct.data_ptr(),
                                            dfe.stride(0), P.gtab, st), "mms_fb3_backward")
            return
        if stage is not None or hook is not None or P.bn_world > 1:
            hi, lo = stage if stage is not None else (3, 0)
            _lib.check(lib.mms_dn121_backward_stage(P.ws.data_ptr(), B, D, H, W, P.ct.data_ptr(), P.ptab, dct.data_ptr(), dfe.stride(0),
                                                    P.gtab, hi, lo, P.bn_world, hook, None, self._opts_arg(P), st), "mms_dn121_backward_stage")
            return
        _lib.check(lib.mms_dn121_backward(P.ws.data_ptr(), B, D, H, W, P.ct.data_ptr(), P.ptab, dct.data_ptr(),
                                          dfe.stride(0), P.gtab, self._opts_arg(P), st), "mms_dn121_backward")

    def _train_body(self, P, skip_if_unusable):
        """zero-grad -> forward -> Cox -> backward -> clip -> Adam, epoch accumulators: the single-GPU step (also what fold sharding runs)."""
        self._zero_step()
        self._forward(P, True, entropy_zeroed=True)
        self._cox_step(P)
        self._backward_from_dhz(P)
        self._update(P, skip_if_unusable)

    def _update(self, P, skip_if_unusable):
        """Global-norm clip + Adam over the flat buffers: the sum-of-squares launch and the update launch, tuned (fine-tuning plan) or plain."""
        st = ops.stream()
        lib = self.lib
        if self.tune_tab is not None:
            tu = P.tune_skip if skip_if_unusable else P.tune
            _lib.check(lib.mms_grad_sumsq_tuned(ctypes.byref(tu), st), "mms_grad_sumsq_tuned")
            _lib.check(lib.mms_clip_adam_tuned(ctypes.byref(tu), st), "mms_clip_adam_tuned")
            return
        ad = P.adam_skip if skip_if_unusable else P.adam
        _lib.check(lib.mms_grad_sumsq(ctypes.byref(ad), st), "mms_grad_sumsq")
        _lib.check(lib.mms_clip_adam(ctypes.byref(ad), st), "mms_clip_adam")
        # (dropout counter and the epoch accumulators self.acc are advanced inside mms_grad_sumsq: AdamP.acc / .rng)

    # ---- public: fused training step ------------------------------------------------------------------
    def load_batch(self, P, ct=None, rna=None, clinical=None, mask=None, time=None, event=None, valid=None, shared_ct=False):
        """shared_ct: the volume is not copied -- the launches read another plan's copy (FoldGroupEngine.forward_eval_shared)."""
        if P.has_enc and not shared_ct:
            P.ct.copy_(ct.reshape(P.ct.shape), non_blocking=True)
        if "rna" in P.buf:
            P.buf["rna"].copy_(rna, non_blocking=True)
        if clinical is not None and "clin" in P.buf:
            P.buf["clin"].copy_(clinical.reshape(P.buf["clin"].shape), non_blocking=True)
        if mask is not None:
            (P.mask2 if P.mix is not None else P.mask).copy_(mask, non_blocking=True)
        if time is not None:
            P.time.copy_(time.reshape(-1), non_blocking=True)
            P.event.copy_(event.reshape(-1).to(torch.float32), non_blocking=True)
        if valid is None:
            P.valid.fill_(1.0)
        else:
            P.valid.copy_(valid.reshape(-1).to(torch.float32), non_blocking=True)

    def gather_block(self, P, cohort, idx_dev, fold=None):
        """-> (GatherP (include/mmsurv.h) that assembles this plan's batch from a cohort dict (data.make_cohort) that lives in HBM
        (data.cohort_to) or in pinned host memory (data.cohort_pin: the gather launch then reads the rows over PCIe): image, rnaseq,
        clinical, mask, label[time, event] and, when present, a float per-patient `valid` column;  per source (role, drop bit): what it
        is to augmentation records (augment.aug_block) -- the CT volume, a row that modality j's drop bit zero-fills, a mask whose
        column j that bit clears, a plain copy).  idx_dev: [B] int64 device tensor that the caller refills before each launch.  With
        a modality mask in the cohort, image / rnaseq rows of patients without that modality are zero-filled instead of read where
        they are all-zero in the cohort (data.absent_rows_zero).  fold: over a cohort with per-fold gene matrices
        (gene_select.GeneSelection.apply) the rnaseq source -- pointer, pitch and width -- is that fold's [N, k] matrix."""
        from .augment import ROLE_MASK, ROLE_PLAIN, ROLE_VOLUME
        from .data import absent_rows_zero
        flags = {}
        if "mask" in cohort:
            flags = {key: cohort["mask"][:, j:] for j, (key, ok) in enumerate(zip(("image", "rnaseq"), absent_rows_zero(cohort))) if ok}
        srcs = []        # (cohort tensor, destination, width or None = all columns, availability flags or None, role, drop bit or -1)
        if "rna" in P.buf:
            rna = cohort["rnaseq"]
            if "rnaseq_folds" in cohort:         # per-fold gene selection: this member's own [N, k] matrix (a zero row keeps zero columns)
                from .gene_select import fold_matrix
                rna = fold_matrix(cohort, fold)
            if rna.shape[1] != P.buf["rna"].shape[1]:
                raise ValueError("the model reads %d RNA-seq columns, the cohort's matrix has %d" % (P.buf["rna"].shape[1], rna.shape[1]))
            srcs.append((rna, P.buf["rna"], None, flags.get("rnaseq"), ROLE_PLAIN, 1))
        if P.has_enc:
            srcs.append((cohort["image"].view(cohort["image"].shape[0], -1), P.ct.view(P.B, -1), None, flags.get("image"), ROLE_VOLUME, 0))
        if "clin" in P.buf:
            srcs.append((cohort["clinical"], P.buf["clin"], None, None, ROLE_PLAIN, 2))
        if P.gate is not None or P.moe is not None:
            srcs.append((cohort["mask"], P.mask, None, None, ROLE_MASK, -1))
        if P.mix is not None:            # [has_image, has_rnaseq] = the first columns of the cohort's modality mask
            srcs.append((cohort["mask"], P.mask2, P.mask2.shape[1], None, ROLE_MASK, -1))
        lab = cohort["label"]
        srcs.append((lab, P.time.view(P.B, 1), 1, None, ROLE_PLAIN, -1))
        srcs.append((lab[:, 1:], P.event.view(P.B, 1), 1, None, ROLE_PLAIN, -1))
        if "valid" in cohort:
            srcs.append((cohort["valid"].view(-1, 1), P.valid.view(P.B, 1), 1, None, ROLE_PLAIN, -1))
        return ops.gather_params(idx_dev, P.B, [s[:4] for s in srcs]), [s[4:] for s in srcs]

    def train_step(self, ct=None, rna=None, clinical=None, mask=None, time=None, event=None, valid=None, skip_if_unusable=True,
                   use_graph=True, ddp_world=1, global_cox=False, sync_bn=False):
        """One optimisation step on one batch (inputs may live on host or device).  Returns nothing: losses are
        accumulated on the device (`epoch_stats()`), exactly one host sync per epoch instead of one per batch.
        ddp_world > 1: data-parallel step on this rank's shard of the global batch (`distributed.DataParallel.step`: bucketed gradient
        all-reduce overlapped with the backward; rank-local BatchNorm; rank-local or global_cox risk sets), or with sync_bn=True the
        exact global-batch step (`DataParallel.step_syncbn`: SyncBN + replicated heads + global risk set; eager launches)."""
        B = (rna if rna is not None else ct).shape[0]
        self.check_train_batch(B, tuple(ct.shape[-3:]) if ct is not None else None, ddp_world if sync_bn else 1)
        P = self.plan(B, tuple(ct.shape[-3:]) if ct is not None else None, bn_world=ddp_world if (sync_bn and ddp_world > 1) else 1)
        self.load_batch(P, ct, rna, clinical, mask, time, event, valid)
        self.sync_packs()
        P.fwd_serial += 1           # (a graph replay does not pass through _forward)
        if ddp_world > 1:
            self._refuse_ddp()
            if P.big and self.prog["encoder"] is not None:
                raise RuntimeError("the data-parallel steps of the imaging models are limited to 32 rows per rank (their staged graphs are "
                                   "built and tested on the small-batch head kernels); got %d -- lower the per-rank batch (the global batch "
                                   "is ddp_world times it) or train large batches on one GPU" % B)
            if P.moe is not None:
                raise RuntimeError("SimMLM_SurvivalNet: the data-parallel step (ddp_world > 1) is not implemented for this model; "
                                   "train its folds as a fold group or one per process instead")
            if self._dp is None:
                from .distributed import DataParallel
                self._dp = DataParallel(self)
            if sync_bn:
                self._dp.step_syncbn(P, ddp_world)
            else:
                self._dp.step(P, ddp_world, global_cox, use_graph)
            return
        if not use_graph:
            self._train_body(P, skip_if_unusable)
            return
        key = ("train", skip_if_unusable)
        if key not in P.graphs:
            P.graphs[key] = capture([self], lambda: self._train_body(P, skip_if_unusable))
        P.graphs[key].replay()

    def forward_eval(self, ct=None, rna=None, clinical=None, mask=None, use_graph=True):
        """Eval-mode forward -> (hazard [B] view of a static buffer, gate [B,3] or None)."""
        B = (rna if rna is not None else ct).shape[0]
        P = self.plan(B, tuple(ct.shape[-3:]) if ct is not None else None)
        self.load_batch(P, ct, rna, clinical, mask)
        self.sync_packs()
        P.fwd_serial += 1           # (a graph replay does not pass through _forward)
        if use_graph:
            if "eval" not in P.graphs:
                P.graphs["eval"] = capture([self], lambda: self._forward(P, False))
            P.graphs["eval"].replay()
        else:
            self._forward(P, False)
        return P.buf["hz"][:, 0], gate_out(P)

    # ---- input-gradient attribution ----------------------------------------------------------------------
    def _attr_blocks(self, P):
        """Parameter blocks of the attribution backward on plan P (B <= 32): every Linear with its prologue in EVAL mode, no weight
        gradient and dx requested down to the raw inputs; the gate without its entropy term, its weight gradients into a private
        scratch; the missing-modality mix without its bias gradient.  Nothing here points into gflat."""
        A = getattr(P, "attr", None)
        if A is not None:
            return A
        S, dev, prog = _S(), self.device, self.prog
        A = dict(dct=torch.zeros_like(P.ct) if P.has_enc else None, lin=[], gate=None, mix=None)
        for k in ("rna", "clin"):
            if k in P.buf:
                A["d" + k] = torch.zeros(P.B, prog["bufs"][k], device=dev)
        for i, L in enumerate(prog["lins"]):
            (xs, xo), (ys, yo) = L.src, L.dst
            x, y, dy = P.buf[xs][:, xo:], P.buf[ys][:, yo:], P.dbuf[ys][:, yo:]
            dx = A["d" + xs] if xs in ("rna", "clin") else P.dbuf[xs][:, xo:]
            A["lin"].append(S["LinearBwdP"](dy.data_ptr(), dy.stride(0), y.data_ptr(), y.stride(0), 1 if L.out_relu else 0,
                                            x.data_ptr(), x.stride(0), P.B, L.lin.in_features, self._prolog(L, i, False),
                                            L.lin.weight.data_ptr(), L.lin.out_features, None, None, dx.data_ptr(), dx.stride(0), None, None))
        if P.gate is not None:
            G = S["GateP"]()
            ctypes.memmove(ctypes.byref(G), ctypes.byref(P.gate), ctypes.sizeof(G))
            A["gate_scratch"] = torch.zeros(64 * 291 + 64 + 3 * 64 + 3, device=dev)
            b = A["gate_scratch"].data_ptr()
            G.ent_weight, G.dgate_ext, G.entropy = 0.0, None, None
            G.dw1, G.db1, G.dw2, G.db2 = b, b + 4 * 64 * 291, b + 4 * (64 * 291 + 64), b + 4 * (64 * 291 + 64 + 192)
            A["gate"] = G
        if P.mix is not None:
            M = S["MixP"]()
            ctypes.memmove(ctypes.byref(M), ctypes.byref(P.mix), ctypes.sizeof(M))
            for i in range(4):
                M.dbias[i] = None
            A["mix"] = M
        if P.has_enc and not P.fallback:     # the encoder's per-layer forms: nothing on this path waits inside a launch
            A["opts"] = ops.dn_opts(self.dn_opts, persist_b3=-1, persist_b4=-1, fuse_layers=-1)
        P.attr = A
        return A

    def _attribute_chunk(self, P, ct, rna, clinical, mask):
        st, lib, prog = ops.stream(), self.lib, self.prog
        A = self._attr_blocks(P)
        self.load_batch(P, ct, rna, clinical, mask)
        self._forward(P, False, enc_opts=ctypes.byref(A["opts"]) if "opts" in A else None)
        P.dbuf["hz"].fill_(1.0)           # d hazard[b] / d hazard[b] = 1: rows do not interact in eval mode
        n_pre = prog["n_pre"]
        for i in range(len(A["lin"]) - 1, n_pre - 1, -1):
            _lib.check(lib.mms_linear_bwd(ctypes.byref(A["lin"][i]), st), "mms_linear_bwd")
        if A["gate"] is not None:
            _lib.check(lib.mms_gate_bwd(ctypes.byref(A["gate"]), st), "mms_gate_bwd")
        if A["mix"] is not None:
            _lib.check(lib.mms_missing_mix_bwd(ctypes.byref(A["mix"]), st), "mms_missing_mix_bwd")
        for i in range(n_pre - 1, -1, -1):
            _lib.check(lib.mms_linear_bwd(ctypes.byref(A["lin"][i]), st), "mms_linear_bwd")
        if P.has_enc:
            B, (D, H, W) = P.B, P.dims
            dfe = P.dbuf["feats"]
            dct = dfe[:, prog["ct_cols"]:]
            if P.fallback:
                _lib.check(lib.mms_fb3_input_grad(P.ws.data_ptr(), P.ws_bytes, P.widths, B, D, H, W, P.ct.data_ptr(), P.ptab, P.btab,
                                                  dct.data_ptr(), dfe.stride(0), A["dct"].data_ptr(), st), "mms_fb3_input_grad")
            else:
                _lib.check(lib.mms_dn121_input_grad(P.ws.data_ptr(), B, D, H, W, P.ct.data_ptr(), P.ptab, P.btab, dct.data_ptr(),
                                                    dfe.stride(0), A["dct"].data_ptr(), ctypes.byref(A["opts"]), st), "mms_dn121_input_grad")
        out = dict(hazard=P.buf["hz"][:, 0].clone(), gate=P.gatew.clone() if P.gate is not None else None)
        out["ct"] = A["dct"].clone() if P.has_enc else None
        out["rna"] = A["drna"].clone() if "drna" in A else None
        out["clinical"] = A["dclin"].clone() if "dclin" in A else None
        return out

    def attribute(self, ct=None, rna=None, clinical=None, mask=None, wrt=("ct", "rna", "clinical")):
        """Input-gradient attribution of an EVAL-mode model: -> dict(hazard [B], gate [B, 3] | None, ct [B, 1, D, H, W], rna [B, rna_dim],
        clinical [B, clinical_dim]); entry m of `wrt` is the gradient of row b's hazard with respect to row b's raw input m (None for an
        input the model does not have or that is not in `wrt`).  BatchNorm statistics are frozen, so rows do not interact and one
        backward with dhazard = 1 per row gives every row's gradient; more than 32 rows run in chunks of 32 (exact).  Eval forward ->
        heads' backward with eval-mode prologues and no weight gradients -> the encoder's input-gradient driver (mms_dn121_input_grad /
        mms_fb3_input_grad).  Touches no .grad, no optimiser state, no running statistic, no conv2 pack and no training graph."""
        check_attribute([self], wrt)
        ref = rna if rna is not None else ct
        B = ref.shape[0]
        dims = tuple(ct.shape[-3:]) if (ct is not None and self.prog["encoder"] is not None) else None
        parts = []
        for b0 in range(0, B, 32):
            b1 = min(B, b0 + 32)
            cut = lambda t: None if t is None else t[b0:b1]
            P = self.plan(b1 - b0, dims)
            parts.append(self._attribute_chunk(P, cut(ct), cut(rna), cut(clinical), cut(mask)))
        out = {}
        for k in ("hazard", "gate", "ct", "rna", "clinical"):
            vals = [p[k] for p in parts]
            keep = k in ("hazard", "gate") or k in wrt
            out[k] = None if (vals[0] is None or not keep) else (vals[0] if len(vals) == 1 else torch.cat(vals, 0))
        return out

    def reset_epoch_stats(self):
        self.acc.zero_()

    def check_b4(self):
        """The sticky time-out word of the block-4 persistent kernels (csrc/dn_b4.hip): a cluster whose workgroups never became
        co-resident (more persistent workgroups in flight than the chip holds) leaves garbage behind and must not pass silently --
        neither in training (epoch_stats) nor in validation / inference (validate_*, validate_lockstep, evaluate_model.py).  One
        device->host read per plan; the word is cleared before raising so that the workspace stays usable."""
        for P in self.plans.values():
            if getattr(P, "has_enc", False) and not P.fallback:
                if getattr(P, "b4_err", None) is None:
                    off, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
                    D, H, W = P.dims
                    _lib.check(self.lib.mms_dn121_region(P.B, D, H, W, b"b4_err", 0, ctypes.byref(off), ctypes.byref(nb)), "mms_dn121_region")
                    P.b4_err = P.ws[off.value:off.value + 4].view(torch.int32)
                if int(P.b4_err.item()) != 0:
                    P.b4_err.zero_()
                    raise RuntimeError("mmsurv: an in-launch hand-off (block-4 persistent kernel or fused block-3 forward) timed out (too many "
                                       "such launches in flight at once?); the results since the last check are invalid -- rerun with "
                                       "dn_opts={'persist_b4': -1, 'fuse_layers': -1}")

    def epoch_stats(self):
        """-> dict(sum_loss, n_usable, sum_entropy, n_batches) (one device->host sync); checks the block-4 time-out word (check_b4)."""
        a = self.acc.tolist()
        self.check_b4()
        return dict(sum_loss=a[0], n_usable=a[1], sum_entropy=a[2], n_batches=a[3])


def engine_of(model, **kw):
    e = getattr(model, "_mms_engine", None)
    if e is None:
        e = SurvivalEngine(model, **kw)
    elif "finetune" in kw:
        from . import transfer
        if transfer.as_plan(kw["finetune"]) != e.finetune:
            raise RuntimeError("this model's engine was built with the fine-tuning plan %r; the plan of a live engine cannot be changed "
                               "(to %r) -- build a fresh model and engine" % (e.finetune, kw["finetune"]))
    return e
