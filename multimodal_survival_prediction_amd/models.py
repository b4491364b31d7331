"""The reference's survival networks as drop-in nn.Modules whose forward/backward run on the HIP engine.

Constructor signatures, forward signatures, sub-module names (state_dict keys) and parameter creation order are
the reference's (final_multimodal.py:59-150, partial_modality_training.py:165-277, simple_fusion.py:160-236,
flexible_multimodal.py:157-256, train_rnaseq_only.py:126-151; MONAI branch).  The nn.Sequential containers only own parameters; they are never called.  Parameters stay ordinary
autograd leaves: `torch.optim.Adam(model.parameters())`, `clip_grad_norm_`, `state_dict()/load_state_dict()` keep
working (the autograd-compatible path), while `training.train_epoch_*` drive the fused HIP-graph step (what each model's loop feeds
it is that style's row of `training._STYLES`).

Weight changes from outside the fused step: the DenseNet121 encoder keeps derived packs of its 58 conv2 weights, and the engine rebuilds
them before its next launch when torch's version counters show a change -- `load_state_dict`, a torch optimiser's `step()`, any in-place
edit of a parameter under `no_grad` (`p.mul_()`, `p.copy_()`).  A write through `p.data` (`p.data.mul_()`, optimisers written in the old
`.data` style) moves no version counter and cannot be seen: call `engine_of(model).sync_packs(force=True)` after one.

One workspace per (batch size, volume size): the forward's activations and BatchNorm statistics live in the engine's plan, not in the
autograd graph.  Every forward at the same batch size and volume size -- training or eval mode, with or without gradients, through the
module or through the engine (`forward_eval`, `train_step`) -- overwrites it; a forward at another batch size or volume size has a
workspace of its own and disturbs nothing.  A backward whose forward is no longer the latest on its workspace raises, and so does a
second backward over the same forward (the first consumed the workspace's BatchNorm-backward accumulators, which only a training
forward zeroes: csrc/dn_net.hip, DESIGN.md "Weight changes and the module surface").
"""
import torch
import torch.nn as nn

from .densenet import DenseNet121
from .engine import engine_of

# The reference picks its CT encoder with a module-level switch set by `try: import monai`
# (final_multimodal.py:34-42).  True -> DenseNet121-3D (MONAI's topology), False -> the in-file 3-conv fallback
# (final_multimodal.py:75-86).  Both run as HIP kernels here; flip it before constructing a model.
USE_MONAI = True


def _ct_encoder(out_dim=128):
    if USE_MONAI:
        return DenseNet121(spatial_dims=3, in_channels=1, out_channels=out_dim, pretrained=False)
    return nn.Sequential(        # parameter holder with the reference's keys (0,1,3,4,6,7); never called
        nn.Conv3d(1, 32, 3, stride=2, padding=1), nn.BatchNorm3d(32), nn.ReLU(),
        nn.Conv3d(32, 64, 3, stride=2, padding=1), nn.BatchNorm3d(64), nn.ReLU(),
        nn.Conv3d(64, out_dim, 3, stride=2, padding=1), nn.BatchNorm3d(out_dim), nn.ReLU(),
        nn.AdaptiveAvgPool3d(1))


def _rna_encoder(rna_dim):
    return nn.Sequential(nn.Linear(rna_dim, 512), nn.BatchNorm1d(512), nn.ReLU(), nn.Dropout(0.3),
                         nn.Linear(512, 128), nn.ReLU())


def _fusion(d):
    return nn.Sequential(nn.Linear(d, 256), nn.BatchNorm1d(256), nn.ReLU(), nn.Dropout(0.3), nn.Linear(256, 128), nn.ReLU())


def _next_dropout_masks(eng):
    """End of a completed training backward on the autograd path: advance the dropout step counter engine.rng[1] (on the device, on the
    current stream, no host sync), as mms_grad_sumsq does for the fused step.  The k-th backward since the engine was created draws
    the masks of counter k -- the fused path's sequence; a forward and its own backward (which recomputes the masks) read the same
    value; two forward/backward rounds before one optimiser step draw two masks, as torch's Dropout does."""
    eng.rng[1:].add_(1)


def _claim_backward(P, serial):
    """The backward of the forward that stamped `serial` on plan P may run only while that forward is the latest on P's workspace,
    and only once."""
    if P.fwd_serial != serial:
        raise RuntimeError("backward: another forward ran on this model's workspace since the forward being differentiated (same batch "
                           "size and volume size share one workspace, eval-mode and no_grad forwards included); its activations and "
                           "BatchNorm statistics are gone -- run each backward before the next forward")
    if P.bwd_serial == serial:
        raise RuntimeError("backward: a second backward over the same forward is not supported (the first one consumed the workspace's "
                           "BatchNorm-backward accumulators, which only a training forward zeroes); run the forward again")
    P.bwd_serial = serial


class _Net(torch.autograd.Function):
    """forward/backward of a whole network on the engine's eager path."""

    @staticmethod
    def forward(ctx, anchor, model, ct, rna, clinical, mask):
        eng = engine_of(model)
        P = eng.plan((rna if rna is not None else ct).shape[0], tuple(ct.shape[-3:]) if ct is not None else None)
        eng.load_batch(P, ct, rna, clinical, mask)
        eng._forward(P, model.training)
        ctx.eng, ctx.P, ctx.train, ctx.serial = eng, P, model.training, P.fwd_serial
        hz = P.buf["hz"][:, 0].clone()
        if P.gate is not None:
            return hz, P.gatew.clone()
        return hz, None

    @staticmethod
    def backward(ctx, dhz, dgate):
        if not ctx.train:
            raise RuntimeError("backward through an eval-mode forward is not supported (BN batch statistics)")
        eng, P = ctx.eng, ctx.P
        _claim_backward(P, ctx.serial)
        if eng.params[0].grad is None:
            eng.gflat.zero_()
            eng.attach_grads()
        if dhz is None:
            P.dbuf["hz"].zero_()
        else:
            P.dbuf["hz"][:, 0].copy_(dhz)
        if P.gate is not None:
            ext = dgate.contiguous() if dgate is not None else None
            P.gate.dgate_ext = ext.data_ptr() if ext is not None else None
            old, P.gate.ent_weight = P.gate.ent_weight, 0.0      # the entropy term arrives through dgate here
            eng._backward_from_dhz(P)
            P.gate.ent_weight, P.gate.dgate_ext = old, None
        else:
            eng._backward_from_dhz(P)
        _next_dropout_masks(eng)
        return None, None, None, None, None, None


def _run(model, ct, rna, clinical, mask):
    if (rna is not None and not rna.is_cuda) or (ct is not None and not ct.is_cuda):
        raise RuntimeError("%s (HIP): inputs must be on an MI355X device; there is no CPU fallback" % type(model).__name__)
    anchor = next(model.parameters())
    if torch.is_grad_enabled() and model.training:
        return _Net.apply(anchor, model, ct, rna, clinical, mask)
    eng = engine_of(model)
    P = eng.plan((rna if rna is not None else ct).shape[0], tuple(ct.shape[-3:]) if ct is not None else None)
    eng.load_batch(P, ct, rna, clinical, mask)
    eng._forward(P, model.training)
    return P.buf["hz"][:, 0].clone(), (P.gatew.clone() if P.gate is not None else None)


class MultiModalSurvivalNet(nn.Module):
    def __init__(self, rna_dim=5005, clinical_dim=1):
        super().__init__()
        self.ct_encoder = _ct_encoder(128)
        self.use_monai = USE_MONAI
        self.ct_pool = nn.AdaptiveAvgPool3d(1)
        self.rna_encoder = _rna_encoder(rna_dim)
        self.clinical_encoder = nn.Sequential(nn.Linear(clinical_dim, 32), nn.ReLU())
        self.fusion = _fusion(128 + 128 + 32)
        self.cox_head = nn.Linear(128, 1)

    def forward(self, ct, rna, clinical):
        return _run(self, ct, rna, clinical, None)[0]


class PartialModalityNet(nn.Module):
    def __init__(self, rna_dim=5005, clinical_dim=1):
        super().__init__()
        self.ct_encoder = _ct_encoder(128)
        self.use_monai = USE_MONAI
        self.ct_pool = nn.AdaptiveAvgPool3d(1)
        self.rna_encoder = _rna_encoder(rna_dim)
        self.clinical_encoder = nn.Sequential(nn.Linear(clinical_dim, 32), nn.ReLU())
        self.gate = nn.Sequential(nn.Linear(128 + 128 + 32 + 3, 64), nn.ReLU(), nn.Linear(64, 3), nn.Softmax(dim=1))
        self.fusion = _fusion(128 + 128 + 32)
        self.cox_head = nn.Linear(128, 1)

    def forward(self, ct, rna, clinical, mask):
        hz, gate = _run(self, ct, rna, clinical, mask)
        return hz, gate


class SimpleFusionModel(nn.Module):
    def __init__(self, rna_dim=5005, img_feature_dim=128, rna_feature_dim=256):
        super().__init__()
        # both widths are free constructor arguments (simple_fusion.py:163); the heads read feature rows with 16-byte loads
        if rna_feature_dim % 4 != 0 or rna_feature_dim <= 0 or img_feature_dim % 4 != 0 or img_feature_dim <= 0:
            raise ValueError("rna_feature_dim and img_feature_dim must be positive multiples of 4 (16-byte aligned feature columns)")
        self.rna_encoder = nn.Sequential(
            nn.Linear(rna_dim, 1024), nn.BatchNorm1d(1024), nn.ReLU(), nn.Dropout(0.3),
            nn.Linear(1024, 512), nn.BatchNorm1d(512), nn.ReLU(), nn.Dropout(0.3),
            nn.Linear(512, rna_feature_dim), nn.ReLU())
        self.image_encoder = _ct_encoder(img_feature_dim)
        self.use_monai = USE_MONAI
        if USE_MONAI:
            self.image_pool = nn.AdaptiveAvgPool3d(1)
        self.fusion = nn.Sequential(
            nn.Linear(rna_feature_dim + img_feature_dim, 256), nn.BatchNorm1d(256), nn.ReLU(), nn.Dropout(0.3),
            nn.Linear(256, 128), nn.ReLU(), nn.Dropout(0.2), nn.Linear(128, 1))

    def forward(self, image, rnaseq):
        return _run(self, image, rnaseq, None, None)[0]


class FlexibleMultimodalModel(nn.Module):
    """flexible_multimodal.py:157-256: SimpleFusion heads on [image | rna] features with a LEARNABLE bias standing in for a
    missing modality (mask (B,2) = [has_image, has_rnaseq]).  Parameter creation order (image_encoder, rna_encoder, the two
    biases via torch.randn, fusion) is the reference's, so a seeded construction draws the same initial weights."""

    def __init__(self, rna_dim=5005, img_feature_dim=128, rna_feature_dim=256):
        super().__init__()
        # both widths are free constructor arguments (simple_fusion.py:163); the heads read feature rows with 16-byte loads
        if rna_feature_dim % 4 != 0 or rna_feature_dim <= 0 or img_feature_dim % 4 != 0 or img_feature_dim <= 0:
            raise ValueError("rna_feature_dim and img_feature_dim must be positive multiples of 4 (16-byte aligned feature columns)")
        self.image_encoder = _ct_encoder(img_feature_dim)
        self.use_monai = USE_MONAI
        if USE_MONAI:
            self.image_pool = nn.AdaptiveAvgPool3d(1)
        self.rna_encoder = nn.Sequential(
            nn.Linear(rna_dim, 1024), nn.BatchNorm1d(1024), nn.ReLU(), nn.Dropout(0.3),
            nn.Linear(1024, 512), nn.BatchNorm1d(512), nn.ReLU(), nn.Dropout(0.3),
            nn.Linear(512, rna_feature_dim), nn.ReLU())
        self.missing_image_bias = nn.Parameter(torch.randn(img_feature_dim))
        self.missing_rna_bias = nn.Parameter(torch.randn(rna_feature_dim))
        self.fusion = nn.Sequential(
            nn.Linear(img_feature_dim + rna_feature_dim, 256), nn.BatchNorm1d(256), nn.ReLU(), nn.Dropout(0.3),
            nn.Linear(256, 128), nn.ReLU(), nn.Dropout(0.2), nn.Linear(128, 1))

    def forward(self, image, rnaseq, mask):
        return _run(self, image, rnaseq, None, mask)[0]


class RNASeqSurvivalModel(nn.Module):
    """train_rnaseq_only.py:126-151: MLP 5005 -> 1024 -> 512 -> 256 -> 1 ([Linear, BatchNorm1d, ReLU, Dropout(0.3)] per hidden
    layer); forward returns the (B, 1) log-hazard like the reference."""

    def __init__(self, input_dim=5005, hidden_dims=[1024, 512, 256]):
        super().__init__()
        layers, in_dim = [], input_dim
        for h in hidden_dims:
            layers.extend([nn.Linear(in_dim, h), nn.BatchNorm1d(h), nn.ReLU(), nn.Dropout(0.3)])
            in_dim = h
        layers.append(nn.Linear(in_dim, 1))
        self.mlp = nn.Sequential(*layers)

    def forward(self, rnaseq):
        return _run(self, None, rnaseq, None, None)[0].unsqueeze(1)


class ImageOnlyModel(nn.Module):
    """generate_km_curves.py:28-54: the CT-only baseline.  3 x [Conv3d(k3, s2, p1) + BatchNorm3d + ReLU] at 1 -> 16 -> 32 -> 64 channels +
    global average pool (always this encoder: the class does not look at USE_MONAI), Linear(64, 32) + ReLU, Linear(32, 1).
    Sub-module names (encoder.{0,1,3,4,6,7}, fc.0, risk_head) and parameter creation order are the reference's, so a seeded construction
    draws its weights and state_dict() interchanges with it.  forward(x [B, 1, D, H, W]) -> risk [B].  No BatchNorm1d: a training batch of
    one patient is legal (BatchNorm3d over that patient's voxels)."""

    def __init__(self):
        super().__init__()
        self.encoder = nn.Sequential(        # parameter holder; never called
            nn.Conv3d(1, 16, 3, stride=2, padding=1), nn.BatchNorm3d(16), nn.ReLU(),
            nn.Conv3d(16, 32, 3, stride=2, padding=1), nn.BatchNorm3d(32), nn.ReLU(),
            nn.Conv3d(32, 64, 3, stride=2, padding=1), nn.BatchNorm3d(64), nn.ReLU(),
            nn.AdaptiveAvgPool3d(1))
        self.fc = nn.Sequential(nn.Linear(64, 32), nn.ReLU())
        self.risk_head = nn.Linear(32, 1)

    def forward(self, x):
        return _run(self, x, None, None, None)[0]


# ---- SimMLM_SurvivalNet (generate_km_curves.py:158-281): gated mixture of modality experts -----------------------------------
class _MoeExpert(nn.Module):
    """Parameter holder with the reference's ModalityExpert names (encoder, [pool,] cox_head); never called."""

    def __init__(self, modality, input_dim=None, output_dim=128):
        super().__init__()
        self.modality_type = modality
        if modality == "image":
            self.encoder = _ct_encoder(output_dim)
            self.use_monai = USE_MONAI
            self.pool = nn.AdaptiveAvgPool3d(1)
        elif modality == "rnaseq":
            self.encoder = nn.Sequential(nn.Linear(input_dim, 512), nn.BatchNorm1d(512), nn.ReLU(), nn.Dropout(0.3),
                                         nn.Linear(512, output_dim), nn.ReLU())
        else:
            self.encoder = nn.Sequential(nn.Linear(input_dim, 64), nn.ReLU(), nn.Linear(64, output_dim), nn.ReLU())
        self.cox_head = nn.Linear(output_dim, 1)


class _MoeGate(nn.Module):
    def __init__(self, feature_dim=128, num_modalities=3):
        super().__init__()
        self.gate = nn.Sequential(nn.Linear(feature_dim * num_modalities + num_modalities, 128), nn.ReLU(), nn.Dropout(0.2),
                                  nn.Linear(128, 64), nn.ReLU(), nn.Linear(64, num_modalities))


class _MoeNet(torch.autograd.Function):
    """forward/backward of SimMLM_SurvivalNet on the engine's eager path; backward takes gradients on all five outputs."""

    @staticmethod
    def forward(ctx, anchor, model, ct, rna, clinical, mask):
        eng = engine_of(model)
        P = eng.plan(rna.shape[0], tuple(ct.shape[-3:]))
        eng.load_batch(P, ct, rna, clinical, mask)
        eng._forward(P, model.training)
        ctx.eng, ctx.P, ctx.train, ctx.serial = eng, P, model.training, P.fwd_serial
        hz = P.buf["hz"]
        return hz[:, 0].clone(), hz[:, 1].clone(), hz[:, 2].clone(), hz[:, 3].clone(), P.gatew.clone()

    @staticmethod
    def backward(ctx, d0, d1, d2, d3, dgate):
        if not ctx.train:
            raise RuntimeError("backward through an eval-mode forward is not supported (BN batch statistics)")
        eng, P = ctx.eng, ctx.P
        _claim_backward(P, ctx.serial)
        if eng.params[0].grad is None:
            eng.gflat.zero_()
            eng.attach_grads()
        dh = P.dbuf["hz"]
        for c, d in enumerate((d0, d1, d2, d3)):
            if d is None:
                dh[:, c].zero_()
            else:
                dh[:, c].copy_(d)
        ext = dgate.contiguous() if dgate is not None else None
        P.moe_bwd[1].dgate_ext = ext.data_ptr() if ext is not None else None
        eng._backward_from_dhz(P)
        P.moe_bwd[1].dgate_ext = None
        _next_dropout_masks(eng)
        return None, None, None, None, None, None


class SimMLM_SurvivalNet(nn.Module):
    """generate_km_curves.py:158-281: one expert per modality (CT, RNA-seq, clinical), each with its own Cox head; a gate MLP on the
    masked features and the mask with a -inf masked softmax; the ensemble Cox head reads the gate-weighted SUM of the masked
    expert features.  Sub-module names and parameter creation order are the reference's (a seeded construction draws its weights).
    forward(image, rnaseq, clinical, mask) -> (ensemble_hazard [B], {'image', 'rnaseq', 'clinical'}: hazards [B], gate_weights [B, 3]).
    A row whose mask is all zero yields NaN gate weights and ensemble hazard (as in torch); its gate / mixture gradient is defined as 0
    (include/mmsurv.h MoeP)."""

    def __init__(self, rna_dim=5005, clinical_dim=1, feature_dim=128):
        super().__init__()
        # the heads read feature rows of width feature_dim; the fallback encoder's last convolution is fixed at 128 channels in the
        # reference (its ModalityExpert ignores output_dim there), so the fallback branch exists at 128 only
        if feature_dim % 4 != 0 or feature_dim <= 0:
            raise ValueError("feature_dim must be a positive multiple of 4 (16-byte aligned feature columns)")
        if not USE_MONAI and feature_dim != 128:
            raise ValueError("the fallback CT encoder (USE_MONAI = False) produces 128 features: feature_dim must be 128")
        self.expert_image = _MoeExpert("image", output_dim=feature_dim)
        self.expert_rnaseq = _MoeExpert("rnaseq", input_dim=rna_dim, output_dim=feature_dim)
        self.expert_clinical = _MoeExpert("clinical", input_dim=clinical_dim, output_dim=feature_dim)
        self.gating = _MoeGate(feature_dim=feature_dim, num_modalities=3)
        self.ensemble_cox = nn.Linear(feature_dim, 1)
        self.feature_dim = feature_dim
        self.use_monai = USE_MONAI

    def forward(self, image, rnaseq, clinical, mask):
        if not rnaseq.is_cuda or not image.is_cuda:
            raise RuntimeError("SimMLM_SurvivalNet (HIP): inputs must be on an MI355X device; there is no CPU fallback")
        anchor = next(self.parameters())
        if torch.is_grad_enabled() and self.training:
            h, hi, hr, hc, g = _MoeNet.apply(anchor, self, image, rnaseq, clinical, mask)
        else:
            eng = engine_of(self)
            P = eng.plan(rnaseq.shape[0], tuple(image.shape[-3:]))
            eng.load_batch(P, image, rnaseq, clinical, mask)
            eng._forward(P, self.training)
            hz = P.buf["hz"]
            h, hi, hr, hc, g = hz[:, 0].clone(), hz[:, 1].clone(), hz[:, 2].clone(), hz[:, 3].clone(), P.gatew.clone()
        return h, {'image': hi, 'rnaseq': hr, 'clinical': hc}, g
