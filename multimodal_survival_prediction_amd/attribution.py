"""Input-gradient attribution of a trained (eval-mode) survival model: which CT voxels, which genes and how much of each modality drove
a patient's log-hazard.  The reference gets these from torch autograd (`ct.requires_grad_(); hazard[b].backward()`); here they come from
SurvivalEngine.attribute -- eval forward, heads' backward with frozen statistics, the encoder's input-gradient driver
(mms_dn121_input_grad / mms_fb3_input_grad, include/mmsurv.h).  Everything below is host-side bookkeeping on its result.

A `batch` is a dict with any of the keys ct (or image) [B, 1, D, H, W], rna (or rnaseq) [B, rna_dim], clinical [B, clinical_dim],
mask [B, 3] (ct | rna | clinical flags; absent = every modality present).
"""
import numpy as np
import torch

_ALIASES = {"ct": ("ct", "image"), "rna": ("rna", "rnaseq"), "clinical": ("clinical",), "mask": ("mask",)}


def _get(batch, key):
    for k in _ALIASES[key]:
        if batch.get(k) is not None:
            return batch[k]
    return None


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def attribute(model, batch, wrt=("ct", "rna", "clinical")):
    """SurvivalEngine.attribute of `model` on `batch`, with the arguments each model class takes (FlexibleMultimodalModel: the mask's
    first two columns)."""
    from .engine import engine_of
    kind = type(model).__name__
    ct, rna, clin, mask = _get(batch, "ct"), _get(batch, "rna"), _get(batch, "clinical"), _get(batch, "mask")
    eng = engine_of(model)
    if kind == "RNASeqSurvivalModel":
        return eng.attribute(None, rna, wrt=wrt)
    if kind == "ImageOnlyModel":
        return eng.attribute(ct, wrt=wrt)
    if kind == "SimpleFusionModel":
        return eng.attribute(ct, rna, wrt=wrt)
    if kind == "FlexibleMultimodalModel":
        return eng.attribute(ct, rna, mask=None if mask is None else mask[:, :2], wrt=wrt)
    if kind == "MultiModalSurvivalNet":
        return eng.attribute(ct, rna, clin, wrt=wrt)
    return eng.attribute(ct, rna, clin, mask=mask, wrt=wrt)          # PartialModalityNet; SimMLM_SurvivalNet raises there


def saliency(model, batch, kind="grad"):
    """-> the attribute() dict; kind = "grad": the raw input gradients, "grad_x_input": each gradient times its input, element-wise."""
    if kind not in ("grad", "grad_x_input"):
        raise ValueError("saliency: kind is 'grad' or 'grad_x_input', got %r" % (kind,))
    res = attribute(model, batch)
    if kind == "grad_x_input":
        for k in ("ct", "rna", "clinical"):
            x = _get(batch, k)
            if res.get(k) is not None and x is not None:
                res[k] = res[k] * x.to(res[k].device).reshape(res[k].shape)
    return res


def gene_scores(model, batch, names=None, top=50):
    """Mean |d hazard / d rna| per gene over the rows that have RNA (mask column 1; every row without a mask) -> the `top` genes as a
    list of (name, score), largest first.  model: a model, or the dict attribute() returned for this batch.  names: gene names
    (default g0, g1, ...)."""
    res = model if isinstance(model, dict) else attribute(model, batch, wrt=("rna",))
    if res.get("rna") is None:
        raise ValueError("gene_scores: the model has no RNA input")
    g = np.abs(_np(res["rna"]).astype(np.float64))
    mask = _get(batch, "mask") if batch is not None else None
    rows = np.ones(g.shape[0], dtype=bool) if mask is None else _np(mask)[:, 1] != 0
    if not rows.any():
        raise ValueError("gene_scores: no row of the batch has RNA")
    score = g[rows].mean(0)
    names = ["g%d" % i for i in range(g.shape[1])] if names is None else list(names)
    if len(names) != g.shape[1]:
        raise ValueError("gene_scores: %d names for %d genes" % (len(names), g.shape[1]))
    order = np.argsort(-score, kind="stable")[:max(0, int(top))]
    return [(names[i], float(score[i])) for i in order]


def modality_shares(result, batch):
    """Per row: sum |grad x input| of each modality, normalised to 1 -> [B, 3] float64 array (ct | rna | clinical); a modality the model
    does not have, or that is masked, has share 0; a row whose three sums are all 0 is all 0."""
    cols = []
    n = None
    for k in ("ct", "rna", "clinical"):
        g, x = result.get(k), _get(batch, k)
        if g is None or x is None:
            cols.append(None)
            continue
        g = _np(g).astype(np.float64)
        x = _np(x).astype(np.float64).reshape(g.shape)
        n = g.shape[0]
        cols.append(np.abs(g * x).reshape(n, -1).sum(1))
    if n is None:
        raise ValueError("modality_shares: result and batch share no modality")
    s = np.stack([c if c is not None else np.zeros(n) for c in cols], 1)
    tot = s.sum(1, keepdims=True)
    return np.divide(s, tot, out=np.zeros_like(s), where=tot > 0)


def encoder_input_grad(encoder, x, dout):
    """The encoders alone, eval mode: -> (features [B, F], dx like x) with dx = gradient of (features * dout).sum() with respect to the
    volume x [B, 1, D, H, W] under frozen BatchNorm statistics.  encoder: densenet.DenseNet121, or the 3-conv nn.Sequential of
    models._ct_encoder / ImageOnlyModel (mms_fb3_forward + mms_fb3_input_grad on a workspace of its own)."""
    import ctypes
    from . import _lib, ops
    from .densenet import DenseNet121
    from .engine import fallback_widths, scalar_widths_ok
    if isinstance(encoder, DenseNet121):
        return encoder.input_grad(x, dout)
    if encoder.training:
        raise RuntimeError("encoder_input_grad needs eval mode (frozen BatchNorm statistics); call .eval() first")
    widths = fallback_widths(encoder)
    if not scalar_widths_ok(widths):
        raise ValueError("3-conv CT encoder widths %s: the input-gradient kernels take widths that divide 256" % (widths,))
    lib = _lib.load_library()
    x = x.contiguous().float()
    dout = dout.contiguous().float()
    B, _, D, H, W = x.shape
    w = (ctypes.c_int * 3)(*widths)
    nbytes = ctypes.c_size_t(0)
    _lib.check(lib.mms_fb3_workspace_bytes(w, B, D, H, W, ctypes.byref(nbytes)), "mms_fb3_workspace_bytes")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=x.device)
    params, bufs = list(encoder.parameters()), list(encoder.buffers())
    ptab = (ctypes.c_void_p * 12)(*[p.data_ptr() for p in params])
    btab = (ctypes.c_void_p * 9)(*[b.data_ptr() for b in bufs])
    st = ops.stream()
    out = torch.empty(B, widths[2], device=x.device)
    dx = torch.empty_like(x)
    _lib.check(lib.mms_fb3_init(ws.data_ptr(), nbytes.value, w, B, D, H, W, btab, st), "mms_fb3_init")
    _lib.check(lib.mms_fb3_forward(ws.data_ptr(), nbytes.value, w, B, D, H, W, x.data_ptr(), ptab, btab, out.data_ptr(), out.stride(0), 0, st),
               "mms_fb3_forward")
    _lib.check(lib.mms_fb3_input_grad(ws.data_ptr(), nbytes.value, w, B, D, H, W, x.data_ptr(), ptab, btab, dout.data_ptr(), dout.stride(0),
                                      dx.data_ptr(), st), "mms_fb3_input_grad")
    return out, dx
