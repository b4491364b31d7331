"""CPU replica of the fine-tuning optimiser step (TuneP, include/mmsurv.h; csrc/finetune.hip), written from its rules, not from the kernel:

per segment s with the base hyper-parameters (lr, b1, b2, eps, wd, max_norm):  lr_s = lr * lr_mult_s,  wd_s = wd * wd_mult_s,  l_s = l2sp_s;
lr_mult_s = 0 freezes the segment -- p, m, v untouched, its gradient outside the global norm, no decay;
coef = min(1, max_norm / (||g_trainable|| + 1e-6))  (torch.nn.utils.clip_grad_norm_ over the parameters that have a gradient);
Adam:  g <- coef g + wd_s w + l_s (w - w0);   AdamW:  w <- w - lr_s wd_s w - lr_s l_s (w - w0), both terms from the old w;  then Adam's step
with ONE step counter t.  fp32 arithmetic (torch CPU), the norm in fp64.  `hyper` is taken as given: a comparison with the kernels passes the
fp32-rounded values they read from AdamP.hyper (with m, v not starting from zero, 1 - 0.999 against 1 - fp32(0.999) is a 1.3e-5 relative
difference of the second bias correction that nothing cancels).
"""
import math

import torch


def trainable_mask(n, bounds, lr_mult):
    mask = torch.zeros(n, dtype=torch.bool)
    for s in range(len(lr_mult)):
        if float(lr_mult[s]) > 0:
            mask[int(bounds[s]):int(bounds[s + 1])] = True
    return mask


def trainable_sumsq(g, bounds, lr_mult):
    """fp64 sum of squares of the trainable gradients"""
    mask = trainable_mask(g.numel(), bounds, lr_mult)
    return float((g.double()[mask] ** 2).sum())


def step(p, g, m, v, t, bounds, lr_mult, wd_mult, l2sp, hyper, adamw, anchor=None):
    """One step in place on the CPU fp32 tensors p, m, v (g is read); t = the step number AFTER this step (1, 2, ...)."""
    lr, b1, b2, eps, wd, maxn = (float(x) for x in hyper)
    norm = math.sqrt(trainable_sumsq(g, bounds, lr_mult))
    coef = min(1.0, maxn / (norm + 1e-6)) if maxn > 0 else 1.0
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    for s in range(len(lr_mult)):
        lm, wm, l2 = float(lr_mult[s]), float(wd_mult[s]), float(l2sp[s])
        if lm == 0.0:
            continue
        sl = slice(int(bounds[s]), int(bounds[s + 1]))
        lr_s, wd_s = lr * lm, wd * wm
        w, gs = p[sl].clone(), g[sl] * coef
        pull = (w - anchor[sl]) if l2 > 0 else torch.zeros_like(w)
        if adamw:
            w = w - (lr_s * wd_s) * w - (lr_s * l2) * pull
        else:
            gs = gs + wd_s * w + l2 * pull
        m[sl] = b1 * m[sl] + (1 - b1) * gs
        v[sl] = b2 * v[sl] + (1 - b2) * gs * gs
        p[sl] = w - (lr_s / bc1) * m[sl] / (v[sl].sqrt() / math.sqrt(bc2) + eps)
