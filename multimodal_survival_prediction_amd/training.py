"""train_epoch / validate of the reference's scripts, driving the fused HIP-graph step.

Signatures are the reference's: train_epoch(model, loader, optimizer, device) / validate(model, loader, device)
(final_multimodal.py:238-305, partial_modality_training.py:382-485, simple_fusion.py:242-333, flexible_multimodal.py:262-357,
train_rnaseq_only.py:157-209; "simmlm" and "image" are project-defined).  `optimizer` may be
  * a `FusedOptimizer` (below): the whole step -- zero-grad, forward, Cox loss, backward, clip_grad_norm_(1.0),
    Adam/AdamW -- is ONE replayed HIP graph per batch, losses accumulate on the device, one host sync per epoch;
  * any torch.optim optimizer ("final" and "image" only): the reference's own loop body runs unchanged on the autograd-compatible path.
Batch-skipping rules, loss averaging and return values follow each script exactly.  What differs between the seven loop styles -- model
inputs, targets, skips, the skip flag, the returned mean, validation's rows, batch rule, loss and C-index -- is stated ONCE, as that
style's row of the table `_STYLES`; the eager loops (_train_epoch / _validate behind the public train_epoch_<style> / validate_<style>)
and the lock-step K-fold drivers (train_epoch_lockstep / validate_lockstep) all read it.
"""
import dataclasses

import torch

from . import losses, ops
from .engine import engine_of


class FusedOptimizer:
    """Handle for the engine-resident Adam/AdamW state (drop-in where the scripts build `optim.Adam(...)`)."""

    def __init__(self, model, lr=1e-4, weight_decay=1e-4, adamw=False, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0,
                 gate_entropy_weight=0.01, cox_ties=None, dn_opts=None, expert_weight=0.1, **kw):
        # kw: further SurvivalEngine arguments (finetune=: a transfer.FineTunePlan or its string)
        # (a model that already belongs to a FoldGroupEngine keeps that engine: this object is then just the handle
        # the LR schedulers talk to -- pass the same hyper-parameters to the group's constructor)
        self.engine = engine_of(model, lr=lr, weight_decay=weight_decay, adamw=adamw, betas=betas, eps=eps,
                                max_norm=max_norm, gate_entropy_weight=gate_entropy_weight, cox_ties=cox_ties, dn_opts=dn_opts,
                                expert_weight=expert_weight, **kw)
        self.param_groups = [dict(lr=lr, weight_decay=weight_decay)]

    def set_lr(self, lr):
        self.param_groups[0]["lr"] = lr
        self.engine.set_lr(lr)

    def zero_grad(self, set_to_none=True):
        pass

    def step(self):
        raise RuntimeError("FusedOptimizer steps inside train_epoch's fused graph; call train_epoch(...)")


class ReduceLROnPlateau:
    """optim.lr_scheduler.ReduceLROnPlateau(mode='max', factor, patience) for FusedOptimizer
    (final_multimodal.py:351: default threshold 1e-4 rel, cooldown 0, min_lr 0)."""

    def __init__(self, optimizer, mode="max", factor=0.5, patience=5, threshold=1e-4):
        assert mode == "max"
        self.opt, self.factor, self.patience, self.threshold = optimizer, factor, patience, threshold
        self.best, self.bad = -float("inf"), 0

    def step(self, metric):
        if metric > self.best * (1 + self.threshold) if self.best > 0 else metric > self.best:
            self.best, self.bad = metric, 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            self.opt.set_lr(self.opt.param_groups[0]["lr"] * self.factor)
            self.bad = 0


class CosineAnnealingLR:
    """optim.lr_scheduler.CosineAnnealingLR(T_max) (simple_fusion.py:392), eta_min = 0."""

    def __init__(self, optimizer, T_max):
        import math
        self.opt, self.T, self.base, self.t, self.math = optimizer, T_max, optimizer.param_groups[0]["lr"], 0, math

    def step(self):
        self.t += 1
        self.opt.set_lr(self.base * (1 + self.math.cos(self.math.pi * self.t / self.T)) / 2)


def _t(x, dev):
    return x.to(dev, non_blocking=True) if isinstance(x, torch.Tensor) else torch.as_tensor(x).to(dev)


# ---- the two autograd fallbacks (any torch.optim optimizer: the reference's own loop body) ------------------------------------------
def _train_epoch_final_autograd(model, loader, optimizer, device):
    model.train()
    total, nb = 0.0, 0
    for batch in loader:
        ct, rna, clin = _t(batch['image'], device), _t(batch['rnaseq'], device), _t(batch['clinical'], device)
        label = _t(batch['label'], device)
        hazard = model(ct, rna, clin)
        loss = losses.cox_loss(hazard, label[:, 1], label[:, 0])
        optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        optimizer.step()
        total += loss.item()
        nb += 1
    return total / nb if nb > 0 else 0


def _train_epoch_image_autograd(model, loader, optimizer, device):
    model.train()
    total, nb = 0.0, 0
    for batch in loader:
        ct, label = _t(batch['image'], device), _t(batch['label'], device)
        risk = model(ct)
        loss = losses.cox_loss(risk, label[:, 1], label[:, 0])
        optimizer.zero_grad()
        if ct.shape[0] >= 2 and float(label[:, 1].sum()) > 0:
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            optimizer.step()
        total += loss.item()
        nb += 1
    return total / nb if nb > 0 else 0


# ---- the style table: ONE row per loop style holds everything that differs between the seven ------------------------------------------
def _labelled(batch, device):
    return torch.as_tensor(batch['has_survival'], dtype=torch.bool, device=device)


def _simmlm_rows(batch, device):
    """labelled patients with at least one modality (the ensemble term's set; a row whose mask is all zero has a NaN ensemble hazard)"""
    return _labelled(batch, device) & (_t(batch['mask'], device) != 0).any(1)


@dataclasses.dataclass(frozen=True)
class _Style:
    inputs: tuple                      # model inputs: keywords of the fused step / eval forward, read from the batch keys of _BATCH_KEY
    label: bool                        # targets: batch['label'][:, 0] / [:, 1] (True) or batch['time'] / batch['event'] reshaped to [B] (False)
    loss: str                          # validation loss and C-index: names in `losses`
    cindex: str
    zero: object                       # the mean of nothing: 0 or 0.0, as the style's script returns it
    mask_cols: int = None              # the model sees only the first columns of batch['mask']
    valid: bool = False                # has_survival is passed as `valid`: unlabelled patients stay out of the loss
    pre_skip: bool = False             # fewer than 2 labelled patients: the batch is skipped BEFORE the forward, training and validation
    skip_if_unusable: bool = True      # a batch whose loss is unusable (< 2 patients in it, or no event) takes no optimiser step
    mean_over: str = "n_batches"       # training result: sum_loss / this count of epoch_stats() ...
    entropy: bool = False              # ... paired with sum_entropy / n_batches
    rows: object = None                # validation: (batch, device) -> the rows that count; None = all
    counts: str = "every"              # validation: a batch counts always ("every"), with >= 2 selected rows and an event ("two_and_event"), or with an event ("event")
    named: bool = False                # validate_lockstep has the named-batch path (_validate_lockstep_named) for it
    autograd: object = None            # train_epoch_<style> with a torch.optim optimizer
    needs: str = "a FusedOptimizer"    # ... or the TypeError's advice


_BATCH_KEY = dict(ct='image', rna='rnaseq', clinical='clinical', mask='mask')
_COX = dict(label=True, loss="cox_loss", cindex="calculate_cindex", zero=0)                      # final_multimodal.py's family
_NPLL = dict(label=False, loss="neg_partial_log_likelihood", cindex="ConcordanceIndex", zero=0.0)   # simple_fusion.py's family
_STYLES = {
    # degenerate batch: loss 0 without graph -> no update (final_multimodal.py:173-176)
    "final": _Style(("ct", "rna", "clinical"), **_COX, named=True, autograd=_train_epoch_final_autograd),
    # entropy term: every batch steps (partial_modality_training.py:418-428)
    "partial": _Style(("ct", "rna", "clinical", "mask"), **_COX, valid=True, skip_if_unusable=False, mean_over="n_usable", entropy=True,
                      rows=_labelled, counts="two_and_event", named=True),
    # project-defined: a batch whose ensemble term is unusable takes no step
    "simmlm": _Style(("ct", "rna", "clinical", "mask"), **_COX, valid=True, mean_over="n_usable", rows=_simmlm_rows,
                     counts="two_and_event"),
    # project-defined: final_multimodal.py's rules on the image alone
    "image": _Style(("ct",), **_COX, autograd=_train_epoch_image_autograd),
    # `continue` before the forward (simple_fusion.py:257-258); no events: forward ran (BN stats moved), no update (:267-268)
    "simple": _Style(("ct", "rna"), **_NPLL, valid=True, pre_skip=True, mean_over="n_usable", rows=_labelled, counts="event", named=True),
    # flexible_multimodal.py:276-277 / :287-288
    "flexible": _Style(("ct", "rna", "mask"), **_NPLL, mask_cols=2, valid=True, pre_skip=True, mean_over="n_usable", rows=_labelled,
                       counts="event"),
    # a batch without events yields loss 0 / zero gradients, and still steps (train_rnaseq_only.py:168-172)
    "rnaseq": _Style(("rna",), **_NPLL, skip_if_unusable=False, needs="a FusedOptimizer(model, adamw=True, max_norm=0)"),
}


def has_named_validation(style):
    """validate_lockstep evaluates lazily NAMED batches of this style with one gather + one graph per lock-step position."""
    return _STYLES[style].named


def styles_without_mask():
    """The styles whose models take no modality mask (augment.MASKLESS_STYLES)."""
    return tuple(s for s, row in _STYLES.items() if "mask" not in row.inputs)


def _n_labelled(batch):
    return sum(bool(x) for x in batch['has_survival'])


def _model_inputs(row, batch):
    """-> keyword inputs of the model, or None when the script skips the batch before the forward."""
    if row.pre_skip and _n_labelled(batch) < 2:
        return None
    kw = {k: batch[_BATCH_KEY[k]] for k in row.inputs}
    if row.mask_cols:
        kw["mask"] = kw["mask"][:, :row.mask_cols]
    return kw


def _batch_size(kw):
    return int((kw["rna"] if "rna" in kw else kw["ct"]).shape[0])


def _targets(row, batch, device=None):
    """-> (time, event) of the batch: as the batch holds them (training), or on `device` (validation)."""
    if row.label:
        label = batch['label'] if device is None else _t(batch['label'], device)
        return label[:, 0], label[:, 1]
    time, event = batch['time'].reshape(-1), batch['event'].reshape(-1)
    return (time, event) if device is None else (_t(time, device), _t(event, device).float())


def _train_kwargs(style, batch):
    """-> keyword arguments of the fused step, or None when the script skips the batch before the forward.  The only place that turns a
    batch into step arguments: the eager loop and train_epoch_lockstep both call it."""
    row = _STYLES[style]
    kw = _model_inputs(row, batch)
    if kw is None:
        return None
    kw["time"], kw["event"] = _targets(row, batch)
    if row.valid:
        kw["valid"] = torch.as_tensor(batch['has_survival'], dtype=torch.float32)
    return kw


def _train_result(row, st):
    """What train_epoch_<style> returns for the epoch statistics st."""
    avg = st["sum_loss"] / st[row.mean_over] if st[row.mean_over] > 0 else row.zero
    return (avg, st["sum_entropy"] / st["n_batches"] if st["n_batches"] > 0 else row.zero) if row.entropy else avg


def _train_epoch(style, model, loader, optimizer, device):
    row = _STYLES[style]
    if not isinstance(optimizer, FusedOptimizer):
        if row.autograd is None:
            raise TypeError(f"train_epoch_{style} drives the fused step; pass {row.needs}")
        return row.autograd(model, loader, optimizer, device)
    model.train()
    eng = optimizer.engine
    eng.reset_epoch_stats()
    for batch in loader:
        kw = _train_kwargs(style, batch)
        if kw is not None:
            eng.train_step(**kw, skip_if_unusable=row.skip_if_unusable)
    return _train_result(row, eng.epoch_stats())


def _score_batch(row, batch, hz, device):
    """One validation batch after its forward -> (loss, hazards, times, events) of the rows that count, or None when the batch does not."""
    t, e = _targets(row, batch, device)
    if row.rows is not None:
        keep = row.rows(batch, device)
        hz, t, e = hz[keep], t[keep], e[keep]
    if row.counts == "two_and_event" and not (hz.shape[0] >= 2 and float(e.sum()) > 0):
        return None
    if row.counts == "event" and float(e.sum()) == 0:
        return None
    h = hz.clone()                                  # hz is a view of a static buffer
    return getattr(losses, row.loss)(h, e, t).item(), h, t, e


def _cindex(row, H, E, T):
    f = getattr(losses, row.cindex)
    return f()(H, E, T).item() if row.cindex == "ConcordanceIndex" else f(H, E, T)


def _val_result(row, scored):
    """(mean loss, C-index) of one model's validation pass: scored = what _score_batch returned for its batches."""
    scored = [s for s in scored if s is not None]
    if not scored:
        return row.zero, 0.5
    loss, hs, ts, es = zip(*scored)
    return sum(loss) / len(loss), _cindex(row, torch.cat(hs), torch.cat(es), torch.cat(ts))


def _validate(style, model, loader, device):
    row = _STYLES[style]
    model.eval()
    eng = engine_of(model)
    scored = []
    for batch in loader:
        kw = _model_inputs(row, batch)
        if kw is not None:
            scored.append(_score_batch(row, batch, eng.forward_eval(**kw)[0], device))
    eng.check_b4()                  # a timed-out block-4 hand-off must not yield a C-index (no-op without the DenseNet encoder)
    return _val_result(row, scored)


# ---- the reference's names: train_epoch(model, loader, optimizer, device) / validate(model, loader, device) of each script ------------
def train_epoch_final(model, loader, optimizer, device):
    """final_multimodal.py:238-266: Cox loss on the whole batch, clip at 1.0.  -> mean loss over all batches."""
    return _train_epoch("final", model, loader, optimizer, device)


def validate_final(model, loader, device):
    """final_multimodal.py:268-305: every batch counts.  -> (mean of the batches' Cox losses, C-index over all patients)."""
    return _validate("final", model, loader, device)


def train_epoch_partial(model, loader, optimizer, device):
    """partial_modality_training.py:382-435: Cox loss over the labelled patients + the gate-entropy term, every batch steps.
    -> (mean Cox loss over the usable batches, mean gate entropy over all batches)."""
    return _train_epoch("partial", model, loader, optimizer, device)


def validate_partial(model, loader, device):
    """partial_modality_training.py:438-485: a batch counts, and its labelled patients enter the C-index, only when >= 2 of them are
    labelled and one has an event."""
    return _validate("partial", model, loader, device)


def train_epoch_simmlm(model, loader, optimizer, device):
    """SimMLM_SurvivalNet (generate_km_curves.py:158-281; the reference ships no training loop for it).  One epoch of the project-defined
    objective L = cox(ensemble; has_survival) + lambda sum_m cox(h_m; has_survival and mask_m) (lambda = the engine's expert_weight),
    fused step per batch; a batch whose ensemble term is unusable takes no step.  -> mean of L over the usable batches."""
    return _train_epoch("simmlm", model, loader, optimizer, device)


def validate_simmlm(model, loader, device):
    """-> (mean ensemble Cox loss over the usable batches, C-index of the ensemble hazard over their labelled patients); the batch
    rule of validate_partial over the labelled patients WITH at least one modality (a row whose mask is all zero has a NaN ensemble
    hazard: it is left out, as it is left out of the training objective)."""
    return _validate("simmlm", model, loader, device)


def train_epoch_image(model, loader, optimizer, device):
    """ImageOnlyModel (generate_km_curves.py:28-54; the reference ships no training loop for it).  The loop of final_multimodal.py:238-266
    on the image alone (project-defined): a forward on every batch (BatchNorm running statistics move even on a
    degenerate one), Cox loss over the whole batch, clip at 1.0; a batch with fewer than 2 patients or without an event has loss 0 and
    takes no optimiser step.  -> mean loss over all batches."""
    return _train_epoch("image", model, loader, optimizer, device)


def validate_image(model, loader, device):
    """Eval-mode forward of every batch -> (mean of the batches' Cox losses, C-index by pair counts over all patients)."""
    return _validate("image", model, loader, device)


def train_epoch_simple(model, loader, optimizer, device):
    """simple_fusion.py:242-279: batches with < 2 labelled patients are skipped before the forward (:257-258), batches without an event
    after it (:267-268).  -> mean loss over the stepped batches."""
    return _train_epoch("simple", model, loader, optimizer, device)


def validate_simple(model, loader, device):
    """simple_fusion.py:281-333: the two skips of the training loop; (0.0, 0.5) when no batch counts."""
    return _validate("simple", model, loader, device)


def train_epoch_flexible(model, loader, optimizer, device):
    """flexible_multimodal.py:262-303 (rows of SURVEY section 8f: same kernels, learnable missing-modality bias): the simple_fusion loop
    with the (B,2) modality mask as a third model input."""
    return _train_epoch("flexible", model, loader, optimizer, device)


def validate_flexible(model, loader, device):
    """flexible_multimodal.py:305-357."""
    return _validate("flexible", model, loader, device)


def train_epoch_rnaseq(model, loader, optimizer, device):
    """train_rnaseq_only.py:157-176: NPLL on the whole batch, every batch steps, NO gradient clipping (build the
    FusedOptimizer with max_norm=0), mean over len(loader)."""
    return _train_epoch("rnaseq", model, loader, optimizer, device)


def validate_rnaseq(model, loader, device):
    """train_rnaseq_only.py:178-209; (0.0, 0.5) on an empty loader."""
    return _validate("rnaseq", model, loader, device)


# ---- K folds in lock-step (fold groups) ------------------------------------------------------------------------------
# The reference trains its folds one after the other; they are independent, so a FoldGroupEngine advances all of them by
# one batch with ONE launch sequence (fold_group.py).  Per fold, batch order, skipping rules, loss averaging and return
# values are those of train_epoch_<style> / validate_<style> above, read from the same table rows; only the interleaving
# of the folds differs.
def _lockstep(loaders, members):
    """Yield, batch position by batch position, {member: batch} of the folds that still have a batch."""
    its = {g: iter(l) for g, l in zip(members, loaders)}
    while its:
        out = {}
        for g in list(its):
            b = next(its[g], None)
            if b is None:
                del its[g]
            else:
                out[g] = b
        if out:
            yield out


def train_epoch_lockstep(group, loaders, style, members=None, concurrent=1):
    """One epoch of the folds `members` (default: all) of a FoldGroupEngine, each on its own loader.
    concurrent = n >= 2: the members are split into n fixed sub-groups that step as n lock-step sub-groups on n HIP streams
    (one sub-group's latency-bound kernels overlap the others').  Every member's loader is iterated under its sub-group's
    stream, so batch tensors are allocated and consumed on the same stream.
    -> per member, what train_epoch_<style> returns for that fold."""
    from .augment import Records             # (augment imports this module's style table)
    row = _STYLES[style]
    members = tuple(range(len(group))) if members is None else tuple(members)
    for g in members:
        group.engines[g].model.train()
        group.engines[g].reset_epoch_stats()

    for ld in loaders:                       # augmentation specs (data.BatchLoader(augment=)) are checked against THIS style
        if getattr(ld, "augment", None) is not None:
            ld.augment.validate(style)
            ld.augment_style = style

    def advance(pos):
        lazy = [(g, b) for g, b in pos.items() if "gather" in b]
        if lazy:        # batches named by index (data.BatchLoader(lazy=True)): one gather launch per (sub-)group step
            by = {}
            for g, b in lazy:
                if row.pre_skip and _n_labelled(b) < 2:
                    continue                          # skipped before the forward
                by.setdefault((len(b["index"]), id(b["gather"]), b["augment"].key if "augment" in b else None), []).append((g, b))
            for items in by.values():                 # (named batches that carry augmentation records: applied inside the gather launch)
                aug = Records.stack([b["augment"] for _, b in items]) if "augment" in items[0][1] else None
                group.train_step_indexed(items[0][1]["gather"], torch.stack([torch.as_tensor(b["index"]) for _, b in items]),
                                         members=tuple(g for g, _ in items), skip_if_unusable=row.skip_if_unusable, augment=aug)
            pos = {g: b for g, b in pos.items() if "gather" not in b}
        by_size = {}
        for g, batch in pos.items():
            kw = _train_kwargs(style, batch)
            if kw is not None:
                by_size.setdefault(_batch_size(kw), []).append((g, kw))
        for items in by_size.values():           # a ragged last batch forms its own (sub-)group step
            group.train_step([kw for _, kw in items], members=tuple(g for g, _ in items), skip_if_unusable=row.skip_if_unusable)

    _run_subgroups(group, loaders, members, concurrent, advance)
    if concurrent > 1:
        torch.cuda.synchronize()
    return [_train_result(row, group.engines[g].epoch_stats()) for g in members]


def subgroup_sizes(n_members, concurrent):
    """Sizes of the fixed, contiguous sub-groups n_members lock-step fold models step as on `concurrent` HIP streams: near-equal, at
    most one sub-group per stream, ONE group when there is a single stream or a single member.  Round 3 measurements (K-fold epoch,
    patients/s): 5 members 2 + 2 + 1 on three streams 2740 (3 + 2 on two: 2640); 3 members 1 + 1 + 1: 2136, 2 + 1: 2056, one group of
    3: 1973; 2 members 1 + 1: 1635, one group of 2: 1588 -- what a rank of the K-fold job holds at N = 2 / 4 GPUs.
    MMS_MIN_SPLIT_MEMBERS (default 2): fewest members that are split at all."""
    import os
    min_split = int(os.environ.get("MMS_MIN_SPLIT_MEMBERS", "2"))
    if concurrent <= 1 or n_members < max(min_split, 2):
        return (n_members,)
    nsub = min(int(concurrent), n_members)
    base, extra = divmod(n_members, nsub)
    return tuple(base + (1 if h < extra else 0) for h in range(nsub))


def _run_subgroups(group, loaders, members, concurrent, advance):
    """Lock-step iteration of the members' loaders: as one group, or as the fixed, contiguous sub-groups of subgroup_sizes(), each
    stepping on its own HIP stream (5 folds on 3 streams: 2 + 2 + 1)."""
    sizes = subgroup_sizes(len(members), concurrent)
    if len(sizes) <= 1:
        for pos in _lockstep(loaders, members):
            advance(pos)
        return
    nsub = len(sizes)
    streams = ops.worker_streams(group.device, nsub)
    cuts, o = [], 0
    for n in sizes:
        cuts.append((members[o:o + n], loaders[o:o + n]))
        o += n
    cur = torch.cuda.current_stream()
    for s in streams[:nsub]:
        s.wait_stream(cur)
    its = [_lockstep(ld, mem) for mem, ld in cuts]
    live = [True] * nsub
    while any(live):
        for h in range(nsub):
            if not live[h]:
                continue
            with torch.cuda.stream(streams[h]):
                pos = next(its[h], None)         # the loaders gather their batches on this stream
                if pos is None:
                    live[h] = False
                else:
                    advance(pos)
    for s in streams[:nsub]:
        cur.wait_stream(s)


def _validate_lockstep_named(group, loaders, style, members, concurrent=1):
    """validate_final / validate_partial over lazily NAMED batches (data.BatchLoader(lazy=True), cohort in HBM or pinned host memory):
    per lock-step position one gather launch + one graph (eval-mode forwards, the batches' Cox values, device-side accumulators); the
    hazards stay on the device and the host is synchronised ONCE, at the end (the reference and the eager path sync per batch).
    Bookkeeping as the reference's loops: final -- every batch counts, loss 0 when it has no event (final_multimodal.py:268-305);
    partial -- a batch counts, and its labelled patients enter the C-index, only when >= 2 of them are labelled and one has an event
    (partial_modality_training.py:438-485); simple -- the same rule (simple_fusion.py:314-349 skips batches with < 2 labelled
    patients before the forward and those without an event after it: in eval mode the skipped forward has no side effect), the
    C-index through ConcordanceIndex as the eager path."""
    dev = group.device
    for g in members:
        group.engines[g].model.eval()
        group.engines[g].acc_eval.zero_()
    n_rows = {g: len(ld.idx) for g, ld in zip(members, loaders)}
    n_bat = {g: len(ld) for g, ld in zip(members, loaders)}
    hz = {g: torch.zeros(n_rows[g], device=dev) for g in members}
    flags = {g: torch.zeros(max(n_bat[g], 1), 2, device=dev) for g in members}
    order = {g: [] for g in members}          # (patient indices, labelled flags) of the batches in the order they were evaluated
    off = {g: 0 for g in members}
    def advance(pos):
        by = {}
        for g, b in pos.items():
            by.setdefault((len(b["index"]), id(b["gather"])), []).append((g, b))
        for items in by.values():
            outs = group.eval_loss_step_indexed(items[0][1]["gather"], torch.stack([torch.as_tensor(b["index"]) for _, b in items]),
                                                members=tuple(g for g, _ in items))
            for (g, b), (h, lf) in zip(items, outs):
                n = len(b["index"])
                hz[g][off[g]:off[g] + n].copy_(h)
                flags[g][len(order[g])].copy_(lf)
                order[g].append((torch.as_tensor(b["index"]), torch.as_tensor(b["has_survival"], dtype=torch.bool)))
                off[g] += n

    _run_subgroups(group, loaders, members, concurrent, advance)
    torch.cuda.synchronize()
    for g in members:
        group.engines[g].check_b4()          # the pass's single sync point: a timed-out block-4 hand-off must not yield a C-index
    row, out = _STYLES[style], []
    for g, ld in zip(members, loaders):
        a = group.engines[g].acc_eval.tolist()
        if not order[g]:
            out.append((row.zero, 0.5))
            continue
        lab = ld.c["label"]
        idx = torch.cat([i for i, _ in order[g]])
        if row.counts == "every":
            keep = torch.ones(len(idx), dtype=torch.bool)
            avg = a[0] / a[3] if a[3] > 0 else row.zero
        else:
            usable = flags[g][:len(order[g]), 1].cpu() > 0
            keep = torch.cat([m & bool(u) for (_, m), u in zip(order[g], usable)])
            avg = a[0] / a[1] if a[1] > 0 else row.zero
        if not bool(keep.any()):
            out.append((row.zero, 0.5))
            continue
        sel = idx[keep].to(lab.device)
        H, T, E = hz[g][keep.to(dev)], lab[sel, 0].to(dev), lab[sel, 1].to(dev)
        out.append((avg, _cindex(row, H, E.float(), T)))
    return out


def validate_lockstep(group, loaders, style, device, members=None, concurrent=1):
    """validate_<style> of the folds `members`, their eval forwards issued as fold-group launches.
    -> per member (val_loss, c_index).  Loaders that NAME their batches (styles with has_named_validation) take _validate_lockstep_named;
    concurrent = n: as train_epoch_lockstep, n sub-groups on n HIP streams (that path only)."""
    row = _STYLES[style]
    members = tuple(range(len(group))) if members is None else tuple(members)
    loaders = [ld.without_augment() if hasattr(ld, "without_augment") else ld for ld in loaders]       # validation is never augmented
    if row.named and all(getattr(ld, "lazy", False) for ld in loaders):
        return _validate_lockstep_named(group, loaders, style, members, concurrent)
    scored = {g: [] for g in members}
    for g in members:
        group.engines[g].model.eval()
    for pos in _lockstep(loaders, members):
        by_size = {}
        for g, batch in pos.items():
            kw = _model_inputs(row, batch)
            if kw is not None:
                by_size.setdefault(_batch_size(kw), []).append((g, kw, batch))
        for items in by_size.values():
            outs = group.forward_eval([kw for _, kw, _ in items], members=tuple(g for g, _, _ in items))
            for (g, _, batch), (hz, _gate) in zip(items, outs):
                scored[g].append(_score_batch(row, batch, hz, device))
    for g in members:
        group.engines[g].check_b4()
    return [_val_result(row, scored[g]) for g in members]
