"""Shared driver pieces of the three entry points (synthetic cohort, K-fold loop, result JSON)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def env_int(name, default):
    return int(os.environ.get(name, default))


def env_float(name, default):
    return float(os.environ.get(name, default))


def env_dims(default=(64, 64, 32)):
    """MMS_VOLUME="D,H,W": CT volume size of the synthetic cohort (default: the reference's target_size 64,64,32)."""
    v = os.environ.get("MMS_VOLUME")
    return tuple(int(x) for x in v.split(",")) if v else tuple(default)


def augment_spec(style):
    """MMS_AUGMENT="flip=0.5,shift=2:4:4,scale=0.9:1.1,offset=-0.05:0.05,moddrop=0.2,seed=0" (unset by default): GPU batch
    augmentation of the TRAINING loaders (multimodal_survival_prediction_amd.augment) -> AugmentSpec checked against the model
    style (moddrop needs a model that takes a modality mask), or None."""
    v = os.environ.get("MMS_AUGMENT")
    if not v:
        return None
    from multimodal_survival_prediction_amd.augment import AugmentSpec
    return AugmentSpec.parse(v).validate(style, env_dims())


def augment_hparams(spec):
    """-> {"augment": "<spec>"} for cv_results.json's hyperparameters; nothing when augmentation is off (today's JSON unchanged)."""
    return {} if spec is None else {"augment": str(spec)}


def select_genes(cohort, train_indices_per_fold, ckpt_path, fold_names=None, rank=0):
    """MMS_SELECT_GENES=k (unset or 0 by default: off, nothing changes): per-fold gene selection by a univariate Cox score screen of each
    fold's TRAINING patients (multimodal_survival_prediction_amd.gene_select), with MMS_SELECT_STABILITY=R bootstrap resamples per fold
    (default 0) drawn from MMS_SELECT_SEED (default 0).  Selects for every fold, leaves the per-fold [N, k] matrices in the cohort
    (GeneSelection.apply: loaders take fold=, the fold group folds=) and, on rank 0, writes fold_{name}_genes.json next to each
    checkpoint ckpt_path(name) (name = fold_names[f], default f + 1).  -> GeneSelection, or None when off."""
    k = env_int("MMS_SELECT_GENES", 0)
    if k <= 0:
        return None
    from multimodal_survival_prediction_amd import gene_select
    sel = gene_select.select_genes(cohort, train_indices_per_fold, k, stability=env_int("MMS_SELECT_STABILITY", 0),
                                   seed=env_int("MMS_SELECT_SEED", 0))
    sel.apply(cohort)
    if rank == 0:
        for f in range(len(sel.columns)):
            name = f + 1 if fold_names is None else fold_names[f]
            d = os.path.dirname(ckpt_path(name)) or "."
            os.makedirs(d, exist_ok=True)
            sel.save(os.path.join(d, f"fold_{name}_genes.json"), fold=f)
        print(f"gene selection: top {k} of {sel.n_genes} genes per fold (stability {sel.stability}, seed {sel.seed}); "
              f"rows screened {sel.rows_screened}", flush=True)
    return sel


def rna_width(sel, name="rna_dim"):
    """Constructor keyword of a model that reads the selected genes: {name: k}; nothing when selection is off (the class default)."""
    return {} if sel is None else {name: sel.k}


def gene_hparams(sel):
    """-> {"select_genes": k, ...} for cv_results.json's hyperparameters; nothing when selection is off (today's JSON unchanged)."""
    return {} if sel is None else {"select_genes": sel.k, "select_stability": sel.stability, "select_seed": sel.seed}


class Transfer:
    """Transfer learning of an entry point (multimodal_survival_prediction_amd.transfer), all unset by default -- the script then behaves
    and writes exactly as before:
      MMS_PRETRAINED=PATH        checkpoint each fold's model starts from (load_pretrained); `{fold}` in it is the fold's name (1, 2, ...)
      MMS_PRETRAINED_GENES=FILE  the source panel's gene names in the source's column order (transfer.read_genes); with it a first RNA
                                 layer of another width is aligned by gene name against the cohort's genes (its `gene_names`, else
                                 transfer.default_gene_names; a fold's selected columns under MMS_SELECT_GENES)
      MMS_FINETUNE=SPEC          FineTunePlan.parse: frozen stages / segments, learning-rate multipliers, L2-SP
    apply(model, fold name, fold id) loads and logs; engine_kw goes to FusedOptimizer / FoldGroupEngine; record() is the `transfer` entry
    of cv_results.json ({} when nothing is set)."""

    def __init__(self, cohort=None, sel=None, rank=0):
        from multimodal_survival_prediction_amd import transfer
        self.path = os.environ.get("MMS_PRETRAINED") or None
        gfile = os.environ.get("MMS_PRETRAINED_GENES") or None
        self.genes_file = gfile
        self.source_genes = transfer.read_genes(gfile) if gfile else None
        spec = os.environ.get("MMS_FINETUNE") or None
        self.plan = transfer.FineTunePlan.parse(spec) if spec else None
        self.cohort, self.sel, self.rank, self.folds, self.described = cohort, sel, rank, [], False
        self.engine_kw = {} if self.plan is None else {"finetune": self.plan}

    def _target_genes(self, fold_id):
        from multimodal_survival_prediction_amd import transfer
        if self.source_genes is None or self.cohort is None or "rnaseq" not in self.cohort:
            return None
        names = self.cohort.get("gene_names") or transfer.default_gene_names(self.cohort["rnaseq"].shape[1])
        if self.sel is not None:
            names = [names[int(c)] for c in self.sel.columns_of(fold_id)]
        return names

    def apply(self, model, fold_name, fold_id=None):
        from multimodal_survival_prediction_amd import transfer
        if self.path is not None:
            rep = transfer.load_pretrained(model, self.path.replace("{fold}", str(fold_name)), source_genes=self.source_genes,
                                           target_genes=self._target_genes(fold_id))
            print(f"[rank {self.rank}] fold {fold_name}: {rep}", flush=True)
            self.folds.append(dict(fold=fold_name, **rep.as_dict()))
        if self.plan is not None and not self.described:
            print(f"[rank {self.rank}] fine-tuning plan {self.plan.spec()!r}:\n{self.plan.describe(model)}", flush=True)
            self.described = True

    def record(self):
        if self.path is None and self.plan is None:
            return {}
        rec = {}
        if self.path is not None:
            rec.update(pretrained=self.path, pretrained_genes=self.genes_file, folds=self.folds)
        if self.plan is not None:
            rec["finetune"] = self.plan.spec()
        return {"transfer": rec}


def setup_device():
    from multimodal_survival_prediction_amd import distributed as D
    world, rank, local = D.init()
    if not torch.cuda.is_available():
        raise SystemExit("these entry points run the HIP hot path and need an MI355X (no CPU fallback)")
    torch.cuda.set_device(local)
    return world, rank, torch.device("cuda", local)


def save_json(path, obj):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(obj, f, indent=2)


def load_or_make_cohort(device, **make_kw):
    """The reference reads data/processed/{full_matching_table.csv, rnaseq_normalized_mapped.csv} relative to the cwd.  If that
    contract is present (real data as it is -- nifti_path naming the .nii.gz volumes of convert_dicom_to_nifti.py, relative paths
    resolved against the cwd, then MMS_DATA_ROOT -- or a cohort written by cohort_io.write_cohort, .npy volumes included) it is loaded
    ONCE into an HBM-resident store with the volume preprocessing done on the GPU; otherwise a seeded synthetic cohort is built."""
    from multimodal_survival_prediction_amd import cohort_io, data
    root = os.environ.get("MMS_DATA_ROOT", ".")
    if os.path.exists(os.path.join(root, cohort_io.TABLE)):
        print(f"loading cohort from {os.path.join(root, cohort_io.TABLE)}", flush=True)
        return cohort_io.load_cohort(root, device, target_size=make_kw.get("dims", (64, 64, 32)))
    return data.cohort_to(data.make_cohort(**make_kw), device)


def data_mod():
    from multimodal_survival_prediction_amd import data
    return data


def lockstep_enabled(n_local_folds, batch_size=None):
    """Folds of this rank train in lock-step as one fold group (MMS_LOCKSTEP=0 restores fold-after-fold order).  batch_size: fold
    groups are limited to 32 rows per model (FoldGroupEngine.plan); above that the folds run one after the other, one engine each."""
    if batch_size is not None and batch_size > 32:
        return False
    return env_int("MMS_LOCKSTEP", 1) != 0 and 2 <= n_local_folds <= 10


def cv_lockstep(style, models, loaders, group_kw, num_epochs, patience, make_scheduler, ckpt_path, device, rank, fold_names,
                log_every=5, fold_ids=None, transfer=None):
    """The per-fold epoch loop of the three scripts (train, validate, scheduler, best-checkpoint, early stopping) run for
    all local folds at once: one FoldGroupEngine advances every still-active fold by one batch per launch sequence.
    loaders: [(train_loader, val_loader)] per fold; make_scheduler(optimizer) -> object with step(metric) or step();
    patience None = no early stopping (simple_fusion.py).  fold_ids: the 0-based cross-validation fold of each model (None: model g is
    fold g) -- which per-fold gene matrix its batches are gathered from (select_genes above).  transfer: a Transfer (above) applied to every
    model before the group is built.  -> per fold dict(best_c_index, best_epoch, patients_per_sec)."""
    import inspect
    import time
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    from multimodal_survival_prediction_amd.training import FusedOptimizer, has_named_validation, train_epoch_lockstep, validate_lockstep
    if transfer is not None:
        for g, m in enumerate(models):
            transfer.apply(m, fold_names[g], fold_ids[g] if fold_ids is not None else g)
        group_kw = dict(group_kw, **transfer.engine_kw)
    group = FoldGroupEngine(models, folds=fold_ids, **group_kw)
    for tl, vl in loaders:                     # cohort in HBM (or pinned host memory): name the batches, let the group gather them
        for ld in ((tl, vl) if has_named_validation(style) else (tl,)):      # (validate_lockstep's named-batch path)
            if env_int("MMS_LAZY_BATCHES", 1) and (ld.c["image"].is_cuda or ld.c["image"].is_pinned()):
                ld.lazy = True
                ld.view = data_mod().gather_view(ld.c, with_valid=(style != "final"))
                ld.hs_cpu = ld.c["has_survival"].cpu().tolist()
    opts = [FusedOptimizer(m, lr=group_kw.get("lr", 1e-4), weight_decay=group_kw.get("weight_decay", 1e-4)) for m in models]
    scheds = [make_scheduler(o) for o in opts]
    takes_metric = [len(inspect.signature(s.step).parameters) > 0 for s in scheds]
    st = [dict(best=0.0, best_epoch=0, bad=0, done=False, t=0.0, n=0, epochs=0) for _ in models]
    for epoch in range(1, num_epochs + 1):
        active = [g for g in range(len(models)) if not st[g]["done"]]
        if not active:
            break
        torch.cuda.synchronize(); t0 = time.perf_counter()
        tr = train_epoch_lockstep(group, [loaders[g][0] for g in active], style, members=active,
                                  concurrent=env_int("MMS_LOCKSTEP_STREAMS", 3))
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        n_ep = sum(len(loaders[g][0].idx) for g in active)
        va = validate_lockstep(group, [loaders[g][1] for g in active], style, device, members=active,
                               concurrent=env_int("MMS_VALIDATE_STREAMS", 2))
        for g, trg, (val_loss, c) in zip(active, tr, va):
            s = st[g]
            s["t"] += dt; s["n"] += n_ep                       # the group's aggregate rate while this fold was active
            s["epochs"] = epoch
            scheds[g].step(c) if takes_metric[g] else scheds[g].step()
            if c > s["best"]:
                s["best"], s["best_epoch"], s["bad"] = c, epoch, 0
                torch.save(models[g].state_dict(), ckpt_path(fold_names[g]))
            else:
                s["bad"] += 1
                if patience is not None and s["bad"] >= patience:
                    s["done"] = True
            if epoch % log_every == 0 or epoch == 1:
                print(f"[rank {rank}] fold {fold_names[g]} epoch {epoch:3d}: train={trg} val_loss={val_loss:.4f} "
                      f"C-index={c:.4f} best={s['best']:.4f}", flush=True)
    return [dict(best_c_index=s["best"], best_epoch=s["best_epoch"], epochs_run=s["epochs"], patients_per_sec=s["n"] / max(s["t"], 1e-9))
            for s in st]
