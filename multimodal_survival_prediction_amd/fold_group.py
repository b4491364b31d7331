"""Fold groups: the K fold models of the reference's cross-validation loop advanced in lock-step on one GPU.

The reference trains fold after fold (final_multimodal.py:316-402, partial_modality_training.py:482-560,
simple_fusion.py:318-436).  The folds are independent models of identical architecture, and one batch-4 step of one
of them is far too small for 256 CUs (most of its 570 kernels are launch/latency bound).  A `FoldGroupEngine` owns G
`SurvivalEngine`s and issues every launch of the training step ONCE for the whole group through the `*_group` entry
points of include/mmsurv.h: same kernels, same per-model arithmetic, G times the workgroups per launch.  The warm-up /
roll-back / capture of a graph is the single engine's (engine.capture).

Per-model state stays per model (parameters, Adam moments, BatchNorm buffers, learning rate, dropout counters,
epoch accumulators): a fold trained in a group follows exactly the trajectory it follows alone.

After training, the same group serves as an ensemble (ensemble.py): `forward_eval_shared` / `attribute_lockstep` run every member on ONE
batch -- one copy of the volumes, one launch sequence -- for a combined prediction and a combined saliency map.
"""
import ctypes

import torch

from . import _lib, augment as _augment, ops
from .engine import SurvivalEngine, capture, check_attribute, gate_out, group_widths_ok

_S = _lib.structs


def _arr(blocks):
    T = type(blocks[0])
    return (T * len(blocks))(*blocks)


def _ptrs(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


class _GroupPlan:
    pass


class FoldGroupEngine:
    MAX = 10     # MMS_MAX_GROUP

    # ImageOnlyModel: pool + both Linear layers in one launch per pass (mms_img_tail_*).  On: measured 5 % faster than the three launches in
    # the entry points' layout (sub-groups on three streams), more than that layout's spread (tools/bench_image_only.py)
    FUSED_IMG_TAIL = True

    def __init__(self, models, fused_tail=None, folds=None, **engine_kw):
        """models: 1..10 modules of the same class/shape, already on the GPU and not yet bound to an engine.
        fused_tail: ImageOnlyModel's tail as one launch per pass (None: FUSED_IMG_TAIL); ignored by the other models.
        folds: the cross-validation fold of each model (None: model g is fold g).  Only read by the indexed steps over a cohort that
        carries per-fold gene matrices (gene_select.GeneSelection.apply): member g's RNA-seq rows are gathered from fold folds[g]'s matrix."""
        self.folds = list(range(len(models))) if folds is None else [int(f) for f in folds]
        if len(self.folds) != len(models):
            raise ValueError("folds must name one fold per model")
        self.fused_tail = self.FUSED_IMG_TAIL if fused_tail is None else bool(fused_tail)
        if not 1 <= len(models) <= self.MAX:
            raise ValueError("a fold group holds 1..%d models" % self.MAX)
        self.lib = _lib.load_library()
        dev = next(models[0].parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("FoldGroupEngine: models must be on the GPU (no CPU fallback)")
        n = sum(p.numel() for p in models[0].parameters())
        n += (-n) % 4
        G = len(models)
        self.device = dev
        # group-wide buffers: zeroing the step's accumulators of the whole group is three contiguous spans of the one zeroing launch
        self.gflat_all = torch.zeros(G, n, device=dev)
        self.sumsq_all = torch.zeros(G, dtype=torch.float64, device=dev)
        self.entropy_all = torch.zeros(G, device=dev)
        # fine-tuning (transfer.FineTunePlan): the tuned optimiser launches read ONE segment table for the whole group
        tune_tab = None
        if engine_kw.get("finetune") is not None:
            from . import transfer
            plan = engine_kw["finetune"] = transfer.as_plan(engine_kw["finetune"])
            segs = [plan.resolve(m) for m in models]
            if any(not all(torch.equal(a, b) for a, b in zip(sg[:4], segs[0][:4])) for sg in segs[1:]):
                raise ValueError("the fine-tuning plan resolves to different segment tables on the group's models")
            sg = segs[0]
            tune_tab = ops.tune_table(sg.bounds.tolist(), sg.lr_mult.tolist(), sg.wd_mult.tolist(), sg.l2sp.tolist(), dev)
            if plan.encoder_frozen(models[0]):        # (the fused ImageOnlyModel tail runs encoder and heads as one launch per pass)
                self.fused_tail = False
        self.engines = []
        for g, m in enumerate(models):
            if getattr(m, "_mms_engine", None) is not None:
                raise RuntimeError("model %d already has an engine; build the group from fresh models" % g)
            if sum(p.numel() for p in m.parameters()) + (-sum(p.numel() for p in m.parameters())) % 4 != n:
                raise ValueError("fold-group models must have identical shapes")
            slots = dict(gflat=self.gflat_all[g], sumsq=self.sumsq_all[g:g + 1], entropy=self.entropy_all[g:g + 1])
            if tune_tab is not None:
                slots["tune_tab"] = tune_tab
            self.engines.append(SurvivalEngine(m, _slots=slots, **engine_kw))
        kinds = {e.prog["kind"] for e in self.engines}
        if len(kinds) != 1:
            raise ValueError("fold-group models must be of one class, got %s" % sorted(kinds))
        if len({bytes(e.dn_opts) for e in self.engines}) != 1:
            raise ValueError("fold-group models must share one encoder shape (class_layers.out width) and launch options")
        self.plans = {}

    def __len__(self):
        return len(self.engines)

    # ---- plans -----------------------------------------------------------------------------------
    def plan(self, B, dims, members=None):
        members = self._members(members)
        key = (B,) + (tuple(dims) if dims is not None else ()) + (members,)
        if key in self.plans:
            return self.plans[key]
        if B > 32:
            raise RuntimeError("fold groups batch the small-batch head kernels, limited to 32 rows per model; got %d -- train "
                               "larger batches with one engine per fold (SurvivalEngine.train_step, fold after fold)" % B)
        eng = [self.engines[i] for i in members]
        Ps = [e.plan(B, dims) for e in eng]
        GP = _GroupPlan()
        # 3-conv fallback encoder (models.USE_MONAI = False): the mms_fb_*_group drivers; none of the DenseNet launch options apply
        GP.fallback = bool(Ps[0].has_enc and Ps[0].fallback)
        GP.members, GP.eng, GP.Ps, GP.B, GP.dims = members, eng, Ps, B, (tuple(dims) if dims is not None else ())
        prog = eng[0].prog
        GP.ng = len(eng)
        GP.has_enc = Ps[0].has_enc
        if GP.has_enc:
            GP.ws = _ptrs([P.ws.data_ptr() for P in Ps])
            GP.x = _ptrs([P.ct.data_ptr() for P in Ps])
            GP.params = _ptrs([ctypes.addressof(P.ptab) for P in Ps])
            GP.buffers = _ptrs([ctypes.addressof(P.btab) for P in Ps])
            GP.grads = _ptrs([ctypes.addressof(P.gtab) for P in Ps])
            cc = prog["ct_cols"]
            GP.out = _ptrs([P.buf["feats"][:, cc:].data_ptr() for P in Ps])
            GP.dout = _ptrs([P.dbuf["feats"][:, cc:].data_ptr() for P in Ps])
            GP.ld = Ps[0].buf["feats"].stride(0)
            if GP.fallback:        # (identical for all members: FoldGroupEngine checks the parameter shapes)
                GP.widths, GP.ws_bytes = Ps[0].widths, Ps[0].ws_bytes
                if any(tuple(P.widths) != tuple(GP.widths) for P in Ps):
                    raise ValueError("fold-group models must share the CT encoder's channel widths")
                if not group_widths_ok(GP.widths):
                    raise ValueError("3-conv CT encoder widths %s: the fold-group kernels take multiples of 16 other than 48 and 112" % (tuple(GP.widths),))
        GP.img_tail = bool(self.fused_tail and GP.fallback and prog["kind"] == "ImageOnlyModel")
        GP.mix = _arr([P.mix for P in Ps]) if Ps[0].mix is not None else None
        nl = len(prog["lins"])
        GP.lin_fwd = {t: [_arr([P.lin_fwd[t][i] for P in Ps]) for i in range(nl)] for t in (True, False)}
        GP.lin_bwd = [_arr([P.lin_bwd[i] for P in Ps]) for i in range(nl)]
        GP.gate = _arr([P.gate for P in Ps]) if Ps[0].gate is not None else None
        GP.moe = GP.moe_bwd = GP.cox4 = None
        if Ps[0].moe is not None:        # SimMLM: the two stages of each pass; the 4 x ng Cox terms in launches of <= MMS_MAX_GROUP blocks
            GP.moe = [_arr([P.moe[s] for P in Ps]) for s in (0, 1)]
            GP.moe_bwd = [_arr([P.moe_bwd[s] for P in Ps]) for s in (0, 1)]
            terms = [P.cox4[c] for P in Ps for c in range(4)]
            GP.cox4 = [(_arr(terms[i:i + 8]), len(terms[i:i + 8])) for i in range(0, len(terms), 8)]
        GP.cox = _arr([P.cox for P in Ps])
        GP.cox_eval = _arr([P.cox_eval for P in Ps])
        GP.adam = {True: _arr([P.adam_skip for P in Ps]), False: _arr([P.adam for P in Ps])}
        GP.tune = None
        if eng[0].tune_tab is not None:
            GP.tune = {True: _arr([P.tune_skip for P in Ps]), False: _arr([P.tune for P in Ps])}
        GP.graphs = {}
        # zeroing: the whole group's buffers when the group is complete and contiguous, else per member
        GP.full = members == tuple(range(len(self.engines)))
        self.plans[key] = GP
        return GP

    # ---- launches ----------------------------------------------------------------------------------
    def _forward(self, GP, train, x=None, enc_opts=None, img_tail=None):
        """x: the members' volume pointers instead of the plans' own (forward_eval_shared: one copy for all); enc_opts: `const MmsDnOpts*`
        of the DenseNet121 driver call instead of _opts_arg's (attribute_lockstep: the per-layer forms); img_tail: False = ImageOnlyModel's
        tail as its three launches whatever the group's setting."""
        st = ops.stream()
        lib, ng = self.lib, GP.ng
        prog = GP.eng[0].prog
        if GP.has_enc:
            x = GP.x if x is None else x
            B, (D, H, W) = GP.B, GP.dims
            if GP.img_tail and img_tail is not False:        # the encoder's pool launch carries the two Linear layers: no head launches
                lf = GP.lin_fwd[train]
                _lib.check(lib.mms_img_forward_group(ng, GP.ws, GP.ws_bytes, GP.widths, B, D, H, W, x, GP.params, GP.buffers, GP.out, GP.ld,
                                                     1 if train else 0, lf[0], lf[1], st), "mms_img_forward_group")
                return
            enc_train = train and not GP.eng[0].enc_eval        # (FineTunePlan.encoder_eval)
            if GP.fallback:
                _lib.check(lib.mms_fb3_forward_group(ng, GP.ws, GP.ws_bytes, GP.widths, B, D, H, W, x, GP.params, GP.buffers, GP.out, GP.ld,
                                                     1 if enc_train else 0, st), "mms_fb3_forward_group")
            else:
                _lib.check(lib.mms_dn121_forward_group(ng, GP.ws, B, D, H, W, x, GP.params, GP.buffers, GP.out, GP.ld,
                                                       1 if enc_train else 0, enc_opts if enc_opts is not None else self._opts_arg(GP), st),
                           "mms_dn121_forward_group")
        self._forward_heads(GP, train)

    def _forward_heads(self, GP, train):
        st = ops.stream()
        lib, ng = self.lib, GP.ng
        prog = GP.eng[0].prog
        lf = GP.lin_fwd[train]
        n_pre = prog["n_pre"]
        for i in range(n_pre):
            _lib.check(lib.mms_linear_fwd_group(lf[i], ng, st), "mms_linear_fwd_group")
        if GP.moe is not None:
            _lib.check(lib.mms_moe_fwd_group(GP.moe[0], ng, st), "mms_moe_fwd_group")
        if GP.gate is not None:
            _lib.check(lib.mms_gate_fwd_group(GP.gate, ng, st), "mms_gate_fwd_group")
        if GP.mix is not None:
            _lib.check(lib.mms_missing_mix_fwd_group(GP.mix, ng, st), "mms_missing_mix_fwd_group")
        for i in range(n_pre, len(lf)):
            _lib.check(lib.mms_linear_fwd_group(lf[i], ng, st), "mms_linear_fwd_group")
        if GP.moe is not None:
            _lib.check(lib.mms_moe_fwd_group(GP.moe[1], ng, st), "mms_moe_fwd_group")

    @staticmethod
    def _sync_packs(GP):
        """Derived conv2 packs of every member current (SurvivalEngine.sync_packs: a no-op unless the weights were changed outside the
        fused step since the last call)."""
        if GP.fallback:        # (no derived weight state on this encoder)
            return
        for e in GP.eng:
            e.sync_packs()

    def _zero(self, GP):
        """The members' step accumulators (flat gradient, sum of squares, gate entropy) zeroed by ONE launch (mms_zero_spans_group)."""
        if getattr(GP, "zero_spans", None) is None:
            if GP.full:        # the whole group: its three buffers are contiguous
                ts = [self.gflat_all, self.sumsq_all, self.entropy_all]
            else:
                ts = [t for e in GP.eng for t in (e.gflat, e.sumsq, e.entropy)]
            GP.zero_spans = ops.zero_spans(ts)
        _lib.check(self.lib.mms_zero_spans_group(GP.zero_spans, len(GP.zero_spans), ops.stream()), "mms_zero_spans_group")

    def _train_body(self, GP, skip_if_unusable):
        """zero-grad -> forward -> Cox -> backward -> clip -> Adam for every member, one launch sequence."""
        st = ops.stream()
        lib, ng = self.lib, GP.ng
        prog = GP.eng[0].prog
        self._zero(GP)
        self._forward(GP, True)
        if GP.cox4 is not None:
            for arr, n in GP.cox4:
                _lib.check(lib.mms_cox_fwd_bwd_group(arr, n, st), "mms_cox_fwd_bwd_group")
            _lib.check(lib.mms_moe_bwd_group(GP.moe_bwd[1], ng, st), "mms_moe_bwd_group")
        else:
            _lib.check(lib.mms_cox_fwd_bwd_group(GP.cox, ng, st), "mms_cox_fwd_bwd_group")
        self._backward_from_dhz(GP)
        if GP.tune is not None:
            tu = GP.tune[bool(skip_if_unusable)]
            _lib.check(lib.mms_grad_sumsq_tuned_group(tu, ng, st), "mms_grad_sumsq_tuned_group")
            _lib.check(lib.mms_clip_adam_tuned_group(tu, ng, st), "mms_clip_adam_tuned_group")
            return
        ad = GP.adam[bool(skip_if_unusable)]
        _lib.check(lib.mms_grad_sumsq_group(ad, ng, st), "mms_grad_sumsq_group")
        _lib.check(lib.mms_clip_adam_group(ad, ng, st), "mms_clip_adam_group")

    def _backward_from_dhz(self, GP):
        """Every member's dbuf['hz'] holds dL/dhazard (SimMLM: after the mixture's backward stage); accumulates every parameter gradient
        into the members' gflat -- the group form of SurvivalEngine._backward_from_dhz."""
        st = ops.stream()
        lib, ng = self.lib, GP.ng
        prog = GP.eng[0].prog
        if GP.img_tail:
            B, (D, H, W) = GP.B, GP.dims
            _lib.check(lib.mms_img_backward_group(ng, GP.ws, GP.ws_bytes, GP.widths, B, D, H, W, GP.x, GP.params, GP.grads,
                                                  GP.lin_bwd[0], GP.lin_bwd[1], st), "mms_img_backward_group")
            return
        n_pre = prog["n_pre"]
        for i in range(len(GP.lin_bwd) - 1, n_pre - 1, -1):
            _lib.check(lib.mms_linear_bwd_group(GP.lin_bwd[i], ng, st), "mms_linear_bwd_group")
        if GP.gate is not None:
            _lib.check(lib.mms_gate_bwd_group(GP.gate, ng, st), "mms_gate_bwd_group")
        if GP.mix is not None:
            _lib.check(lib.mms_missing_mix_bwd_group(GP.mix, ng, st), "mms_missing_mix_bwd_group")
        if GP.moe is not None:
            _lib.check(lib.mms_moe_bwd_group(GP.moe_bwd[0], ng, st), "mms_moe_bwd_group")
        for i in range(n_pre - 1, -1, -1):
            _lib.check(lib.mms_linear_bwd_group(GP.lin_bwd[i], ng, st), "mms_linear_bwd_group")
        if GP.has_enc and not GP.eng[0].enc_frozen:
            B, (D, H, W) = GP.B, GP.dims
            if GP.eng[0].block_lo > 0 and GP.moe is None:        # (SimMLM_SurvivalNet: optimiser-only, as in SurvivalEngine._backward_encoder)
                _lib.check(lib.mms_dn121_backward_group_from(ng, GP.ws, B, D, H, W, GP.x, GP.params, GP.dout, GP.ld, GP.grads,
                                                             GP.eng[0].block_lo, self._opts_arg(GP), st), "mms_dn121_backward_group_from")
            elif GP.fallback:
                _lib.check(lib.mms_fb3_backward_group(ng, GP.ws, GP.ws_bytes, GP.widths, B, D, H, W, GP.x, GP.params, GP.dout, GP.ld, GP.grads, st),
                           "mms_fb3_backward_group")
            else:
                _lib.check(lib.mms_dn121_backward_group(ng, GP.ws, B, D, H, W, GP.x, GP.params, GP.dout, GP.ld, GP.grads, self._opts_arg(GP), st),
                           "mms_dn121_backward_group")

    def _opts_arg(self, GP):
        """`const MmsDnOpts*` of the group's driver calls (the members share one block: same class, same options).  The persistent
        per-block kernels (csrc/dn_cl.hip, dn_b4.hip) hand data between co-resident workgroups and one such launch per worker stream
        may be in flight: where those workgroups could outnumber the CUs, the per-layer path is taken (ops.persistent_opts) -- decided
        at launch (= graph-capture) time from the number of worker streams the process has created, and passed to the drivers as an
        ARGUMENT."""
        o = ops.persistent_opts(GP.eng[0].dn_opts, self.device, GP.ng, GP.B, GP.dims)
        GP.opts_live = o
        return ctypes.byref(o)

    def _graph(self, GP, key, body):
        """The plan's HIP graph of body(), captured on first use (engine.capture: warm-up, roll-back of every member, capture)."""
        if key not in GP.graphs:
            GP.graphs[key] = capture(GP.eng, body)
        return GP.graphs[key]

    def _members(self, members):
        return tuple(range(len(self.engines))) if members is None else tuple(members)

    @staticmethod
    def _rows(batch):
        return (batch["rna"] if batch.get("rna") is not None else batch["ct"]).shape[0]       # (a CT-only model has no rna input)

    def _step(self, GP, skip_if_unusable, use_graph):
        """The training step on the batches the plan's input buffers hold: eager launches, or the replay of their graph."""
        self._sync_packs(GP)
        if not use_graph:
            self._train_body(GP, skip_if_unusable)
            return
        self._graph(GP, ("train", bool(skip_if_unusable)), lambda: self._train_body(GP, skip_if_unusable)).replay()

    # ---- public ------------------------------------------------------------------------------------------
    def train_step(self, batches, members=None, skip_if_unusable=True, use_graph=True):
        """One optimisation step of every member on its own batch.  batches: one dict per member with the keyword
        arguments of SurvivalEngine.load_batch (ct, rna, clinical, mask, time, event, valid); all of one batch size."""
        members = self._members(members)
        if len(batches) != len(members):
            raise ValueError("one batch per member")
        has_enc = self.engines[0].prog["encoder"] is not None
        B = self._rows(batches[0])
        dims = tuple(batches[0]["ct"].shape[-3:]) if has_enc else None
        self.engines[0].check_train_batch(B, dims)
        for b in batches:
            if self._rows(b) != B or (has_enc and tuple(b["ct"].shape[-3:]) != dims):
                raise ValueError("fold-group batches must share one shape; split ragged tails into their own step")
        GP = self.plan(B, dims, members)
        for e, P, b in zip(GP.eng, GP.Ps, batches):
            e.load_batch(P, **b)
        self._step(GP, skip_if_unusable, use_graph)

    def _ring(self, GP, cohort):
        """Per (plan, cohort): the members' GatherP array and the staging ring that feeds it.  A lane is one device buffer plus one
        pinned buffer per slot; lane "idx" holds the indices, a lane per record kind is added on first use (_lane).  The async copy
        reads a pinned buffer when the stream gets there, so a slot is only rewritten after the event recorded behind its previous
        copies -- one event per slot covers all lanes."""
        cache = GP.__dict__.setdefault("gather", {})
        if id(cohort) not in cache:
            ring = dict(lanes={}, evs=[None] * 4, k=0, blocks={}, cohort=cohort)       # the cohort reference keeps the source pointers alive
            dev_idx, _ = self._lane(ring, "idx", (GP.ng, GP.B), torch.int64)
            pairs = [e.gather_block(P, cohort, dev_idx[g], fold=self.folds[GP.members[g]]) for g, (e, P) in enumerate(zip(GP.eng, GP.Ps))]
            ring["G"], ring["roles"] = _arr([G for G, _ in pairs]), [roles for _, roles in pairs]
            if "valid" not in cohort:
                for P in GP.Ps:
                    P.valid.fill_(1.0)
            cache[id(cohort)] = ring
        return cache[id(cohort)]

    def _lane(self, ring, name, shape, dtype):
        if name not in ring["lanes"]:
            ring["lanes"][name] = (torch.zeros(shape, dtype=dtype, device=self.device),
                                   [torch.zeros(shape, dtype=dtype).pin_memory() for _ in ring["evs"]])
        return ring["lanes"][name]

    def _gather_indexed(self, GP, cohort, idx, augment=None):
        """Index copy (pinned ring -> device) + the ONE gather launch that assembles the group's batches in the plans' input buffers.
        augment: [len(members)][B] augment.Records (or bare 8-word records): every array they hold rides the ring in a lane of its
        own and decides the launch (augment.launch_gather); None: the plain gather."""
        ring = self._ring(GP, cohort)
        recs = None if augment is None else _augment.Records.of(augment)
        # (validated before the ring is touched: a refused step leaves no copy without its event)
        blocks = [] if recs is None else self._aug_blocks(GP, ring, recs)
        k = ring["k"]
        ring["k"] = (k + 1) % len(ring["evs"])
        if ring["evs"][k] is not None:
            ring["evs"][k].synchronize()
        for name, src in [("idx", idx)] + ([] if recs is None else [(kd.name, a) for kd, a in recs.held()]):
            dev, pin = ring["lanes"][name]
            pin[k].copy_(src)
            dev.copy_(pin[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        ring["evs"][k] = ev
        _augment.launch_gather(self.lib, ring["G"], *blocks, ng=GP.ng)

    def _aug_blocks(self, GP, ring, recs):
        """Validates the step's records on the host (they are host data, so the launch cannot be refused with a bare code) -> the
        members' launch block arrays [AugP, AffP, ElaP][:kinds held] over the ring's record lanes.  Lanes and arrays are created on
        first use of a kind (ElaP: one array per spacing); the bounds the blocks carry are refreshed from this step's records."""
        has_mask = all(P.gate is not None or P.moe is not None or P.mix is not None for P in GP.Ps)
        dims = GP.dims if GP.has_enc else None
        mx, amp = recs.check((GP.ng, GP.B), dims, has_mask)
        bound = dict(rec=mx if recs.aff is None else [0, 0, 0], ela=amp)       # (only mms_gather_aug_group reads the records' shifts)
        out = []
        for kd, _ in recs.held():
            dev, _ = self._lane(ring, kd.name, (GP.ng, GP.B, kd.words), torch.int32)
            key = (kd.name, recs.spacing if kd.per_spacing else None)
            if key not in ring["blocks"]:
                ring["blocks"][key] = _arr([kd.block(dev[g], bound.get(kd.name), ring["roles"][g], dims, recs.spacing, 0) for g in range(GP.ng)])
            if kd.bound:         # (one bound per launch: the largest of the step's records, every member)
                for g in range(GP.ng):
                    getattr(ring["blocks"][key][g], kd.bound)[:] = bound[kd.name]
            out.append(ring["blocks"][key])
        return out

    def train_step_indexed(self, cohort, indices, members=None, skip_if_unusable=True, use_graph=True, augment=None):
        """Same step with the batches named by patient indices into a cohort that lives in HBM (data.cohort_to) or in pinned host
        memory (data.cohort_pin: the gather launch reads the rows over PCIe): indices: [len(members)][B] integer array-like (host).  The batch assembly of the whole group is one small
        host-to-device copy of the indices plus ONE gather launch (mms_gather_rows_group) instead of ~10 torch
        indexing/copy kernels per member.  augment: the rows' augmentation records, an augment.Records with leading axes
        [len(members)][B] (Records.stack of the members' bundles, as a lazy data.BatchLoader yields them) or a bare [len(members)][B]
        array of 8-word records (augment.make_records / augment.sample_records, host int32): the gather launch applies them while it
        copies -- CT flips, shifts and intensity map, modality dropout (mms_gather_aug_group); with affine records rotation / zoom
        resampling and additive noise (mms_gather_affine_group; the flip / shift fields of the 8-word records are not read, they are
        folded into the matrices); with elastic records a free-form deformation before the affine map (mms_gather_elastic_group).
        None: no augmentation, the plain gather."""
        members = self._members(members)
        idx = torch.as_tensor(indices, dtype=torch.int64)
        if idx.dim() != 2 or idx.shape[0] != len(members):
            raise ValueError("indices must be [len(members)][B]")
        B = idx.shape[1]
        dims = tuple(cohort["image"].shape[-3:]) if self.engines[0].prog["encoder"] is not None else None
        self.engines[0].check_train_batch(B, dims)
        GP = self.plan(B, dims, members)
        self._gather_indexed(GP, cohort, idx, augment)
        self._step(GP, skip_if_unusable, use_graph)

    def _eval_loss_body(self, GP):
        """Eval-mode forward of every member + the Cox value of its batch (no gradient) + the validation accumulators."""
        self._forward(GP, False)
        _lib.check(self.lib.mms_cox_fwd_bwd_group(GP.cox_eval, GP.ng, ops.stream()), "mms_cox_fwd_bwd_group")
        for e, P in zip(GP.eng, GP.Ps):
            e.acc_eval[:2] += P.cox_eval_out         # (the loss is 0 when the batch is unusable)
            e.acc_eval[3] += 1.0

    def eval_loss_step_indexed(self, cohort, indices, members=None):
        """validate_*'s step with the batches named by patient indices (as train_step_indexed): gather + ONE graph (eval-mode forward,
        Cox value of each member's batch, accumulators SurvivalEngine.acc_eval).  -> per member (hazard [B], (loss | usable) [2]):
        views of static buffers, valid until the next step of this plan."""
        members = self._members(members)
        idx = torch.as_tensor(indices, dtype=torch.int64)
        if idx.dim() != 2 or idx.shape[0] != len(members):
            raise ValueError("indices must be [len(members)][B]")
        dims = tuple(cohort["image"].shape[-3:]) if self.engines[0].prog["encoder"] is not None else None
        GP = self.plan(idx.shape[1], dims, members)
        self._gather_indexed(GP, cohort, idx)
        self._sync_packs(GP)
        self._graph(GP, "evalloss", lambda: self._eval_loss_body(GP)).replay()
        return [(P.buf["hz"][:, 0], P.cox_eval_out) for P in GP.Ps]

    def attribute(self, *args, **kw):
        """Input-gradient attribution is a single-model path (SurvivalEngine.attribute)."""
        raise RuntimeError("FoldGroupEngine.attribute: input-gradient attribution is not implemented for fold groups (no lock-step "
                           "form of mms_dn121_input_grad / mms_fb3_input_grad); call SurvivalEngine.attribute on each fold's model")

    # ---- one batch seen by every member (ensembles) ----------------------------------------------------------
    def _shared_plan(self, batch, members):
        members = self._members(members)
        has_enc = self.engines[0].prog["encoder"] is not None
        dims = tuple(batch["ct"].shape[-3:]) if has_enc else None
        GP = self.plan(self._rows(batch), dims, members)
        if GP.has_enc and getattr(GP, "x_shared", None) is None:
            GP.x_shared = _ptrs([GP.Ps[0].ct.data_ptr()] * GP.ng)       # member 0's input buffer is the group's one copy of the volume
        return GP

    def _load_shared(self, GP, batch):
        """The volume once (into member 0's input buffer); the small head inputs (rna, clinical, mask) per member."""
        for g, (e, P) in enumerate(zip(GP.eng, GP.Ps)):
            e.load_batch(P, shared_ct=g > 0, **batch)

    def forward_eval_shared(self, batch, members=None, use_graph=True):
        """Eval-mode forward of every member on ONE batch (a dict of SurvivalEngine.load_batch's keywords): the CT volume is stored once and
        every member's launch block names that copy -> forward_eval's result."""
        GP = self._shared_plan(batch, members)
        self._load_shared(GP, batch)
        self._sync_packs(GP)
        x = GP.x_shared if GP.has_enc else None
        if use_graph:
            self._graph(GP, "eval_shared", lambda: self._forward(GP, False, x=x)).replay()
        else:
            self._forward(GP, False, x=x)
        return [(P.buf["hz"][:, 0], gate_out(P)) for P in GP.Ps]

    def _attr_group(self, GP):
        """The members' attribution blocks (SurvivalEngine._attr_blocks) as the arrays of the *_group entry points."""
        AG = getattr(GP, "attr", None)
        if AG is not None:
            return AG
        As = [e._attr_blocks(P) for e, P in zip(GP.eng, GP.Ps)]
        AG = dict(members=As, lin=[_arr([A["lin"][i] for A in As]) for i in range(len(As[0]["lin"]))],
                  gate=_arr([A["gate"] for A in As]) if As[0]["gate"] is not None else None,
                  mix=_arr([A["mix"] for A in As]) if As[0]["mix"] is not None else None,
                  opts=As[0].get("opts"))                    # (the members share one options block: checked by the constructor)
        if GP.has_enc:
            cc = GP.eng[0].prog["ct_cols"]
            AG["dout"] = _ptrs([P.dbuf["feats"][:, cc:].data_ptr() for P in GP.Ps])
            AG["dx"] = _ptrs([A["dct"].data_ptr() for A in As])
        GP.attr = AG
        return AG

    def _check_attribute(self, wrt):
        check_attribute(self.engines, wrt)

    def _attribute_lockstep_run(self, batch, members=None):
        """attribute_lockstep's launches -> (GP, AG): the members' hazards are in their plans' buffers, their input gradients in
        AG['members'][g]['dct' | 'drna' | 'dclin'], valid until the next call on this plan."""
        st, lib = ops.stream(), self.lib
        GP = self._shared_plan(batch, members)
        ng, prog = GP.ng, GP.eng[0].prog
        AG = self._attr_group(GP)
        self._load_shared(GP, batch)
        self._sync_packs(GP)
        enc_opts = ctypes.byref(AG["opts"]) if AG["opts"] is not None else None
        if ng == 1:
            # a group of one IS the single model: its own launch sequence (on the 3-conv encoder the scalar forward of mms_fb3_forward,
            # whose summation order the group's MFMA forward does not share)
            GP.eng[0]._forward(GP.Ps[0], False, enc_opts=enc_opts)
        else:
            # ImageOnlyModel: the fused tail's forward does leave feats, the hidden layer and the hazard where the heads' backward reads
            # them (img_tail_fwd_kernel writes all three); the three-launch tail is taken anyway, so that this path runs the sequence of
            # SurvivalEngine._attribute_chunk for every class
            self._forward(GP, False, x=GP.x_shared if GP.has_enc else None, enc_opts=enc_opts, img_tail=False)
        for P in GP.Ps:
            P.dbuf["hz"].fill_(1.0)           # d hazard[b] / d hazard[b] = 1: rows do not interact in eval mode
        n_pre = prog["n_pre"]
        for i in range(len(AG["lin"]) - 1, n_pre - 1, -1):
            _lib.check(lib.mms_linear_bwd_group(AG["lin"][i], ng, st), "mms_linear_bwd_group")
        if AG["gate"] is not None:
            _lib.check(lib.mms_gate_bwd_group(AG["gate"], ng, st), "mms_gate_bwd_group")
        if AG["mix"] is not None:
            _lib.check(lib.mms_missing_mix_bwd_group(AG["mix"], ng, st), "mms_missing_mix_bwd_group")
        for i in range(n_pre - 1, -1, -1):
            _lib.check(lib.mms_linear_bwd_group(AG["lin"][i], ng, st), "mms_linear_bwd_group")
        if GP.has_enc:
            B, (D, H, W) = GP.B, GP.dims
            if GP.fallback:
                GP.eng[0]._check_scalar_path(GP.Ps[0])
                _lib.check(lib.mms_fb3_input_grad_group(ng, GP.ws, GP.ws_bytes, GP.widths, B, D, H, W, GP.x_shared, GP.params, GP.buffers,
                                                        AG["dout"], GP.ld, AG["dx"], st), "mms_fb3_input_grad_group")
            else:
                _lib.check(lib.mms_dn121_input_grad_group(ng, GP.ws, B, D, H, W, GP.x_shared, GP.params, GP.buffers, AG["dout"], GP.ld,
                                                          AG["dx"], enc_opts, st), "mms_dn121_input_grad_group")
        return GP, AG

    def attribute_lockstep(self, batch, members=None, wrt=("ct", "rna", "clinical")):
        """Input-gradient attribution of every member on ONE batch (<= 32 rows; a dict of load_batch's keywords), in lock-step: the
        group form of SurvivalEngine._attribute_chunk.  Shared-input eval forward in the per-layer forms -> dhazard = 1 -> the heads'
        backward (eval prologues, no weight gradients, the gate's gradients into private scratch) -> the group input-gradient driver
        (mms_dn121_input_grad_group / mms_fb3_input_grad_group), every launch once for the group.  -> per member what
        SurvivalEngine.attribute returns.  Touches no .grad, no optimiser state, no running statistic, no conv2 pack and no training graph."""
        self._check_attribute(wrt)
        GP, AG = self._attribute_lockstep_run(batch, members)
        res = []
        for P, A in zip(GP.Ps, AG["members"]):
            has_gate = P.gate is not None
            out = dict(hazard=P.buf["hz"][:, 0].clone(), gate=P.gatew.clone() if has_gate else None)
            out["ct"] = A["dct"].clone() if (P.has_enc and "ct" in wrt) else None
            out["rna"] = A["drna"].clone() if ("drna" in A and "rna" in wrt) else None
            out["clinical"] = A["dclin"].clone() if ("dclin" in A and "clinical" in wrt) else None
            res.append(out)
        return res

    def forward_eval(self, batches, members=None, use_graph=True):
        """Eval-mode forward of every member -> list of (hazard [B] view, gate [B,3] or None) per member."""
        members = self._members(members)
        dims = tuple(batches[0]["ct"].shape[-3:]) if self.engines[0].prog["encoder"] is not None else None
        GP = self.plan(self._rows(batches[0]), dims, members)
        for e, P, b in zip(GP.eng, GP.Ps, batches):
            e.load_batch(P, **b)
        self._sync_packs(GP)
        if use_graph:
            self._graph(GP, "eval", lambda: self._forward(GP, False)).replay()
        else:
            self._forward(GP, False)
        return [(P.buf["hz"][:, 0], gate_out(P)) for P in GP.Ps]

    def reset_epoch_stats(self):
        for e in self.engines:
            e.reset_epoch_stats()

    def epoch_stats(self):
        return [e.epoch_stats() for e in self.engines]
