"""Multi-GPU: one process per GPU, torch.distributed (backend "nccl" == RCCL over xGMI on ROCm; "gloo" on CPU tests).

Two ways the path shards:
  * K-fold level -- independent units, zero data-path exchange: fold k runs on rank k mod world; only the per-fold
    result records are gathered at the end (`gather_fold_results`).  Reproduces single-GPU results exactly.
  * patient/batch level (DDP): each rank steps on its shard of the global batch; the flat gradient buffer is
    all-reduced between backward and the clip+Adam kernels: one blocking collective (`allreduce_mean_`), or -- the default of
    the staged step -- SUM in 5 buckets (`gradient_buckets`: heads, then the DenseNet121 backward stages 3..0), each launched
    asynchronously as soon as its stage has been enqueued (`allreduce_ranges_async`) so that it overlaps the rest of the backward; the
    update waits for all of them and divides by the world size.  (The RCCL branch has not run on hardware yet: 1-GPU leases; the gloo
    CPU tests take the same async code path.)
    Cox risk set: rank-local (default), or GLOBAL over the world*B patients of the step (`train_step(..., ddp_world=N,
    global_cox=True)`).  BatchNorm: rank-local, or `sync_bn=True` = exact global-batch semantics.
    The steps live here too, built from the engine's launch primitives: `DataParallel` (one per engine, made by its first data-parallel
    train_step) holds their state and runs `step` (graph-captured parts in the order of `step_sequence`) and `step_syncbn` (eager).
"""
import ctypes
import os

import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib, ops


def env_world():
    return int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))


def init(backend=None):
    """-> (world, rank, local device index).  Backend: argument, else $MMS_DIST_BACKEND, else nccl (= RCCL) when a GPU is
    present.  `gloo` lets several ranks share one card (rehearsals on a 1-GPU box); the local index wraps accordingly."""
    world, rank, local = env_world()
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        backend = backend or os.environ.get("MMS_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        dist.init_process_group(backend, rank=rank, world_size=world)
    if torch.cuda.is_available():
        local = local % max(torch.cuda.device_count(), 1)
    return world, rank, local


def folds_of_rank(n_folds, world, rank):
    """fold k -> rank k mod world."""
    return [k for k in range(n_folds) if k % world == rank]


def gather_fold_results(local_results, world):
    """local_results: list of dicts (each with a 'fold' key) -> all folds' records, ordered by fold, on every rank."""
    if world <= 1:
        return sorted(local_results, key=lambda r: r["fold"])
    out = [None] * world
    dist.all_gather_object(out, local_results)
    return sorted([r for part in out for r in part], key=lambda r: r["fold"])


def _sum_over_ranks(t):
    """In-place SUM of t over the ranks.  gloo reduces through host memory (rehearsal path: several ranks sharing one card)."""
    if t.is_cuda and dist.get_backend() == "gloo":
        h = t.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM)
        t.copy_(h)
    else:
        dist.all_reduce(t, op=dist.ReduceOp.SUM)


def allreduce_sum_(flat, world):
    """In-place sum over ranks (gradients of a loss that is already global: each rank holds its samples' share)."""
    if world > 1:
        _sum_over_ranks(flat)
    return flat


def all_gather_into(out, local, world):
    """out[r * n:(r + 1) * n] = rank r's `local` (n elements, same on every rank): the (hazard, time, event, valid) exchange
    of the global Cox risk set -- 4 collectives of world * B floats."""
    if world <= 1:
        out.copy_(local.reshape(-1))
        return out
    if local.is_cuda and dist.get_backend() == "gloo":
        parts = [torch.empty(local.numel()) for _ in range(world)]
        dist.all_gather(parts, local.detach().reshape(-1).cpu())
        out.copy_(torch.cat(parts))
    else:
        dist.all_gather_into_tensor(out, local.detach().reshape(-1).contiguous())
    return out


def allreduce_mean_(flat, world):
    """In-place mean of a flat gradient buffer over ranks (one bucket: the buffer is already contiguous)."""
    if world > 1:
        _sum_over_ranks(flat)
        flat.div_(world)
    return flat


def allreduce_ranges_async(flat, ranges, world):
    """SUM over ranks of the slices flat[a:a+n] of one gradient bucket, launched asynchronously: RCCL runs the collective on its
    own stream behind the work already enqueued on the current stream, so it overlaps whatever the caller enqueues next.
    -> a callable that makes the CURRENT stream wait for the bucket.  (gloo rehearsal path: synchronous, through host memory.)"""
    if world <= 1:
        return lambda: None
    if flat.is_cuda and dist.get_backend() == "gloo":
        for a, n in ranges:
            _sum_over_ranks(flat[a:a + n])
        return lambda: None
    works = [dist.all_reduce(flat[a:a + n], op=dist.ReduceOp.SUM, async_op=True) for a, n in ranges]

    def wait():
        for w in works:
            w.wait()
    return wait


ENC_STAGE_CUTS = (0, 39, 114, 261, 364)     # csrc/dn_net.hip Idx: parameter-table index where dense block b's backward stage begins (b = 0..3)


def gradient_buckets(params, encoder_params, staged):
    """Gradient buckets of the data-parallel step in the order the backward finalises them: the heads, then (staged = DenseNet121
    encoder) its backward stages 3, 2, 1, 0 -- each a list of contiguous (offset, length) ranges of the flat gradient buffer, in which
    the parameters lie in `params` order.  -> [[(offset, length), ...], ...]; together the ranges cover the buffer exactly once."""
    offs, o = {}, 0
    for q in params:
        offs[id(q)] = (o, q.numel())
        o += q.numel()

    def ranges(ids):
        out = []
        for a, n in sorted(offs[i] for i in ids):
            if out and out[-1][0] + out[-1][1] == a:
                out[-1] = (out[-1][0], out[-1][1] + n)
            else:
                out.append((a, n))
        return out
    eids = [id(q) for q in encoder_params]
    eset = set(eids)
    hids = [id(q) for q in params if id(q) not in eset]
    if staged:
        c = ENC_STAGE_CUTS
        if len(eids) != c[-1]:
            raise ValueError("staged buckets are defined for the DenseNet121 encoder (%d parameter tensors), got %d" % (c[-1], len(eids)))
        return [ranges(hids)] + [ranges(eids[c[b]:c[b + 1]]) for b in (3, 2, 1, 0)]
    return [ranges(hids + eids)]


def step_sequence(staged, global_cox):
    """The data-parallel step as a list of compute parts -- ("part", name), each one HIP graph -- and communication points: ("gather",)
    = the exchange of the global risk set, ("bucket", k) = launch the all-reduce of bucket k of gradient_buckets(..., staged), ("wait",)
    = wait for every bucket.  The update part follows the list.  Pure: no engine, no GPU, no process group."""
    seq = [("part", "fwd"), ("gather",), ("part", "coxheads")] if global_cox else [("part", "gradheads")]
    if staged:
        seq.append(("bucket", 0))
        for k, b in enumerate((3, 2, 1, 0)):
            seq += [("part", ("enc", b)), ("bucket", k + 1)]
    else:
        seq += [("part", ("enc", None)), ("bucket", 0)]
    return seq + [("wait",)]


class DataParallel:
    """The data-parallel steps of ONE SurvivalEngine (one process per GPU) and every piece of state they keep
    between calls.  The launches are the engine's: its library handle, options block and stream are taken at call time."""

    def __init__(self, engine):
        self.engine = engine
        enc = engine.prog["encoder"]
        self.staged = enc is not None and not isinstance(enc, nn.Sequential)       # DenseNet121: one gradient bucket per backward stage
        self.buckets = gradient_buckets(engine.params, list(enc.parameters()) if enc is not None else [], self.staged)
        self.gcox = {}        # (plan, world) -> buffers of the global risk set WITH the CoxP block that points into them
        self.hooks = {}       # plan -> its SyncBN hook (_lib.SYNC_FN: the drivers call through it, so it lives as long as the plan's entry)
        self.share = {}       # world -> [n] factor per gradient element before the SyncBN step's SUM (1/world where every rank holds the global value)

    def _global_cox(self, P, world):
        if (P, world) not in self.gcox:
            e, n = self.engine, world * P.B
            G = {k: torch.zeros(n, device=e.device) for k in ("h", "time", "event", "lse", "dh", "frac")}
            G["valid"] = torch.ones(n, device=e.device)
            G["cox"] = _lib.structs()["CoxP"](G["h"].data_ptr(), 1, G["time"].data_ptr(), G["event"].data_ptr(), G["valid"].data_ptr(), n, 1.0,
                                              G["lse"].data_ptr(), G["dh"].data_ptr(), 1, P.cox_out.data_ptr(), e.tie_mode, G["frac"].data_ptr())
            self.gcox[(P, world)] = G
        G = self.gcox[(P, world)]
        G["rank"] = dist.get_rank() if dist.is_initialized() else 0
        return G

    def _part(self, P, G, part):
        """One compute part of `step` on the current stream: "fwd" | "coxheads" (loss over the gathered world*B hazards, own slice of
        dL/dh, heads' backward) | "gradheads" (rank-local risk set: zero-grad, forward, Cox, heads' backward) | ("enc", b) = stage b of
        the encoder backward (None = all of it) | ("update", scale): the gradients arrived as a SUM over ranks."""
        e = self.engine
        if part == "fwd":
            e._zero_step()
            e._forward(P, True, entropy_zeroed=True)
        elif part == "coxheads":
            _lib.check(e.lib.mms_cox_fwd_bwd(ctypes.byref(G["cox"]), ops.stream()), "mms_cox_fwd_bwd")
            P.dbuf["hz"][:, 0].copy_(G["dh"][G["rank"] * P.B:(G["rank"] + 1) * P.B])
            e._backward_heads(P)
        elif part == "gradheads":
            e._zero_step()
            e._forward(P, True, entropy_zeroed=True)
            e._cox_step(P)
            e._backward_heads(P)
        elif part[0] == "enc":
            e._backward_encoder(P, stage=None if part[1] is None else (part[1], part[1]))
        else:
            if part[1] != 1.0:
                e.gflat.mul_(part[1])          # mean for rank-local losses
            e.sumsq.zero_()                    # mms_grad_sumsq ADDS into it; the part that zeroes it is not in this graph
            e._update(P, False)

    def step(self, P, world, global_cox, use_graph):
        """Rank-local BatchNorm statistics.  The flat gradient buffer is all-reduced (SUM) bucket by bucket, each bucket launched as
        soon as the backward stage that finalises it has been enqueued, so the collective of stage k runs beside the kernels of
        stage k+1 (torch.distributed enqueues an async collective behind the current stream's work and runs it on its own
        stream; the update waits for all of them).  Rank-local risk sets: gradients are averaged (1/world folded into the update
        graph).  global_cox: risk sets over the world*B patients (all-gather of hazard/time/event/valid), gradients summed."""
        e = self.engine
        e._refuse_ddp()
        seq = step_sequence(self.staged, global_cox)
        upd = ("update", 1.0 if global_cox else 1.0 / world)
        G = self._global_cox(P, world) if global_cox else None

        def run(run_part):
            works = []
            for item in seq:
                if item[0] == "part":
                    run_part(item[1])
                elif item[0] == "gather":
                    all_gather_into(G["h"], P.buf["hz"][:, 0], world)
                    all_gather_into(G["time"], P.time, world); all_gather_into(G["event"], P.event, world)
                    all_gather_into(G["valid"], P.valid, world)
                elif item[0] == "bucket":
                    works.append(allreduce_ranges_async(e.gflat, self.buckets[item[1]], world))
                else:
                    for w in works:
                        w()
            run_part(upd)
        eager = lambda part: self._part(P, G, part)
        if not use_graph:
            run(eager)
            return
        key = ("ddp", global_cox, world)
        if key not in P.graphs:
            # the parts depend on each other through the workspace (statistic accumulators are zeroed by the first part only), so
            # they are warmed up as ONE eager step (on the current stream: the collectives stay where they are), rolled back, and then
            # captured without being executed
            snap = e.snapshot()
            run(eager)
            torch.cuda.synchronize()
            e.restore(snap)
            graphs = {}
            for part in [it[1] for it in seq if it[0] == "part"] + [upd]:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    eager(part)
                graphs[part] = g
            P.graphs[key] = graphs
        graphs = P.graphs[key]
        run(lambda part: graphs[part].replay())

    def _sync_hook(self, P, world):
        """mms_sync_fn (include/mmsurv.h) of a plan: all-reduce freshly written BatchNorm accumulator words over the ranks."""
        if P not in self.hooks:
            e = self.engine
            base0 = P.ws.data_ptr()
            ws64 = P.ws[:P.ws.numel() // 8 * 8].view(torch.float64)

            def hook(user, base, nrep, rstride, ncols, pstride, stream):
                try:
                    e.sync_collectives += 1      # (reported by bench.py --mode ddp --sync-bn)
                    t = ws64.as_strided((nrep, 2, ncols), (rstride, pstride, 1), (base - base0) // 8)
                    buf = t.contiguous()
                    allreduce_sum_(buf, world)
                    if buf.data_ptr() != t.data_ptr():
                        t.copy_(buf)
                    return 0
                except Exception as ex:      # never raise through the C frame
                    print("mmsurv: SyncBN hook failed: %r" % (ex,), flush=True)
                    return -2
            self.hooks[P] = _lib.SYNC_FN(hook)
        return self.hooks[P]

    def _share_of(self, world):
        if world not in self.share:
            e = self.engine
            enc = e.prog["encoder"]
            sh = torch.full_like(e.gflat, 1.0 / world)        # heads + BatchNorm3d parameters: global value on every rank
            o = 0
            bn_ids = {id(q) for m in enc.modules() if isinstance(m, nn.BatchNorm3d) for q in m.parameters()}
            eids = {id(q) for q in enc.parameters()}
            for q in e.params:
                if id(q) in eids and id(q) not in bn_ids:
                    sh[o:o + q.numel()] = 1.0                 # conv / class_layers weights: rank-local partial sums
                o += q.numel()
            self.share[world] = sh
        return self.share[world]

    def step_syncbn(self, P, world):
        """Exact single-process semantics for a global batch of world*B patients (SURVEY.md section 8e ii-iii), eager launches.
        Collectives per step: ONE all-reduce per statistic-producing kernel (all replicas and both moments of its channels in one
        message): 121 in the forward (conv0, pool0, conv1 + conv2 of the 58 dense layers, 3 transitions), 121 in the backward, + the
        feature / label all-gathers and the gradient all-reduce -- 2 per BatchNorm layer and pass, the same count torch's SyncBatchNorm
        issues.  It cannot be lower without changing the arithmetic: layer l's conv2 normalises with the statistics of ITS conv1's
        output and layer l+1's conv1 with those of layer l's conv2 output, so the chain y1-stats(l) -> z-stats(l) -> y1-stats(l+1) is
        strictly sequential (the slab's OLDER channels are reduced once, when they are produced, and reused by every later layer).
        The engine's `sync_collectives` counts them; bench.py --mode ddp --sync-bn reports the count per step.
          * encoder: every BatchNorm3d statistic (forward sums, backward sums) is all-reduced between the kernel that produces it
            and the kernels that consume it (the drivers' hook);
          * heads (BatchNorm1d over the batch, gate, Cox risk set): replicated -- the encoder features and the small per-patient
            inputs are all-gathered and every rank runs the heads on the GLOBAL batch, then back-propagates its own patients'
            feature gradient through its encoder;
          * gradients: encoder weights hold rank-local partial sums -> SUM; head parameters and BatchNorm3d gamma/beta hold the
            global value on every rank -> pre-scaled by 1/world so that the same SUM returns them; then clip + Adam."""
        e = self.engine
        e._refuse_ddp()
        if not P.has_enc or P.fallback:
            raise RuntimeError("sync_bn: the DenseNet121-3D imaging models only")
        prog = e.prog
        rank = dist.get_rank() if dist.is_initialized() else 0
        B, (Dd, H, W) = P.B, P.dims
        Pg = e.plan(world * B, P.dims, heads_only=True)
        hook = self._sync_hook(P, world)
        cc = prog["ct_cols"]
        e.gflat.zero_(); e.sumsq.zero_()
        feats = P.buf["feats"]
        _lib.check(e.lib.mms_dn121_forward_sync(P.ws.data_ptr(), B, Dd, H, W, P.ct.data_ptr(), P.ptab, P.btab, feats[:, cc:].data_ptr(),
                                                feats.stride(0), world, hook, None, e._opts_arg(P), ops.stream()), "mms_dn121_forward_sync")

        def gather(dst, src):
            tmp = torch.empty(world * src.shape[0], *src.shape[1:], device=e.device)
            all_gather_into(tmp.view(-1), src.contiguous().view(-1), world)
            dst.copy_(tmp.view(dst.shape))
        ew = prog.get("enc_width", 128)
        gather(Pg.buf["feats"][:, cc:cc + ew], feats[:, cc:cc + ew])
        for name in ("rna", "clin"):
            if name in P.buf:
                gather(Pg.buf[name], P.buf[name])
        if P.gate is not None:
            gather(Pg.mask, P.mask)
        if P.mix is not None:
            gather(Pg.mask2, P.mask2)
        gather(Pg.time, P.time); gather(Pg.event, P.event); gather(Pg.valid, P.valid)
        e._forward(Pg, True)                                      # heads only (Pg.has_enc is False)
        e._cox_step(Pg)
        e._backward_heads(Pg)
        P.dbuf["feats"][:, cc:cc + ew].copy_(Pg.dbuf["feats"][rank * B:(rank + 1) * B, cc:cc + ew])
        e._backward_encoder(P, hook=hook)
        e.gflat.mul_(self._share_of(world))
        allreduce_sum_(e.gflat, world)
        e._update(Pg, False)          # (the heads plan's AdamP: its cox_out is the global loss)


def max_over_ranks(x, device):
    if not dist.is_initialized():
        return x
    t = torch.tensor([x], dtype=torch.float64, device="cpu" if dist.get_backend() == "gloo" else device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def barrier():
    if dist.is_initialized():
        dist.barrier()
