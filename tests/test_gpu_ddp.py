"""Data-parallel step with the GLOBAL Cox risk set (SURVEY section 8e ii), 2 ranks sharing the card through gloo:
[zero-grad, forward] | all-gather (h, time, event, valid) | [global Cox, own slice of dL/dh, backward] | all-reduce SUM |
[clip, Adam] -- against the CPU oracle doing the same thing with torch autograd (local BatchNorm statistics on both sides)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["MMS_ROOT"])
import numpy as np, torch, torch.distributed as dist
from multimodal_survival_prediction_amd import distributed as D, models as HM
from multimodal_survival_prediction_amd.training import FusedOptimizer
from oracle import models as OM, losses as OL
BACKEND = os.environ.get("MMS_TEST_BACKEND", "gloo")      # "nccl" (= RCCL): one GPU per rank, the engine's collectives run on device tensors
world, rank, local = D.init(BACKEND)
dev = torch.device("cuda", rank if BACKEND == "nccl" else 0)
torch.cuda.set_device(dev)
cpu_pg = dist.new_group(backend="gloo") if BACKEND == "nccl" else None      # the CPU oracle's own collectives
torch.set_num_threads(max(4, (os.cpu_count() or 8) // 4))
B, rna_dim = 6, 64
torch.manual_seed(3)
ref = OM.RNASeqSurvivalModel(input_dim=rna_dim, hidden_dims=[96, 48])
for m in ref.modules():
    if isinstance(m, torch.nn.Dropout): m.p = 0.0
net = HM.RNASeqSurvivalModel(input_dim=rna_dim, hidden_dims=[96, 48]); net.load_state_dict(ref.state_dict())
for m in net.modules():
    if isinstance(m, torch.nn.Dropout): m.p = 0.0
net.to(dev).train(); ref.train()
fo = FusedOptimizer(net, lr=1e-3, weight_decay=1e-3, adamw=True, max_norm=1.0)
opt = torch.optim.AdamW(ref.parameters(), lr=1e-3, weight_decay=1e-3)
for it in range(3):
    rng = np.random.default_rng(100 + it)                       # the GLOBAL batch, identical on both ranks
    rna = torch.tensor(rng.normal(0, 1, (world * B, rna_dim)).astype(np.float32))
    t = torch.tensor((rng.exponential(1000, world * B) + 1 + np.arange(world * B) * 1e-3).astype(np.float32))
    e = torch.tensor((rng.random(world * B) < 0.6).astype(np.float32)); e[0] = 1
    sl = slice(rank * B, (rank + 1) * B)
    # oracle: local forward (local BN statistics), global risk set, own slice carries the gradient, SUM over ranks, clip, AdamW
    hz = ref(rna[sl]).squeeze()
    parts = [torch.zeros(B) for _ in range(world)]
    dist.all_gather(parts, hz.detach(), group=cpu_pg)
    parts[rank] = hz
    loss = OL.neg_partial_log_likelihood(torch.cat(parts), e.bool(), t)
    opt.zero_grad(); loss.backward()
    for p in ref.parameters():
        dist.all_reduce(p.grad, op=dist.ReduceOp.SUM, group=cpu_pg)
    torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
    opt.step()
    fo.engine.train_step(None, rna[sl], time=t[sl], event=e[sl], skip_if_unusable=False, ddp_world=world, global_cox=True,
                         use_graph=it > 0)
    torch.cuda.synchronize()
    st = fo.engine.epoch_stats()
    got = st["sum_loss"] - (prev if it else 0.0); prev = st["sum_loss"]
    # every step, graph replays included (weights drift by Adam noise on zero-gradient parameters only: 1e-3)
    assert abs(got - loss.item()) <= (1e-4 if it == 0 else 1e-3) * max(1.0, abs(loss.item())), (it, got, loss.item())
# a Linear bias that feeds a training-mode BatchNorm has an exactly-zero gradient: Adam turns its rounding noise into +-lr moves
gmax = max(float(p.grad.abs().max()) for p in ref.parameters())
worst = max(float((p.detach() - q.detach().cpu()).abs().max()) for p, q in zip(ref.parameters(), net.parameters())
            if float(p.grad.abs().max()) > 1e-5 * gmax)
assert worst <= 2e-5, worst
D.barrier()
print("ok", rank, worst)
'''


def test_ddp_global_cox_two_ranks(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MMS_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT="29617", WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    logs = [open(tmp_path / f"rank{r}.log", "w") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=logs[r], stderr=subprocess.STDOUT, text=True) for r in range(2)]
    _wait_all(procs, 300)
    outs = [(tmp_path / f"rank{r}.log").read_text() for r in range(2)]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"ok {r}" in o, o


def test_ddp_global_cox_two_ranks_rccl(tmp_path):
    """The same step over RCCL (torch.distributed backend "nccl"), one GPU per rank: the engine's all-gather of (hazard, time, event,
    valid) and its gradient all-reduce run on device tensors -- the branches the gloo rehearsals above cannot reach.  Needs two GPUs."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs (one rank per GPU over RCCL)")
    script = tmp_path / "w.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MMS_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT="29619", WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0",
               MMS_TEST_BACKEND="nccl")
    logs = [open(tmp_path / f"rank{r}.log", "w") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=logs[r], stderr=subprocess.STDOUT, text=True) for r in range(2)]
    _wait_all(procs, 300)
    outs = [(tmp_path / f"rank{r}.log").read_text() for r in range(2)]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"ok {r}" in o, o


def _wait_all(procs, timeout):
    """Wait for every rank; whatever happens (time-out, a failed sibling), no rank process is left behind holding the GPU."""
    try:
        for p in procs:
            p.wait(timeout=timeout)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()


# ---- imaging model, two ranks sharing the card (gloo): bucketed staged backward and SyncBN --------------------------------------
_WORKER_IMG = r'''
import os, sys
sys.path.insert(0, os.environ["MMS_ROOT"]); sys.path.insert(0, os.path.join(os.environ["MMS_ROOT"], "tests"))
import numpy as np, torch, torch.distributed as dist
from multimodal_survival_prediction_amd import distributed as D, models as HM
from multimodal_survival_prediction_amd.training import FusedOptimizer
from oracle import models as OM, losses as OL
from gpu_util import _Recorder
from test_gpu_densenet import structured_volumes
world, rank, local = D.init("gloo")
dev = torch.device("cuda", 0)
torch.set_num_threads(max(4, (os.cpu_count() or 8) // 4))      # two ranks run their CPU oracle at the same time: do not oversubscribe the host


def run_mode(MODE):
    # rank-local BatchNorm over 2 rows is +-1 whatever the input (ill-conditioned in ANY implementation): 4 patients per rank there
    B, rna_dim, dims = (2 if MODE == "sync_bn" else 4), 64, tuple(int(v) for v in os.environ.get("MMS_DDP_DIMS", "64,64,32").split(","))
    torch.manual_seed(5)
    ref = OM.MultiModalSurvivalNet(rna_dim=rna_dim, use_monai=True)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, (torch.nn.BatchNorm3d, torch.nn.BatchNorm1d)):
                m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.1)
            if isinstance(m, torch.nn.Dropout): m.p = 0.0
    net = HM.MultiModalSurvivalNet(rna_dim=rna_dim); net.load_state_dict(ref.state_dict())
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout): m.p = 0.0
    net.to(dev).train(); ref.train()
    fo = FusedOptimizer(net, lr=1e-4, weight_decay=1e-4, adamw=False, max_norm=1.0)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-4, weight_decay=1e-4)
    p0 = [p.detach().clone() for p in ref.parameters()]
    # Two steps (the first = eager warm-up, rolled back, + capture + REPLAY of the captured parts; the second = replay; sync_bn: eager).
    # The second step's loss is taken at weights that one Adam step has moved by lr * sign(g) wherever |g| is within rounding of zero,
    # so two fp32 implementations no longer agree at 1e-4 there.  How far a correct fp32 implementation may drift is MEASURED: the
    # same step runs a third time in fp64 (exact for this purpose) and the HIP result must lie within 4x the fp32 oracle's own
    # distance from it (one random draw per implementation: see tests/test_gpu_epoch_parity.py for measured single-batch ratios).
    n_it = int(os.environ.get("MMS_DDP_STEPS", "2"))
    import copy
    ref64 = copy.deepcopy(ref).double() if n_it > 1 else None
    opt64 = torch.optim.Adam(ref64.parameters(), lr=1e-4, weight_decay=1e-4) if n_it > 1 else None

    def oracle_step(model, optim, ct, rna, clin, e, t, sl, dt):
        ct, rna, clin, t = ct.to(dt), rna.to(dt), clin.to(dt), t.to(dt)
        optim.zero_grad()
        if MODE == "sync_bn":
            hz = model(ct, rna, clin)
            loss = OL.cox_loss(hz, e, t)
            loss.backward()
        else:
            hz = model(ct[sl], rna[sl], clin[sl])
            if MODE == "global_cox":
                parts = [torch.zeros(B, dtype=dt) for _ in range(world)]
                dist.all_gather(parts, hz.detach()); parts[rank] = hz
                loss = OL.cox_loss(torch.cat(parts), e, t)
            else:
                loss = OL.cox_loss(hz, e[sl], t[sl])
            loss.backward()
            for p in model.parameters():
                if p.grad is None: p.grad = torch.zeros_like(p)
                dist.all_reduce(p.grad, op=dist.ReduceOp.SUM)
                if MODE == "local": p.grad /= world
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        optim.step()
        return float(loss.item())

    for it in range(n_it):
        rng = np.random.default_rng(200 + it)                       # the GLOBAL batch, identical on both ranks
        n = world * B
        ct = structured_volumes(n, dims, 40 + it)
        rna = torch.tensor(rng.normal(0, 1, (n, rna_dim)).astype(np.float32))
        clin = torch.tensor((np.clip(rng.normal(60, 11, (n, 1)), 30, 90) / 100).astype(np.float32))
        t = torch.tensor((rng.exponential(1000, n) + 1 + np.arange(n) * 1e-3).astype(np.float32))
        e = torch.tensor((rng.random(n) < 0.6).astype(np.float32)); e[0] = 1; e[B] = 1
        sl = slice(rank * B, (rank + 1) * B)
        opt.zero_grad()
        if MODE == "sync_bn":
            # ONE process stepping on the concatenated global batch: global BatchNorm statistics, global risk set
            hz = ref(ct, rna, clin)
            loss = OL.cox_loss(hz, e, t)
            loss.backward()
            hz_mine = hz.detach()[sl]
        else:
            hz = ref(ct[sl], rna[sl], clin[sl])                      # rank-local BatchNorm statistics
            if MODE == "global_cox":
                parts = [torch.zeros(B) for _ in range(world)]
                dist.all_gather(parts, hz.detach()); parts[rank] = hz
                loss = OL.cox_loss(torch.cat(parts), e, t)
            else:
                loss = OL.cox_loss(hz, e[sl], t[sl])
            loss.backward()
            for p in ref.parameters():
                if p.grad is None: p.grad = torch.zeros_like(p)
                dist.all_reduce(p.grad, op=dist.ReduceOp.SUM)
                if MODE == "local": p.grad /= world
            hz_mine = hz.detach()
        gref = [p.grad.detach().clone() for p in ref.parameters()]
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
        opt.step()
        acc0 = fo.engine.epoch_stats()["sum_loss"]
        fo.engine.train_step(ct[sl], rna[sl], clin[sl], time=t[sl], event=e[sl], skip_if_unusable=False, ddp_world=world,
                             global_cox=MODE == "global_cox", sync_bn=MODE == "sync_bn", use_graph=True)
        torch.cuda.synchronize()
        got_loss = fo.engine.epoch_stats()["sum_loss"] - acc0
        if it == 0:
            assert abs(got_loss - loss.item()) <= 1e-4 * max(1.0, abs(loss.item())), (MODE, it, got_loss, loss.item())
        if ref64 is not None:
            l64 = oracle_step(ref64, opt64, ct, rna, clin, e, t, sl, torch.float64)
            d_hip, d_f32 = abs(got_loss - l64), abs(loss.item() - l64)
            print("step", it, MODE, rank, "loss fp64 %.8f | fp32 oracle off by %.2e | HIP off by %.2e" % (l64, d_f32, d_hip), flush=True)
            assert d_hip <= 4.0 * d_f32 + 1e-5 * max(1.0, abs(l64)), (MODE, it, got_loss, loss.item(), l64)
        if it == 0:
            # hazards of this rank's patients in the training-mode forward of the first step
            eng = fo.engine
            if MODE == "sync_bn":
                Pg = [P for k, P in eng.plans.items() if "heads" in k][0]
                hz_hip = Pg.buf["hz"][:, 0].cpu()[sl]
            else:
                hz_hip = [P for k, P in eng.plans.items() if "heads" not in k][0].buf["hz"][:, 0].cpu()
            err = float((hz_hip - hz_mine).abs().max() / hz_mine.abs().max())
            assert err <= 1e-4, (MODE, "hazards", err)
            # the all-reduced gradient (before clipping) of the first step: heads strict; encoder flip-aware (tests/test_gpu_models.py;
            # measured global L2 1.4e-3 / 2.2e-2 / 3.6e-2 for sync_bn / local / global_cox, heads 3e-5)
            gmax = max(float(g.abs().max()) for g in gref)
            num = den = 0.0; hworst = 0.0
            names = [k for k, _ in ref.named_parameters()]
            for k, g, hv in zip(names, gref, eng.gviews):      # (the engine's gradient views: conv2 tensors are strided views of packed storage)
                h = hv.cpu().double()
                num += float(((h - g.double()) ** 2).sum()); den += float((g.double() ** 2).sum())
                if "ct_encoder" not in k and float(g.abs().max()) > 1e-5 * gmax:
                    er = float((h - g.double()).abs().max() / g.abs().max())
                    if os.environ.get("MMS_DDP_DEBUG"): print("head", k, er, float(g.abs().max()), flush=True)
                    hworst = max(hworst, er)
            assert (num / den) ** 0.5 <= 6e-2 and hworst <= 2e-4, (MODE, (num / den) ** 0.5, hworst)
            print("grad", MODE, rank, (num / den) ** 0.5, hworst)
    # weights after the step(s): Adam moves a weight by <= lr per step; everything with a real gradient must agree closely
    tot = sum(p.numel() for p in ref.parameters())
    close = sum(float(((p.detach() - q.detach().cpu()).abs() <= 2e-5).double().sum()) for p, q in zip(ref.parameters(), net.parameters()))
    # (two steps: the second gradient is taken at weights that already differ by Adam noise -- measured 0.81 after two steps, 0.93 after one)
    assert close / tot >= (0.90 if n_it == 1 else 0.70), (MODE, close / tot)
    # BatchNorm running statistics (sync_bn: global statistics, identical on both ranks).  One step: 1e-4.  Two steps: within twice the
    # fp32 oracle's own distance from the fp64 run, x4 (+ 1e-4 of the buffer's scale)
    b64 = dict(ref64.named_buffers()) if ref64 is not None else {}
    for (k, b), (_, c) in zip(ref.named_buffers(), net.named_buffers()):
        if "num_batches" in k:
            assert int(b) == int(c), k
        elif n_it == 1:
            err = float((c.cpu() - b).abs().max() / (b.abs().max() + 1e-30))
            assert err <= 1e-4, (MODE, k, err)
        else:
            x = b64[k]
            sc_ = float(x.abs().max()) + 1e-30
            e_hip, e_f32 = float((c.cpu().double() - x).abs().max()) / sc_, float((b.double() - x).abs().max()) / sc_
            assert e_hip <= 4.0 * e_f32 + 1e-4, (MODE, k, e_hip, e_f32)
    # Launch order of the mode: one more eager step on the last batch, the library handle wrapped in the recorder (both ranks: the
    # collectives pair up).  The lists are what the step launched before the data-parallel steps moved to distributed.DataParallel.
    fo.engine.lib = rec = _Recorder(fo.engine.lib)
    fo.engine.train_step(ct[sl], rna[sl], clin[sl], time=t[sl], event=e[sl], skip_if_unusable=False, ddp_world=world,
                         global_cox=MODE == "global_cox", sync_bn=MODE == "sync_bn", use_graph=False)
    torch.cuda.synchronize()
    fo.engine.lib = rec._lib
    heads = ["mms_linear_fwd"] * 6 + ["mms_cox_fwd_bwd"] + ["mms_linear_bwd"] * 6
    want = (["mms_dn121_forward_sync"] + heads + ["mms_dn121_backward_stage"] if MODE == "sync_bn" else
            ["mms_zero_spans_group", "mms_dn121_forward"] + heads + ["mms_dn121_backward_stage"] * 4) + ["mms_grad_sumsq", "mms_clip_adam"]
    assert rec.calls == want, (MODE, rec.calls)
    D.barrier()
    print("mode ok", rank, MODE, close / tot, flush=True)


for mode in os.environ["MMS_DDP_MODE"].split(","):      # "local" | "global_cox" | "sync_bn"
    run_mode(mode)
print("ok", rank)
'''


def _run_two_ranks(tmp_path, worker, port, extra_env):
    script = tmp_path / "w.py"
    script.write_text(worker)
    env = dict(os.environ, MMS_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0",
               **extra_env)
    logs = [open(tmp_path / f"rank{r}.log", "w") for r in range(2)]        # files, not pipes: a chatty rank cannot stall the other
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=logs[r],
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    _wait_all(procs, 900)
    outs = [(tmp_path / f"rank{r}.log").read_text() for r in range(2)]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"ok {r}" in o, o[-4000:]


@pytest.mark.parametrize("mode,port", [("local,global_cox", 29631), ("sync_bn", 29633)])
def test_ddp_imaging_model_two_ranks(tmp_path, mode, port):
    """MultiModalSurvivalNet (DenseNet121-3D on 64x64x32 volumes), 2 ranks, 4 patients per rank (sync_bn: 2):
    local      -- rank-local BatchNorm + rank-local risk sets, gradients averaged over ranks in 5 buckets launched stage by stage
                  (graph-captured parts: the step = eager warm-up, rolled back, + capture + replay);
    global_cox -- rank-local BatchNorm, risk set over the 4 patients, gradients summed;
    sync_bn    -- the step ONE process would take on the concatenated batch of 4: global BatchNorm3d/BatchNorm1d statistics and
                  global risk set; hazards 1e-4, BatchNorm running statistics 1e-4, head gradients 2e-4."""
    _run_two_ranks(tmp_path, _WORKER_IMG, port, dict(MMS_DDP_MODE=mode))


def test_ddp_config4_shape_sync_bn(tmp_path):
    """BASELINE config 4's per-rank problem: CT 128x128x64, 2 patients per rank, SyncBN + global risk set, 2 ranks -- against ONE process
    stepping on the concatenated batch of 4 (block-1 grid 32x32x16: the widest multi-tap window, 8 statistic replicas per level)."""
    _run_two_ranks(tmp_path, _WORKER_IMG, 29634, dict(MMS_DDP_MODE="sync_bn", MMS_DDP_DIMS="128,128,64", MMS_DDP_STEPS="1"))
