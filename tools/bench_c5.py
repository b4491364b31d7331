"""BASELINE config 5: RNA-seq-only model (5005 -> 1024 -> 512 -> 256 -> 1), batch 2048, one full training step per replay
(zero-grad, forward, O(B^2) Cox partial likelihood, backward, AdamW) as a captured HIP graph.  Profiling aid (tools/prof_c5.sh):
prints one JSON line with the GPU rate only; the judged line with roofline and cpu_baseline is `python bench.py --workload c5 --full`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    from multimodal_survival_prediction_amd import models
    from multimodal_survival_prediction_amd.training import FusedOptimizer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = models.RNASeqSurvivalModel(input_dim=5005).to(dev).train()
    fo = FusedOptimizer(net, lr=1e-4, weight_decay=1e-3, adamw=True, max_norm=0.0)
    B = a.batch
    rng = np.random.default_rng(0)
    rna = torch.tensor(rng.normal(0, 1, (B, 5005)).astype(np.float32), device=dev)
    t = torch.tensor((rng.exponential(1000, B) + 1 + np.arange(B) * 1e-3).astype(np.float32), device=dev)
    e = torch.tensor((rng.random(B) < 0.6).astype(np.float32), device=dev)
    for _ in range(a.warmup):
        fo.engine.train_step(None, rna, time=t, event=e, skip_if_unusable=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        fo.engine.train_step(None, rna, time=t, event=e, skip_if_unusable=False)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    flops = 3 * 2 * B * (5005 * 1024 + 1024 * 512 + 512 * 256 + 256) - 2 * B * 5005 * 1024      # no dX for the first layer
    out = dict(workload="C5 rnaseq-only B=%d" % B, ms_per_step=dt * 1e3, patients_per_s=B / dt, gemm_tflops=flops / dt / 1e12,
               loss=fo.engine.epoch_stats()["sum_loss"] / (a.steps + a.warmup))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
