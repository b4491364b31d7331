#!/usr/bin/env python
"""mms_td_metrics (IPCW Brier / cumulative-dynamic AUC under bootstrap multiplicities, csrc/td_metrics.hip) at the sizes
absolute_risk.prediction_error is used at: M = 8 models, H = 32 horizons, n in {348, 608} patients (two thirds events, times in whole
days), R in {2 000, 10 000} replicates -- beside the test reference's vectorised numpy form on the same host, in one process.  Per shape:

  kernel      the launch alone on device-resident inputs (ops.td_metrics(plan_only=True) uploads and checks once): HIP events around one
              call, --warmup calls first, --reps timed calls; median, min, max, spread.  "lane_steps" counts one (position, model,
              horizon) visit per replicate (R M H n): the classify-and-accumulate step every lane does; "g_lane_steps_per_s" is that
              over the kernel time -- a rate of this kernel's own unit of work, not a share of any peak.
  numpy       tests/td_metrics_ref.py metrics_vec (float64, threads as the environment sets them, host clock) on the first
              --numpy-replicates weight rows, per replicate, and scaled to all R.
  end to end  absolute_risk.prediction_error (weight draw, input preparation, upload, launch, download, statistics), host clock, 3 runs;
              the draw of the R weight rows alone is timed beside it.

The kernel's brier and auc_num of the timed rows are compared with numpy's (1e-9 relative) before anything is recorded.
Writes --out as JSON and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def one_shape(M, H, n, R, args):
    import numpy as np
    import torch
    import td_metrics_ref as REF
    from multimodal_survival_prediction_amd import absolute_risk as AR, ops
    from multimodal_survival_prediction_amd.bootstrap import bootstrap_weights

    rng = np.random.default_rng(n)
    t = np.ceil(rng.exponential(900.0, n))
    e = (rng.random(n) < 0.67).astype(np.int64)
    risk = np.stack([-np.log(t) * (m / M) + rng.normal(size=n) for m in range(M)])
    tau = AR.default_horizons(t, e, H)
    surv = np.stack([AR.breslow_baseline(r, t, e).survival(r, tau) for r in risk])
    t0 = time.perf_counter()
    w = bootstrap_weights(n, R, 0)
    draw_ms = (time.perf_counter() - t0) * 1e3
    order, trank, es, hcut, rord = AR.metric_inputs(risk, t, e, tau)
    p, keep, out = ops.td_metrics(trank, es, hcut, rord, np.ascontiguousarray(surv[:, order, :]), np.ascontiguousarray(w[:, order]), plan_only=True)
    for _ in range(args.warmup):
        ops.call("mms_td_metrics", p)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.call("mms_td_metrics", p)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    steps = R * M * H * n
    res = {"M": M, "H": H, "n": n, "R": R, "events": int(e.sum()), "distinct_times": int(len(np.unique(t))),
           "kernel_ms": {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4)},
           "kernel_us_per_replicate": round(med * 1e3 / R, 4), "lane_steps": steps, "g_lane_steps_per_s": round(steps / (med * 1e-3) / 1e9, 1)}
    got = {k: v.cpu().numpy() for k, v in out.items()}
    nt = min(args.numpy_replicates, R)
    t_np = 0.0
    for r in range(nt):
        t0 = time.perf_counter()
        ref = REF.metrics_vec(t, e, risk, surv, tau, w[r])
        t_np += time.perf_counter() - t0
        for k in ("brier", "auc_num"):
            assert np.abs(got[k][r] - ref[k]).max() <= 1e-9 * max(1.0, np.abs(ref[k]).max()), "kernel and numpy differ on replicate %d (%s)" % (r, k)
    res["numpy_ms_per_replicate"] = round(t_np * 1e3 / nt, 4)
    res["numpy_replicates_timed"] = nt
    res["numpy_ms_scaled_to_all"] = round(t_np * 1e3 / nt * R, 1)
    res["numpy_over_kernel"] = round(res["numpy_ms_scaled_to_all"] / med, 1)
    res["agrees_with_numpy"] = True
    del keep
    e2e = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        AR.prediction_error(surv, risk, t, e, tau, R=R, seed=0)
        e2e.append((time.perf_counter() - t0) * 1e3)
    res["prediction_error_ms"] = [round(v, 1) for v in e2e]
    res["bootstrap_weights_ms"] = round(draw_ms, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=8)
    ap.add_argument("--horizons", type=int, default=32)
    ap.add_argument("--n", type=int, nargs="+", default=[348, 608])
    ap.add_argument("--replicates", type=int, nargs="+", default=[2000, 10000])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--numpy-replicates", type=int, default=50)
    ap.add_argument("--out", default=os.path.join("profiles", "td_metrics_bench.json"))
    args = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": args.reps,
           "numpy_threads": os.environ.get("OMP_NUM_THREADS", "unset"),
           "shapes": [one_shape(args.models, args.horizons, n, R, args) for n in args.n for R in args.replicates]}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
