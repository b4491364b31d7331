"""Gradient-boosted trees on the Cox partial likelihood (R gbm "coxph", XGBoost "survival:cox") as the third classical baseline: every
problem of a nested cross-validation in lock-step.

The K (J + 1) |grid| boosters of a nested cross-validation read ONE patient x gene matrix and differ only in one multiplicity per
patient (0 = held out), a few scalars and a hash stream, so they advance together (include/mmsurv.h: GbmGradP, GbmSplitP, GbmUpdateP,
GbmPredictP; csrc/gbm.hip).  A round is one launch for the gradients -- Breslow ties, fp64, then QUANTISED to int64 fixed point so that
every later sum is an exact integer --, one call per level of the tree (exhaustive split search over all genes on LDS histograms, a
fixed-order argmax, routing) and one launch for the leaf values, F and the C-index pair counts of each problem's evaluation rows.  There
is no CPU fallback.

Binning is done once per call with torch: bins - 1 quantile edges per gene from the rows handed in.  The edges read no label, so sharing
them between the folds of a cross-validation leaks nothing (per-fold honesty concerns the labels); a cut is stored as the raw threshold
edges[gene][bin], and raw values predict with x <= thr -> left.  With per-fold gene selection (gene_select.fold_matrix) each outer fold's
problems are their own fit call: one matrix per call.

The hash contract (restated in tests/gbm_ref.py, which replicates all of this in numpy), h = csrc/common.h's hash_u32:
    problem key hk = h(seed ^ (id * 0x85ebca6b)),   round key hm = h((m + 1) * 0x85ebca6b + hk),
    row i (of the matrix handed in) is in round m's sample iff h((i + 1) * 0x9E3779B9 + hm) <= subsample threshold,
    gene j is admitted in round m iff h((j + 1) * 0x9E3779B9 + (hm ^ 0xB5297A4D)) <= colsample threshold   (0xFFFFFFFF = always).
The gradient always uses all training rows; the tree is fitted on the sampled ones; F is updated for every row."""
from dataclasses import dataclass, field

import numpy as np

from .risk_sets import descending_groups, to_numpy
from .survival_forest import GOLDEN, STREAM, DRAW, hash_u32, tree_key

_M32 = np.uint64(0xFFFFFFFF)
ALWAYS = 0xFFFFFFFF
TABLES = ("feat", "bin", "thr", "gain", "value", "n_node", "G", "H")


def rate_threshold(rate):
    """A sampling rate in [0, 1] -> the uint32 threshold a hash is compared with (<=): 1 -> 0xFFFFFFFF (always), 0 -> 0."""
    r = np.asarray(rate, np.float64)
    if (r < 0).any() or (r > 1).any():
        raise ValueError("a sampling rate must lie in [0, 1]")
    return np.minimum(np.floor(r * 4294967296.0), float(ALWAYS)).astype(np.int64)


def round_key(seed, problem_id, m):
    return hash_u32(((np.asarray(m, np.uint64) + np.uint64(1)) * np.uint64(STREAM) + tree_key(seed, problem_id)) & _M32)


def row_sample(seed, problem_id, m, n, threshold):
    """bool [n]: the rows of round m's sample of problem `problem_id`"""
    i = np.arange(1, int(n) + 1, dtype=np.uint64)
    return hash_u32((i * np.uint64(GOLDEN) + round_key(seed, problem_id, m)) & _M32) <= np.uint64(int(threshold))


def gene_sample(seed, problem_id, m, p, threshold):
    """bool [p]: the genes round m of problem `problem_id` admits"""
    j = np.arange(1, int(p) + 1, dtype=np.uint64)
    return hash_u32((j * np.uint64(GOLDEN) + (round_key(seed, problem_id, m) ^ np.uint64(DRAW))) & _M32) <= np.uint64(int(threshold))


def quantile_edges(x, bins=32):
    """x: fp32 [n, p] device matrix -> fp32 [p, bins - 1] ascending edges: the k / bins quantiles (torch.quantile, linear) of every column.
    Label-free.  Duplicate edges (a gene with few distinct values) leave empty bins."""
    import torch
    B = int(bins)
    q = torch.arange(1, B, dtype=torch.float32, device=x.device) / B
    out = [torch.quantile(x[:, c:c + 1024], q, dim=0) for c in range(0, x.shape[1], 1024)]      # (quantile's input size is limited)
    return torch.cat(out, dim=1).t().contiguous()


def bin_matrix(x, edges):
    """x: fp32 [R, p], edges: fp32 [p, B - 1] -> uint8 [p, R]: bin = the number of the gene's edges < x (searchsorted, side "left")"""
    import torch
    return torch.searchsorted(edges, x.t().contiguous(), right=False).to(torch.uint8).contiguous()


def _per_problem(v, P, dtype, name):
    a = np.asarray(v, dtype=dtype).reshape(-1)
    if len(a) == 1:
        a = np.repeat(a, P)
    if len(a) != P:
        raise ValueError("%s must be a scalar or one value per problem" % name)
    return a


@dataclass
class Booster:
    tables: dict              # device tensors [P, M, nn]: feat (-1 = leaf or absent), bin, thr, gain, value, n_node, G, H
    edges: object             # float32 [p, B - 1] device
    p: int
    hyper: dict               # per-problem arrays: learning_rate, max_depth, min_leaf, l2, min_gain, subsample, colsample (thresholds); bins, seed
    problem_ids: np.ndarray
    curve: dict = field(default_factory=dict)      # loglik [P, M + 1] (before round m; [M] = after the last), conc2 / comparable int64 [P, M], c_index [P, M]
    F: object = None          # float64 [P, n] device: F of every row of fit's matrix after the last round, in the rows' order (not saved)
    trace: dict = None        # fit(trace=True): qg, qh [M, P, n] (position order), levels [M][level] = dict(n, G, H), order

    @property
    def n_problems(self):
        return int(self.tables["feat"].shape[0])

    @property
    def rounds(self):
        return int(self.tables["feat"].shape[1])

    def predict(self, x, rounds=None):
        """x: fp32 [R, p] device matrix of RAW values; rounds: an int or an ascending sequence of round counts in 0..M (None: M).
        -> float64 [P, R] (an int or None) or [P, K, R] numpy: F after that many rounds, summed in round order."""
        from . import ops
        at = [self.rounds] if rounds is None else ([int(rounds)] if np.ndim(rounds) == 0 else list(rounds))
        out = ops.gbm_predict(x, self.tables["feat"], self.tables["thr"], self.tables["value"], at).cpu().numpy()
        return out[:, 0] if rounds is None or np.ndim(rounds) == 0 else out

    def importance(self, problems=None, rounds=None):
        """-> (split counts int64 [p], summed gain float64 [p]) over the problems (an index array, None = all) and their first `rounds`
        rounds (None = all), from the tables."""
        feat, gain = to_numpy(self.tables["feat"]), to_numpy(self.tables["gain"])
        if problems is not None:
            feat, gain = feat[np.asarray(problems)], gain[np.asarray(problems)]
        if rounds is not None:
            feat, gain = feat[:, :int(rounds)], gain[:, :int(rounds)]
        ok = feat >= 0
        return (np.bincount(feat[ok], minlength=self.p).astype(np.int64), np.bincount(feat[ok], weights=gain[ok], minlength=self.p))

    def shap(self, x, problems=None, rounds=None, timings=None):
        """Path-dependent TreeSHAP of the listed problems (an index sequence, None = all) after their first `rounds` rounds (None: all;
        an int, or one round count per listed problem -- nested_cv's chosen counts differ per fold) for the RAW rows x: fp32 [R, p]
        device.  The trees are gathered into contiguous [T, nn] tables, one group per problem; the cover is n_node, the round's sample.
        -> tree_shap.ShapValues with one group per listed problem: base[g] + phi[g].sum(1) == predict(x, rounds)[problem] to rounding,
        and exp(phi) is a gene's hazard-ratio multiplier for that patient.  timings: receives ("launch", milliseconds)."""
        import torch
        from . import tree_shap
        P, M = self.n_problems, self.rounds
        probs = np.arange(P, dtype=np.int64) if problems is None else np.asarray(problems, np.int64).reshape(-1)
        rds = _per_problem(M if rounds is None else rounds, len(probs), np.int64, "rounds") if len(probs) else np.zeros(0, np.int64)
        if len(probs) and (probs.min() < 0 or probs.max() >= P or rds.min() < 0 or rds.max() > M):
            raise ValueError("problems must lie in 0..%d and rounds in 0..%d" % (P - 1, M))
        goff = np.concatenate([[0], np.cumsum(rds)])
        dev = self.tables["feat"].device
        pi = torch.from_numpy(np.repeat(probs, rds)).to(dev)
        ri = torch.from_numpy(np.concatenate([np.arange(r) for r in rds]).astype(np.int64) if len(rds) else np.zeros(0, np.int64)).to(dev)
        tab = [self.tables[k][pi, ri].contiguous() for k in ("feat", "thr", "value", "n_node")]
        phi, base, genes = tree_shap.launch(x, *tab, goff, timings=timings)
        return tree_shap.from_launch(phi, base, genes)

    def save(self, path):
        keys = sorted(self.hyper)
        np.savez(path, **{k: to_numpy(self.tables[k]) for k in TABLES}, edges=to_numpy(self.edges), p=np.int64(self.p),
                 problem_ids=np.asarray(self.problem_ids, np.int64), hyper_keys=np.array(keys),
                 **{"hyper_" + k: np.asarray(self.hyper[k]) for k in keys}, **{"curve_" + k: np.asarray(v) for k, v in self.curve.items()})


def load(path, device="cuda"):
    import torch
    with np.load(path if str(path).endswith(".npz") else str(path) + ".npz") as z:
        return Booster({k: torch.from_numpy(z[k]).to(device) for k in TABLES}, torch.from_numpy(z["edges"]).to(device), int(z["p"]),
                       {str(k): z["hyper_" + str(k)] for k in z["hyper_keys"]}, z["problem_ids"],
                       {k[6:]: z[k] for k in z.files if k.startswith("curve_")})


def save(booster, path):
    booster.save(path)


def fit(x, time, event, mults, *, rounds, learning_rate=0.1, max_depth=2, min_leaf=10, l2=1.0, min_gain=0.0, subsample=1.0, colsample=1.0,
        bins=32, seed=0, eval_masks=None, problem_ids=None, trace=False, form=0, timings=None):
    """Boost len(mults) problems in lock-step for `rounds` rounds.  x: fp32 [n, p] device matrix; time / event: [n]; mults: [P, n]
    multiplicities 0..255 over x's rows (0 = held out).  learning_rate, max_depth (1..6), min_leaf, l2, min_gain, subsample, colsample:
    scalars or one value per problem.  eval_masks: [P, n] the rows each problem is scored on after every round (None: no scores).
    problem_ids: the hash stream of each problem (None: 0..P-1).  trace: keep qg / qh of every round and the prefixed histograms of every
    level (tests; memory grows with M p B).  form: the histogram form of mms_gbm_split (0 = default).  timings: a list that receives
    (launch name, milliseconds) from HIP events (tools/bench_gbm.py; it synchronises after each).  -> Booster."""
    import torch
    from . import _lib, ops
    lim = _lib.defines("MMS_GBM_")
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise TypeError("x must be a float32 [n, p] device tensor")
    n, p = int(x.shape[0]), int(x.shape[1])
    time, ev = to_numpy(time, "time").astype(np.float64).reshape(-1), to_numpy(event).reshape(-1) != 0
    mults = np.asarray(to_numpy(mults))
    if mults.ndim != 2 or mults.shape[1] != n or len(time) != n or len(ev) != n:
        raise ValueError("time / event must be [n] and mults [P, n] for x [n, p]")
    if mults.size and (mults.min() < 0 or mults.max() > lim["MAX_MULT"]):
        raise ValueError("multiplicities must lie in 0..%d" % lim["MAX_MULT"])
    P, M, B = len(mults), int(rounds), int(bins)
    if not (1 <= n <= lim["MAX_N"]) or P > lim["MAX_P"] or M < 1 or not (2 <= B <= lim["MAX_BINS"]) or p < 1:
        raise ValueError("n must be in 1..%d, problems <= %d, rounds >= 1, bins in 2..%d" % (lim["MAX_N"], lim["MAX_P"], lim["MAX_BINS"]))
    hy = dict(learning_rate=_per_problem(learning_rate, P, np.float64, "learning_rate"), max_depth=_per_problem(max_depth, P, np.int32, "max_depth"),
              min_leaf=_per_problem(min_leaf, P, np.int32, "min_leaf"), l2=_per_problem(l2, P, np.float64, "l2"),
              min_gain=_per_problem(min_gain, P, np.float64, "min_gain"), subsample=rate_threshold(_per_problem(subsample, P, np.float64, "subsample")),
              colsample=rate_threshold(_per_problem(colsample, P, np.float64, "colsample")))
    if P and (hy["max_depth"].min() < 1 or hy["max_depth"].max() > lim["MAX_DEPTH"] or hy["min_leaf"].min() < 1 or hy["l2"].min() < 0
              or hy["min_gain"].min() < 0 or not np.isfinite(hy["learning_rate"]).all()):
        raise ValueError("max_depth must lie in 1..%d, min_leaf >= 1, l2 >= 0, min_gain >= 0" % lim["MAX_DEPTH"])
    ids = np.arange(P, dtype=np.int64) if problem_ids is None else np.asarray(problem_ids, np.int64).reshape(-1)
    if len(ids) != P:
        raise ValueError("problem_ids must name one hash stream per problem")
    dev = x.device
    order, _, gid, _, _ = descending_groups(time)
    inv = np.empty(n, np.int64); inv[order] = np.arange(n)
    edges = quantile_edges(x, B)
    xb = bin_matrix(x[torch.from_numpy(order).to(dev)], edges)        # [p, n] in position order, built once
    if bool(torch.isnan(x).any()):
        raise ValueError("x contains NaN (missing values are not supported)")
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dt)
    mult_d = up(mults[:, order].astype(np.uint8), torch.uint8).reshape(P, n)
    event_d, tgroup_d, rowid_d = up(ev[order].astype(np.int32), torch.int32), up(gid.astype(np.int32), torch.int32), up(order.astype(np.int32), torch.int32)
    pid_d = up(ids.astype(np.int32), torch.int32)
    evalm_d = None
    if eval_masks is not None:
        em = np.asarray(to_numpy(eval_masks)) != 0
        if em.shape != (P, n):
            raise ValueError("eval_masks must be [P, n]")
        evalm_d = up(em[:, order].astype(np.uint8), torch.uint8).reshape(P, n)
    D = int(hy["max_depth"].max()) if P else 1
    nn = (2 << D) - 1
    prm = dict(lr=up(hy["learning_rate"], torch.float64), depth=up(hy["max_depth"], torch.int32), min_leaf=up(hy["min_leaf"], torch.int32),
               l2=up(hy["l2"], torch.float64), min_gain=up(hy["min_gain"], torch.float64))
    sub_d, col_d = ops._gbm_u32(up(hy["subsample"], torch.int64)), ops._gbm_u32(up(hy["colsample"], torch.int64))
    state, tab = ops.gbm_state(P, n, M, dev), ops.gbm_tables(P, M, nn, dev)
    scratch = [ops.gbm_scratch(P, p, level, dev) for level in range(D)]
    tr = dict(qg=[], qh=[], levels=[], order=order) if trace else None

    def timed(name, fn):
        if timings is None:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        timings.append((name, e0.elapsed_time(e1)))
        return out

    for m in range(M if P else 0):
        timed("grad", lambda: ops.gbm_grad(mult_d, event_d, tgroup_d, rowid_d, sub_d, state, tab, m, seed, pid=pid_d))
        if trace:
            tr["qg"].append(state["qg"].clone()); tr["qh"].append(state["qh"].clone()); tr["levels"].append([])
        for level in range(D):
            t = timed("split_level_%d" % level, lambda: ops.gbm_split(xb, edges, state, tab, prm, col_d, level, m, seed, pid=pid_d, form=form,
                                                                       trace=trace, scratch=scratch[level]))
            if trace:
                tr["levels"][-1].append(t)
        timed("update", lambda: ops.gbm_update(event_d, tgroup_d, state, tab, prm, m, evalm=evalm_d))
    if P:
        timed("grad", lambda: ops.gbm_grad(mult_d, event_d, tgroup_d, rowid_d, sub_d, state, tab, M, seed, pid=pid_d, last=True))
    curve = dict(loglik=state["loglik"].cpu().numpy())
    if evalm_d is not None:
        c2, cm = state["conc2"].cpu().numpy(), state["comparable"].cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            curve.update(conc2=c2, comparable=cm, c_index=np.where(cm > 0, c2 / (2.0 * np.maximum(cm, 1)), np.nan))
    if trace:
        tr["qg"], tr["qh"] = [torch.stack(tr[k]) if tr[k] else None for k in ("qg", "qh")]
    hy.update(bins=np.int64(B), seed=np.int64(int(seed)))
    return Booster(tab, edges, p, hy, ids, curve, state["F"][:, torch.from_numpy(inv).to(dev)] if P else state["F"], tr)


def select_rounds(inner_c):
    """inner_c: [G, J, M] inner-fold C-index of grid point g after m + 1 rounds (NaN: fold not scored) -> (grid index, round count,
    mean curve [G, M]): the best mean over the scored inner folds; ties go to the fewer rounds, then the earlier grid point.  A (grid
    point, round) no fold scored counts as -inf; if nothing was scored at all: (0, 1)."""
    c = np.asarray(inner_c, np.float64)
    cnt = (~np.isnan(c)).sum(1)
    with np.errstate(invalid="ignore"):
        mean = np.where(cnt > 0, np.nansum(c, 1) / np.maximum(cnt, 1), -np.inf)
    g, m = np.nonzero(mean == mean.max())
    k = np.lexsort((g, m))[0]                           # the fewest rounds first, then the earliest grid point
    return int(g[k]), int(m[k]) + 1, mean


def default_grid(learning_rate=(0.1,), max_depth=(2,)):
    return [dict(learning_rate=float(a), max_depth=int(d)) for a in learning_rate for d in max_depth]


def nested_cv(cohort, folds, inner=5, rounds=300, grid=None, seed=0, *, min_leaf=10, l2=1.0, min_gain=0.0, subsample=1.0, colsample=1.0,
              bins=32, x=None, timings=None, shap=False):
    """Nested cross-validation of the boosted Cox trees: all K (J + 1) |grid| problems in ONE fit (one fit per outer fold when the cohort
    carries per-fold gene matrices, gene_select.fold_matrix: one matrix per call; the problems keep their ids).  grid: a list of dicts
    overriding learning_rate / max_depth / min_leaf / l2 / min_gain / subsample / colsample (None: one point, the defaults).  Problem
    (f, j, g), id (f (J + 1) + j) |grid| + g: j < J trains on outer fold f's training patients without inner fold j (coxnet.nested_problems)
    and is scored on that inner fold after every round; j = J trains on all of them.  Per outer fold the (grid point, round count) with the
    best mean inner C-index is chosen (select_rounds) and the validation fold is scored ONCE at that choice through predict; the curve of
    the validation fold is recorded (outer_curve) and never consulted.
    -> list per fold of dict(fold, grid_index, grid_point, rounds, c_index, inner [G, J, M], inner_mean [G, M], outer_curve [G, M],
    val_rows, val_F, train_rows, train_F, importance = (counts, gain sums) of the chosen booster's first `rounds` rounds, n_train, n_val,
    booster, problem).  shap=True adds `shap`: the TreeSHAP values (Booster.shap -> tree_shap.ShapValues, one group) of the chosen booster
    at the chosen round count on that fold's VALIDATION rows only, in val_rows' order: out-of-fold, so honest."""
    import torch
    from . import coxnet, gene_select
    from .survival_stats import concordance_index
    grid = [dict()] if not grid else list(grid)
    base = dict(learning_rate=0.1, max_depth=2, min_leaf=min_leaf, l2=l2, min_gain=min_gain, subsample=subsample, colsample=colsample)
    pts = [dict(base, **g) for g in grid]
    rr, mults, plan = coxnet.nested_problems(cohort, folds, inner, seed)
    K, J1, n = mults.shape
    J, G, M = J1 - 1, len(pts), int(rounds)
    N = int(to_numpy(cohort["label"]).shape[0])
    per_fold = "rnaseq_folds" in cohort and x is None
    groups = [[f] for f in range(K)] if per_fold else [list(range(K))]
    results = [None] * K
    for grp in groups:
        xg = gene_select.fold_matrix(cohort, grp[0] if per_fold else None) if x is None else x
        xe = xg[torch.as_tensor(rr.rows, device=xg.device)].contiguous()
        m = np.repeat(mults[grp].reshape(-1, n), G, axis=0)                     # [(f, j, g)] rows
        ev = np.zeros((len(grp), J1, G, n), bool)
        for i, f in enumerate(grp):
            for j in range(J):
                ev[i, j, :, rr.positions(plan[f]["inner_val"][j], N)] = True
            ev[i, J, :, rr.positions(plan[f]["val"], N)] = True
        ids = np.concatenate([np.arange(f * J1 * G, (f + 1) * J1 * G) for f in grp])
        kw = {k: np.tile([pt[k] for pt in pts], len(grp) * J1) for k in base}
        bst = fit(xe, rr.time, rr.event, m, rounds=M, bins=bins, seed=seed, eval_masks=ev.reshape(-1, n), problem_ids=ids, timings=timings, **kw)
        cidx = bst.curve["c_index"].reshape(len(grp), J1, G, M)
        for i, f in enumerate(grp):
            inner_c = np.transpose(cidx[i, :J], (1, 0, 2))                      # [G, J, M]
            g, r, mean = select_rounds(inner_c)
            prob = (i * J1 + J) * G + g
            tr, va = rr.positions(plan[f]["train"], N), rr.positions(plan[f]["val"], N)
            Fp = bst.predict(xe, rounds=r)[prob]
            try:
                c = float(concordance_index(rr.time[va], -Fp[va], rr.event[va]))
            except ZeroDivisionError:
                c = float("nan")
            results[f] = dict(fold=f, grid_index=g, grid_point=pts[g], rounds=r, c_index=c, inner=inner_c, inner_mean=mean,
                              outer_curve=cidx[i, J], val_rows=plan[f]["val"], val_F=Fp[va], train_rows=plan[f]["train"], train_F=Fp[tr],
                              importance=bst.importance([prob], r), n_train=int(len(tr)), n_val=int(len(va)), booster=bst, problem=prob)
            if shap:
                results[f]["shap"] = bst.shap(xe[torch.as_tensor(va, device=xe.device)].contiguous(), problems=[prob], rounds=r)
    return results
