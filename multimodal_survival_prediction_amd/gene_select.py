"""Per-fold gene selection: a univariate Cox score screen of every RNA-seq column, inside each cross-validation fold.

The reference's only feature selection is unsupervised and happens once, before the split (top 5000 genes by variance,
preprocess_genomic.py:119-126); "feature selection (5005 genes -> top 500)" is on its list of future work (final_comparison.py:331-335).
A supervised screen has to see a fold's TRAINING patients only -- otherwise the validation C-index is contaminated by the labels -- so it
runs once per fold, and with stability selection once per bootstrap resample of the fold as well.

The statistic is the Cox partial-likelihood score test of one gene at beta = 0 with Breslow ties, in closed form (include/mmsurv.h:
GeneScreenP): for an ordered list of patient rows (time descending) U = sum_k a_k x_k, V = sum_k b_k x_k^2 - sum_k q_k S1_k^2 with S1
the running column sum, stat = U^2 / V (chi-square, 1 dof).  a, b, q depend on the labels only (score_coefficients, on
risk_sets.risk_set_table, in float64); the sums over the patients for all genes of all problems are ONE launch of mms_gene_screen over
the device-resident matrix.  A row listed twice is a tie, so a bootstrap resample is an index list with repeats and needs no weights.  There is no CPU
fallback for the sums, like the rest of the package.

Reproducibility contract of the resamples (select_genes(stability=R)): fold f's multiplicities are
bootstrap.bootstrap_weights(n_f, R, seed=[seed, f]) over its eligible training rows in the order given; resample r lists every row as
often as it was drawn."""
import json
from dataclasses import dataclass, field

import numpy as np

from .risk_sets import risk_set_table, score_chi2 as score_statistic, to_numpy


def score_coefficients(time, event, rows=None):
    """-> (order, a, b, q) of one problem.  time / event: per-patient arrays; rows: the problem's patient rows (repeats allowed; None =
    all patients once).  order: positions into `rows`, time descending (stable: equal times keep their order in `rows`) -- the problem's
    risk order is rows[order]; a, b, q: float64 per position of that order (GeneScreenP in include/mmsurv.h)."""
    T = risk_set_table(time, event, rows)
    q = np.zeros(len(T.e))
    q[T.last] = T.d_u / (T.n_u * T.n_u)
    return T.order, T.e - T.b, T.b, q


def cox_score_screen(x_dev, time, event, index_lists):
    """Score test of every column of x_dev (fp32 [N, G] device tensor; a padded row pitch is fine) on every problem of index_lists (each
    a list of patient rows, repeats allowed) in ONE launch -> (U, V, stat): float64 numpy [P, G]; stat = U^2 / V, and 0 wherever V <= 0
    (a constant gene, a problem without events, a single-row problem)."""
    from . import ops
    time, event = to_numpy(time), to_numpy(event)
    off, rows, coefs = [0], [], []
    for lst in index_lists:
        lst = np.asarray(lst, dtype=np.int64).reshape(-1)
        order, a, b, q = score_coefficients(time, event, lst)
        rows.append(lst[order])
        coefs.append(np.stack([a, b, q], 1))
        off.append(off[-1] + len(lst))
    row = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    coef = np.concatenate(coefs) if coefs else np.zeros((0, 3))
    U, V = ops.gene_screen(x_dev, off, row, coef)
    U, V = U.cpu().numpy(), V.cpu().numpy()
    return U, V, score_statistic(U, V)


def top_k(stat, k):
    """The k largest of stat, the lower gene index winning ties -> their indices in rank order."""
    return np.argsort(-np.asarray(stat, dtype=np.float64), kind="stable")[:k]


def eligible_rows(cohort, indices):
    """The patients of `indices` that have RNA-seq and a survival label, in the order given."""
    idx = np.asarray(to_numpy(indices), dtype=np.int64).reshape(-1)
    ok = to_numpy(cohort["has_survival"]).astype(bool)
    if "mask" in cohort:
        ok = ok & (to_numpy(cohort["mask"])[:, 1] != 0)
    return idx[ok[idx]]


def fold_problems(cohort, train_indices_per_fold, stability=0, seed=0):
    """-> (problems, rows per fold): the index lists of select_genes' launch, fold after fold, a fold's full sample first and its
    `stability` resamples behind it (the module docstring's contract)."""
    from .bootstrap import bootstrap_weights
    event = to_numpy(cohort["label"])[:, 1]
    problems, rows_f = [], []
    for f, idx in enumerate(train_indices_per_fold):
        rows = eligible_rows(cohort, idx)
        if len(rows) == 0 or not (event[rows] != 0).any():
            raise ValueError("fold %d has no eligible patient with an event (RNA-seq, a survival label and event = 1)" % f)
        rows_f.append(rows)
        problems.append(rows)
        if stability:
            w = bootstrap_weights(len(rows), stability, [int(seed), f])
            problems += [np.repeat(rows, w[r]) for r in range(stability)]
    return problems, rows_f


def rank_fold(stat_full, stat_resamples, k):
    """-> (the k winners in rank order, frequency or None).  Without resamples: by stat descending, then gene index.  With them: a
    resample without any positive stat is left out; frequency[j] = share of the others whose top-k holds gene j; rank by frequency,
    then the full-sample stat, then gene index."""
    G = len(stat_full)
    if stat_resamples is None or len(stat_resamples) == 0:
        return top_k(stat_full, k), None
    keep = [s for s in stat_resamples if (s > 0).any()]
    freq = np.zeros(G)
    for s in keep:
        freq[top_k(s, k)] += 1.0
    if keep:
        freq /= len(keep)
    return np.lexsort((np.arange(G), -np.asarray(stat_full, dtype=np.float64), -freq))[:k], freq


@dataclass
class GeneSelection:
    columns: list                      # per fold: int64 [k] selected gene columns, ascending
    k: int
    n_genes: int
    stability: int = 0
    seed: int = 0
    rows_screened: list = field(default_factory=list)     # per fold: patients in its full-sample problem
    frequency: list = None             # per fold float64 [G] (stability > 0)
    stat: list = None                  # per fold float64 [G]: the full-sample statistic (not saved)
    gene_names: list = None            # per fold: the selected genes' names (cohort["gene_names"]), or None
    folds: list = None                 # the fold numbers of `columns` (None: 0 .. K-1)

    def fold_ids(self):
        return list(range(len(self.columns))) if self.folds is None else list(self.folds)

    def columns_of(self, fold):
        return self.columns[self.fold_ids().index(int(fold))]

    def apply(self, cohort):
        """Materialise one [N, k] matrix per fold next to cohort["rnaseq"] (same memory: HBM or pinned host) as cohort["rnaseq_folds"]:
        rows 16-byte aligned, pitch a multiple of 4 floats.  The batch paths (data.BatchLoader(fold=), the fold groups' gather launch) read
        fold f's matrix in place of the full one; an absent patient's all-zero row stays all-zero.  -> the cohort."""
        import torch
        x = cohort["rnaseq"]
        if x.shape[1] != self.n_genes:
            raise ValueError("the selection was made over %d genes, the cohort has %d" % (self.n_genes, x.shape[1]))
        ld = (self.k + 3) // 4 * 4
        mats = []
        for cols in self.columns:
            full = torch.zeros(x.shape[0], ld, dtype=x.dtype, device=x.device)
            if x.is_pinned():
                full = full.pin_memory()
            full[:, :self.k] = x[:, torch.as_tensor(np.asarray(cols), device=x.device)]
            mats.append(full[:, :self.k])
        for key in [key for key in cohort if str(key).startswith("_gather_view_")]:       # (views made before the matrices existed)
            del cohort[key]
        cohort["rnaseq_folds"] = mats
        cohort["rnaseq_fold_ids"] = self.fold_ids()
        cohort["gene_columns"] = [np.asarray(c, dtype=np.int64) for c in self.columns]
        return cohort

    def _entry(self, i):
        e = dict(fold=self.fold_ids()[i], columns=[int(c) for c in self.columns[i]],
                 rows_screened=int(self.rows_screened[i]) if i < len(self.rows_screened) else None)
        if self.gene_names is not None:
            e["genes"] = list(self.gene_names[i])
        return e

    def save(self, path, fold=None):
        """JSON: k, the number of genes screened, the stability resamples R, the seed and per fold its number, column indices, gene
        names (when the cohort had them) and the number of rows screened.  fold: write that fold's entry alone."""
        ids = self.fold_ids()
        which = range(len(ids)) if fold is None else [ids.index(int(fold))]
        with open(path, "w") as f:
            json.dump(dict(k=int(self.k), n_genes=int(self.n_genes), stability=int(self.stability), seed=int(self.seed),
                           folds=[self._entry(i) for i in which]), f, indent=2)

    @classmethod
    def load(cls, path):
        with open(path) as f:
            d = json.load(f)
        fs = d["folds"]
        names = [e["genes"] for e in fs] if fs and all("genes" in e for e in fs) else None
        return cls(columns=[np.asarray(e["columns"], dtype=np.int64) for e in fs], k=int(d["k"]), n_genes=int(d["n_genes"]),
                   stability=int(d["stability"]), seed=int(d["seed"]), rows_screened=[e["rows_screened"] for e in fs],
                   gene_names=names, folds=[int(e["fold"]) for e in fs])


def fold_matrix(cohort, fold):
    """The RNA-seq matrix fold `fold`'s model reads: cohort["rnaseq"] unless GeneSelection.apply left per-fold matrices; then the fold
    must be named (there is no default: a model of width k cannot read another fold's genes by accident)."""
    if "rnaseq_folds" not in cohort:
        return cohort["rnaseq"]
    if fold is None:
        raise ValueError("this cohort carries per-fold gene matrices (GeneSelection.apply): name the fold (BatchLoader(fold=), "
                         "FoldGroupEngine(folds=))")
    ids = cohort.get("rnaseq_fold_ids") or list(range(len(cohort["rnaseq_folds"])))
    if int(fold) not in ids:
        raise ValueError("fold %r has no gene matrix in this cohort (folds %s)" % (fold, ids))
    return cohort["rnaseq_folds"][ids.index(int(fold))]


def select_genes(cohort, train_indices_per_fold, k, stability=0, seed=0):
    """Per-fold top-k genes by the univariate Cox score test on each fold's training patients that have RNA-seq and a survival label.
    cohort["rnaseq"] must live in HBM (data.cohort_to).  stability = R > 0: stability selection over R bootstrap resamples per fold (the
    module docstring); all K (R + 1) problems are one launch.  -> GeneSelection."""
    x = cohort["rnaseq"]
    G = int(x.shape[1])
    k, stability = int(k), int(stability)
    if k < 1 or k > G:
        raise ValueError("k must be in 1..%d (the cohort's genes), got %d" % (G, k))
    if stability < 0:
        raise ValueError("stability must be >= 0 resamples")
    problems, rows_f = fold_problems(cohort, train_indices_per_fold, stability, seed)
    label = to_numpy(cohort["label"])
    _, _, stat = cox_score_screen(x, label[:, 0], label[:, 1], problems)
    cols, freqs, stats = [], [], []
    for f in range(len(rows_f)):
        s = stat[f * (stability + 1):(f + 1) * (stability + 1)]
        win, freq = rank_fold(s[0], s[1:] if stability else None, k)
        cols.append(np.sort(win).astype(np.int64))
        freqs.append(freq)
        stats.append(s[0])
    names = cohort.get("gene_names")
    return GeneSelection(columns=cols, k=k, n_genes=G, stability=stability, seed=int(seed), rows_screened=[len(r) for r in rows_f],
                         frequency=freqs if stability else None, stat=stats,
                         gene_names=[[names[int(c)] for c in cc] for cc in cols] if names is not None else None)
