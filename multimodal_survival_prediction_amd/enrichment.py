"""Gene-set enrichment of the Cox scores with a label-permutation null (Subramanian et al. 2005, the phenotype-permutation form).

The statistic.  rows = the analysed patients (gene_select.eligible_rows), n >= 2, in the order given.  m [n] = the null martingale
residuals with Breslow ties, m_i = delta_i - sum over the event times u <= t_i of d_u / n_u (null_residuals: risk_sets.risk_set_table's
e - b scattered back to list positions; it is the `a` of gene_select.score_coefficients, and sum m = 0).  At beta = 0 the Cox score of
gene g is U_g = sum_i m_i x_ig, and relabelling the patients permutes m, so with perm [R + 1, n] (row 0 the identity, row r >= 1 =
risk_strata.draw_permutations(n, R, seed)[r - 1]; replicate r gives list position i the residual m[perm[r][i]])

    Z[r][g] = s_g * sum_i m[perm[r][i]] x[rows[i]][g],      s_g = 1 / sqrt( (sum m^2 / (n - 1)) * sum_i (x_ig - mean_g)^2 ),

the exact permutation variance of the sum (because sum m = 0); s_g = 0 and Z = 0 for a constant gene or when sum m^2 = 0.  This Z is
NOT the U / sqrt(V) of gene_select.cox_score_screen, whose V is the model-based (information) variance: the numerators agree up to
summation order, the denominators do not.  All R + 1 relabellings of all G genes are one fp64 matrix product on the matrix cores
(ops.gsea_scores), and the R + 1 rankings and (R + 1) x S running sums are one launch (ops.gsea_es); include/mmsurv.h (GseaScoreP,
GseaEsP) has the ranking (Z descending, the lower gene index first), the enrichment score, its peak and the weight 0 / 1 rule.  There is
no CPU fallback for either.

Per set (summarise; host, numpy, float64): e_j = ES[0][j] and its sign class (>= 0 or < 0); only the nulls e_rj of the same class are
compared with it.  p_j = (1 + #{r: |e_rj| >= |e_j|}) / (1 + #same-class nulls).  NES = ES / the mean |ES| of the same-class nulls of that
set (nan without any); null NES values are formed the same way, by their own class.  fdr of NES_j >= 0 = (share of all non-negative
null NES, pooled over sets and replicates, that are >= NES_j) / (share of the non-negative observed NES that are >= NES_j), capped at 1,
mirrored for negative values; nan NES are left out of the pools.  fwer_j = (1 + #{r: max_k |NES_rk| >= |NES_j|}) / (R + 1).  The
leading edge is the members ranked at or before the peak when ES >= 0, after it when ES < 0.

Preranked mode (enrich_preranked) serves scores without labels behind them (attribution gene scores, forest importances, elastic-net
coefficients): ONE row of scores, and replicate r >= 1 ranks z'[g] = z[gperm[r - 1][g]], gperm = draw_permutations(G, R, seed).  That
null shuffles gene labels: it IGNORES gene-gene correlation and is anti-conservative; wherever labels exist, enrich (the label
permutation) is the analysis to run."""
import json
from dataclasses import dataclass, field

import numpy as np

from .risk_sets import risk_set_table, to_numpy


def read_gmt(path, descriptions=False):
    """A .gmt file (tab-separated lines: name, description, genes...) -> {name: [genes]} in file order; duplicate genes inside a set are
    collapsed (the first occurrence stays), empty fields are skipped, a set name given twice raises.  descriptions: -> (sets,
    {name: description})."""
    sets, desc = {}, {}
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            parts = line.split("\t")
            if len(parts) < 2:
                raise ValueError("%s:%d: a .gmt line holds name, description and genes, tab-separated" % (path, ln))
            name = parts[0].strip()
            if not name or name in sets:
                raise ValueError("%s:%d: %s" % (path, ln, "empty set name" if not name else "set name %r appears twice" % name))
            sets[name] = list(dict.fromkeys(g.strip() for g in parts[2:] if g.strip()))
            desc[name] = parts[1]
    return (sets, desc) if descriptions else sets


def write_gmt(path, sets, descriptions=None):
    """{name: [genes]} -> a .gmt file (read_gmt's inverse; the description column is descriptions[name] or "na")."""
    with open(path, "w") as f:
        for name, genes in sets.items():
            bad = [s for s in [name] + list(genes) if "\t" in str(s) or "\n" in str(s)]
            if bad:
                raise ValueError("a tab or a line break in %r" % bad[0])
            f.write("\t".join([str(name), str((descriptions or {}).get(name, "na"))] + [str(g) for g in genes]) + "\n")


def index_sets(sets, gene_names, min_size=15, max_size=500):
    """Match the sets' gene names exactly against gene_names (the matrix columns) -> (set_off int64 [S + 1], set_gene int64, the kept
    names, report).  A set is kept when min_size <= its matched genes <= min(max_size, G - 1); report = dict(dropped = {name: "too
    small (k matched)" / "too large (k matched)"}, unmatched = {name: [its genes not among the columns]} for every set that has any,
    kept or not)."""
    col = {}
    for j, g in enumerate(gene_names):
        col.setdefault(str(g), j)
    G = len(gene_names)
    off, gene, kept, dropped, unmatched = [0], [], [], {}, {}
    for name, genes in sets.items():
        genes = list(dict.fromkeys(str(g) for g in genes))
        idx = sorted({col[g] for g in genes if g in col})
        miss = [g for g in genes if g not in col]
        if miss:
            unmatched[name] = miss
        if len(idx) < max(int(min_size), 1):
            dropped[name] = "too small (%d matched)" % len(idx)
        elif len(idx) > min(int(max_size), G - 1):
            dropped[name] = "too large (%d matched)" % len(idx)
        else:
            kept.append(name)
            gene += idx
            off.append(len(gene))
    return np.asarray(off, dtype=np.int64), np.asarray(gene, dtype=np.int64), kept, dict(dropped=dropped, unmatched=unmatched)


def null_residuals(time, event, rows=None):
    """-> m float64 [n]: the martingale residuals of the null Cox model (Breslow ties) of the patients `rows` (None: all), per LIST
    position; sum m = 0 up to rounding."""
    T = risk_set_table(to_numpy(time), to_numpy(event), rows)
    m = np.empty(len(T.e))
    m[T.order] = T.e - T.b
    return m


def ranking(z):
    """-> the genes in rank order: z descending, the lower gene index first on equal values (-0.0 equals +0.0)."""
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    return np.lexsort((np.arange(len(z)), -z))


def _class_means(null):
    """-> (mean of the null ES >= 0, mean |null ES < 0|) per set, nan where a class is empty"""
    S = null.shape[1]
    mp, mn = np.full(S, np.nan), np.full(S, np.nan)
    for j in range(S):
        col = null[:, j]
        pos = col >= 0
        if pos.any():
            mp[j] = np.mean(col[pos])
        if not pos.all():
            mn[j] = np.mean(-col[~pos])
    return mp, mn


def _tail_share(pool_sorted, v, upper):
    """share of the sorted pool that is >= v (upper) or <= v"""
    n = len(pool_sorted)
    c = n - np.searchsorted(pool_sorted, v, side="left") if upper else np.searchsorted(pool_sorted, v, side="right")
    return c / n


def summarise(es):
    """es: float64 [R + 1, S], row 0 observed -> dict(es, nes, p, fdr, fwer: float64 [S]) by the module docstring's formulas.  Pure
    numpy."""
    es = np.asarray(es, dtype=np.float64)
    if es.ndim != 2 or es.shape[0] < 1:
        raise ValueError("es must be [R + 1, S]")
    obs, null = es[0], es[1:]
    R, S = null.shape
    up, npos = obs >= 0, null >= 0
    same = np.where(up[None, :], npos, ~npos)
    p = (1.0 + (same & (np.abs(null) >= np.abs(obs)[None, :])).sum(0)) / (1.0 + same.sum(0))
    mp, mn = _class_means(null)
    with np.errstate(divide="ignore", invalid="ignore"):
        nes = obs / np.where(up, mp, mn)
        nnes = null / np.where(npos, mp[None, :], mn[None, :])
    pool_pos, pool_neg = np.sort(nnes[npos & ~np.isnan(nnes)]), np.sort(nnes[~npos & ~np.isnan(nnes)])
    obs_pos, obs_neg = np.sort(nes[up & ~np.isnan(nes)]), np.sort(nes[~up & ~np.isnan(nes)])
    absmax = np.fmax.reduce(np.abs(nnes), axis=1, initial=-np.inf) if S else np.full(R, -np.inf)
    fdr, fwer = np.full(S, np.nan), np.full(S, np.nan)
    for j in range(S):
        if np.isnan(nes[j]):
            continue
        pool, ob = (pool_pos, obs_pos) if up[j] else (pool_neg, obs_neg)
        fdr[j] = min(1.0, _tail_share(pool, nes[j], up[j]) / _tail_share(ob, nes[j], up[j]))
        fwer[j] = (1.0 + (absmax >= abs(nes[j])).sum()) / (R + 1.0)
    return dict(es=obs.copy(), nes=nes, p=p, fdr=fdr, fwer=fwer)


def leading_edge(z, members, es, peak):
    """-> the members (gene indices) of the leading edge in rank order: ranked at or before `peak` when es >= 0, after it otherwise"""
    order = ranking(z)
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    mem = np.asarray(members, dtype=np.int64)
    mem = mem[np.argsort(rank[mem])]
    r = rank[mem]
    return mem[r <= peak] if es >= 0 else mem[r > peak]


@dataclass
class EnrichmentResult:
    names: list                         # the kept sets
    size: np.ndarray                    # int64 [S] matched genes
    es: np.ndarray
    nes: np.ndarray
    p: np.ndarray
    fdr: np.ndarray
    fwer: np.ndarray
    peak: np.ndarray                    # int64 [S] 0-based position of the observed ranking
    leading_edge: list                  # per set: gene names in rank order
    z: np.ndarray                       # float64 [G] the observed gene statistics
    mode: str = "label_permutation"     # or "preranked"
    R: int = 0
    seed: int = 0
    weight: int = 1
    n: int = 0                          # analysed patients (0: preranked)
    report: dict = field(default_factory=dict)     # index_sets' report

    def to_frame(self):
        import pandas as pd
        return pd.DataFrame({"set": self.names, "size": self.size, "es": self.es, "nes": self.nes, "p": self.p, "fdr": self.fdr,
                             "fwer": self.fwer, "peak": self.peak, "leading_edge_size": [len(e) for e in self.leading_edge]})

    def save(self, path):
        """JSON: the settings, index_sets' report and per set its name, size, ES, NES, p, fdr, fwer, peak and leading-edge genes (nan as
        null)."""
        num = lambda v: None if np.isnan(v) else float(v)       # noqa: E731
        sets = [dict(set=self.names[j], size=int(self.size[j]), es=float(self.es[j]), nes=num(self.nes[j]), p=float(self.p[j]),
                     fdr=num(self.fdr[j]), fwer=num(self.fwer[j]), peak=int(self.peak[j]), leading_edge=list(self.leading_edge[j]))
                for j in range(len(self.names))]
        with open(path, "w") as f:
            json.dump(dict(mode=self.mode, R=int(self.R), seed=int(self.seed), weight=int(self.weight), n=int(self.n),
                           n_genes=int(len(self.z)), report=self.report, sets=sets), f, indent=2)


def _sets_of(sets):
    return read_gmt(sets) if isinstance(sets, (str, bytes)) or hasattr(sets, "__fspath__") else sets


def _finish(es, peak, z, off, gene, kept, names, report, **meta):
    s = summarise(es)
    edges = [[names[int(g)] for g in leading_edge(z, gene[off[j]:off[j + 1]], s["es"][j], int(peak[j]))] for j in range(len(kept))]
    return EnrichmentResult(names=list(kept), size=np.diff(off), es=s["es"], nes=s["nes"], p=s["p"], fdr=s["fdr"], fwer=s["fwer"],
                            peak=np.asarray(peak, dtype=np.int64), leading_edge=edges, z=np.asarray(z, dtype=np.float64), report=report,
                            **meta)


def permutation_table(n, R, seed=0):
    """-> int64 [R + 1, n]: row 0 the identity, row r >= 1 = risk_strata.draw_permutations(n, R, seed)[r - 1]"""
    from .risk_strata import draw_permutations
    return np.concatenate([np.arange(n, dtype=np.int64)[None, :], draw_permutations(n, R, seed)], 0)


def enrich(cohort, sets, rows=None, R=1000, seed=0, weight=1, min_size=15, max_size=500):
    """Label-permutation enrichment of `sets` ({name: [gene names]} or a .gmt path) on the cohort's patients `rows` (None: all) that
    have RNA-seq and a survival label.  cohort["rnaseq"] must live in HBM (data.cohort_to); genes are matched by name against
    cohort["gene_names"], or transfer.default_gene_names(G) when the cohort carries none.  -> EnrichmentResult."""
    from . import ops
    from .gene_select import eligible_rows
    from .transfer import default_gene_names
    x = cohort["rnaseq"]
    if not (hasattr(x, "is_cuda") and x.is_cuda):
        raise ValueError("cohort['rnaseq'] must live in HBM (data.cohort_to): the scores are computed on the GPU, there is no CPU fallback")
    G, R = int(x.shape[1]), int(R)
    if R < 1:
        raise ValueError("R must be >= 1 relabellings")
    rows = eligible_rows(cohort, np.arange(x.shape[0]) if rows is None else rows)
    if len(rows) < 2:
        raise ValueError("enrichment needs at least 2 patients with RNA-seq and a survival label, got %d" % len(rows))
    names = cohort.get("gene_names")
    names = default_gene_names(G) if names is None else list(names)
    off, gene, kept, report = index_sets(_sets_of(sets), names, min_size, max_size)
    if not kept:
        raise ValueError("no gene set is left after matching and the size limits %d..%d (dropped: %d)" % (min_size, max_size, len(report["dropped"])))
    label = to_numpy(cohort["label"])
    m = null_residuals(label[:, 0], label[:, 1], rows)
    _, Z = ops.gsea_scores(x, rows, m, permutation_table(len(rows), R, seed))
    es, peak = ops.gsea_es(Z, off, gene, weight=weight)
    return _finish(es.cpu().numpy(), peak[0].cpu().numpy(), Z[0].cpu().numpy(), off, gene, kept, names, report, mode="label_permutation",
                   R=R, seed=int(seed), weight=int(weight), n=len(rows))


def enrich_preranked(scores, gene_names, sets, R=1000, seed=0, weight=1, min_size=15, max_size=500):
    """Preranked enrichment of one score per gene (scores [G], finite; gene_names [G]) with a gene-label permutation null.  This null
    ignores gene-gene correlation and is anti-conservative (the module docstring): use enrich whenever the labels exist.
    -> EnrichmentResult."""
    from . import ops
    from .risk_strata import draw_permutations
    z = np.asarray(to_numpy(scores), dtype=np.float64).reshape(-1)
    names, R = list(gene_names), int(R)
    if len(names) != len(z) or not np.isfinite(z).all():
        raise ValueError("scores must hold one finite value per gene name")
    if R < 1:
        raise ValueError("R must be >= 1 permutations")
    off, gene, kept, report = index_sets(_sets_of(sets), names, min_size, max_size)
    if not kept:
        raise ValueError("no gene set is left after matching and the size limits %d..%d (dropped: %d)" % (min_size, max_size, len(report["dropped"])))
    es, peak = ops.gsea_es(z[None, :], off, gene, gperm=draw_permutations(len(z), R, seed), weight=weight)
    return _finish(es.cpu().numpy(), peak[0].cpu().numpy(), z, off, gene, kept, names, report, mode="preranked", R=R, seed=int(seed),
                   weight=int(weight), n=0)
