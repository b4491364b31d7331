"""numpy references of the bootstrap pair counts (no GPU, no package code): the DEFINITION on literally resampled arrays and the
bilinear form in the multiplicity vector.  Both return int64 [M + 1, R]: row m = 2*concordant + tied of model m, row M = comparable pairs.
pair_rule 0: e_i and t_j > t_i; 1 (lifelines): additionally e_i and not e_j and t_i == t_j.  strata: pairs inside one stratum only."""
import numpy as np


def pair_matrices(risk, time, event, strata=None, pair_rule=0):
    """-> (S [M, n, n] in {0,1,2}, P [n, n] in {0,1}) as int64; first index i = the member with the observed earlier event."""
    risk = np.atleast_2d(np.asarray(risk))
    t, e = np.asarray(time), np.asarray(event).astype(bool)
    P = e[:, None] & (t[None, :] > t[:, None])
    if pair_rule == 1:
        P = P | (e[:, None] & ~e[None, :] & (t[:, None] == t[None, :]))
    if strata is not None:
        s = np.asarray(strata)
        P = P & (s[:, None] == s[None, :])
    P = P.astype(np.int64)
    S = np.stack([P * (2 * (h[:, None] > h[None, :]).astype(np.int64) + (h[:, None] == h[None, :])) for h in risk])
    return S, P


def literal_counts(risk, time, event, indices, strata=None, pair_rule=0):
    """Gather the arrays by each row of `indices` (bootstrap_indices) and count the pairs of the resampled cohort by broadcasting."""
    risk = np.atleast_2d(np.asarray(risk))
    t, e = np.asarray(time), np.asarray(event)
    out = np.zeros((risk.shape[0] + 1, len(indices)), dtype=np.int64)
    for r, idx in enumerate(indices):
        S, P = pair_matrices(risk[:, idx], t[idx], e[idx], None if strata is None else np.asarray(strata)[idx], pair_rule)
        out[:-1, r] = S.sum(axis=(1, 2))
        out[-1, r] = P.sum()
    return out


def weighted_counts(risk, time, event, weights, strata=None, pair_rule=0, float_matmul=False):
    """w'Sw and w'Pw per row w of `weights` in int64; float_matmul: the products as float64 BLAS matmuls (exact below 2^53), for large n."""
    S, P = pair_matrices(risk, time, event, strata, pair_rule)
    W = np.asarray(weights).astype(np.int64)
    out = np.zeros((len(S) + 1, len(W)), dtype=np.int64)
    for m, A in enumerate(list(S) + [P]):
        if float_matmul:
            Wf = W.astype(np.float64)
            v = ((Wf @ A.astype(np.float64)) * Wf).sum(1)
            assert v.max() < 2.0 ** 53
            out[m] = v.astype(np.int64)
        else:
            out[m] = ((W @ A) * W).sum(1)
    return out


def make_cohort(n, M, seed, n_times=None, n_risks=None, event_rate=0.6, n_strata=0):
    """Few distinct times and risks (ties abound), asymmetric in every array.  -> dict(risk float32 [M, n], time float32, event int, strata)"""
    rng = np.random.default_rng(seed)
    n_times = n_times or max(2, n // 3)
    n_risks = n_risks or max(2, n // 4)
    return dict(risk=(rng.integers(0, n_risks, size=(M, n)) * 0.37 - 1.0).astype(np.float32),
                time=(rng.integers(0, n_times, size=n) * 1.5 + 3.0).astype(np.float32),
                event=(rng.random(n) < event_rate).astype(np.int64),
                strata=rng.integers(0, n_strata, size=n) if n_strata else None)
