"""CPU restatement of the diversity-aware re-ranking (b4r_rerank_diverse, include/b4r.h), for the diversity tests only: numpy fp32
on top of tests/catalogue_ref.py (the fma chain is oracle/rank_oracle.c's, through chain_scores).  rnorm is an input, so a comparison
with the kernel fed the same rnorm is bit for bit and does not depend on a device reciprocal square root.  Every product and
difference of the mmr formula is rounded through np.float32 on its own."""
import numpy as np

from tests import catalogue_ref as ref

F32 = np.float32


def sim_matrix(table, rnorm):
    """sim[q, c] = fl32((chain_k(qhat_q[k] * table[c][k]) + 0.0f) * rnorm[c]) with qhat_q = fl32(table[q] * rnorm[q]): [V, V] float32,
    b4r_item_neighbours' cosine of (query q, item c).  Not symmetric in bits."""
    table = np.ascontiguousarray(table, F32)
    rnorm = np.asarray(rnorm, F32)
    qhat = (table * rnorm[:, None]).astype(F32)
    return ref.scaled(ref.chain_scores(qhat, table), rnorm)


def rerank(table, rnorm, pool_ids, pool_scores, lam, K, sim=None):
    """b4r_rerank_diverse restated; all rows advance together, one pick per step.  sim: sim_matrix(table, rnorm) when the caller
    has it already.  Returns (ids [R, K] int64, scores [R, K] float32, mmr [R, K] float32)."""
    ids = np.asarray(pool_ids, np.int64)
    sc = np.asarray(pool_scores, F32)
    R, M = ids.shape
    V = np.asarray(table).shape[0]
    assert 1 <= M <= 1024 and 0 <= K <= M
    if sim is None:
        sim = sim_matrix(table, rnorm)
    lam = F32(lam)
    rest = F32(F32(1.0) - lam)
    live = (ids >= 0) & (ids < V) & np.isfinite(sc)
    item = np.where(live, ids, 0)
    with np.errstate(all="ignore"):
        plus = (sc + F32(0.0)).astype(F32)                         # -0.0 counts as +0.0 in s_max / s_min
        smax = np.where(live, plus, -np.inf).astype(F32).max(axis=1)
        smin = np.where(live, plus, np.inf).astype(F32).min(axis=1)
        span = (smax - smin).astype(F32)
        rel = ((sc - smin[:, None]).astype(F32) / span[:, None]).astype(F32)
    rel = np.where((smax == smin)[:, None], F32(1.0), rel).astype(F32)
    pen = np.zeros((R, M), F32)
    is_open = live.copy()
    out_ids = np.full((R, K), -1, np.int64)
    out_sc = np.full((R, K), -np.inf, F32)
    out_mmr = np.full((R, K), -np.inf, F32)
    rows = np.arange(R)
    for t in range(K):
        with np.errstate(all="ignore"):
            a = (lam * rel).astype(F32)
            b = (rest * pen).astype(F32)
            mmr = (a - b).astype(F32)
        has = is_open.any(axis=1)
        if not has.any():
            break
        # the largest mmr among the open entries, the first (lowest p) of equals; -0.0 == +0.0 as floats
        best = np.where(is_open, mmr, -np.inf).max(axis=1)
        w = np.argmax(is_open & (mmr == best[:, None]), axis=1)
        hr = rows[has]
        out_ids[hr, t] = ids[hr, w[hr]]
        out_sc[hr, t] = sc[hr, w[hr]]
        out_mmr[hr, t] = mmr[hr, w[hr]]
        is_open[hr, w[hr]] = False
        q = item[rows, w]
        s = sim[q[:, None], item]                                  # [R, M]: sim(c, q), the picked item as the query
        new = s if t == 0 else np.where(s > pen, s, pen)           # the earlier value stays on equality
        pen = np.where(has[:, None], new, pen).astype(F32)
    return out_ids, out_sc, out_mmr
