"""CPU restatement of b4r_item_ranks and b4r_rank_metrics_multi (include/b4r.h), for the item-rank tests only.  The scores come from
tests/catalogue_ref.chain_scores (oracle/rank_oracle.c) and its one-multiply scale step; the ranks are counted in integers with numpy
on the order-preserving image of the scores; the seven metric families are summed with math.fsum over math.log2 terms."""
import math

import numpy as np

STRICT, SELF, JOINT = 0, 1, 2
COUNT, HIT, NDCG, MRR, RECALL, MAP, AUC = range(7)


def score_image(s):
    """uint32: a > b <=> image(a) > image(b); -0.0 counts as +0.0 (b4r_wave.h: score_key)"""
    u = np.ascontiguousarray(s, np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def item_keys(sc_row):
    """uint64 per item: j stands before q <=> key(j) > key(q) (score descending, ties to the lower id)"""
    j = np.arange(sc_row.shape[0], dtype=np.uint64)
    return (score_image(sc_row).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - j)


def item_ranks(sc, ok, query, first, mode):
    """sc [R, V] fp32: s(r, j); ok [R, V] bool: A(r) (catalogue_ref.allowed_mask without gt); query [R, Q] int64.
    Returns (ranks int32 [R, Q], query_scores fp32 [R, Q], row_n int32 [R], member uint8 [R, Q])."""
    R, V = sc.shape
    Q = query.shape[1]
    ranks = np.zeros((R, Q), np.int32)
    scores = np.full((R, Q), -np.inf, np.float32)
    member = np.zeros((R, Q), np.uint8)
    row_n = np.zeros(R, np.int32)
    for r in range(R):
        keys = item_keys(sc[r])
        valid = [first <= int(q) < V for q in query[r]]
        allowed = ok[r].copy()
        if mode == JOINT:
            for q, v in zip(query[r], valid):
                if v:
                    allowed[int(q)] = True
        ranked = np.sort(keys[allowed])
        row_n[r] = ranked.size
        for i, (q, v) in enumerate(zip(query[r], valid)):
            if not v:
                continue
            q = int(q)
            scores[r, i] = sc[r, q]
            member[r, i] = 1 if ok[r, q] else 0
            if mode == STRICT and not ok[r, q]:
                continue
            ranks[r, i] = 1 + ranked.size - int(np.searchsorted(ranked, keys[q], side="right"))   # keys are unique: q never counts itself
    return ranks, scores, row_n, member


def dcg_term(rank):
    return 1.0 if rank == 1 else 1.0 / math.log2(rank + 1.0)


def row_gain(rho, family, k, n_ranked=None):
    """gain of one row: rho = its ranks > 0 (n >= 1 of them), n_ranked = row_n (the AUC family only)"""
    n = len(rho)
    best = min(rho)
    if family == COUNT:
        return float(n)
    if family == HIT:
        return 1.0 if best <= k else 0.0
    if family == MRR:
        return 1.0 / best
    if family == RECALL:
        return sum(1 for v in rho if v <= k) / n
    top = min(n, k)
    if family == NDCG:
        return math.fsum(dcg_term(v) for v in rho if v <= k) / math.fsum(dcg_term(i) for i in range(1, top + 1)) if top > 0 else 0.0
    if family == MAP:
        return math.fsum(sum(1 for w in rho if w <= v) / v for v in rho if v <= k) / top if top > 0 else 0.0
    if family == AUC:
        others = n_ranked - n
        if others <= 0:
            return 1.0
        return math.fsum(1.0 - (v - 1 - sum(1 for w in rho if w < v)) / others for v in rho) / n
    raise ValueError(family)


def multi_metrics(ranks, row_n, table):
    """b4r_rank_metrics_multi restated: table = [(family, cutoff)].  Returns ([gain sum per metric], the rows with a target)."""
    ranks = np.asarray(ranks)
    rows = [[int(v) for v in row if v > 0] for row in ranks]
    live = [(rho, None if row_n is None else int(row_n[r])) for r, rho in enumerate(rows) if rho]
    return [math.fsum(row_gain(rho, fam, k, nr) for rho, nr in live) for fam, k in table], len(live)
