"""CPU restatement of the re-ranking under category quotas (b4r_rerank_quota, include/b4r.h), for the quota tests only: tests/diverse_ref.py's
greedy MMR (its sim_matrix and its roundings: every product and difference of the mmr formula goes through np.float32 on its own) with
the caps added.  rnorm is an input, so a comparison with the kernel fed the same rnorm is bit for bit and does not depend on a device
reciprocal square root.

A quota is Quota(item_group [V] ints, n_groups, cap, group_cap = None): item j is in group item_group[j] when that lies in
[0, n_groups), else in none; the group's cap is group_cap[g] when group_cap is given, else cap."""
import collections

import numpy as np

from tests import diverse_ref as dref

F32 = np.float32
Quota = collections.namedtuple("Quota", "item_group n_groups cap group_cap", defaults=(None,))


def entry_groups(quotas, item, live):
    """(grp [A, R, M] int64: the group of every pool entry under every quota, -1 = none; left [A, R, M] int64: that group's cap)"""
    R, M = item.shape
    grp = np.full((len(quotas), R, M), -1, np.int64)
    left = np.ones((len(quotas), R, M), np.int64)
    for a, q in enumerate(quotas):
        g = np.asarray(q.item_group, np.int64)[item]
        has = live & (g >= 0) & (g < q.n_groups)
        grp[a] = np.where(has, g, -1)
        caps = np.full(max(q.n_groups, 1), q.cap, np.int64) if q.group_cap is None else np.asarray(q.group_cap, np.int64)
        left[a] = np.where(has, caps[np.where(has, g, 0)], 1)
    return grp, left


def rerank(table, rnorm, pool_ids, pool_scores, lam, K, quotas, sim=None):
    """b4r_rerank_quota restated; all rows advance together, one pick per step.  sim: dref.sim_matrix(table, rnorm) when the caller
    has it already.  Returns (ids [R, K] int64, scores [R, K] float32, mmr [R, K] float32, pos [R, K] int32)."""
    ids = np.asarray(pool_ids, np.int64)
    sc = np.asarray(pool_scores, F32)
    R, M = ids.shape
    V = np.asarray(table).shape[0]
    assert 1 <= M <= 1024 and 0 <= K <= M and 0 <= len(quotas) <= 4
    if sim is None:
        sim = dref.sim_matrix(table, rnorm)
    lam = F32(lam)
    rest = F32(F32(1.0) - lam)
    live = (ids >= 0) & (ids < V) & np.isfinite(sc)
    item = np.where(live, ids, 0)
    with np.errstate(all="ignore"):
        plus = (sc + F32(0.0)).astype(F32)                         # -0.0 counts as +0.0 in s_max / s_min
        smax = np.where(live, plus, -np.inf).astype(F32).max(axis=1)   # over the live entries, closed or not
        smin = np.where(live, plus, np.inf).astype(F32).min(axis=1)
        span = (smax - smin).astype(F32)
        rel = ((sc - smin[:, None]).astype(F32) / span[:, None]).astype(F32)
    rel = np.where((smax == smin)[:, None], F32(1.0), rel).astype(F32)
    pen = np.zeros((R, M), F32)
    grp, left = entry_groups(quotas, item, live)
    is_open = live & (left > 0).all(axis=0)                        # closed at the start: some group with a cap <= 0
    out_ids = np.full((R, K), -1, np.int64)
    out_sc = np.full((R, K), -np.inf, F32)
    out_mmr = np.full((R, K), -np.inf, F32)
    out_pos = np.full((R, K), -1, np.int32)
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
        out_pos[hr, t] = w[hr]
        is_open[hr, w[hr]] = False
        for a_ in range(len(quotas)):                              # the pick counts against its groups
            wg = grp[a_, rows, w]
            same = is_open & has[:, None] & (wg >= 0)[:, None] & (grp[a_] == wg[:, None])
            left[a_] -= same
            is_open &= ~(same & (left[a_] <= 0))
        q = item[rows, w]
        s = sim[q[:, None], item]                                  # [R, M]: sim(c, q), the picked item as the query
        new = s if t == 0 else np.where(s > pen, s, pen)           # the earlier value stays on equality
        pen = np.where(has[:, None], new, pen).astype(F32)
    return out_ids, out_sc, out_mmr, out_pos


def sequential_scan(pool_ids, pool_scores, V, K, quotas):
    """lambda = 1 said plainly: walk the pool in order and admit a live entry iff every one of its groups still has room.  Returns
    the admitted pool positions per row (lists of at most K)."""
    ids = np.asarray(pool_ids, np.int64)
    sc = np.asarray(pool_scores, F32)
    out = []
    for r in range(ids.shape[0]):
        room = [dict() for _ in quotas]
        picked = []
        for p in range(ids.shape[1]):
            if len(picked) == K:
                break
            j = int(ids[r, p])
            if not (0 <= j < V and np.isfinite(sc[r, p])):
                continue
            mine = []
            for a, q in enumerate(quotas):
                g = int(q.item_group[j])
                if 0 <= g < q.n_groups:
                    cap = int(q.cap if q.group_cap is None else q.group_cap[g])
                    mine.append((a, g, room[a].get(g, cap)))
            if all(left > 0 for _, _, left in mine):
                for a, g, left in mine:
                    room[a][g] = left - 1
                picked.append(p)
        out.append(picked)
    return out


def violations(out_ids, V, quotas):
    """The (row, quota, group) triples whose cap an output list exceeds; empty = every cap is respected."""
    bad = []
    for r, row in enumerate(np.asarray(out_ids)):
        for a, q in enumerate(quotas):
            count = collections.Counter()
            for j in row:
                if 0 <= j < V:
                    g = int(q.item_group[int(j)])
                    if 0 <= g < q.n_groups:
                        count[g] += 1
            for g, n in count.items():
                cap = int(q.cap if q.group_cap is None else q.group_cap[g])
                if n > cap:
                    bad.append((r, a, g))
    return bad
