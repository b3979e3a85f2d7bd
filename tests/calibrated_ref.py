"""CPU restatement of the calibrated re-ranking (b4r_rerank_calibrated, include/b4r.h), for the calibration tests only: numpy over
tests/sample_ref.py's restatement of b4r_xln, with the contract's rounding points -- every fp64 step is one numpy operation on
float64 arrays (numpy rounds every operation on its own and never fuses), every fp32 step one on float32 arrays.

rerank() is the kernel's contract.  The rows are independent, so lam and alpha may be given per row: the rows of several calls are
then restated in one (the pick loop's cost is numpy's per-operation overhead, not its arithmetic).  objective() is the quantity the
greedy step maximises, said plainly with math.log, for the test that the contract's pick is its argmax."""
import math

import numpy as np

from tests import sample_ref as sref

F32, F64 = np.float32, np.float64


def target_shares(target_mass):
    """p [R, G] float64 and T [R] (python ints): p_g = fl64((double) mass_g / (double) T) over the masses clamped at 0; T = 0: zeros."""
    mass = np.maximum(np.asarray(target_mass, np.int64), 0)
    T = [sum(int(x) for x in row) for row in mass]                 # exact
    assert all(t < 1 << 63 for t in T)
    p = np.zeros(mass.shape, F64)
    for r, t in enumerate(T):
        if t > 0:
            p[r] = mass[r].astype(F64) / F64(float(t))             # (float(int) and astype round to nearest, as the device's conversion)
    return p, T


def share(A, c, m, ap):
    """qt(g, c, m) = fl64(fl64(fl64(A * c) / m) + ap), ap = fl64(alpha * p_g)"""
    x = A * np.asarray(c, F64)
    y = x / np.asarray(m, F64)
    return y + ap


def per_row(x, R, dtype):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype), (R,)))


def rerank(pool_ids, pool_scores, V, K, item_group, G, target_mass, lam, alpha):
    """b4r_rerank_calibrated restated; all rows advance together, one pick per step.  lam, alpha: one number, or one per row.  Returns
    (ids [R, K] int64, scores [R, K] float32, value [R, K] float32, pos [R, K] int32, kl [R] float64)."""
    ids = np.asarray(pool_ids, np.int64)
    sc = np.asarray(pool_scores, F32)
    R, M = ids.shape
    lam = per_row(lam, R, F32)
    alpha = per_row(alpha, R, F64)
    assert 1 <= M <= 1024 and 0 <= K <= M and 1 <= G <= 1024 and ((alpha > 0.0) & (alpha < 1.0)).all()
    lr = (F32(1.0) - lam).astype(F32)
    A = 1.0 - alpha
    live = (ids >= 0) & (ids < V) & np.isfinite(sc)
    item = np.where(live, ids, 0)
    lab = np.asarray(item_group, np.int64)[item]
    lab = np.where(live & (lab >= 0) & (lab < G), lab, -1)         # -1: in no group
    with np.errstate(all="ignore"):
        plus = (sc + F32(0.0)).astype(F32)                         # -0.0 counts as +0.0 in s_max / s_min
        smax = np.where(live, plus, -np.inf).astype(F32).max(axis=1)
        smin = np.where(live, plus, np.inf).astype(F32).min(axis=1)
        span = (smax - smin).astype(F32)
        rel = ((sc - smin[:, None]).astype(F32) / span[:, None]).astype(F32)
    rel = np.where((smax == smin)[:, None], F32(1.0), rel).astype(F32)
    with np.errstate(all="ignore"):
        a = (lr[:, None] * rel).astype(F32)                        # fl32((1 - lambda) * rel): the same at every step
    p, T = target_shares(target_mass)
    ap = alpha[:, None] * p
    # the groups with p_g > 0, as (row, group) pairs in ascending (row, group): only they have a gain and a term
    act_r, act_g = np.nonzero(p > 0.0)
    pa, apa, Aa = p[act_r, act_g], ap[act_r, act_g], A[act_r]
    n_g = np.zeros((R, G), np.int64)
    n = np.zeros(R, np.int64)
    is_open = live.copy()
    out_ids = np.full((R, K), -1, np.int64)
    out_sc = np.full((R, K), -np.inf, F32)
    out_val = np.full((R, K), -np.inf, F32)
    out_pos = np.full((R, K), -1, np.int32)
    rows = np.arange(R)
    lab0 = np.maximum(lab, 0)
    gain = np.zeros((R, G), F32)                                   # 0.0f where p_g = 0
    for t in range(K):
        has = is_open.any(axis=1)
        if not has.any():
            break
        # gain_g at the step that makes pick number t + 1 (a row that still picks has n = t)
        c = n_g[act_r, act_g]
        d = sref.xln(share(Aa, c + 1, t + 1, apa)) - sref.xln(share(Aa, c, t + 1, apa))
        gain[act_r, act_g] = (pa * d).astype(F32)
        gc = np.where(lab >= 0, gain[rows[:, None], lab0], F32(0.0)).astype(F32)      # 0.0f for an item in no group
        with np.errstate(all="ignore"):
            b = (lam[:, None] * gc).astype(F32)
            val = (a + b).astype(F32)
        best = np.where(is_open, val, -np.inf).max(axis=1)
        w = np.argmax(is_open & (val == best[:, None]), axis=1)    # the first (lowest p) of equals; -0.0 == +0.0 as floats
        hr = rows[has]
        out_ids[hr, t] = ids[hr, w[hr]]
        out_sc[hr, t] = sc[hr, w[hr]]
        out_val[hr, t] = val[hr, w[hr]]
        out_pos[hr, t] = w[hr]
        is_open[hr, w[hr]] = False
        wl = lab[hr, w[hr]]
        grouped = wl >= 0
        n_g[hr[grouped], wl[grouped]] += 1
        n[hr] += 1
    # out_kl: the terms fl64(p_g * fl64(ln p_g - ln qt(g, n_g, n))) of the groups with p_g > 0, added in ascending g, one fp64 add each
    kl = np.full(R, np.nan, F64)
    with np.errstate(all="ignore"):
        terms = pa * (sref.xln(pa) - sref.xln(share(Aa, n_g[act_r, act_g], np.maximum(n, 1)[act_r], apa)))
    for r in range(R):
        if T[r] > 0 and n[r] > 0:
            total = 0.0
            for x in terms[act_r == r].tolist():                   # (python floats are IEEE doubles: one rounded add each)
                total += x
            kl[r] = total
    return out_ids, out_sc, out_val, out_pos, kl


# ---- the objective, said plainly ------------------------------------------------------------------------------------------------
def relevance(pool_ids_row, pool_scores_row, V):
    """(live [M] bool, rel [M] float64) of one row, in fp64: the test compares objective values, not bits"""
    ids = np.asarray(pool_ids_row, np.int64)
    sc = np.asarray(pool_scores_row, F64)
    live = (ids >= 0) & (ids < V) & np.isfinite(sc)
    lo, hi = sc[live].min(), sc[live].max()
    rel = np.ones_like(sc) if hi == lo else (np.where(live, sc, lo) - lo) / (hi - lo)
    return live, rel


def objective(picked, rel, labels, p, lam, alpha):
    """(1 - lambda) * sum of rel over the picked pool positions - lambda * KL(p || (1 - alpha) q + alpha p), q the picks' label shares
    (an unlabelled pick counts in the denominator), with math.log in fp64."""
    n = len(picked)
    counts = {}
    for c in picked:
        if labels[c] >= 0:
            counts[labels[c]] = counts.get(labels[c], 0) + 1
    kl = 0.0
    for g, pg in enumerate(p):
        if pg > 0.0:
            qt = (1.0 - alpha) * counts.get(g, 0) / n + alpha * pg
            kl += pg * (math.log(pg) - math.log(qt))
    return (1.0 - lam) * sum(rel[c] for c in picked) - lam * kl
