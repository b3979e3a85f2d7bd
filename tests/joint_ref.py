"""CPU restatement of b4r_rank_joint (one full-catalogue top-K list per party of users), for the joint-recommendation tests only.
The per-row quantities come from the existing restatements: s and allowed(r) from tests/catalogue_ref.py (chain_scores, scaled,
allowed_mask: b4r_rank_full_ex's), t = fl32(s * inv_temperature) from tests/score_dist_ref.py (scaled_scores).  Restated here:

  u(r, j)   = fl32((double) t(r, j) - row_lse[r]): the fp64 subtraction rounded once to fp32 (u = t without row_lse)
  a(p, j)   additive: acc = 0.0f, acc = fmaf(w, u, acc) over the present members in slot order, the fp32 fma emulated exactly;
            least misery / most pleasure: the minimum / maximum, equal values keeping the earlier member's bits
  allowed(p), the veto, the stable descending order with ties to the lower id, party_n and member_util.

fma32 emulates the fp32 fma through fp64 with ROUND TO ODD: the product of two fp32 values is exact in fp64 (48 bits); the fp64 sum
with the fp32 addend is rounded once, to nearest; an error-free transformation (TwoSum) tells whether it was exact and on which side
the true value lies, and an inexact even result is moved to its odd neighbour on that side.  Rounding a 53-bit round-to-odd value to
24 bits gives the correctly rounded fp32 result (53 >= 2 * 24 + 2), which the plain double rounding does not.  fma32_exact is the
same operation in exact rational arithmetic; tests/test_joint_host.py proves the two equal on random and on adversarial cases."""
from fractions import Fraction

import numpy as np

from tests import catalogue_ref as ref
from tests import score_dist_ref as sdr

ADDITIVE, LEAST_MISERY, MOST_PLEASURE = 0, 1, 2
MODES = {"additive": ADDITIVE, "least_misery": LEAST_MISERY, "most_pleasure": MOST_PLEASURE}
MAX_MEMBERS = 16


def fma32(w, u, acc):
    """fl32(w * u + acc) with one rounding, elementwise over fp32 arrays (finite values)."""
    w, u, acc = (np.asarray(x, np.float32).astype(np.float64) for x in (w, u, acc))
    with np.errstate(invalid="ignore", over="ignore"):   # (an infinite operand: the sum as it is)
        p = w * u                       # exact: 24 + 24 bits
        s = p + acc                     # rounded to nearest even in fp64
        bb = s - p
        err = (p - (s - bb)) + (acc - bb)   # TwoSum: p + acc = s + err exactly
        even = (s.view(np.int64) & 1) == 0
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(np.isfinite(err) & (err != 0) & even, np.nextafter(s, toward), s)   # round to odd
        return s.astype(np.float32)


def fma32_exact(w, u, acc):
    """The same value for three Python / numpy scalars in exact rational arithmetic: the fp32 nearest (ties to even) to w * u + acc."""
    w, u, acc = (float(np.float32(x)) for x in (w, u, acc))
    x = Fraction(w) * Fraction(u) + Fraction(acc)
    if x == 0:
        return np.float32(-0.0) if (np.signbit(w) != np.signbit(u)) and np.signbit(acc) else np.float32(0.0)
    lo = np.float32(float(x))   # float(Fraction) is correctly rounded to fp64; its fp32 neighbours bracket x
    cands = {float(lo), float(np.nextafter(lo, np.float32(np.inf))), float(np.nextafter(lo, np.float32(-np.inf)))}
    best = None
    for c in sorted(cands):
        d = abs(Fraction(c) - x)
        even = (int(np.float32(c).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, c, even)
    return np.float32(best[1])


def row_quantities(hidden, table, bias=None, item_scale=None, inv_temperature=1.0, first=0, exclude=None, words=None, row_filter=None):
    """The existing per-row quantities: (t [R, V] fp32 = fl32(s * inv_temperature) with s b4r_rank_full_ex's score, allowed(r) [R, V]
    bool with gt = NULL).  words: packed uint32 [F, W] or None; row_filter [R] or None."""
    t = sdr.scaled_scores(hidden, table, bias, item_scale, np.float32(inv_temperature))
    R, V = t.shape
    return t, ref.allowed_mask(V, first, exclude, None, R, words, row_filter)


def utilities(t, row_lse=None):
    """u [R, V] fp32 = fl32((double) t - row_lse[r]); row_lse None: t itself."""
    t = np.asarray(t, np.float32)
    if row_lse is None:
        return t.copy()
    with np.errstate(invalid="ignore"):
        return (t.astype(np.float64) - np.asarray(row_lse, np.float64)[:, None]).astype(np.float32)


def members_of(party_rows, R):
    """present [NP, M] bool: the entries of party_rows in [0, R)"""
    pr = np.asarray(party_rows, np.int64)
    if pr.ndim != 2 or not 1 <= pr.shape[1] <= MAX_MEMBERS:
        raise ValueError(f"party_rows is [NP, M] with 1 <= M <= {MAX_MEMBERS}, got shape {pr.shape}")
    return pr, (pr >= 0) & (pr < R)


def aggregate(u, party_rows, mode, weights=None):
    """a [NP, V] fp32 over the present members in slot order (a party without members: the mode's start value)."""
    u = np.asarray(u, np.float32)
    R, V = u.shape
    pr, present = members_of(party_rows, R)
    NP, M = pr.shape
    start = {ADDITIVE: 0.0, LEAST_MISERY: np.inf, MOST_PLEASURE: -np.inf}[mode]
    a = np.full((NP, V), start, np.float32)
    for p in range(NP):
        for m in range(M):
            if not present[p, m]:
                continue
            um = u[pr[p, m]]
            if mode == ADDITIVE:
                w = np.float32(1.0) if weights is None else np.float32(np.asarray(weights, np.float32)[p, m])
                a[p] = fma32(np.full(V, w, np.float32), um, a[p])
            elif mode == LEAST_MISERY:
                a[p] = np.where(um < a[p], um, a[p])
            else:
                a[p] = np.where(um > a[p], um, a[p])
    return a


def party_allowed(u, ok, party_rows, min_util=-np.inf, row_lse=None, row_dead=None):
    """allowed(p) [NP, V] bool: allowed(r) of every member, minus the ids some member vetoes (u < min_util); empty for a party
    without members or with a member that can be served nothing (row_lse not > -inf, or row_dead[r]: no hidden row)."""
    u = np.asarray(u, np.float32)
    R, V = u.shape
    pr, present = members_of(party_rows, R)
    NP, M = pr.shape
    out = np.zeros((NP, V), bool)
    for p in range(NP):
        rows = [int(pr[p, m]) for m in range(M) if present[p, m]]
        if not rows:
            continue
        if row_lse is not None and any(not (float(row_lse[r]) > -np.inf) for r in rows):
            continue
        if row_dead is not None and any(bool(row_dead[r]) for r in rows):
            continue
        okp = np.ones(V, bool)
        for r in rows:
            okp &= np.asarray(ok[r], bool) & ~(u[r] < np.float32(min_util))
        out[p] = okp
    return out


def order(a, okp, K):
    """The first K of the allowed ids by a descending (-0.0 = +0.0), ties to the lower id: ids [NP, K] (-1 tail), scores (-inf tail)."""
    NP, V = a.shape
    ids = np.full((NP, K), -1, np.int64)
    scores = np.full((NP, K), -np.inf, np.float32)
    for p in range(NP):
        o = np.argsort(-a[p].astype(np.float64), kind="stable")
        o = o[okp[p, o]][:K]
        ids[p, :len(o)] = o
        scores[p, :len(o)] = a[p, o]
    return ids, scores


def member_utilities(u, party_rows, ids):
    """member_util [NP, K, M] fp32: u(member m, ids[p][i]); -inf for an absent slot and for the -1 tail."""
    u = np.asarray(u, np.float32)
    pr, present = members_of(party_rows, u.shape[0])
    NP, M = pr.shape
    K = ids.shape[1]
    out = np.full((NP, K, M), -np.inf, np.float32)
    for p in range(NP):
        for m in range(M):
            if present[p, m]:
                live = ids[p] >= 0
                out[p, live, m] = u[pr[p, m], ids[p, live]]
    return out


def rank_joint(t, ok, party_rows, mode, K, row_lse=None, weights=None, min_util=-np.inf, row_dead=None):
    """b4r_rank_joint restated on t [R, V] fp32 and allowed(r) ok [R, V]: (ids [NP, K] int64, scores [NP, K] fp32, n [NP] int64,
    member_util [NP, K, M] fp32)."""
    u = utilities(t, row_lse)
    okp = party_allowed(u, ok, party_rows, min_util, row_lse, row_dead)
    a = aggregate(u, party_rows, mode, weights if mode == ADDITIVE else None)
    ids, scores = order(a, okp, K)
    return ids, scores, okp.sum(axis=1).astype(np.int64), member_utilities(u, party_rows, ids)
