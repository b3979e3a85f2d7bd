"""CPU restatement of b4r_group_mass (category affinity: the probability mass of every item group under each row's catalogue
softmax), for the group-mass tests only.  The scores and the allowed set come from tests/catalogue_ref.py (b4r_rank_full_ex's, with
gt = NULL), t = fl32(s * inv_temperature) from tests/score_dist_ref.py; u and c are formed in numpy fp64:

  u(r, j) = fl32((double) t - row_lse[r])            b4r_score_dist's query_logp bits
  c(r, j) = rint(exp(min((double) u, 0.0)) * 2^40)   b4r_audience_merge's demand term (numpy's fp64 exp, good to 1 ulp)

and summed as integers per (row, label); labels outside [0, G) go to `rest`.  A row with a negative hidden_row, or with row_lse
-inf or NaN, is all zeros.

Against the device: the counts are exact.  u has the same bits on both sides, two exponentials good to 1 ulp differ by at most
2 ulp of a value <= 2^40, which moves the rounded integer by at most 1: |device - restatement| <= group_n units (tol_mass)."""
import numpy as np

ONE = float(1 << 40)


def units(t, row_lse):
    """c(r, j) int64 [R, V] for every (row, id), allowed or not; a dead row (row_lse -inf or NaN) is all zeros."""
    t = np.asarray(t, np.float32)
    lse = np.asarray(row_lse, np.float64)
    live = lse > -np.inf                                   # False for NaN too
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        u = (t.astype(np.float64) - np.where(live, lse, 0.0)[:, None]).astype(np.float32)
        c = np.rint(np.exp(np.minimum(u.astype(np.float64), 0.0)) * ONE).astype(np.int64)
    c[~live] = 0
    return c


def group_mass(t, ok, row_lse, item_group, G, dead=None):
    """(group_mass int64 [R, G], group_n int32 [R, G], rest_mass int64 [R], rest_n int32 [R]).  ok: the allowed mask [R, V] (gt = None);
    dead: rows with a negative hidden_row."""
    ok = np.array(ok, bool)
    R, V = ok.shape
    lse = np.asarray(row_lse, np.float64)
    gone = ~(lse > -np.inf)
    if dead is not None:
        gone |= np.asarray(dead, bool)
    ok[gone] = False
    c = np.where(ok, units(t, lse), 0)
    lab = np.asarray(item_group, np.int64)
    inside = (lab >= 0) & (lab < G)
    mass, n = np.zeros((R, max(G, 1)), np.int64), np.zeros((R, max(G, 1)), np.int64)
    for r in range(R):
        at = inside & ok[r]
        np.add.at(mass[r], lab[at], c[r, at])                  # integers: exact in any order
        n[r] = np.bincount(lab[at], minlength=max(G, 1))[:max(G, 1)]
    rest = ok & ~inside[None, :]
    return mass[:, :G], n[:, :G].astype(np.int32), np.where(rest, c, 0).sum(axis=1), rest.sum(axis=1).astype(np.int32)


def brute_force(t, ok, item_group, G):
    """fp64 softmax of every row over its allowed items, grouped by label: (probabilities [R, G], the rest [R], lse [R])."""
    t = np.asarray(t, np.float32).astype(np.float64)
    R, V = t.shape
    lab = np.asarray(item_group, np.int64)
    inside = (lab >= 0) & (lab < G)
    p_g, p_rest, lse = np.zeros((R, G)), np.zeros(R), np.full(R, -np.inf)
    for r in range(R):
        if not ok[r].any():
            continue
        m = t[r][ok[r]].max()
        e = np.where(ok[r], np.exp(t[r] - m), 0.0)
        S = e.sum()
        lse[r] = m + np.log(S)
        p = e / S
        np.add.at(p_g[r], lab[inside], p[inside])
        p_rest[r] = p[~inside].sum()
    return p_g, p_rest, lse


def tol_mass(n):
    """one unit per item of the group"""
    return np.asarray(n, np.int64)


def tol_total(row_n):
    """|sum of all masses - 2^40| when every allowed item is counted: half a unit of rounding per item, the normaliser's own bound
    (include/b4r.h: |lse error| <= 2^-21 + 2^-24 ln n, so the probabilities sum to 1 within that, relative), and the unit per item
    that two exponentials may differ by."""
    n = np.maximum(np.asarray(row_n, np.float64), 1.0)
    return n / 2.0 + ONE * (2.0 ** -21 + 2.0 ** -24 * np.log(n)) + n
