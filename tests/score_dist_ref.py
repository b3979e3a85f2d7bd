"""CPU restatement of b4r_score_dist (the catalogue softmax: normaliser, entropy, log probabilities of queried items), for the
score-distribution tests only.  The scores and the allowed set come from tests/catalogue_ref.py (chain_scores, scaled,
allowed_mask): b4r_rank_full_ex's.  Two versions of the normaliser and the entropy over the same fp32 t:

  blocked   the prescribed arithmetic: per chunk of 1024 ids m_c, x = fl32(t - m_c), e = numpy's fp32 exp, fp64 sums S_c and W_c;
            per row m, f_c = exp(m_c - m), S, W; lse = m + log S, entropy = log S - W / S
  plain     fp64 throughout: the shifted log-sum-exp and -sum p log p with p = exp(t - lse)

Derived tolerances of the device against `plain` (tol_lse, tol_entropy): with fp64 sums the only errors are the fp32 exponential's
(taken as at most 3 ulp = 3 * 2^-24 relative, rounded up to 2^-22 per term) and the rounding of x (2^-24 relative, |x| up to about
ln n where the term still matters)."""
import numpy as np

from tests import catalogue_ref as ref

CHUNK = 1024


def scaled_scores(hidden, table, bias=None, item_scale=None, inv_temperature=1.0):
    """t(r, j) = fl32(s(r, j) * inv_temperature), s = b4r_rank_full_ex's score: [R, V] float32."""
    s = ref.scaled(ref.chain_scores(hidden, table, bias), item_scale)
    return (s.astype(np.float32) * np.float32(inv_temperature)).astype(np.float32)


def blocked(t, ok, chunk=CHUNK):
    """(n int64, max fp32, lse fp64, entropy fp64), each [R], by the prescribed blocked arithmetic."""
    t = np.asarray(t, np.float32)
    R, V = t.shape
    n = np.zeros(R, np.int64)
    mx = np.full(R, -np.inf, np.float32)
    lse = np.full(R, -np.inf, np.float64)
    ent = np.zeros(R, np.float64)
    for r in range(R):
        recs = []
        for c0 in range(0, V, chunk):
            tc = t[r, c0:c0 + chunk][ok[r, c0:c0 + chunk]]
            if tc.size == 0:
                continue
            mc = np.float32(tc.max())
            x = (tc - mc).astype(np.float32)
            with np.errstate(under="ignore"):
                e = np.exp(x).astype(np.float32)
            e64, x64 = e.astype(np.float64), x.astype(np.float64)
            recs.append((tc.size, mc, e64.sum(), np.where(e > 0, e64 * x64, 0.0).sum()))
        if not recs:
            continue
        n[r] = sum(rec[0] for rec in recs)
        m = np.float32(max(rec[1] for rec in recs))
        S = W = 0.0
        for _, mc, Sc, Wc in recs:
            d = float(mc) - float(m)
            f = np.exp(d)
            S += Sc * f
            W += (Wc + d * Sc) * f
        mx[r] = m
        lse[r] = float(m) + np.log(S)
        ent[r] = np.log(S) - W / S
    return n, mx, lse, ent


def plain(t, ok):
    """(n, lse fp64, entropy fp64) in fp64 over the same fp32 t: shifted log-sum-exp, entropy = log S - sum e z / S, z = t - max."""
    t = np.asarray(t, np.float32)
    R = t.shape[0]
    n = ok.sum(axis=1).astype(np.int64)
    lse = np.full(R, -np.inf, np.float64)
    ent = np.zeros(R, np.float64)
    for r in range(R):
        if n[r] == 0:
            continue
        z = t[r][ok[r]].astype(np.float64)
        m = z.max()
        z = z - m
        e = np.exp(z)
        S = e.sum()
        lse[r] = m + np.log(S)
        ent[r] = np.log(S) - (e * z).sum() / S
    return n, lse, ent


def query_logp(t, ok, lse, query):
    """fl32((double) t(r, q) - lse[r]) where q = query[r, i] is allowed for the row, else -inf: [R, K] float32."""
    t = np.asarray(t, np.float32)
    R, V = t.shape
    query = np.asarray(query, np.int64)
    out = np.full(query.shape, -np.inf, np.float32)
    for r in range(R):
        for i, q in enumerate(query[r].tolist()):
            if 0 <= q < V and ok[r, q]:
                out[r, i] = np.float32(float(t[r, q]) - float(lse[r]))
    return out


def tol_lse(n):
    """2^-21 + 2^-24 ln n"""
    n = np.maximum(np.asarray(n, np.float64), 1.0)
    return 2.0 ** -21 + 2.0 ** -24 * np.log(n)


def tol_entropy(n):
    """2^-21 (1 + 2 ln n) + 2^-24 (ln n + ln^2 n)"""
    ln = np.log(np.maximum(np.asarray(n, np.float64), 1.0))
    return 2.0 ** -21 * (1.0 + 2.0 * ln) + 2.0 ** -24 * (ln + ln * ln)
