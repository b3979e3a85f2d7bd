"""CPU restatement of the sampled recommendations (b4r_sample_full, b4r_sample_pool) and of their noise, for the sampling tests only.

The noise is include/b4r.h's sequence of individually rounded fp64 operations, written with numpy scalars-in-arrays (numpy rounds
every operation on its own and never fuses).  The unperturbed scores and the allowed set come from tests/catalogue_ref.py over
oracle/rank_oracle.c; the draw order is the stable sort by (key descending, id ascending)."""
import math

import numpy as np

from tests import catalogue_ref as ref

F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64
M32 = 0xFFFFFFFF
G_MIN, G_MAX = -2.8115408, 16.635532   # the noise's range over the 2^23 words


def hash32(x):
    """b4r_hash32 on a uint32 array (computed in uint64, masked: no overflow warnings)."""
    x = np.asarray(x, U64) & U64(M32)
    x = x ^ (x >> U64(16))
    x = (x * U64(0x7FEB352D)) & U64(M32)
    x = x ^ (x >> U64(15))
    x = (x * U64(0x846CA68B)) & U64(M32)
    x = x ^ (x >> U64(16))
    return x.astype(U32)


def sample_word(seed, stream, ids):
    """word(seed, stream, id) of include/b4r.h; seed in [0, 2^64) (a python int), stream any int64 (a python int, or an int64 array that
    broadcasts against ids), ids an integer array."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if isinstance(stream, np.ndarray):
        st = stream.astype(np.int64).astype(U64)
    else:
        st = np.asarray(int(stream) & 0xFFFFFFFFFFFFFFFF, dtype=U64)
    ids = (np.asarray(ids, np.int64).astype(U64)) & U64(M32)
    h = hash32(ids ^ U64(seed & M32))
    h = hash32(((h.astype(U64) ^ (st & U64(M32))) + U64(seed >> 32)) & U64(M32))
    return hash32(h.astype(U64) ^ (st >> U64(32)))


def xln(x):
    """ln of positive normal doubles by the fixed sequence: every * and + rounded on its own."""
    x = np.asarray(x, F64)
    b = x.view(U64)
    e = (b >> U64(52)).astype(np.int64) - 1023
    m = ((b & U64(0x000FFFFFFFFFFFFF)) | U64(0x3FF0000000000000)).view(F64)
    big = m > 1.4142135623730951
    m = np.where(big, m * 0.5, m)
    e = np.where(big, e + 1, e)
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = np.full_like(z, 1.0 / 15.0)
    for d in (13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = p * z + 1.0 / d
    p = p * z + 1.0
    return e.astype(F64) * 0.6931471805599453 + (2.0 * s) * p


def uniform(words):
    """b4r_uniform23's value, exact in fp64"""
    return ((np.asarray(words, U32) >> U32(9)).astype(F64) + 0.5) * (1.0 / 8388608.0)


def gumbel_from_word(words):
    """g = fl32(0 - xln(0 - xln(u)))"""
    return (0.0 - xln(0.0 - xln(uniform(words)))).astype(F32)


def gumbel(seed, stream, ids):
    return gumbel_from_word(sample_word(seed, stream, ids))


def streams_of(R, row_stream=None, stream0=0):
    """stream(r) = row_stream[r], or stream0 + r wrapped to int64"""
    if row_stream is not None:
        return [int(x) for x in row_stream]
    out = []
    for r in range(R):
        s = (int(stream0) + r) & 0xFFFFFFFFFFFFFFFF
        out.append(s - (1 << 64) if s >= 1 << 63 else s)
    return out


def keys_of(scores, inv_t, seed, streams):
    """key(r, j) = fl32(fl32(s * inv_t) + g(word(seed, stream(r), j))) for every (r, j): [R, V] float32"""
    scores = np.asarray(scores, F32)
    R, V = scores.shape
    t = (scores * F32(inv_t)).astype(F32)
    j = np.arange(V, dtype=np.int64)
    g = np.stack([gumbel(seed, streams[r], j) for r in range(R)]) if R else np.zeros((0, V), F32)
    return (t + g).astype(F32)


def sample_full(scores, ok, K, inv_t, seed, row_stream=None, stream0=0):
    """b4r_sample_full restated on the unperturbed scores [R, V] and the allowed mask: (ids, scores, keys) [R, K], the first K of
    the allowed ids by key descending (-0.0 as +0.0), ties to the lower id; -1 / -inf / -inf behind the allowed ones."""
    scores = np.asarray(scores, F32)
    R, V = scores.shape
    keys = keys_of(scores, inv_t, seed, streams_of(R, row_stream, stream0))
    ids = np.full((R, K), -1, np.int64)
    out_s = np.full((R, K), -np.inf, F32)
    out_k = np.full((R, K), -np.inf, F32)
    for r in range(R):
        order = np.argsort(-(keys[r].astype(F64) + 0.0), kind="stable")
        order = order[ok[r, order]][:K]
        ids[r, :len(order)] = order
        out_s[r, :len(order)] = scores[r, order]
        out_k[r, :len(order)] = keys[r, order]
    return ids, out_s, out_k


def sample_pool(pool_ids, pool_scores, V, K, inv_t, seed, row_stream=None, stream0=0):
    """b4r_sample_pool restated: live = id in [0, V) and a finite score; the noise goes by the item id; order by (key descending,
    id ascending, pool position ascending).  Returns (ids, scores, keys, pos) [R, K], -1 / -inf / -inf / -1 behind the live ones."""
    pool_ids = np.asarray(pool_ids, np.int64)
    pool_scores = np.asarray(pool_scores, F32)
    R, M = pool_ids.shape
    streams = streams_of(R, row_stream, stream0)
    ids = np.full((R, K), -1, np.int64)
    out_s = np.full((R, K), -np.inf, F32)
    out_k = np.full((R, K), -np.inf, F32)
    pos = np.full((R, K), -1, np.int32)
    for r in range(R):
        live = (pool_ids[r] >= 0) & (pool_ids[r] < V) & np.isfinite(pool_scores[r])
        idx = np.flatnonzero(live)
        t = (pool_scores[r, idx] * F32(inv_t)).astype(F32)
        key = (t + gumbel(seed, streams[r], pool_ids[r, idx])).astype(F32)
        order = np.lexsort((idx, pool_ids[r, idx], -(key.astype(F64) + 0.0)))[:K]
        n = len(order)
        ids[r, :n] = pool_ids[r, idx[order]]
        out_s[r, :n] = pool_scores[r, idx[order]]
        out_k[r, :n] = key[order]
        pos[r, :n] = idx[order]
    return ids, out_s, out_k, pos


def scores_and_allowed(hidden, table, bias, item_scale, first, exclude, gt, words=None, row_filter=None):
    """s(r, j) and allowed(r) of b4r_rank_full_ex through tests/catalogue_ref.py"""
    R, V = hidden.shape[0], table.shape[0]
    sc = ref.scaled(ref.chain_scores(hidden, table, bias), item_scale)
    ok = ref.allowed_mask(V, first, exclude, gt, R, words, row_filter)
    return sc, ok


# ---- the law: Plackett-Luce probabilities of the first two draws ----------------------------------------------------------------
def plackett_luce_first_two(t):
    """t [n] fp64 scaled scores: (p1 [n], p2 [n]) the exact probabilities that item i is the first / the second draw without
    replacement from softmax(t)."""
    t = np.asarray(t, F64)
    p = np.exp(t - t.max())
    p /= p.sum()
    p2 = np.array([sum(p[j] * p[i] / (1.0 - p[j]) for j in range(len(p)) if j != i) for i in range(len(p))])
    return p, p2


def chi_square_p(counts, probs):
    """p-value of Pearson's chi-square of integer counts against the probabilities (df = n - 1), by the regularised upper incomplete
    gamma function (continued fraction / series, no scipy)."""
    counts = np.asarray(counts, F64)
    expected = counts.sum() * np.asarray(probs, F64)
    stat = float(((counts - expected) ** 2 / expected).sum())
    return gammaincc(0.5 * (len(counts) - 1), 0.5 * stat)


def gammaincc(a, x):
    """Q(a, x) = Gamma(a, x) / Gamma(a) (Numerical Recipes' gser / gcf)"""
    if x <= 0.0:
        return 1.0
    lg = math.lgamma(a)
    if x < a + 1.0:
        term = total = 1.0 / a
        n = a
        for _ in range(10000):
            n += 1.0
            term *= x / n
            total += term
            if abs(term) < abs(total) * 1e-16:
                break
        return 1.0 - total * math.exp(-x + a * math.log(x) - lg)
    tiny = 1e-300
    b = x + 1.0 - a
    c = 1.0 / tiny
    d = 1.0 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return math.exp(-x + a * math.log(x) - lg) * h
