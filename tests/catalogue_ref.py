"""CPU restatement of the catalogue filter, the item scale and the item-to-item neighbours (b4r_rank_full_ex, b4r_item_neighbours),
for the catalogue-filter tests only.  The chain scores come from oracle/rank_oracle.c (the binding of the full-rank tests; a zero
bias where none is given); the scale step is one fp32 multiply; the allowed set, the stable descending order and gt_rank are
restated in integers."""
import ctypes as C
import os
import subprocess

import numpy as np

F32P, I64P = C.POINTER(C.c_float), C.POINTER(C.c_int64)
_ORACLE = None


def c_oracle():
    global _ORACLE
    if _ORACLE is None:
        here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
        so = os.path.join(here, "librank_oracle.so")
        if not os.path.exists(so):
            subprocess.check_call(["make", "-C", here])
        _ORACLE = C.CDLL(so)
    return _ORACLE


def chain_scores(hidden, table, bias=None):
    """rank_oracle_scores of every row against every item: [R, V] float32 (k-ascending fp32 fma chain, + bias; bias None: + 0.0f)."""
    hidden, table = (np.ascontiguousarray(x, dtype=np.float32) for x in (hidden, table))
    R, H = hidden.shape
    V = table.shape[0]
    bias = np.zeros(V, np.float32) if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    cand = np.ascontiguousarray(np.tile(np.arange(V, dtype=np.int64), (R, 1)))
    out = np.zeros((R, V), np.float32)
    c_oracle().rank_oracle_scores(hidden.ctypes.data_as(F32P), table.ctypes.data_as(F32P), bias.ctypes.data_as(F32P),
                                  cand.ctypes.data_as(I64P), C.c_int64(R), C.c_int64(V), C.c_int64(H), out.ctypes.data_as(F32P))
    return out


def scaled(scores, item_scale):
    """s(r, j) = fl32(chain(r, j) * item_scale[j]): one fp32 multiply."""
    return scores if item_scale is None else (scores.astype(np.float32) * np.asarray(item_scale, np.float32)[None, :]).astype(np.float32)


def pack_bits(mask):
    """The bit-by-bit packing of a [V] or [F, V] mask: uint32 [F, ceil(V / 32)], bit (j & 31) of word (j >> 5) = item j."""
    mask = np.asarray(mask) != 0
    if mask.ndim == 1:
        mask = mask[None]
    F, V = mask.shape
    out = [[0] * ((V + 31) // 32) for _ in range(F)]
    for f in range(F):
        for j in range(V):
            if mask[f, j]:
                out[f][j >> 5] |= 1 << (j & 31)
    return np.asarray(out, dtype=np.uint32).reshape(F, (V + 31) // 32)


def allowed_mask(V, first, exclude, gt, R, words=None, row_filter=None):
    """allowed(r) = { j in [first, V) : bit j of filter(r) set, j not in exclude[r] } plus gt[r] when it lies in [first, V).
    words: packed uint32 [F, W] or None; row_filter [R] or None (filter 0); an index outside [0, F) = no filter."""
    ok = np.zeros((R, V), bool)
    for r in range(R):
        f = -1
        if words is not None:
            f = 0 if row_filter is None else int(row_filter[r])
            if f < 0 or f >= words.shape[0]:
                f = -1
        j = np.arange(V)
        bit = np.ones(V, np.int64) if f < 0 else (words[f, j >> 5].astype(np.int64) >> (j & 31)) & 1
        ok[r] = (j >= first) & (bit == 1)
        if exclude is not None:
            for j in exclude[r]:
                if 0 <= j < V:
                    ok[r, j] = False
        if gt is not None and first <= gt[r] < V:
            ok[r, gt[r]] = True
    return ok


def expected(sc, ok, gt, K, first=0):
    """The stable descending order over the allowed ids cut / padded to K (ids -1, scores -inf), and gt_rank = 1 + #{allowed j:
    s_j > s_gt} + #{allowed j < gt: s_j == s_gt} (0 when gt is None or outside [first, V))."""
    R, V = sc.shape
    ids = np.full((R, K), -1, np.int64)
    scores = np.full((R, K), -np.inf, np.float32)
    ranks = np.zeros(R, np.int64)
    j = np.arange(V)
    for r in range(R):
        order = np.argsort(-sc[r].astype(np.float64), kind="stable")
        order = order[ok[r, order]][:K]
        ids[r, :len(order)] = order
        scores[r, :len(order)] = sc[r, order]
        if gt is not None and first <= gt[r] < V:
            s, g = sc[r], int(gt[r])
            ranks[r] = 1 + int((ok[r] & (s > s[g])).sum()) + int((ok[r] & (s == s[g]) & (j < g)).sum())
    return ids, scores, ranks


def neighbours(table, query, first, metric, K, rnorm=None, words=None, row_filter=None):
    """b4r_item_neighbours restated.  metric 0: dot; 1: cosine with the given rnorm [V] (the device's own values):
    qhat = fl32(table[q] * rnorm[q]), s = fl32(chain(qhat, table[j]) * rnorm[j]).  A query outside [first, V): -1 / -inf."""
    table = np.ascontiguousarray(table, np.float32)
    V = table.shape[0]
    query = np.asarray(query, np.int64)
    R = len(query)
    valid = (query >= first) & (query < V)
    q = np.where(valid, query, 0)
    rows = table[q]
    if metric == 1:
        rows = (rows * np.asarray(rnorm, np.float32)[q][:, None]).astype(np.float32)
    sc = scaled(chain_scores(rows, table), rnorm if metric == 1 else None)
    ok = allowed_mask(V, first, query[:, None], None, R, words, row_filter)
    ok[~valid] = False
    ids, scores, _ = expected(sc, ok, None, K)
    return ids, scores
