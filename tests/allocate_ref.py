"""CPU restatement of the stock-aware allocation (b4r_allocate, include/b4r.h), for the allocation tests only.

greedy() is the contract said plainly: every live pool entry of every row is an edge, the edges are sorted ONCE into the global order
(utility descending with -0.0 = +0.0, then the lower user id, the lower row, the lower pool position) and walked ONCE; an edge is
assigned when its row holds fewer than K and its item fewer than its capacity.  It is deliberately not written as rounds: the device
computes the same thing by deferred acceptance, which is another procedure.

blocking_edges() checks a result independently of how it was made (stability), feasible() checks an intermediate state, and the
generators below build the pools, capacities and user ids both test files walk through."""
import itertools

import numpy as np

F32 = np.float32
BIG = (1 << 31) - 1


def live_edges(pool_ids, pool_util, capacity):
    ids = np.asarray(pool_ids, np.int64)
    util = np.asarray(pool_util, F32)
    cap = np.asarray(capacity, np.int64)
    V = cap.shape[0]
    ok = (ids >= 0) & (ids < V) & np.isfinite(util)
    ok &= cap[np.where(ok, ids, 0)] > 0                               # capacity is read at live ids only
    return ids, util, cap, ok


def edge_order(ids, util, ok, user_ids):
    """(rows, positions) of the live edges in the global order"""
    R, M = ids.shape
    uid = np.arange(R, dtype=np.int64) if user_ids is None else np.asarray(user_ids, np.int64)
    r, p = np.nonzero(ok)
    with np.errstate(all="ignore"):
        neg = -(util[r, p] + F32(0.0))                               # exact; every zero becomes the same word
    order = np.lexsort((p, r, uid[r], neg))                          # the last key is the first criterion
    return r[order], p[order]


def greedy(pool_ids, pool_util, K, capacity, user_ids=None):
    """-> dict(ids [R, K] int64, util [R, K] float32, pos [R, K] int32, row_n [R] int32, remaining [V] int32, assigned [R, M] bool)"""
    ids, util, cap, ok = live_edges(pool_ids, pool_util, capacity)
    R, M = ids.shape
    assert 1 <= M <= 1024 and 0 <= K <= M
    er, ep = edge_order(ids, util, ok, user_ids)
    left = cap.copy()
    row_n = np.zeros(R, np.int64)
    assigned = np.zeros((R, M), bool)
    for r, p in zip(er.tolist(), ep.tolist()):                       # the walk
        j = ids[r, p]
        if row_n[r] < K and left[j] > 0:
            assigned[r, p] = True
            row_n[r] += 1
            left[j] -= 1
    out = dict(ids=np.full((R, K), -1, np.int64), util=np.full((R, K), -np.inf, F32), pos=np.full((R, K), -1, np.int32),
               row_n=row_n.astype(np.int32), remaining=left.astype(np.int32), assigned=assigned)
    for r in range(R):
        p = np.nonzero(assigned[r])[0]                               # ascending pool position
        out["ids"][r, :p.size], out["util"][r, :p.size], out["pos"][r, :p.size] = ids[r, p], util[r, p], p
    return out


def blocking_edges(pool_ids, pool_util, K, capacity, user_ids, assigned):
    """The unassigned live edges that both their row and their item would rather have: the row has room or holds an edge that stands
    later in the global order, AND the item has room or holds a later edge.  A stable result has none."""
    ids, util, cap, ok = live_edges(pool_ids, pool_util, capacity)
    R, M = ids.shape
    er, ep = edge_order(ids, util, ok, user_ids)
    rank = np.full((R, M), -1, np.int64)
    rank[er, ep] = np.arange(er.size)
    assigned = np.asarray(assigned, bool)
    assert not (assigned & ~ok).any()
    row_n = assigned.sum(axis=1)
    worst_row = np.where(assigned, rank, -1).max(axis=1)
    item_n = np.zeros(cap.shape[0], np.int64)
    worst_item = np.full(cap.shape[0], -1, np.int64)
    ar, ap = np.nonzero(assigned)
    np.add.at(item_n, ids[ar, ap], 1)
    np.maximum.at(worst_item, ids[ar, ap], rank[ar, ap])
    assert (row_n <= K).all() and (item_n <= np.maximum(cap, 0)).all()
    j = np.where(ok, ids, 0)
    row_wants = (row_n[:, None] < K) | (rank < worst_row[:, None])
    item_wants = (item_n[j] < cap[j]) | (rank < worst_item[j])
    return np.argwhere(ok & ~assigned & row_wants & item_wants)


def feasible(out, pool_ids, pool_util, K, capacity):
    """An output set describes a feasible state: every listed entry is a live entry of its row at the stated position, positions
    ascend, the tail is -1 / -inf / -1, no row holds more than K and no item gives more than its capacity; remaining agrees."""
    ids, util, cap, ok = live_edges(pool_ids, pool_util, capacity)
    R, M = ids.shape
    used = np.zeros(cap.shape[0], np.int64)
    for r in range(R):
        n = int(out["row_n"][r])
        if not 0 <= n <= K:
            return False
        p = out["pos"][r, :n].astype(np.int64)
        if (p < 0).any() or (p >= M).any() or (np.diff(p) <= 0).any() or not ok[r, p].all():
            return False
        if not np.array_equal(out["ids"][r, :n], ids[r, p]) or out["util"][r, :n].tobytes() != util[r, p].tobytes():
            return False
        if (out["ids"][r, n:] != -1).any() or (out["pos"][r, n:] != -1).any() or not np.isneginf(out["util"][r, n:]).all():
            return False
        np.add.at(used, ids[r, p], 1)
    return bool((used <= np.maximum(cap, 0)).all() and np.array_equal(out["remaining"].astype(np.int64), cap - used))


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
POOL_KINDS = ("skewed", "same", "ties")
CAP_KINDS = ("zeros", "ones", "mixed", "negative", "exactly_R", "plenty")
UID_KINDS = ("none", "shuffled", "repeats")


def make_pool(R, M, V, seed, kind="skewed", dead=0.15):
    """A pool as b4r_rank_full leaves it -- every row's live entries in descending utility -- with everything a caller may also hand
    in: utilities on a coarse grid (ties inside a row and across rows), both zeros, repeated ids within a row, NaN / +inf / -inf
    utilities, ids below 0 and at or past V, and a -1 / -inf tail.  kind "same": every row holds the same entries (the largest
    contention); "ties": two utility values only."""
    rng = np.random.default_rng([R, M, V, seed])
    ids = np.minimum((V * rng.random((R, M)) ** 3).astype(np.int64), V - 1)          # popularity-skewed towards the low ids
    steps = 2 if kind == "ties" else 9
    util = (rng.integers(0, steps, size=(R, M)) - steps // 2).astype(F32) / F32(4.0)
    if kind == "same":
        ids[:], util[:] = ids[0], util[0]
    order = np.argsort(-util, axis=1, kind="stable")
    ids, util = np.take_along_axis(ids, order, 1), np.take_along_axis(util, order, 1)
    util = np.where((util == 0) & (rng.random((R, M)) < 0.5), F32(-0.0), util).astype(F32)   # -0.0 beside +0.0, in either order
    hit = rng.random((R, M)) < dead
    what = rng.integers(0, 7, size=(R, M))
    util = np.where(hit & (what == 0), F32(np.nan), util)
    util = np.where(hit & (what == 1), F32(np.inf), util)
    util = np.where(hit & (what == 2), F32(-np.inf), util)
    for w, bad in ((3, -1), (4, -7), (5, V), (6, (1 << 40) + 3)):
        ids = np.where(hit & (what == w), bad, ids)
    tail = rng.integers(0, M + 1, size=R) * (rng.random(R) < 0.3)                  # some rows end in rank_full's own tail
    cut = np.arange(M)[None, :] >= (M - tail)[:, None]
    return np.where(cut, -1, ids).astype(np.int64), np.where(cut, F32(-np.inf), util).astype(F32)


def make_capacity(V, R, kind, seed=0):
    rng = np.random.default_rng([V, R, seed])
    if kind == "zeros":
        return np.zeros(V, np.int32)
    if kind == "ones":
        return np.ones(V, np.int32)
    if kind == "mixed":
        return rng.choice(np.array([0, 1, 2, BIG], np.int32), size=V)
    if kind == "negative":
        return rng.choice(np.array([-BIG - 1, -3, -1, 0, 1, 2], np.int32), size=V)
    if kind == "exactly_R":
        return np.full(V, R, np.int32)
    assert kind == "plenty"
    return np.full(V, BIG, np.int32)


def make_user_ids(R, kind, seed=0):
    rng = np.random.default_rng([R, seed])
    if kind == "none":
        return None
    if kind == "shuffled":
        return (rng.permutation(R).astype(np.int64) - R // 2) * 1000003       # distinct, some negative, far apart
    assert kind == "repeats"
    return rng.integers(0, 3, size=R).astype(np.int64)                        # the row breaks the tie


R_GRID = (1, 2, 5, 64, 65, 257)
M_GRID = (1, 2, 63, 64, 65, 256, 1024)
V_GRID = (4, 33, 1027)


def shapes():
    """(R, M) of the grid; at M = 1024 only R <= 5"""
    return [(R, M) for R in R_GRID for M in M_GRID if M < 1024 or R <= 5]


def cases_of(R, M):
    """The cases of one (R, M): every K of {1, 3, 10, M} that fits, and beside it V, the pool kind, the capacities and the user ids
    in rotation, so that every value of each meets every shape class and the whole grid stays a few hundred small calls."""
    turn = itertools.count(R_GRID.index(R) * 7 + M_GRID.index(M))
    out = []
    for K in sorted({min(k, M) for k in (1, 3, 10, M)}):
        for _ in range(2):
            t = next(turn)
            out.append(dict(R=R, M=M, K=K, V=V_GRID[t % 3], pool=POOL_KINDS[(t // 3) % 3], cap=CAP_KINDS[t % 6], uid=UID_KINDS[(t // 2) % 3],
                            seed=t))
    return out


TILE_CASES = [dict(R=5, M=64, K=51, V=33, pool="skewed", cap="ones", uid="none", seed=1),         # 255 held slots at most
              dict(R=64, M=5, K=4, V=4, pool="same", cap="mixed", uid="shuffled", seed=2),        # 256
              dict(R=2, M=256, K=128, V=33, pool="ties", cap="ones", uid="repeats", seed=3),      # 256
              dict(R=257, M=2, K=1, V=4, pool="same", cap="exactly_R", uid="none", seed=4)]       # 257


def build_case(c):
    ids, util = make_pool(c["R"], c["M"], c["V"], c["seed"], c["pool"])
    return ids, util, make_capacity(c["V"], c["R"], c["cap"], c["seed"]), make_user_ids(c["R"], c["uid"], c["seed"])


def chain_fixture(n=40):
    """n rows, capacities 1.  Row 0 wants item 1 only, with the highest utility of all; row r >= 1 wants item r first (a_r), then
    item r + 1 (b_r), a_1 > b_1 > a_2 > b_2 > ...  Every row first takes item r; row 0 displaces row 1 from item 1, row 1 then
    displaces row 2 from item 2, and so on: one displacement per round, n rounds in all, and in the end row r holds item r + 1."""
    M, V = 2, n + 2
    ids = np.full((n, M), -1, np.int64)
    util = np.full((n, M), -np.inf, F32)
    ids[0, 0], util[0, 0] = 1, F32(1000.0)
    for r in range(1, n):
        ids[r] = (r, r + 1)
        util[r] = (F32(500 - 2 * r), F32(500 - 2 * r - 1))
    return ids, util, np.ones(V, np.int32)
