"""CPU restatement of b4r_audience_merge (include/b4r.h) in numpy: the merge of one batch of users into the K best users of every
item, and both accumulators.  Every output bit of the kernel except `demand` is reproduced (demand: the device's exp against libm's,
one unit per live entry at the most)."""
import numpy as np

F32 = np.float32
NINF = F32(-np.inf)
DEMAND_ONE = float(1 << 40)


def order_image(x):
    """uint32 image of float32 values whose unsigned order is the float order, -0.0 counting as +0.0"""
    x = np.array(x, dtype=F32)
    x[x == 0] = F32(0.0)
    u = x.view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def users_of(R, user_ids=None, user0=0):
    if user_ids is not None:
        return np.asarray(user_ids, np.int64)
    with np.errstate(over="ignore"):
        return (np.asarray(user0, np.int64).astype(np.uint64) + np.arange(R, dtype=np.uint64)).astype(np.int64)   # wraps as the kernel's


def init_state(Q, K):
    return (np.full((Q, K), -1, np.int64), np.full((Q, K), NINF, F32), np.zeros(Q, np.int64), np.zeros(Q, np.int64))


def demand_terms(x):
    """llrint(exp((double) x) * 2^40) of float32 log probabilities (round to nearest even, as llrint in the default mode)"""
    return np.rint(np.exp(np.asarray(x, F32).astype(np.float64)) * DEMAND_ONE).astype(np.int64)


def audience_merge(logp, Q, K, best_user, best_logp, reach=None, demand=None, user_ids=None, user0=0, min_logp=NINF):
    """logp [R, ld >= Q] float32; best_user / best_logp [Q, K]; reach / demand [Q] int64 or None.  Returns NEW arrays (best_user,
    best_logp, reach, demand).  Order: logp descending (-0.0 = +0.0), then the lower user id, then running before new (then the
    earlier entry).  A running entry is live when user >= 0 and logp > -inf, a new one likewise (a NaN is dead)."""
    logp = np.asarray(logp, F32)
    R = logp.shape[0]
    users = users_of(R, user_ids, user0)
    out_u, out_x = np.full((Q, K), -1, np.int64), np.full((Q, K), NINF, F32)
    out_reach = None if reach is None else np.array(reach, np.int64)
    out_demand = None if demand is None else np.array(demand, np.int64)
    min_logp = F32(min_logp)
    assert not np.isnan(min_logp)
    with np.errstate(invalid="ignore"):
        for q in range(Q):
            col = logp[:, q] if R else np.zeros(0, F32)
            new_live = (users >= 0) & (col > NINF)
            run_live = (best_user[q] >= 0) & (best_logp[q] > NINF)
            u = np.concatenate([best_user[q][run_live], users[new_live]])
            x = np.concatenate([best_logp[q][run_live], col[new_live]])
            origin = np.concatenate([np.zeros(int(run_live.sum()), np.int64), np.ones(int(new_live.sum()), np.int64)])
            index = np.concatenate([np.flatnonzero(run_live), np.flatnonzero(new_live)])
            # lexsort: the last key is the primary one
            order = np.lexsort((index, origin, u, (~order_image(x)).astype(np.uint32)))[:K]
            out_u[q, :order.size] = u[order]
            out_x[q, :order.size] = x[order]
            if out_reach is not None:
                out_reach[q] += int((new_live & (col >= min_logp)).sum())
            if out_demand is not None:
                out_demand[q] += int(demand_terms(col[new_live]).sum())
    return out_u, out_x, out_reach, out_demand


def merge_in_slices(logp, users, Q, K, slices, min_logp=NINF):
    """The state after one audience_merge call per slice (index arrays into the rows), from the initial state"""
    state = init_state(Q, K)
    for rows in slices:
        state = audience_merge(logp[rows], Q, K, *state, user_ids=users[rows], min_logp=min_logp)
    return state
