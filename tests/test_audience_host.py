"""Audience selection without a GPU: the restatement of tests/audience_ref.py against a brute-force sort of all (user, logp) pairs,
its invariance under any slicing and order of the users, the argument checks of the C entry point (all made before any launch) and of
the Python layers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, engine as engine_mod, models
from bert4rec_amd.apps import Recommender
from tests import audience_ref as ar

F32 = np.float32
NINF = F32(-np.inf)


def planted_audience(R, Q, ld, seed, ids="shuffled", id0=1000):
    """Log probabilities on a coarse grid in [-4, 0] (exact ties across users are the rule), -0.0 against +0.0, -inf and NaN entries,
    dead users (negative ids), and from two items on a column without a live user.  ids: "shuffled" = user_ids out of order (a
    permutation of id0 .. id0 + R - 1, some of them replaced by negative ids); "user0" = the user0 + r form, which starts three rows
    below zero.  Returns (logp [R, ld] with garbage in the columns >= Q, user_ids or None, user0)."""
    rng = np.random.default_rng(seed)
    logp = (-np.round(rng.random((R, ld)) * 16) / 4).astype(F32)
    logp[rng.random((R, ld)) < 0.08] = NINF
    logp[rng.random((R, ld)) < 0.04] = np.nan
    zero = logp == 0
    logp[zero & (rng.random((R, ld)) < 0.5)] = F32(-0.0)
    if Q >= 2:
        logp[:, 1] = np.where(rng.random(R) < 0.5, NINF, np.nan)             # nobody can be served item 1
    logp[:, Q:] = F32(7.0)                                                   # never read: columns beyond Q
    if ids == "user0":
        return logp, None, id0 - 3 if id0 == 0 else id0
    users = (id0 + rng.permutation(R)).astype(np.int64)
    users[rng.random(R) < 0.05] = -1
    if R >= 4:
        users[3] = -(1 << 40)
    return logp, users, 0


def brute_force(pairs, K):
    """pairs: (user, logp, origin, index) of the live entries of one item; the stated order by a comparison sort"""
    def cmp(a, b):
        xa, xb = float(a[1]), float(b[1])                                    # -0.0 == 0.0
        if xa != xb:
            return -1 if xa > xb else 1
        if a[0] != b[0]:
            return -1 if a[0] < b[0] else 1
        return -1 if (a[2], a[3]) < (b[2], b[3]) else 1
    return sorted(pairs, key=functools.cmp_to_key(cmp))[:K]


def live_pairs(logp, users, q, origin):
    with np.errstate(invalid="ignore"):
        return [(int(users[r]), logp[r, q], origin, r) for r in range(logp.shape[0]) if users[r] >= 0 and logp[r, q] > NINF]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the restatement = a brute-force sort -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Q,K,ids", [(1, 1, 1, "shuffled"), (40, 3, 5, "shuffled"), (40, 3, 64, "user0"), (257, 4, 17, "shuffled"),
                                       (300, 2, 300, "user0"), (0, 2, 4, "user0")])
def test_restatement_equals_a_brute_force_sort(R, Q, K, ids):
    for seed in range(3):
        logp, users, user0 = planted_audience(R, Q, Q + 2, seed, ids, id0=0 if ids == "user0" else 1000)
        names = ar.users_of(R, users, user0)
        got_u, got_x, reach, demand = ar.audience_merge(logp, Q, K, *ar.init_state(Q, K), user_ids=users, user0=user0, min_logp=F32(-2.0))
        # a second batch into the pre-filled lists, ids interleaved with the first one's, the first rows tie with the K-th entries
        logp2, users2, _ = planted_audience(50, Q, Q + 2, seed + 100, "shuffled", id0=5000)
        users2[::2] = np.arange(0, 50, 2) * 7 + 1                            # some ids below every id of the first batch
        for q in range(Q):
            if got_u[q, K - 1] >= 0:
                logp2[q % 50, q] = got_x[q, K - 1]
        two = ar.audience_merge(logp2, Q, K, got_u, got_x, reach, demand, user_ids=users2, min_logp=F32(-2.0))
        for q in range(Q):
            first = brute_force(live_pairs(logp, names, q, 1), K)
            assert got_u[q, :len(first)].tolist() == [p[0] for p in first] and (got_u[q, len(first):] == -1).all()
            assert same(got_x[q, :len(first)], np.asarray([p[1] for p in first], F32).reshape(-1)) and np.isneginf(got_x[q, len(first):]).all()
            running = [(int(got_u[q, e]), got_x[q, e], 0, e) for e in range(len(first))]
            second = brute_force(running + live_pairs(logp2, users2, q, 1), K)
            assert two[0][q, :len(second)].tolist() == [p[0] for p in second] and (two[0][q, len(second):] == -1).all()
            assert same(two[1][q, :len(second)], np.asarray([p[1] for p in second], F32).reshape(-1))
            live1, live2 = live_pairs(logp, names, q, 1), live_pairs(logp2, users2, q, 1)
            assert reach[q] == sum(float(p[1]) >= -2.0 for p in live1)
            assert two[2][q] == reach[q] + sum(float(p[1]) >= -2.0 for p in live2)
            assert two[3][q] == int(ar.demand_terms(np.asarray([p[1] for p in live1 + live2], F32)).sum())
        if Q >= 2:
            assert (got_u[1] == -1).all() and reach[1] == 0 and demand[1] == 0


def test_restatement_orders_ties_zeros_and_running_entries():
    logp = np.asarray([[-1.0, 0.0], [-1.0, -0.0], [-0.5, np.nan], [-np.inf, -3.0], [-1.0, 0.0]], F32)
    users = np.asarray([9, 4, 7, 1, -2], np.int64)
    u, x, reach, demand = ar.audience_merge(logp, 2, 3, *ar.init_state(2, 3), user_ids=users, min_logp=F32(-1.0))
    assert u.tolist() == [[7, 4, 9], [4, 9, 1]] and x[0].tolist() == [-0.5, -1.0, -1.0]
    assert np.signbit(x[1, 0]) and not np.signbit(x[1, 1]) and x[1, 2] == -3.0      # -0.0 ties with +0.0: the lower id first, own bits
    assert reach.tolist() == [3, 2] and demand[1] == 2 * (1 << 40) + int(np.rint(np.exp(np.float64(-3.0)) * 2.0 ** 40))
    # the same user and logp again: the running entry stays in front, the list does not change
    again = ar.audience_merge(logp[:1], 1, 3, u[:1], x[:1], user_ids=users[:1])
    assert same(again[0], u[:1]) and same(again[1], x[:1]) and again[2] is None and again[3] is None
    # K = 1 against a tie with the running entry: the lower id wins from either side
    low = ar.audience_merge(np.asarray([[-0.5]], F32), 1, 1, u[:1, :1], x[:1, :1], user_ids=np.asarray([3], np.int64))
    high = ar.audience_merge(np.asarray([[-0.5]], F32), 1, 1, u[:1, :1], x[:1, :1], user_ids=np.asarray([8], np.int64))
    assert low[0].tolist() == [[3]] and high[0].tolist() == [[7]]


# ---- invariance: any slicing, any order -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 7, 64, 400])
def test_restatement_does_not_depend_on_the_slicing_nor_on_the_order(K):
    R, Q = 300, 3
    logp, users, _ = planted_audience(R, Q, Q, seed=K)
    whole = ar.merge_in_slices(logp, users, Q, K, [np.arange(R)], min_logp=F32(-1.5))
    rng = np.random.default_rng(K)
    for step in (1, 7, 64, 299):
        slices = [np.arange(s, min(R, s + step)) for s in range(0, R, step)]
        for order in (slices, slices[::-1], [slices[i] for i in rng.permutation(len(slices))], [s[::-1] for s in slices]):
            got = ar.merge_in_slices(logp, users, Q, K, order, min_logp=F32(-1.5))
            assert all(same(g, w) for g, w in zip(got, whole)), step
    assert (whole[0][0] >= 0).sum() == min(K, int(((users >= 0) & (logp[:, 0] > NINF)).sum()))


# ---- the C entry point checks before it launches ------------------------------------------------------------------------------------
ORDER = ("logp", "ld", "R", "Q", "user_ids", "user0", "min_logp", "K", "best_user", "best_logp", "reach", "demand")


def merge_call(**change):
    x = [C.create_string_buffer(64) for _ in range(6)]                       # never dereferenced: the checks come first
    ptr = [C.addressof(b) for b in x]
    a = dict(logp=ptr[0], ld=4, R=1, Q=4, user_ids=ptr[1], user0=0, min_logp=-np.inf, K=2, best_user=ptr[2], best_logp=ptr[3],
             reach=ptr[4], demand=ptr[5])
    a.update(change)
    return _lib.load().b4r_audience_merge(*[a[k] for k in ORDER], None)


def test_audience_merge_argument_errors_need_no_gpu():
    for change in (dict(K=0), dict(K=1025), dict(K=-1), dict(Q=0), dict(Q=-2), dict(ld=3), dict(ld=0), dict(R=-1)):
        assert merge_call(**change) == -2 and "b4r_audience_merge" in _lib.last_error(), (change, _lib.last_error())
    for name in ("logp", "best_user", "best_logp"):
        assert merge_call(**{name: None}) == -1 and "null" in _lib.last_error(), name
    assert merge_call(min_logp=float("nan")) == -1 and "NaN" in _lib.last_error()
    assert merge_call(R=1, K=0, logp=None) == -2                             # the shape comes first
    # nothing to do: R = 0 succeeds with the legal shapes at their ends, and launches nothing
    for change in (dict(R=0), dict(R=0, K=1024, Q=1, ld=1), dict(R=0, user_ids=None, reach=None, demand=None), dict(R=0, min_logp=0.0)):
        assert merge_call(**change) == 0, _lib.last_error()
    assert merge_call(R=0, K=1025) == -2 and merge_call(R=0, logp=None) == -1 and merge_call(R=0, min_logp=float("nan")) == -1


# ---- the Python layers ----------------------------------------------------------------------------------------------------------------
def fake_state(item_ids, k):
    Q = len(item_ids)
    return {"users": torch.full((Q, k), -1, dtype=torch.int64), "logp": torch.full((Q, k), -np.inf), "reach": torch.zeros(Q, dtype=torch.int64),
            "demand": torch.zeros(Q, dtype=torch.int64), "item_ids": torch.as_tensor(item_ids, dtype=torch.int64), "next_user": 0}


def test_python_layers_refuse_bad_arguments_before_any_work():
    check = engine_mod.check_audience_args
    assert check(100) == (100, -np.inf) and check(np.int64(1), 1.0) == (1, 0.0) and check(1024, 1) == (1024, 0.0)
    k, least = check(5, 0.01)
    assert k == 5 and least == float(F32(np.log(0.01))) and F32(least) == F32(np.log(0.01))
    for k in (0, 1025, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="k"):
            check(k)
    for p in (0, 0.0, -0.1, 1.5, True, "0.5", float("nan")):
        with pytest.raises(ValueError, match="min_probability"):
            check(5, p)

    model = object.__new__(models.BERT4RecModel)            # the checks come before anything of the model's engine is touched
    model.vocab_size = 50
    call = models.BERT4RecModel.audience_tensor
    one = torch.zeros((2, 6), dtype=torch.int64)
    one[:, 0] = 1
    batch = {"input_word_ids": torch.zeros((2, 24), dtype=torch.int64), "masked_lm_positions": torch.zeros((2, 6), dtype=torch.int64),
             "masked_lm_weights": one}
    items = torch.as_tensor([5, 9, 7])
    two = one.clone()
    two[1, 3] = 1                                                            # two ranked slots in a row
    none = one.clone()
    none[0, 0] = 0
    for b, it, kw, match in ((batch, items, dict(state=fake_state([5, 9, 8], 100)), "other item_ids"),
                             (batch, items, dict(state=fake_state([5, 9], 100)), "other item_ids"),
                             (batch, items, dict(state=fake_state([5, 9, 7], 10)), "k = 10"),
                             (batch, items, dict(state=fake_state([5, 9, 7], 10), k=11), "k = 10"),
                             (batch, items, dict(state={"users": None}), "state"),
                             ({**batch, "masked_lm_weights": two}, items, {}, "one ranked slot"),
                             ({**batch, "masked_lm_weights": none}, items, {}, "one ranked slot"),
                             ({k: v for k, v in batch.items() if k != "masked_lm_weights"}, items, {}, "one ranked slot"),
                             ({**batch, "masked_lm_weights": two}, items, dict(state=fake_state([5, 9, 7], 100)), "one ranked slot"),
                             (batch, items, dict(min_probability=0.0), "min_probability"), (batch, items, dict(min_probability=1.01), "min_probability"),
                             (batch, items, dict(min_probability=-1), "min_probability"),
                             (batch, items, dict(temperature=0.0), "temperature"), (batch, items, dict(temperature=-2.0), "temperature"),
                             (batch, items, dict(k=0), "k"), (batch, items, dict(k=1025), "k"),
                             (batch, torch.zeros(0, dtype=torch.int64), {}, "item_ids"), (batch, torch.zeros((2, 2), dtype=torch.int64), {}, "item_ids"),
                             (batch, torch.zeros(3), {}, "item_ids"),
                             (batch, items, dict(user_ids=torch.zeros(3, dtype=torch.int64)), "for 2 rows"),
                             (batch, items, dict(user_ids=torch.zeros(2)), "integer"),
                             (batch, items, dict(row_filter=torch.zeros(2, dtype=torch.int32)), "row_filter"),
                             (batch, items, dict(allow=torch.ones(49, dtype=torch.bool)), "allow"),
                             ({}, items, {}, "prepare_inference"),
                             ({"input_word_ids": torch.zeros(24, dtype=torch.int64), "masked_lm_positions": one}, items, {}, "prepare_inference")):
        with pytest.raises(ValueError, match=match):
            call(model, b, it, **kw)

    rec = Recommender(None, None)
    for kw, match in ((dict(k=0), "k"), (dict(k=1025), "k"), (dict(min_probability=0), "min_probability"), (dict(min_probability=2), "min_probability"),
                      (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"), (dict(batch_size=0), "batch_size"),
                      (dict(user_ids=["a", "b"]), "user ids"), (dict(allowed_items=["a"], allowed_items_per_user=[["a"]]), "not both"),
                      (dict(allowed_items_per_user=[["a"], ["b"]]), "allow-lists")):
        with pytest.raises(ValueError, match=match):
            rec.audience(["x"], [[1, 2]], **kw)
