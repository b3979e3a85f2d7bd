"""Joint recommendations (b4r_rank_joint) without a GPU: the restatement tests/joint_ref.py against brute force, its emulated fp32 fma
against exact rational arithmetic, the invariances the contract promises, the C entry point's argument errors and the Python layers'
ValueErrors.  The GPU suite (tests/test_gpu_joint.py) compares the device with this restatement bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, engine as engine_mod, models
from bert4rec_amd.apps import Recommender
from tests import catalogue_ref as ref
from tests import joint_ref as jr
from tests import score_dist_ref as sdr

F32 = np.float32
NINF = -np.inf
MODES = (jr.ADDITIVE, jr.LEAST_MISERY, jr.MOST_PLEASURE)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return a.shape == b.shape and np.array_equal(a.astype(np.int64), b.astype(np.int64))


def problem(seed, R=7, V=90, H=8, E=3, first=3, temperature=0.8):
    """t [R, V], allowed(r) [R, V], lse [R] of a small random model, with exact ties (twin table rows with equal bias)"""
    rng = np.random.default_rng(seed)
    hidden = rng.standard_normal((R, H)).astype(F32)
    table = rng.standard_normal((V, H)).astype(F32)
    bias = (0.1 * rng.standard_normal(V)).astype(F32)
    table[V // 2] = table[5]; bias[V // 2] = bias[5]
    table[V - 1] = table[6]; bias[V - 1] = bias[6]
    exclude = rng.integers(-1, V, size=(R, E)).astype(np.int64)
    t, ok = jr.row_quantities(hidden, table, bias, None, F32(1.0 / temperature), first, exclude)
    lse = sdr.blocked(t, ok)[2]
    return t, ok, lse


# ---- the emulated fma -----------------------------------------------------------------------------------------------------------------
def test_emulated_fma_equals_exact_rational_arithmetic():
    rng = np.random.default_rng(11)
    n = 4000
    w = np.abs(rng.standard_normal(n)).astype(F32)
    u = (rng.standard_normal(n) * 10).astype(F32)
    acc = (rng.standard_normal(n) * 10).astype(F32)
    # adversarial for the double rounding: products that land a hair off the midpoint of two fp32 neighbours of the sum
    k = n // 4
    acc[:k] = F32(1.0) + rng.integers(0, 1 << 10, k).astype(F32) * F32(2.0 ** -23)
    w[:k] = F32(2.0 ** -24) + F32(2.0 ** -47) * rng.integers(-1, 2, k).astype(F32)
    u[:k] = F32(1.0) + F32(2.0 ** -23) * rng.integers(-1, 2, k).astype(F32)
    # cancellation, zeros and signed zeros
    acc[k:k + 50] = -(w[k:k + 50] * u[k:k + 50])
    u[k + 50:k + 60] = F32(-0.0); acc[k + 50:k + 55] = F32(0.0); acc[k + 55:k + 60] = F32(-0.0)
    got = jr.fma32(w, u, acc)
    want = np.asarray([jr.fma32_exact(a, b, c) for a, b, c in zip(w, u, acc)], F32)
    assert same(got, want)
    plain = (w.astype(np.float64) * u.astype(np.float64) + acc.astype(np.float64)).astype(F32)
    assert not same(plain, want), "the adversarial cases must catch the plain double rounding"


# ---- the restatement against brute force ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("calibrated", (True, False))
def test_restatement_equals_a_brute_force_sort(mode, calibrated):
    t, ok, lse = problem(3)
    R, V = t.shape
    rng = np.random.default_rng(5)
    parties = np.asarray([[0, 1, -1], [2, -1, 3], [4, 5, 6], [-1, -1, -1], [1, 1, 4], [6, 99, -7]], np.int64)
    weights = rng.uniform(0.0, 2.0, size=parties.shape).astype(F32)
    min_util = F32(-12.0) if calibrated else F32(-1.0)         # a veto that binds and leaves something
    K = 12
    ids, scores, n, util = jr.rank_joint(t, ok, parties, mode, K, lse if calibrated else None, weights, min_util)
    for p in range(len(parties)):
        rows = [int(r) for r in parties[p] if 0 <= r < R]
        slots = [m for m, r in enumerate(parties[p]) if 0 <= r < R]
        cand = []
        for j in range(V):
            if not rows:
                break
            us = [F32(float(t[r, j]) - float(lse[r])) if calibrated else t[r, j] for r in rows]
            if not all(ok[r, j] for r in rows) or any(x < min_util for x in us):
                continue
            if mode == jr.ADDITIVE:
                a = F32(0.0)
                for m, x in zip(slots, us):
                    a = jr.fma32_exact(weights[p, m], x, a)
            else:
                a = F32(min(us) if mode == jr.LEAST_MISERY else max(us))
            cand.append((-float(a), j, a, us))
        cand.sort(key=lambda c: (c[0], c[1]))
        assert n[p] == len(cand)
        top = cand[:K]
        assert ids[p, :len(top)].tolist() == [c[1] for c in top] and (ids[p, len(top):] == -1).all()
        assert same(scores[p, :len(top)], np.asarray([c[2] for c in top], F32)) and (scores[p, len(top):] == NINF).all()
        for i, c in enumerate(top):
            assert same(util[p, i, slots], np.asarray(c[3], F32))
        absent = [m for m in range(parties.shape[1]) if m not in slots]
        assert (util[p][:, absent] == NINF).all() and (util[p, len(top):] == NINF).all()
    assert n[3] == 0 and n[0] > 0


def test_restatement_orders_ties_and_signed_zeros():
    u = np.asarray([[1.0, -0.0, 0.0, 1.0, -2.0, 0.0]], F32)
    ok = np.ones((1, 6), bool)
    ids, scores, n, _ = jr.rank_joint(u, ok, np.asarray([[0]]), jr.LEAST_MISERY, 8)
    assert ids[0].tolist() == [0, 3, 1, 2, 5, 4, -1, -1] and n[0] == 6
    assert np.signbit(scores[0, 2]) and not np.signbit(scores[0, 3])          # -0.0 ties with +0.0: the lower id first, own bits
    two = np.asarray([[0.0, -0.0], [-0.0, 0.0]], F32)                         # equal values: the earlier member's bits
    for mode in (jr.LEAST_MISERY, jr.MOST_PLEASURE):
        a = jr.aggregate(two, np.asarray([[0, 1]]), mode)
        assert not np.signbit(a[0, 0]) and np.signbit(a[0, 1])


# ---- a party of one is rank_full over that row ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_a_party_of_one_returns_rank_fulls_order(mode):
    t, ok, _ = problem(9, temperature=1.0)
    R = t.shape[0]
    K = 20
    parties = np.arange(R, dtype=np.int64)[:, None]
    ids, scores, n, util = jr.rank_joint(t, ok, parties, mode, K)
    want_ids, want_scores, _ = ref.expected(t, ok, None, K)
    assert same(ids, want_ids) and same(scores, want_scores) and same(n, ok.sum(axis=1))
    assert same(util[:, :, 0], scores)
    padded = np.full((R, 5), -1, np.int64)
    padded[:, 3] = np.arange(R)                                               # the member sits in another slot
    again = jr.rank_joint(t, ok, padded, mode, K)
    assert same(again[0], ids) and same(again[1], scores) and same(again[3][:, :, 3], scores)


# ---- invariances --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_result_does_not_depend_on_the_order_the_sharing_or_the_tile_of_the_parties(mode):
    t, ok, lse = problem(21)
    R = t.shape[0]
    rng = np.random.default_rng(2)
    NP, M, K = 11, 3, 9
    parties = rng.integers(-1, R, size=(NP, M)).astype(np.int64)
    weights = rng.uniform(0.5, 1.5, size=(NP, M)).astype(F32)
    whole = jr.rank_joint(t, ok, parties, mode, K, lse, weights, F32(-7.0))
    # the order of the parties
    perm = rng.permutation(NP)
    moved = jr.rank_joint(t, ok, parties[perm], mode, K, lse, weights[perm], F32(-7.0))
    assert all(same(m, w[perm]) for m, w in zip(moved, whole))
    # one party at a time (another tile, nobody to share a tile with), and among copies of itself
    for p in range(NP):
        alone = jr.rank_joint(t, ok, parties[p:p + 1], mode, K, lse, weights[p:p + 1], F32(-7.0))
        assert all(same(a[0], w[p]) for a, w in zip(alone, whole))
    # the rows duplicated, so that no two parties share a row
    t2, ok2, lse2 = (np.concatenate([x] * NP) for x in (t, ok, lse))
    own = np.where(parties >= 0, parties + R * np.arange(NP)[:, None], -1)
    apart = jr.rank_joint(t2, ok2, own, mode, K, lse2, weights, F32(-7.0))
    assert all(same(a, w) for a, w in zip(apart, whole))


def test_dead_members_empty_the_party():
    t, ok, lse = problem(4)
    lse = lse.copy()
    lse[2] = NINF
    got = jr.rank_joint(t, ok, np.asarray([[0, 2], [0, 1]]), jr.ADDITIVE, 5, lse)
    assert got[2].tolist()[0] == 0 and (got[0][0] == -1).all() and (got[1][0] == NINF).all() and (got[3][0] == NINF).all()
    assert got[2][1] > 0 and not np.isnan(got[1]).any() and not np.isnan(got[3]).any()


# ---- the C entry point checks before it launches ------------------------------------------------------------------------------------
ORDER = ("hidden", "hidden_ld", "hidden_row", "table", "bias", "H", "V", "first_item", "R", "exclude", "E", "allow_bits", "n_filters",
         "row_filter", "item_scale", "inv_temperature", "row_lse", "party_rows", "NP", "M", "member_weight", "mode", "min_member_util", "K",
         "topk_ids", "topk_scores", "party_n", "member_util", "scratch", "scratch_bytes")


def joint_call(**change):
    x = [C.create_string_buffer(256) for _ in range(12)]                     # never dereferenced: the checks come first
    ptr = [(C.addressof(b) + 15) & ~15 for b in x]
    a = dict(hidden=ptr[0], hidden_ld=8, hidden_row=None, table=ptr[1], bias=ptr[2], H=8, V=40, first_item=3, R=4, exclude=ptr[3], E=2,
             allow_bits=None, n_filters=0, row_filter=None, item_scale=None, inv_temperature=1.0, row_lse=ptr[4], party_rows=ptr[5], NP=2,
             M=2, member_weight=None, mode=0, min_member_util=-np.inf, K=5, topk_ids=ptr[6], topk_scores=ptr[7], party_n=ptr[8],
             member_util=ptr[9], scratch=ptr[10], scratch_bytes=16)
    a.update(change)
    return _lib.load().b4r_rank_joint(*[a[k] for k in ORDER], None)


def test_rank_joint_argument_errors_need_no_gpu():
    lib = _lib.load()
    for change in (dict(M=0), dict(M=17), dict(M=-1), dict(K=-1), dict(K=1025), dict(NP=-1), dict(R=-1), dict(E=-1), dict(first_item=-1),
                   dict(H=0), dict(H=6), dict(H=4100), dict(hidden_ld=4), dict(V=0), dict(allow_bits=1 << 12, n_filters=0)):
        assert joint_call(**change) == -2 and "b4r_rank_joint" in _lib.last_error(), (change, _lib.last_error())
    for change in (dict(mode=3), dict(mode=-1), dict(inv_temperature=0.0), dict(inv_temperature=-1.0), dict(inv_temperature=np.inf),
                   dict(inv_temperature=np.nan), dict(min_member_util=np.nan), dict(hidden=None), dict(table=None), dict(party_rows=None),
                   dict(exclude=None)):
        assert joint_call(**change) == -1 and "b4r_rank_joint" in _lib.last_error(), (change, _lib.last_error())
    assert joint_call(M=17, mode=7) == -2                                     # the shape comes first
    assert joint_call(table=(C.addressof(C.create_string_buffer(64)) | 4)) == -3
    # a scratch too small for one tile
    assert joint_call() == -5 and "too small" in _lib.last_error()
    assert joint_call(scratch=None, scratch_bytes=0) == -5
    # nothing to do: NP = 0 or K = 0 succeeds and launches nothing, whatever the pointers are
    for change in (dict(NP=0), dict(K=0), dict(NP=0, hidden=None, table=None, party_rows=None, scratch=None), dict(K=0, M=16, scratch=None),
                   dict(NP=0, K=1024, M=1)):
        assert joint_call(**change) == 0, (change, _lib.last_error())
    assert joint_call(NP=0, M=17) == -2 and joint_call(K=0, mode=5) == -1 and joint_call(NP=0, inv_temperature=0.0) == -1
    # the scratch grows with the parties, the chunks and K, not with V * NP
    sb = lib.b4r_rank_joint_scratch_bytes
    assert sb(0, 2, 40, 5) == 0 and sb(2, 0, 40, 5) == 0 and sb(2, 17, 40, 5) == 0 and sb(2, 2, 0, 5) == 0 and sb(2, 2, 40, 1025) == 0
    assert sb(2, 2, 40, 5) == 2 * (1 * (5 * 8 + 8) + 5 * 8) + 64
    assert sb(3, 16, 2051, 1024) == 3 * (3 * (1024 * 8 + 8) + 1024 * 8) + 64


# ---- the Python layers ----------------------------------------------------------------------------------------------------------------
def test_python_layers_refuse_bad_arguments_before_any_work():
    check = engine_mod.check_joint_args
    p, k, mode, w, least, inv_t = check([[0, 1, -1], [2, -5, 1]], 7, "least_misery", None, 0.01, True, 2.0, 3)
    assert p.dtype == torch.int32 and p.tolist() == [[0, 1, -1], [2, -1, 1]] and (k, mode, w, inv_t) == (7, 1, None, 0.5)
    assert least == float(F32(np.log(0.01)))
    assert check(np.zeros((0, 4), np.int64), 0)[0].shape == (0, 4)
    assert check([[0]], 3, "additive", [[2]])[3].tolist() == [[2.0]] and check([[0]], 3)[4] == NINF
    good = [[0, 1], [1, -1]]
    for args, match in ((([0, 1], 5), "parties"), (([[0.0, 1.0]], 5), "parties"), (([[True]], 5), "parties"), (([[[0]]], 5), "parties"),
                        ((np.zeros((2, 17), np.int64), 5), "member slots"), ((np.zeros((2, 0), np.int64), 5), "member slots"),
                        ((good, -1), "k"), ((good, 1025), "k"), ((good, 2.5), "k"),
                        ((good, 5, "average"), "strategy"), ((good, 5, None), "strategy"),
                        ((good, 5, "least_misery", [[1, 1], [1, 1]]), "additive"), ((good, 5, "most_pleasure", [[1, 1], [1, 1]]), "additive"),
                        ((good, 5, "additive", [[1, 1]]), "shape of parties"), ((good, 5, "additive", [[1, -1], [1, 1]]), "finite and >= 0"),
                        ((good, 5, "additive", [[1, np.nan], [1, 1]]), "finite and >= 0"),
                        ((good, 5, "additive", None, 0.0), "min_member_probability"), ((good, 5, "additive", None, 1.5), "min_member_probability"),
                        ((good, 5, "additive", None, True), "min_member_probability"),
                        ((good, 5, "additive", None, 0.5, False), "calibrated"), ((good, 5, "additive", None, None, False, 2.0), "calibrated"),
                        ((good, 5, "additive", None, None, True, 0.0), "temperature"), ((good, 5, "additive", None, None, True, -1.0), "temperature"),
                        ((good, 5, "additive", None, None, True, 1.0, 1), "row 1 of 1")):
        with pytest.raises(ValueError, match=match):
            check(*args)

    model = object.__new__(models.BERT4RecModel)            # the checks come before anything of the model's engine is touched
    model.vocab_size = 50
    call = models.BERT4RecModel.recommend_joint_tensor
    one = torch.zeros((3, 6), dtype=torch.int64)
    one[:, 0] = 1
    batch = {"input_word_ids": torch.zeros((3, 24), dtype=torch.int64), "masked_lm_positions": torch.zeros((3, 6), dtype=torch.int64),
             "masked_lm_weights": one}
    for b, parties, kw, match in ((batch, [[0, 3]], {}, "row 3 of 3"), (batch, [0, 1], {}, "parties"), (batch, np.zeros((1, 17), np.int64), {}, "member slots"),
                                  (batch, good, dict(k=1025), "k"), (batch, good, dict(strategy="mean"), "strategy"),
                                  (batch, good, dict(strategy="least_misery", weights=[[1, 1], [1, 1]]), "additive"),
                                  (batch, good, dict(weights=[[1, 1]]), "shape of parties"),
                                  (batch, good, dict(calibrated=False, temperature=0.5), "calibrated"),
                                  (batch, good, dict(calibrated=False, min_member_probability=0.1), "calibrated"),
                                  (batch, good, dict(min_member_probability=2), "min_member_probability"),
                                  (batch, good, dict(temperature=0.0), "temperature"),
                                  (batch, good, dict(exclude=torch.zeros(3, dtype=torch.int64)), "exclude"),
                                  (batch, good, dict(row_filter=torch.zeros(3, dtype=torch.int32)), "row_filter"),
                                  (batch, good, dict(allow=torch.ones(49, dtype=torch.bool)), "allow"),
                                  ({}, good, {}, "prepare_inference"),
                                  ({"input_word_ids": torch.zeros(24, dtype=torch.int64)}, good, {}, "prepare_inference")):
        with pytest.raises(ValueError, match=match):
            call(model, b, parties, **kw)
    with pytest.raises(ValueError, match="row 3 of 3"):
        models.BERT4RecModel.recommend_joint(model, batch, [[3]])

    rec = Recommender(None, None)
    seq = ["a", "b"]
    for parties, kw, match in (([[seq] * 17], {}, "members"), ([[]], {}, "members"), ([[seq]], dict(k=1025), "k"), ([[seq]], dict(k=-1), "k"),
                               ([[seq]], dict(strategy="sum"), "strategy"), ([[seq, seq]], dict(weights=[[1]]), "one number per member"),
                               ([[seq, seq]], dict(weights=[[1, 1], [1]]), "one number per member"),
                               ([[seq, seq]], dict(weights=[[1, -1]]), "finite and >= 0"),
                               ([[seq, seq]], dict(strategy="least_misery", weights=[[1, 1]]), "additive"),
                               ([[seq]], dict(min_member_probability=0), "min_member_probability"),
                               ([[seq]], dict(min_member_probability=1.2), "min_member_probability")):
        with pytest.raises(ValueError, match=match):
            rec.recommend_together(parties, **kw)
    assert rec.recommend_together([]) == []
