"""The stock-aware allocation without a GPU: the plain-Python restatement (tests/allocate_ref.py) checked independently -- its result
is stable and feasible on every case the GPU tests walk, and without a binding capacity it is each row's first K live entries --, the
Python-level argument checks, and b4r_allocate's argument errors, which return before any launch."""
import numpy as np
import pytest
import torch

from bert4rec_amd import _lib
from bert4rec_amd import engine as engine_mod
from tests import allocate_ref as ar

OK, BADARG, SHAPE, NOMEM = 0, -1, -2, -5


# ---- the restatement, checked by something that is not the restatement ---------------------------------------------------------------
def check_case(c):
    ids, util, cap, uid = ar.build_case(c)
    want = ar.greedy(ids, util, c["K"], cap, uid)
    assert ar.feasible(want, ids, util, c["K"], cap), c
    assert len(ar.blocking_edges(ids, util, c["K"], cap, uid, want["assigned"])) == 0, c
    return ids, util, cap, uid, want


@pytest.mark.parametrize("R,M", ar.shapes())
def test_the_restated_result_is_stable_and_feasible(R, M):
    for c in ar.cases_of(R, M):
        check_case(c)


def test_the_restated_result_is_stable_at_the_tile_cases_and_the_chain():
    for c in ar.TILE_CASES:
        check_case(c)
    ids, util, cap = ar.chain_fixture(40)
    want = ar.greedy(ids, util, 1, cap)
    assert len(ar.blocking_edges(ids, util, 1, cap, None, want["assigned"])) == 0
    assert want["ids"][:, 0].tolist() == list(range(1, 41)) and want["pos"][:, 0].tolist() == [0] + [1] * 39   # row r ends with item r + 1


def test_the_stability_check_sees_a_wrong_result():
    """the check is not vacuous: moving one unit from the edge that won it to the edge that lost it is a blocking pair"""
    ids = np.array([[3, 4], [3, 5]], np.int64)
    util = np.array([[2.0, 1.0], [3.0, 0.5]], np.float32)
    cap = np.ones(6, np.int32)
    want = ar.greedy(ids, util, 1, cap)
    assert want["ids"].tolist() == [[4], [3]] and want["remaining"].tolist() == [1, 1, 1, 0, 0, 1]
    wrong = np.array([[True, False], [False, True]])
    assert ar.blocking_edges(ids, util, 1, cap, None, wrong).tolist() == [[1, 0]]
    assert ar.blocking_edges(ids, util, 1, cap, np.array([5, 2]), want["assigned"]).tolist() == []


def test_the_cases_cover_what_they_claim():
    cases = [c for R, M in ar.shapes() for c in ar.cases_of(R, M)] + ar.TILE_CASES
    assert {c["K"] for c in cases} >= {1, 3, 10, 63, 64, 65, 256, 1024} and {c["V"] for c in cases} == set(ar.V_GRID)
    assert {c["cap"] for c in cases} == set(ar.CAP_KINDS) and {c["uid"] for c in cases} == set(ar.UID_KINDS)
    assert {c["pool"] for c in cases} == set(ar.POOL_KINDS) and all(c["R"] <= 5 for c in cases if c["M"] == 1024)
    assert sorted(c["R"] * c["K"] for c in ar.TILE_CASES) == [255, 256, 256, 257]
    seen = dict(nan=False, pinf=False, ninf=False, neg=False, past=False, negzero=False, poszero=False, repeat=False, tie_rows=False, tail=False)
    for c in cases:
        ids, util, cap, uid = ar.build_case(c)
        seen["nan"] |= bool(np.isnan(util).any())
        seen["pinf"] |= bool(np.isposinf(util).any())
        seen["ninf"] |= bool((np.isneginf(util) & (ids >= 0)).any())
        seen["tail"] |= bool((np.isneginf(util[:, -1]) & (ids[:, -1] == -1)).any())
        seen["neg"] |= bool((ids < -1).any())
        seen["past"] |= bool((ids >= c["V"]).any())
        seen["negzero"] |= bool(((util == 0) & np.signbit(util)).any())
        seen["poszero"] |= bool(((util == 0) & ~np.signbit(util)).any())
        _, _, _, ok = ar.live_edges(ids, util, cap)
        for r in range(min(c["R"], 3)):
            live = ids[r][ok[r]]
            seen["repeat"] |= live.size != np.unique(live).size
            u = util[r][ok[r]]
            assert (np.diff(u) <= 0).all(), c                          # the contract: a row's live entries in descending utility
        if c["R"] > 1 and ok[0].any() and ok[1].any():
            seen["tie_rows"] |= bool(np.intersect1d(util[0][ok[0]], util[1][ok[1]]).size)
    assert all(seen.values()), seen


@pytest.mark.parametrize("R,M,K,V", ((5, 7, 3, 33), (64, 65, 10, 4), (3, 1024, 1024, 1027)))
def test_without_a_binding_capacity_every_row_keeps_its_first_live_entries(R, M, K, V):
    ids, util = ar.make_pool(R, M, V, seed=7)
    for cap in (np.full(V, R * M, np.int32), ar.make_capacity(V, R, "plenty")):   # a row may hold an id more than once: R * M suffices
        want = ar.greedy(ids, util, K, cap, ar.make_user_ids(R, "shuffled"))
        live = (ids >= 0) & (ids < V) & np.isfinite(util)
        for r in range(R):
            p = np.nonzero(live[r])[0][:K]
            assert want["row_n"][r] == p.size and want["pos"][r, :p.size].tolist() == p.tolist() and (want["pos"][r, p.size:] == -1).all()
            assert want["ids"][r, :p.size].tolist() == ids[r, p].tolist()
        assert int((cap.astype(np.int64) - want["remaining"]).sum()) == int(want["row_n"].sum())


# ---- Python-level argument errors ---------------------------------------------------------------------------------------------------
def test_python_argument_checks():
    assert engine_mod.check_allocate_args(10, 4096, 100) == (10, None, 32)
    assert engine_mod.check_allocate_args(0, 0, 1, max_rounds=5, chunk=1) == (0, 5, 1)
    for bad in (dict(k=-1), dict(k=101), dict(k=2.5), dict(k=True), dict(max_rounds=0), dict(max_rounds=1.5), dict(chunk=0),
                dict(n_rows=(1 << 20) + 1, k=0), dict(n_rows=1 << 17, k=9)):
        with pytest.raises(ValueError):
            engine_mod.check_allocate_args(**{"k": 10, "n_rows": 8, "pool_width": 100, **bad})
    cap = engine_mod.check_capacity(np.array([0, -1, 5, (1 << 31) - 1], np.int64), 4)
    assert cap.dtype == torch.int32 and cap.tolist() == [0, -1, 5, (1 << 31) - 1]
    for bad in (np.zeros(3, np.int64), np.zeros((4, 1), np.int64), np.zeros(4, np.float32), np.zeros(4, bool), np.array([0, 0, 0, 1 << 31])):
        with pytest.raises(ValueError):
            engine_mod.check_capacity(bad, 4)
    assert engine_mod.check_allocate_user_ids(None, 3) is None
    assert engine_mod.check_allocate_user_ids([5, -2, 5], 3).dtype == torch.int64
    for bad in ([1, 2], [[1, 2, 3]], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            engine_mod.check_allocate_user_ids(bad, 3)
    cap = engine_mod.stock_capacity({3: 500, 5: 0, 6: -4}, 8)
    big = engine_mod.ALLOCATE_UNLIMITED
    assert cap.dtype == torch.int32 and cap.tolist() == [big, big, big, 500, big, 0, 0, big]
    for bad in ({3: 1.5}, {3: True}, {3: 1 << 31}):
        with pytest.raises(ValueError):
            engine_mod.stock_capacity(bad, 8)


# ---- C-level argument errors that return before any launch --------------------------------------------------------------------------
FAKE = 4096        # a non-NULL, 8-byte aligned value that is never dereferenced: every call below returns before its launch


def call(lib, R=5, M=7, K=3, V=50, rounds=1, resume=0, nbytes=None, **ptr):
    p = dict(pool_ids=FAKE, pool_util=FAKE, capacity=FAKE, user_ids=None, out_ids=FAKE, out_util=FAKE, out_pos=FAKE, row_n=FAKE, remaining=FAKE,
             unsettled=FAKE, scratch=FAKE)
    p.update(ptr)
    if nbytes is None:
        nbytes = max(lib.b4r_allocate_scratch_bytes(R, M, K, V), 0)
    return lib.b4r_allocate(p["pool_ids"], p["pool_util"], R, M, K, V, p["capacity"], p["user_ids"], rounds, resume, p["out_ids"], p["out_util"],
                            p["out_pos"], p["row_n"], p["remaining"], p["unsettled"], p["scratch"], nbytes, None)


def test_the_binding_exists():
    assert "b4r_allocate" in _lib.PROTOTYPES and "b4r_allocate_scratch_bytes" in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES["b4r_allocate"]
    assert len(args) == 19 and hasattr(_lib.load(), "b4r_allocate")


def test_scratch_bytes():
    lib = _lib.load()
    assert lib.b4r_allocate_scratch_bytes(5, 7, 3, 50) == 4 * (16 + 5 + 2 * 50 + 4 * 15 + 1)
    assert lib.b4r_allocate_scratch_bytes(0, 1, 0, 1) == 4 * (16 + 2)
    assert lib.b4r_allocate_scratch_bytes(1 << 20, 1, 1, 1) == 4 * (16 + (1 << 20) + 2 + 4 * (1 << 20) + (1 << 12))
    assert lib.b4r_allocate_scratch_bytes(257, 2, 1, 4) == 4 * (16 + 257 + 8 + 4 * 257 + 2)
    assert lib.b4r_allocate_scratch_bytes(1 << 10, 1024, 1024, 1 << 30) > 1 << 33            # no 32-bit arithmetic
    for bad in ((-1, 7, 3, 50), (5, 0, 0, 50), (5, 1025, 3, 50), (5, 7, 8, 50), (5, 7, -1, 50), (5, 7, 3, 0), ((1 << 20) + 1, 7, 0, 50),
                ((1 << 19) + 1, 7, 2, 50)):
        assert lib.b4r_allocate_scratch_bytes(*bad) == -1, bad
        assert "bad shape" in _lib.last_error()


def test_allocate_argument_errors():
    lib = _lib.load()
    for bad in (dict(R=-1), dict(M=0, K=0), dict(M=1025), dict(K=8), dict(K=-1), dict(V=0), dict(R=(1 << 19) + 1, K=2), dict(R=(1 << 20) + 1, K=0)):
        assert call(lib, **bad) == SHAPE, bad
        assert "bad shape" in _lib.last_error()
    for bad in (dict(rounds=0), dict(rounds=-3), dict(resume=2), dict(resume=-1)):
        assert call(lib, **bad) == BADARG, bad
        assert "rounds" in _lib.last_error()
    for null in ("pool_ids", "pool_util", "capacity", "scratch"):
        assert call(lib, **{null: None}) == BADARG and "null" in _lib.last_error(), null
    assert call(lib, scratch=FAKE + 4) == BADARG and "aligned" in _lib.last_error()
    need = lib.b4r_allocate_scratch_bytes(5, 7, 3, 50)
    assert call(lib, nbytes=need - 1) == NOMEM and f"{need} needed" in _lib.last_error()
    # R = 0 or K = 0 launches nothing; without `remaining` it touches nothing at all
    assert call(lib, R=0, pool_ids=None, pool_util=None, scratch=None, remaining=None, nbytes=0) == OK
    assert call(lib, K=0, pool_ids=None, pool_util=None, scratch=None, remaining=None, nbytes=0) == OK
    assert call(lib, K=0, remaining=FAKE, capacity=FAKE, nbytes=0) == OK                        # the stock is its own remainder: no copy
