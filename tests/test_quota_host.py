"""Host side of the re-ranking under category quotas (no GPU): the restatement (tests/quota_ref.py) on a hand case and against the
uncapped restatement and a plain sequential scan, the argument checks of the Python layer and of the C ABI, and the binding of the new
symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, apps
from bert4rec_amd import engine as engine_mod
from tests import diverse_ref as dref
from tests import quota_ref as qref
from tests.quota_ref import Quota

F32 = np.float32

# test_diverse_host.py's four items (exact fp32 products; with rnorm = 1 the similarity is the inner product) and a fifth:
#   sim(1, 0) = 0.75   sim(2, 0) = 0   sim(3, 0) = 0.5   sim(4, 0) = 0   sim(1, 4) = 0.125   sim(2, 4) = 0.25   sim(3, 4) = 0.25
HAND_TABLE = np.array([[1, 0, 0, 0], [0.75, 0.5, 0, 0], [0, 1, 0, 0], [0.5, 0, 0.5, 0], [0, 0.25, 0.5, 0]], F32)
HAND_RNORM = np.ones(5, F32)


def random_case(seed, V=30, E=8, R=5, M=14):
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((V, E)).astype(F32)
    rnorm = (1.0 / np.sqrt((table.astype(np.float64) ** 2).sum(1))).astype(F32)
    ids = np.stack([rng.permutation(V)[:M] for _ in range(R)]).astype(np.int64)
    sc = -np.sort(-rng.standard_normal((R, M)).astype(F32), axis=1)
    ids[1, 3] = -1                                                  # dead entries: a bad id, an id past V, a score that is not finite
    ids[2, 0] = V
    sc[3, 5] = -np.inf
    ids[3, 9:] = -1; sc[3, 9:] = -np.inf                            # the sweep's tail
    return table, rnorm, ids, sc


def test_hand_case_written_out():
    """Pool 0, 1, 2, 3, 4 with scores 4, 3, 2, 0, 1 -> rel 1, 0.75, 0.5, 0, 0.25; lambda = 0.5.  One quota, cap 1: items 0 and 2 are
    in group 0, items 1 and 3 in group 1, item 4 in none (its group id 7 lies beyond n_groups = 2).
    step 0: mmr = 0.5, 0.375, 0.25, 0, 0.125                    -> item 0 (0.5); group 0 is full: item 2 closes;
                                                                  pen = -, 0.75, x, 0.5, 0
    step 1: mmr = -, 0.375 - 0.375 = 0, x, 0 - 0.25, 0.125 - 0  -> item 4 (0.125), where plain MMR takes item 2 (0.25);
                                                                  pen 1 = max(0.75, 0.125), pen 3 = max(0.5, 0.25)
    step 2: mmr = -, 0, x, -0.25, -                             -> item 1 (0.0); group 1 is full: item 3 closes
    step 3: no open entry                                       -> -1 / -inf / -inf / -1."""
    sim = dref.sim_matrix(HAND_TABLE, HAND_RNORM)
    assert sim[0].tolist() == [1, 0.75, 0, 0.5, 0] and sim[4, 1] == 0.125 and sim[4, 3] == 0.25
    pool = np.array([[0, 1, 2, 3, 4]])
    scores = np.array([[4, 3, 2, 0, 1]], F32)
    plain = dref.rerank(HAND_TABLE, HAND_RNORM, pool, scores, 0.5, 5)
    assert plain[0].tolist()[0][:2] == [0, 2] and plain[2].tolist()[0][:2] == [0.5, 0.25]
    quota = Quota(np.array([0, 1, 0, 1, 7]), 2, 1)
    ids, sc, mmr, pos = qref.rerank(HAND_TABLE, HAND_RNORM, pool, scores, 0.5, 5, [quota])
    assert ids.tolist() == [[0, 4, 1, -1, -1]] and pos.tolist() == [[0, 4, 1, -1, -1]]
    assert sc.tolist() == [[4, 1, 3, -np.inf, -np.inf]] and mmr.tolist() == [[0.5, 0.125, 0.0, -np.inf, -np.inf]]
    # K below M is the prefix
    ids2, _, mmr2, pos2 = qref.rerank(HAND_TABLE, HAND_RNORM, pool, scores, 0.5, 2, [quota])
    assert ids2.tolist() == [[0, 4]] and mmr2.tolist() == [[0.5, 0.125]] and pos2.tolist() == [[0, 4]]
    assert pos.dtype == np.int32 and not qref.violations(ids, 5, [quota])


@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
def test_without_quotas_it_is_the_diverse_restatement(lam):
    for seed in range(4):
        table, rnorm, ids, sc = random_case(seed)
        want = dref.rerank(table, rnorm, ids, sc, lam, 14)
        got = qref.rerank(table, rnorm, ids, sc, lam, 14, [])
        assert np.array_equal(got[0], want[0])
        for g, w in zip(got[1:3], want[1:3]):
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
        live = (ids >= 0) & (ids < 30) & np.isfinite(sc)
        for r in range(ids.shape[0]):                               # pos names the picked entries
            n = int(live[r].sum())
            assert sorted(got[3][r, :n].tolist()) == np.flatnonzero(live[r]).tolist() and (got[3][r, n:] == -1).all()
            assert np.array_equal(ids[r, got[3][r, :n]], got[0][r, :n])
        # a quota whose caps never bind changes nothing either
        loose = Quota(np.arange(30) % 3, 3, 14)
        same = qref.rerank(table, rnorm, ids, sc, lam, 14, [loose])
        assert all(np.array_equal(a, b) for a, b in zip(same, got))


def test_lambda_one_is_a_sequential_scan():
    V = 30
    quotas = [Quota(np.arange(V) % 4, 4, 0, np.array([2, 1, 3, 0])), Quota(np.arange(V) // 7, 5, 2),
              Quota(np.where(np.arange(V) % 5 == 0, -3, np.arange(V) % 3 + 1), 3, 4)]       # group ids 3 = beyond n_groups, -3: none
    for seed in range(4):
        table, rnorm, ids, sc = random_case(10 + seed)
        for n in (1, 2, 3):
            for K in (3, 14):
                got = qref.rerank(table, rnorm, ids, sc, 1.0, K, quotas[:n])
                scan = qref.sequential_scan(ids, sc, V, K, quotas[:n])
                for r, picked in enumerate(scan):
                    assert got[3][r, :len(picked)].tolist() == picked and (got[3][r, len(picked):] == -1).all()
                    assert got[0][r, :len(picked)].tolist() == ids[r, picked].tolist() and (got[0][r, len(picked):] == -1).all()
                    assert np.array_equal(got[1][r, :len(picked)], sc[r, picked]) and (got[2][r, len(picked):] == -np.inf).all()
                assert not qref.violations(got[0], V, quotas[:n])
        assert any(len(p) < 14 for p in scan)                       # the caps bind


def test_special_cases():
    table, rnorm, ids, sc = random_case(3)
    V = 30
    sim = dref.sim_matrix(table, rnorm)
    # a cap of 0 bars the group from the start, but its entries still set the relevance scale: the mmr of the first pick is
    # lambda * rel of that entry, below lambda when the best entry is barred
    barred = int(ids[0, 0])
    groups = np.where(np.arange(V) == barred, 0, 1)
    got = qref.rerank(table, rnorm, ids[:1], sc[:1], 0.5, 14, [Quota(groups, 2, 0, np.array([0, 99]))], sim)
    assert barred not in got[0][0] and got[0][0, 0] == ids[0, 1] and got[3][0, 0] == 1
    rel1 = F32(F32(sc[0, 1] - sc[0, 13]) / F32(sc[0, 0] - sc[0, 13]))
    assert got[2][0, 0] == F32(F32(0.5) * rel1) and got[2][0, 0] < 0.5
    assert (got[0][0, :13] >= 0).all() and got[0][0, 13] == -1
    # uniform cap 0: nothing is picked; every group id outside [0, n_groups): nothing is capped
    none = qref.rerank(table, rnorm, ids, sc, 0.5, 14, [Quota(np.zeros(V, np.int64), 1, 0)], sim)
    assert (none[0] == -1).all() and (none[3] == -1).all() and (none[1] == -np.inf).all()
    free = qref.rerank(table, rnorm, ids, sc, 0.5, 14, [Quota(np.where(np.arange(V) % 2 == 0, 5, -1), 5, 0)], sim)
    plain = dref.rerank(table, rnorm, ids, sc, 0.5, 14, sim)
    assert np.array_equal(free[0], plain[0]) and np.array_equal(free[2].view(np.uint32), plain[2].view(np.uint32))
    # n_groups = 0: every id is outside
    assert np.array_equal(qref.rerank(table, rnorm, ids, sc, 0.5, 14, [Quota(np.zeros(V, np.int64), 0, 0)], sim)[0], plain[0])
    # a repeated id is one entry per occurrence: the second occurrence counts against the cap
    twice = np.array([[3, 3, 3, 7, 8]])
    t_sc = np.array([[5, 4, 3, 2, 1]], F32)
    by_id = Quota(np.arange(V), V, 2)
    got = qref.rerank(table, rnorm, twice, t_sc, 1.0, 5, [by_id], sim)
    assert got[0].tolist() == [[3, 3, 7, 8, -1]] and got[3].tolist() == [[0, 1, 3, 4, -1]]
    # two quotas: an entry closes as soon as either of its groups is full
    both = [Quota(np.arange(V) % 2, 2, 1), Quota(np.arange(V) % 3, 3, 1)]
    pool = np.array([[0, 2, 3, 1, 5, 7]])                           # groups (0,0) (0,2) (1,0) (1,1) (1,2) (1,1)
    got = qref.rerank(table, rnorm, pool, np.array([[6, 5, 4, 3, 2, 1]], F32), 1.0, 6, both, sim)
    assert got[0].tolist() == [[0, 1, -1, -1, -1, -1]]               # 0 fills (even, 0 mod 3); 2 is even, 3 is 0 mod 3; 1 fills odd


def test_pack_item_groups_and_check_quota_args():
    pack, check = engine_mod.pack_item_groups, engine_mod.check_quota_args
    assert apps.pack_item_groups is pack
    spec = pack([0, 1, -5, 2, 1], 2)
    assert spec.item_group.dtype == torch.int32 and spec.item_group.tolist() == [0, 1, -1, 2, 1]
    assert spec.group_cap is None and spec.n_groups == 3 and spec.cap == 2 and isinstance(spec, tuple)
    with pytest.raises((AttributeError, TypeError)):
        spec.cap = 3
    per = pack(np.array([0, 1, 1, 4]), np.array([1, 0, 7]))
    assert per.group_cap.dtype == torch.int32 and per.group_cap.tolist() == [1, 0, 7] and per.n_groups == 3
    assert pack([0, 1], 1, n_groups=1).n_groups == 1 and pack([-1, -1], 1).n_groups == 0
    assert pack(torch.tensor([0, 1]), np.int64(3)).cap == 3 and pack([0], 2 ** 40).cap == 2 ** 31 - 1
    for groups, cap, n in (([0.5, 1.0], 1, None), ([[0, 1]], 1, None), ([], 1, None), ([True, False], 1, None), ([0, 1], 1.5, None),
                           ([0, 1], True, None), ([0, 1], "2", None), ([0, 1], None, None), ([0, 1], [1.0, 2.0], None),
                           ([0, 1], [1, 2, 3], 2), ([0, 1], [[1, 2]], None), ([0, 1], 1, -1), ([0, 1], 1, 2.5), ([0, 2 ** 31], 1, None)):
        with pytest.raises(ValueError):
            pack(groups, cap, n)
    assert check(None, 5) == [] and check(spec, 5) == [spec] and check([spec, spec], 5) == [spec, spec] and check([], 5) == []
    assert check((spec, spec, spec, spec), 5) == [spec] * 4 and check(spec) == [spec]
    for bad, V in (([spec] * 5, 5), (spec, 6), ([spec, per], 5), ([(spec.item_group, None, 3, 2)], 5), ("abc", 5), (3, 5),
                   (engine_mod.ItemGroups((spec.item_group, None, 3, 2.0)), 5), (engine_mod.ItemGroups((spec.item_group, None, 3, True)), 5),
                   (engine_mod.ItemGroups((spec.item_group.to(torch.int64), None, 3, 2)), 5),
                   (engine_mod.ItemGroups((spec.item_group, torch.zeros(2, dtype=torch.int32), 3, 2)), 5)):
        with pytest.raises(ValueError):
            check(bad, V)


def test_lib_binds_the_new_symbols():
    lib = _lib.load()
    for name in ("b4r_rerank_quota", "b4r_rerank_quota_scratch_bytes"):
        assert name in _lib.PROTOTYPES, name
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert lib.b4r_rerank_quota_scratch_bytes(17, 100, 2051) >= 4 * 2051
    assert lib.b4r_rerank_quota_scratch_bytes(17, 100, 2051) == lib.b4r_rerank_diverse_scratch_bytes(17, 100, 2051)
    assert lib.b4r_rerank_quota_scratch_bytes(0, 100, 2051) == 0 and lib.b4r_rerank_quota_scratch_bytes(17, 1025, 2051) == 0
    # b4r_item_quota: two pointers and two int32, as the header declares it
    assert C.sizeof(_lib.ItemQuota) == 2 * C.sizeof(C.c_void_p) + 8 == 24
    assert [(n, C.sizeof(t)) for n, t in _lib.ItemQuota._fields_] == [("item_group", 8), ("group_cap", 8), ("n_groups", 4), ("cap", 4)]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "b4r.h")).read()
    body = re.search(r"typedef struct b4r_item_quota \{(.*?)\} b4r_item_quota;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(const int32_t\*|int32_t)\s+(\w+);", body) == [("const int32_t*", "item_group"), ("const int32_t*", "group_cap"),
                                                                       ("int32_t", "n_groups"), ("int32_t", "cap")]
    assert "enum { B4R_QUOTA_MAX = 4 };" in header and _lib.QUOTA_MAX == 4


def test_c_abi_refuses_bad_arguments_before_touching_the_device():
    lib = _lib.load()
    fake = 4096                                                     # a non-null "device" address: nothing may look at it

    def call(R=4, M=100, K=10, lam=0.5, width=64, ld=None, table=None, quotas=None, n_quotas=0):
        return lib.b4r_rerank_quota(table, width if ld is None else ld, width, 1000, None, None, None, R, M, lam, K, quotas, n_quotas,
                                    None, None, None, None, None, 0, None)

    def quota_array(*fields):
        arr = (_lib.ItemQuota * max(len(fields), 1))()
        for q, (ig, gc, n, cap) in zip(arr, fields):
            q.item_group, q.group_cap, q.n_groups, q.cap = ig, gc, n, cap
        return arr
    good = quota_array((fake, None, 3, 1), (fake, fake, 0, 0))
    for kw in (dict(M=0), dict(M=1025), dict(K=11, M=10), dict(K=-1), dict(R=-1), dict(ld=68), dict(width=6), dict(width=4100),
               dict(n_quotas=-1), dict(n_quotas=5), dict(n_quotas=-1, quotas=good), dict(n_quotas=5, quotas=good)):
        assert call(**kw) == -2 and "b4r_rerank_quota" in _lib.last_error(), kw
    assert "n_quotas" in _lib.last_error()
    for lam in (-0.1, 1.5, float("nan")):
        assert call(lam=lam) == -1 and "lambda" in _lib.last_error()
    for n in (1, 4):
        assert call(n_quotas=n) == -1 and "quotas" in _lib.last_error()               # NULL quotas
    assert call(quotas=quota_array((None, None, 3, 1)), n_quotas=1) == -1 and "item_group" in _lib.last_error()
    assert call(quotas=quota_array((fake, None, 3, 1), (None, fake, 3, 1)), n_quotas=2) == -1 and "quota 1" in _lib.last_error()
    assert call(quotas=quota_array((fake, None, -1, 1)), n_quotas=1) == -1 and "n_groups" in _lib.last_error()
    assert call(quotas=quota_array((fake, None, 3, 1), (None, None, -1, 1)), n_quotas=1, R=0) == 0   # only n_quotas entries are read
    assert call(quotas=quota_array((None, None, 3, 1)), n_quotas=1, R=0) == -1       # the quota array is checked whatever R and K are
    # nothing to do: no launch, no device pointer is looked at
    assert call(R=0) == 0 and call(K=0) == 0 and call(R=0, quotas=good, n_quotas=2) == 0 and call(K=0, quotas=good, n_quotas=2) == 0
    assert call() == -1 and "null" in _lib.last_error()
    assert call(quotas=good, n_quotas=2) == -1 and "null" in _lib.last_error()       # good quotas, then the NULL table
