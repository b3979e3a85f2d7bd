"""Host side of the diversity-aware re-ranking (no GPU): the restatement on hand cases, the argument checks of the Python layer and
of the C ABI, and the binding of the new symbols."""
import numpy as np
import pytest

from bert4rec_amd import _lib
from bert4rec_amd import engine as engine_mod
from tests import diverse_ref as dref

F32 = np.float32

# four items whose products are exact in fp32; with rnorm = 1 the similarity is the inner product:
#   sim(1, 0) = 0.75   sim(2, 0) = 0   sim(3, 0) = 0.5   sim(2, 1) = 0.5   sim(3, 1) = 0.375   sim(3, 2) = 0
HAND_TABLE = np.array([[1, 0, 0, 0], [0.75, 0.5, 0, 0], [0, 1, 0, 0], [0.5, 0, 0.5, 0]], F32)
HAND_RNORM = np.ones(4, F32)


def test_hand_case_written_out():
    """scores 4, 3, 2, 0 -> rel 1, 0.75, 0.5, 0; lambda = 0.5:
    step 0: mmr = 0.5, 0.375, 0.25, 0                          -> item 0 (0.5);   pen = -, 0.75, 0, 0.5
    step 1: mmr = -, 0.375 - 0.375 = 0, 0.25 - 0, 0 - 0.25      -> item 2 (0.25);  pen = -, max(0.75, 0.5), -, max(0.5, 0)
    step 2: mmr = -, 0, -, -0.25                               -> item 1 (0.0);   pen 3 = max(0.5, 0.375)
    step 3: item 3 (-0.25)."""
    sim = dref.sim_matrix(HAND_TABLE, HAND_RNORM)
    assert np.array_equal(sim, np.array([[1, 0.75, 0, 0.5], [0.75, 0.8125, 0.5, 0.375], [0, 0.5, 1, 0], [0.5, 0.375, 0, 0.5]], F32))
    pool = np.array([[0, 1, 2, 3]])
    scores = np.array([[4, 3, 2, 0]], F32)
    ids, sc, mmr = dref.rerank(HAND_TABLE, HAND_RNORM, pool, scores, 0.5, 4)
    assert ids.tolist() == [[0, 2, 1, 3]] and sc.tolist() == [[4, 2, 3, 0]] and mmr.tolist() == [[0.5, 0.25, 0.0, -0.25]]
    # K below M is the prefix
    ids2, _, mmr2 = dref.rerank(HAND_TABLE, HAND_RNORM, pool, scores, 0.5, 2)
    assert ids2.tolist() == [[0, 2]] and mmr2.tolist() == [[0.5, 0.25]]


def test_lambda_one_returns_the_first_live_entries():
    rng = np.random.default_rng(0)
    V, E, R, M = 30, 8, 4, 12
    table = rng.standard_normal((V, E)).astype(F32)
    rnorm = (1.0 / np.sqrt((table.astype(np.float64) ** 2).sum(1))).astype(F32)
    ids = np.stack([rng.permutation(V)[:M] for _ in range(R)]).astype(np.int64)
    sc = -np.sort(-rng.standard_normal((R, M)).astype(F32), axis=1)
    ids[1, 3] = -1                                                  # dead entries: a bad id, an id past V, a score that is not finite
    ids[2, 0] = V
    sc[3, 5] = -np.inf
    ids[3, 8:] = -1; sc[3, 8:] = -np.inf                            # the sweep's tail
    got = dref.rerank(table, rnorm, ids, sc, 1.0, 8)
    for r in range(R):
        live = [p for p in range(M) if 0 <= ids[r, p] < V and np.isfinite(sc[r, p])][:8]
        assert got[0][r, :len(live)].tolist() == ids[r, live].tolist() and (got[0][r, len(live):] == -1).all()
        assert np.array_equal(got[1][r, :len(live)], sc[r, live]) and (got[1][r, len(live):] == -np.inf).all()
    assert (got[0][3, 7:] == -1).all() and (got[2][3, 7:] == -np.inf).all()   # row 3 has 7 live entries


def test_lambda_zero_picks_the_least_similar_second():
    rng = np.random.default_rng(1)
    V, E, M = 25, 8, 25
    table = rng.standard_normal((V, E)).astype(F32)
    rnorm = (1.0 / np.sqrt((table.astype(np.float64) ** 2).sum(1))).astype(F32)
    sim = dref.sim_matrix(table, rnorm)
    ids = rng.permutation(V)[None, :M].astype(np.int64)
    sc = -np.sort(-rng.standard_normal((1, M)).astype(F32), axis=1)
    got_ids, _, got_mmr = dref.rerank(table, rnorm, ids, sc, 0.0, 2, sim)
    first = int(ids[0, 0])                                          # every mmr is 0 at step 0: the lowest position
    assert got_ids[0, 0] == first and got_mmr[0, 0] == 0.0
    others = ids[0, 1:]
    assert got_ids[0, 1] == others[np.argmin(sim[first, others])]
    assert got_mmr[0, 1] == -sim[first, got_ids[0, 1]]
    # equal scores: rel = 1 for all, so lambda = 1 keeps the order and every mmr is 1
    same = dref.rerank(table, rnorm, ids, np.full((1, M), 2.5, F32), 1.0, 5, sim)
    assert same[0].tolist() == ids[:, :5].tolist() and (same[2] == 1.0).all()
    # a repeated id is two entries; the second is penalised by the first (sim(c, c) is about 1)
    twice = np.array([[3, 3, 7]])
    got = dref.rerank(table, rnorm, twice, np.array([[3, 2, 1]], F32), 0.5, 3, sim)
    assert sorted(got[0][0].tolist()) == [3, 3, 7] and got[0][0, 0] == 3


def test_check_rerank_args():
    check = engine_mod.check_rerank_args
    assert check(10, None, 0.25) == (10, 100, 0.75) and check(1, None, 0)[1] == 50 and check(0, None, 1.0) == (0, 50, 0.0)
    assert check(500, None, 0.5)[1] == 1024 and check(10, 10, 0.5)[:2] == (10, 10) and check(0, 1, 0.5)[:2] == (0, 1)
    assert check(3, 7, np.float32(0.7))[2] == float(np.float32(1.0 - float(np.float32(0.7))))
    for k, pool, diversity in ((-1, None, 0.5), (1025, None, 0.5), (2.5, None, 0.5), (10, 9, 0.5), (10, 1025, 0.5), (0, 0, 0.5),
                               (10, 20.0, 0.5), (10, None, -0.1), (10, None, 1.5), (10, None, float("nan")), (10, None, None),
                               (10, None, "0.5"), (10, None, True)):
        with pytest.raises(ValueError):
            check(k, pool, diversity)


def test_lib_binds_the_new_symbols():
    lib = _lib.load()
    for name in ("b4r_rerank_diverse", "b4r_rerank_diverse_scratch_bytes"):
        assert name in _lib.PROTOTYPES, name
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert lib.b4r_rerank_diverse_scratch_bytes(17, 100, 2051) >= 4 * 2051
    assert lib.b4r_rerank_diverse_scratch_bytes(0, 100, 2051) == 0 and lib.b4r_rerank_diverse_scratch_bytes(17, 1025, 2051) == 0


def test_c_abi_refuses_bad_arguments_before_touching_the_device():
    lib = _lib.load()

    def call(R=4, M=100, K=10, lam=0.5, width=64, ld=None, table=None):
        return lib.b4r_rerank_diverse(table, width if ld is None else ld, width, 1000, None, None, None, R, M, lam, K, None, None, None,
                                      None, 0, None)
    for kw in (dict(M=0), dict(M=1025), dict(K=11, M=10), dict(K=-1), dict(R=-1), dict(ld=68), dict(width=6), dict(width=4100)):
        assert call(**kw) == -2 and "b4r_rerank_diverse" in _lib.last_error(), kw
    for lam in (-0.1, 1.5, float("nan")):
        assert call(lam=lam) == -1 and "lambda" in _lib.last_error()
    assert call(R=0) == 0 and call(K=0) == 0                        # nothing to do: no launch, no pointer is looked at
    assert call() == -1 and "null" in _lib.last_error()
