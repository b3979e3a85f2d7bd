"""Host side of the beyond-accuracy list metrics (no GPU): the binding of the new symbols, the argument checks of the C ABI, the CPU
restatement against float64 numpy, the evaluator's construction rules, and the host formulas (self-information, coverage, Gini)."""
import numpy as np
import pytest

from bert4rec_amd import _lib, evaluation
from bert4rec_amd.apps import item_self_information
from bert4rec_amd.evaluation import bert4rec_evaluator as ev_mod
from tests import list_metrics_ref as lref

F32 = np.float32
NAMES = ("b4r_list_metrics", "b4r_list_metrics_scratch_bytes")


def test_lib_binds_the_new_symbols():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.PROTOTYPES, name
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert lib.b4r_list_metrics_scratch_bytes(17, 10, 2051) >= 4 * 2051
    for R, K in ((0, 10), (17, 0), (17, 1025)):
        assert lib.b4r_list_metrics_scratch_bytes(R, K, 2051) == 0, (R, K)


def test_c_abi_refuses_bad_arguments_before_touching_the_device():
    lib = _lib.load()

    def call(R=4, K=10, width=64, ld=None, table=None):
        return lib.b4r_list_metrics(table, width if ld is None else ld, width, 1000, 3, None, None, R, K, None, None, None, None, None,
                                    None, None, None, None, None, 0, None)
    for kw in (dict(K=0), dict(K=1025), dict(width=6), dict(width=4100), dict(ld=68), dict(R=-1)):
        assert call(**kw) == -2 and "b4r_list_metrics" in _lib.last_error(), kw          # B4R_E_SHAPE
    assert call() == -1 and "b4r_list_metrics" in _lib.last_error() and "null" in _lib.last_error()   # B4R_E_BADARG: a NULL table
    assert call(R=0) == 0                                           # nothing to do: no launch, no pointer is looked at


def float64_ild(table, ids):
    """The mean over the list's pairs of 1 - cos, in float64."""
    e = table[ids].astype(np.float64)
    e = e / np.linalg.norm(e, axis=1, keepdims=True)
    cos = e @ e.T
    k = len(ids)
    return float((1.0 - cos)[np.triu_indices(k, 1)].mean())


@pytest.mark.parametrize("width", [4, 64, 132, 256])
def test_restatement_against_float64(width):
    rng = np.random.default_rng(width)
    V, R, K = 60, 6, 12
    table = rng.standard_normal((V, width)).astype(F32)
    rnorm = (1.0 / np.sqrt((table.astype(np.float64) ** 2).sum(1))).astype(F32)
    ids = np.stack([rng.permutation(V)[:K] for _ in range(R)]).astype(np.int64)
    ids[1, 5:] = -1                                                 # a short list, and one with dead entries in it
    ids[2, [0, 4]] = [V, 2 ** 40]
    got = lref.list_metrics(table, rnorm, ids)
    for r in range(R):
        live = [int(j) for j in ids[r] if 0 <= j < V]
        assert got["n"][r] == len(live)
        pairs = len(live) * (len(live) - 1) // 2
        assert abs(got["dist"][r] / 2 ** 30 / pairs - float64_ild(table, live)) < 1e-5, r
    assert got["exposure"].sum() == got["n"].sum() and got["counts"] == [R, R]
    # lists of one item repeated: every distance is 1 - sim(c, c), zero up to the rounding of the chain
    same = np.tile(np.arange(3, 9)[:, None], (1, 5)).astype(np.int64)
    got = lref.list_metrics(table, rnorm, same)
    assert (np.abs(got["dist"] / 2 ** 30 / 10) < 1e-6).all()
    assert got["exposure"][3:9].tolist() == [5] * 6


def test_restatement_hand_case():
    """The four items of the re-ranking's hand case (products exact in fp32, rnorm = 1): sim(q, c) = the inner product.
    list 0, 1, 2, 3: distances 1 - {0.75, 0, 0.5, 0.5, 0.375, 0} = 0.25 + 1 + 0.5 + 0.5 + 0.625 + 1 = 3.875."""
    table = np.array([[1, 0, 0, 0], [0.75, 0.5, 0, 0], [0, 1, 0, 0], [0.5, 0, 0.5, 0]], F32)
    weight = np.array([1.5, 0.25, 2.0, 3.0], F32)
    ids = np.array([[0, 1, 2, 3], [2, -1, 0, 9], [7, -1, -1, -1], [-1, 3, -1, -1]], np.int64)
    got = lref.list_metrics(table, np.ones(4, F32), ids, gt=np.array([2, 0, 1, 3]), item_weight=weight, first_item=1)
    assert got["n"].tolist() == [4, 2, 0, 1]
    assert got["dist"].tolist() == [int(3.875 * 2 ** 30), 2 ** 30, 0, 0]
    assert got["nov"].tolist() == [int(6.75 * 2 ** 30), int(3.5 * 2 ** 30), 0, 3 * 2 ** 30]
    assert got["hit_pos"].tolist() == [3, 0, 0, 2]                   # row 1: gt 0 lies below first_item; row 2: absent
    assert got["exposure"].tolist() == [2, 1, 2, 2]
    assert got["counts"] == [2, 3] and got["sums"] == [3.875 / 6 + 1.0, 6.75 / 4 + 3.5 / 2 + 3.0]


def test_evaluator_construction():
    assert [m.name for m in evaluation.default_metrics()] == ["Valid Ranks", "NDCG@1", "NDCG@5", "NDCG@10", "HR@1", "HR@5", "HR@10", "MAP"]
    plain = evaluation.get(full_ranking=True)
    assert plain.list_k is None
    assert list(plain.get_metrics_results()) == [m.name for m in evaluation.default_metrics()]
    with pytest.raises(ValueError, match="full_ranking"):
        evaluation.get(list_k=10)
    with pytest.raises(ValueError, match="MAP"):
        evaluation.get(full_ranking=True, list_k=10, diversity=0.2)
    with pytest.raises(ValueError, match="NDCG@20"):
        evaluation.get(full_ranking=True, list_k=10, diversity=0.2, metrics=[evaluation.HR(10), evaluation.NDCG(20)])
    for bad in (dict(diversity=0.2), dict(candidate_pool=50), dict(item_counts=[1, 2]), dict(full_ranking=True, list_k=0),
                dict(full_ranking=True, list_k=1025), dict(full_ranking=True, list_k=10, candidate_pool=50),
                dict(full_ranking=True, list_k=10, diversity=1.5, metrics=[evaluation.HR(10)]),
                dict(full_ranking=True, list_k=10, diversity=0.5, candidate_pool=9, metrics=[evaluation.HR(10)])):
        with pytest.raises(ValueError):
            evaluation.get(**bad)
    ev = evaluation.get(full_ranking=True, list_k=10)                # the default metrics are fine without re-ranking
    assert list(ev.get_metrics_results()) == [m.name for m in evaluation.default_metrics()] + ["ILD@10", "Coverage@10", "Gini@10"]
    metrics = [evaluation.Counter(name="Valid Ranks"), evaluation.HR(1), evaluation.HR(10), evaluation.NDCG(10)]
    ev = evaluation.get(full_ranking=True, list_k=10, diversity=0.2, item_counts=np.ones(50), metrics=metrics)
    assert list(ev.get_metrics_results()) == ["Valid Ranks", "HR@1", "HR@10", "NDCG@10", "ILD@10", "Novelty@10", "Coverage@10", "Gini@10"]
    assert all(v == 0 for v in ev.get_metrics_results().values())
    ev.reset_metrics()


def test_item_self_information():
    got = item_self_information([0, 1, 2, 5, 8])                     # 16 interactions; a count of 0 counts as 1
    assert got.dtype == np.float32
    assert got.tolist() == [4.0, 4.0, 3.0, float(F32(-np.log2(5 / 16))), 1.0]
    assert item_self_information(np.zeros(3)).tolist() == [0.0, 0.0, 0.0]


def test_coverage_and_gini():
    n = 8
    assert ev_mod.exposure_gini(np.full(n, 5)) == 0.0 and ev_mod.exposure_coverage(np.full(n, 5)) == 1.0
    one = np.zeros(n, np.int64); one[3] = 40
    assert ev_mod.exposure_gini(one) == pytest.approx((n - 1) / n, abs=1e-15) and ev_mod.exposure_coverage(one) == 1 / n
    assert ev_mod.exposure_gini(np.zeros(n)) == 0.0 and ev_mod.exposure_coverage(np.zeros(n)) == 0.0
    c = np.array([3, 0, 1, 0, 6])                                   # ascending 0 0 1 3 6: (-4*0 - 2*0 + 0*1 + 2*3 + 4*6) / (5 * 10) = 0.6
    assert ev_mod.exposure_gini(c) == pytest.approx(0.6, abs=1e-15) and ev_mod.exposure_coverage(c) == 0.6
    full = np.concatenate([[9, 9, 9], c])                           # the restatement skips the three specials
    assert lref.gini(full) == pytest.approx(0.6, abs=1e-15) and lref.coverage(full) == 0.6
