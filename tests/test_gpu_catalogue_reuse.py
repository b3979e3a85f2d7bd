"""The catalogue calls of one Engine share its scratch buffers between calls: a buffer is kept, grows when a call needs more and is
then used oversized by every smaller call.  None of that may show in a result.

One Engine (V = 203, the smallest hidden size of tests/geometry_matrix.py, one layer, random parameters) runs rank_full, sample_full,
score_distribution, item_neighbours, rerank_diverse, rerank_quota and list_metrics, in that order, at R = 3 / k = 5, then at R = 40 /
k = 17 (above the 16-row group floor: every scratch grows), then at R = 3 / k = 5 again (in the oversized buffers).  Every output of
every call is compared bit for bit with the same call on a fresh Engine holding the same parameters, and the first pass with the CPU
restatements (tests/catalogue_ref.py, tests/sample_ref.py, tests/quota_ref.py), bit for bit as their own tests do."""
import types

import numpy as np
import pytest
import torch

from bert4rec_amd.engine import Engine, SPECIAL_IDS, check_rerank_args, check_temperature, item_self_information, make_model_config, \
    pack_item_groups
from tests import catalogue_ref as cref
from tests import quota_ref as qref
from tests import sample_ref as sref
from tests.geometry_matrix import CELLS
from tests.test_gpu_diverse import device_rnorm

pytestmark = pytest.mark.gpu

DEV = "cuda"
V = 203
SMALLEST = min(CELLS.values(), key=lambda c: (c.H, c.inner))
PASSES = ((3, 5), (40, 17), (3, 5))
SEED, STREAM0, TEMPERATURE, DIVERSITY = (1 << 63) + 12345, -2, 0.5, 0.3
CALLS = ("rank_full", "sample_full", "score_distribution", "item_neighbours", "rerank_diverse", "rerank_quota", "list_metrics")


def new_engine(params=None):
    eng = Engine(make_model_config(V, SMALLEST.H, 1, SMALLEST.heads, 32, SMALLEST.inner, 0.0, 0.0), DEV)
    if params is None:
        eng.init_parameters(seed=9)
        g = torch.Generator().manual_seed(10)
        eng.view("cls/predictions/output_bias/bias").copy_((torch.randn((1, V), generator=g) * 0.01).to(DEV))
    else:
        eng.params.copy_(params)
    return eng


def case(R, k):
    """The arguments of one pass: an exclude list, a ground truth and a two-filter allow with row_filter (one row without a filter)."""
    rng = np.random.default_rng(100 * R + k)
    g = torch.Generator().manual_seed(R)
    exclude = rng.integers(0, V, size=(R, 6)).astype(np.int64)
    exclude[:, 4:] = -1
    exclude[0, :] = -1
    row_filter = (np.arange(R) % 2).astype(np.int32)
    row_filter[R - 1] = -1
    counts = rng.integers(0, 50, size=V)
    return dict(R=R, k=k, hidden=torch.randn((R, SMALLEST.H), generator=g), exclude=exclude, gt=rng.integers(SPECIAL_IDS, V, size=R).astype(np.int64),
                allow=rng.random((2, V)) < 0.5, row_filter=row_filter, query=rng.integers(-1, V + 2, size=(R, k)).astype(np.int64),
                items=np.concatenate([[1], rng.integers(SPECIAL_IDS, V, size=R - 1)]).astype(np.int64),
                groups=np.arange(V) % 7, weight=item_self_information(counts))


def call(eng, name, c, pool=None):
    """One of CALLS on `eng`; the re-rankers take rank_full's (ids, scores) as their pool, list_metrics rerank_quota's ids."""
    t = {key: torch.as_tensor(c[key]) for key in ("exclude", "gt", "allow", "row_filter", "query", "items", "weight")}
    hidden, k = c["hidden"].to(DEV), c["k"]
    sweep = (hidden, None, t["exclude"], SPECIAL_IDS, t["gt"])
    if name == "rank_full":
        return eng.rank_full(*sweep, k, t["allow"], t["row_filter"])
    if name == "sample_full":
        return eng.sample_full(*sweep, k, SEED, t["allow"], t["row_filter"], TEMPERATURE, None, STREAM0)
    if name == "score_distribution":
        return eng.score_distribution(*sweep, t["allow"], t["row_filter"], TEMPERATURE, t["query"])
    if name == "item_neighbours":
        return eng.item_neighbours(t["items"], k, "cosine", SPECIAL_IDS, t["allow"], t["row_filter"])
    if name == "rerank_diverse":
        return eng.rerank_diverse(pool[0], pool[1], k, DIVERSITY)
    if name == "rerank_quota":
        return eng.rerank_quota(pool[0], pool[1], k, DIVERSITY, pack_item_groups(c["groups"], 1))
    return eng.list_metrics(pool, t["gt"], t["weight"])


def host(outputs):
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outputs]


def run_pass(eng, c, fresh):
    """The seven calls on `eng`; each also on fresh() with the same inputs.  Returns {call: (outputs, the fresh engine's outputs)}."""
    got, pool = {}, None
    for name in CALLS:
        out = call(eng, name, c, pool)
        got[name] = (host(out), host(call(fresh(), name, c, pool)))
        if name == "rank_full":
            pool = out[:2]
        elif name == "rerank_quota":
            pool = out[0]
    return got


@pytest.fixture(scope="module")
def passes():
    eng = new_engine()
    params = eng.params.clone()
    cases = [case(R, k) for R, k in PASSES]
    return eng, [(c, run_pass(eng, c, lambda: new_engine(params))) for c in cases]


def test_the_second_pass_outgrows_every_scratch_and_the_third_runs_in_it(passes):
    lib = passes[0].lib
    (R0, k0), (R1, k1) = PASSES[:2]
    assert R1 > 16 and lib.b4r_rank_full_scratch_bytes(R1, V, k1) > lib.b4r_rank_full_scratch_bytes(R0, V, k0)
    assert lib.b4r_sample_full_scratch_bytes(R1, V, k1) > lib.b4r_sample_full_scratch_bytes(R0, V, k0)
    assert lib.b4r_score_dist_scratch_bytes(R1, V) > lib.b4r_score_dist_scratch_bytes(R0, V)
    assert lib.b4r_item_neighbours_scratch_bytes(R1, V, k1, SMALLEST.H) > lib.b4r_item_neighbours_scratch_bytes(R0, V, k0, SMALLEST.H)


@pytest.mark.parametrize("n", range(len(PASSES)), ids=[f"pass{n}_R{R}_k{k}" for n, (R, k) in enumerate(PASSES)])
def test_every_output_equals_a_fresh_engines_bit_for_bit(passes, n):
    c, got = passes[1][n]
    for name in CALLS:
        ours, fresh = got[name]
        assert len(ours) == len(fresh) and len(ours) >= 2
        for i, (a, b) in enumerate(zip(ours, fresh)):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{name}: output {i}"
    assert (got["rank_full"][0][0] >= 0).any() and (got["rerank_quota"][0][0] >= 0).any()
    if n == 2:                                                      # the third pass is the first one over again
        for name in CALLS:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got[name][0], passes[1][0][1][name][0])), name


def test_the_first_pass_equals_the_restatements(passes):
    eng, (first, *_) = passes
    c, got = first
    R, k = c["R"], c["k"]
    table = eng.view("word_embeddings/embeddings").cpu().numpy()
    bias = eng.view("cls/predictions/output_bias/bias").cpu().numpy().reshape(-1)
    words = cref.pack_bits(c["allow"])
    hidden = c["hidden"].numpy()
    sc, ok = sref.scores_and_allowed(hidden, table, bias, None, SPECIAL_IDS, c["exclude"], c["gt"], words, c["row_filter"])
    assert ok[R - 1].sum() > ok[:R - 1].sum(axis=1).max()           # the row without a filter has the larger catalogue

    ids, scores, gt_rank = got["rank_full"][0]
    want = cref.expected(sc, ok, c["gt"], k, SPECIAL_IDS)
    assert np.array_equal(ids, want[0]) and scores.tobytes() == want[1].tobytes() and np.array_equal(gt_rank, want[2])

    want = sref.sample_full(sc, ok, k, check_temperature(TEMPERATURE), SEED, None, STREAM0)
    for a, b, what in zip(got["sample_full"][0], want, ("ids", "scores", "keys")):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"sample_full {what}"

    rnorm = device_rnorm(types.SimpleNamespace(engine=eng))
    want = cref.neighbours(table, c["items"], SPECIAL_IDS, 1, k, rnorm, words, c["row_filter"])
    nb_ids, nb_scores = got["item_neighbours"][0]
    assert np.array_equal(nb_ids, want[0]) and nb_scores.tobytes() == want[1].tobytes()
    assert (nb_ids[0] == -1).all() and (nb_ids[1:, 0] >= 0).all()   # [MASK] is no item

    lam = check_rerank_args(k, k, DIVERSITY)[2]
    quota = qref.Quota(c["groups"], 7, 1)
    want = qref.rerank(table, rnorm, ids, scores, lam, k, (quota,))
    for a, b, what in zip(got["rerank_quota"][0], want, ("ids", "scores", "mmr", "pos")):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"rerank_quota {what}"
    assert not qref.violations(got["rerank_quota"][0][0], V, (quota,))
    assert not np.array_equal(got["rerank_quota"][0][0], got["rerank_diverse"][0][0])     # the cap binds
