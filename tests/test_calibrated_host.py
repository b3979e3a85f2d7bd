"""Host side of the calibrated re-ranking (no GPU): the restatement (tests/calibrated_ref.py) against the objective it is greedy for and
on cases written out by hand, the argument checks of the C ABI and of the Python layers, and the history counts."""
import math
import types

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, evaluation, models
from bert4rec_amd import engine as engine_mod
from bert4rec_amd.apps.recommender import Recommender
from tests import calibrated_ref as cref

F32 = np.float32


def random_case(seed, V=60, R=4, M=30, G=5):
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.permutation(V)[:M] for _ in range(R)]).astype(np.int64)
    sc = -np.sort(-rng.standard_normal((R, M)).astype(F32), axis=1)
    ids[1, 3] = -1                                                  # dead entries: a bad id, an id past V, a score that is not finite
    ids[2, 0] = V
    sc[3, 5] = -np.inf
    labels = rng.integers(-1, G + 1, size=V)                        # -1 and G: in no group
    target = rng.integers(0, 9, size=(R, G)).astype(np.int64)
    target[0, 1] = 0                                                # a group without mass
    return ids, sc, labels, target


@pytest.mark.parametrize("lam", [0.2, 0.5, 0.9, 1.0])
@pytest.mark.parametrize("alpha", [0.01, 0.5])
def test_every_pick_is_the_argmax_of_the_objective(lam, alpha):
    """(1 - lambda) * sum rel - lambda * KL(p || q~(list + c)), with math.log in fp64 and rel the contract's fp32 value: wherever the
    best two candidates of a step differ by more than 1e-9 the restatement picks the best."""
    V, G, K = 60, 5, 12
    checked = 0
    for seed in range(6):
        ids, sc, labels, target = random_case(seed, V=V, G=G)
        got = cref.rerank(ids, sc, V, K, labels, G, target, lam, alpha)
        p, _ = cref.target_shares(target)
        for r in range(ids.shape[0]):
            live, _ = cref.relevance(ids[r], sc[r], V)
            lo, hi = F32(sc[r][live].min()), F32(sc[r][live].max())
            rel = [float(F32(F32(s - lo) / F32(hi - lo))) if ok else 0.0 for s, ok in zip(sc[r], live)]
            lab = [int(labels[i]) if ok and 0 <= labels[i] < G else -1 for i, ok in zip(np.where(live, ids[r], 0), live)]
            picked = []
            for t in range(K):
                cands = [c for c in range(ids.shape[1]) if live[c] and c not in picked]
                obj = sorted(((cref.objective(picked + [c], rel, lab, p[r], float(F32(lam)), alpha), -c) for c in cands), reverse=True)
                if obj[0][0] - obj[1][0] > 1e-9:
                    assert got[3][r, t] == -obj[0][1], f"seed {seed} row {r} step {t}"
                    checked += 1
                picked.append(int(got[3][r, t]))
    # 6 seeds x 4 rows x 12 steps.  With a relevance term few steps have a near tie; at lambda = 1 the candidates of one group tie
    # exactly, and a step counts only when the best group holds one open candidate
    assert checked > (200 if lam < 1.0 else 20)


def test_hand_case_written_out():
    """Pool 0 .. 5 with scores 5 .. 0: rel 1, 0.8, 0.6, 0.4, 0.2, 0; items 0 .. 3 are drama (group 0), 4 and 5 comedy (group 1); the target
    is 1 : 1; lambda = 0.5, alpha = 0.5.  qt = c / (2 m) + 0.25.
    step 0 (m = 1): both groups gain 0.5 ln(0.75 / 0.25), so the relevance decides                         -> item 0
    step 1 (m = 2): drama 0.5 ln(0.75 / 0.5) = 0.2027, comedy 0.5 ln(0.5 / 0.25) = 0.3466;
                    val(1) = 0.4 + 0.1014 = 0.5014, val(4) = 0.1 + 0.1733 = 0.2733                         -> item 1
    step 2 (m = 3): drama 0.5 ln((3/6 + .25) / (2/6 + .25)) = 0.1257, comedy 0.5 ln((1/6 + .25) / .25) = 0.2554;
                    val(2) = 0.3 + 0.0628 = 0.3628, val(4) = 0.1 + 0.1277 = 0.2277                         -> item 2
    at lambda = 0.9 the second pick is comedy: val(1) = 0.08 + 0.1824 = 0.2624 < val(4) = 0.02 + 0.3119 = 0.3319; at lambda = 1 the gains
    alone decide and equal gains go to the lower position: drama, comedy, drama, comedy."""
    pool = np.array([[0, 1, 2, 3, 4, 5]])
    scores = np.array([[5, 4, 3, 2, 1, 0]], F32)
    labels = np.array([0, 0, 0, 0, 1, 1])
    target = np.array([[7, 7]], np.int64)
    ids, sc, val, pos, kl = cref.rerank(pool, scores, 6, 3, labels, 2, target, 0.5, 0.5)
    assert ids.tolist() == [[0, 1, 2]] and pos.tolist() == [[0, 1, 2]] and pos.dtype == np.int32 and sc.tolist() == [[5, 4, 3]]
    g0 = 0.5 * math.log(3.0)
    assert val[0].tolist() == pytest.approx([0.5 + 0.5 * g0, 0.4 + 0.25 * math.log(1.5), 0.3 + 0.25 * math.log(0.75 / (2 / 6 + 0.25))], rel=1e-6)
    assert kl[0] == pytest.approx(0.5 * math.log(0.5 / 0.75) + 0.5 * math.log(0.5 / 0.25), rel=1e-12)       # three dramas, no comedy
    assert cref.rerank(pool, scores, 6, 2, labels, 2, target, 0.9, 0.5)[0].tolist() == [[0, 4]]
    ids1, _, _, _, kl1 = cref.rerank(pool, scores, 6, 4, labels, 2, target, 1.0, 0.5)
    assert ids1.tolist() == [[0, 4, 1, 5]]                                                                   # ties to the lower position
    assert kl1[0] == pytest.approx(0.0, abs=1e-15) and kl1[0] < kl[0]                                       # 2 : 2 is the target
    # K beyond the live entries: the tail; an unlabelled pick counts in n
    short = cref.rerank(np.array([[0, -1, 9, 4]]), np.array([[3, 2, 1, 0]], F32), 10, 4, np.array([0, 0, 0, 0, 1, 1, 0, 0, 0, 5]), 2,
                        target, 1.0, 0.5)
    assert short[0].tolist() == [[0, 4, 9, -1]] and short[3].tolist() == [[0, 3, 2, -1]] and short[1][0, 3] == -np.inf
    assert short[4][0] == pytest.approx(2 * 0.5 * math.log(0.5 / (0.5 / 3 + 0.25)), rel=1e-12)               # shares 1/3, 1/3 of n = 3


@pytest.mark.parametrize("alpha", [0.01, 0.5])
def test_lambda_zero_is_the_pool_order(alpha):
    for seed in range(3):
        ids, sc, labels, target = random_case(20 + seed)
        V, M = 60, ids.shape[1]
        got = cref.rerank(ids, sc, V, M, labels, 5, target, 0.0, alpha)
        live = (ids >= 0) & (ids < V) & np.isfinite(sc)
        for r in range(ids.shape[0]):
            order = np.flatnonzero(live[r])
            n = len(order)
            assert got[3][r, :n].tolist() == order.tolist() and (got[3][r, n:] == -1).all()
            assert got[0][r, :n].tolist() == ids[r, order].tolist() and (got[0][r, n:] == -1).all()
            assert np.array_equal(got[1][r, :n].view(np.uint32), sc[r, order].view(np.uint32)) and (got[1][r, n:] == -np.inf).all()
        # the miscalibration of the plain top K; a stronger calibration does not raise it on these rows
        k10 = cref.rerank(ids, sc, V, 10, labels, 5, target, 0.0, alpha)
        full = cref.rerank(ids, sc, V, 10, labels, 5, target, 1.0, alpha)
        assert np.isfinite(k10[4]).all() and (full[4] <= k10[4]).all() and (full[4] < k10[4]).any()


def test_targets_without_mass():
    ids, sc, labels, target = random_case(7)
    target[1] = 0
    target[2] = [-5, -1, 0, -9, -2]                                 # negative entries count as 0
    target[3, :] = [3, -4, 0, 0, 0]
    got = cref.rerank(ids, sc, 60, 8, labels, 5, target, 0.7, 0.01)
    plain = cref.rerank(ids, sc, 60, 8, labels, 5, target, 0.0, 0.01)
    assert np.isnan(got[4][1]) and np.isnan(got[4][2]) and np.isfinite(got[4][[0, 3]]).all()
    assert np.array_equal(got[3][1:3], plain[3][1:3])               # no target: the pool order
    p, T = cref.target_shares(target)
    assert T[1:] == [0, 0, 3] and p[3].tolist() == [1.0, 0, 0, 0, 0]
    assert np.isnan(cref.rerank(ids, sc, 60, 0, labels, 5, target, 0.7, 0.01)[4]).all()    # nothing picked


def test_history_counts_against_a_plain_loop():
    rng = np.random.default_rng(3)
    V, G, R, L = 50, 6, 9, 24
    labels = rng.integers(-2, G + 2, size=V)
    tokens = rng.integers(0, V, size=(R, L))
    tokens[0, :] = 0                                                # an all-[PAD] row
    tokens[1, :5] = [1, 2, 1, 0, 2]                                 # [MASK], [UNK]
    tokens[2, 3] = V + 7; tokens[2, 4] = -1                         # ids outside the vocabulary
    want = np.zeros((R, G), np.int64)
    for r in range(R):
        for t in tokens[r]:
            if engine_mod.SPECIAL_IDS <= t < V and 0 <= labels[t] < G:
                want[r, labels[t]] += 1
    for dtype in (torch.int32, torch.int64):
        got = engine_mod.group_history_counts(torch.as_tensor(tokens), torch.as_tensor(labels).to(dtype), G)
        assert got.dtype == torch.int64 and got.is_contiguous() and np.array_equal(got.numpy(), want)
    assert want[0].sum() == 0 and want.sum() > 50
    assert engine_mod.group_history_counts(torch.zeros((0, L), dtype=torch.int64), torch.as_tensor(labels), G).shape == (0, G)


def test_lib_binds_the_new_symbol():
    lib = _lib.load()
    assert "b4r_rerank_calibrated" in _lib.PROTOTYPES
    assert lib.b4r_rerank_calibrated.argtypes == _lib.PROTOTYPES["b4r_rerank_calibrated"][1]
    assert len(lib.b4r_rerank_calibrated.argtypes) == 17


def test_c_abi_refuses_bad_arguments_before_touching_the_device():
    lib = _lib.load()
    fake = 4096                                                     # a non-null "device" address: nothing may look at it

    def call(R=4, M=100, K=10, V=1000, G=20, lam=0.5, alpha=0.01, ids=fake, sc=fake, lab=fake, target=fake, out=None):
        return lib.b4r_rerank_calibrated(ids, sc, R, M, K, V, lab, G, target, lam, alpha, out, out, out, out, out, None)
    for kw in (dict(M=0), dict(M=1025), dict(K=11, M=10), dict(K=-1), dict(R=-1), dict(V=0), dict(G=0), dict(G=1025), dict(G=-3)):
        assert call(**kw) == -2 and "b4r_rerank_calibrated" in _lib.last_error(), kw
    assert "G = " in _lib.last_error()
    for lam in (-0.1, 1.5, float("nan")):
        assert call(lam=lam) == -1 and "lambda" in _lib.last_error()
    for alpha in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")):
        assert call(alpha=alpha) == -1 and "alpha" in _lib.last_error()
    for kw in (dict(ids=None), dict(sc=None), dict(lab=None), dict(target=None)):
        assert call(**kw) == -1 and "null" in _lib.last_error(), kw
        assert call(K=0, **kw) == -1                                # the checks come before an empty call returns
    # the shape comes first, then G, lambda, alpha, then the pointers
    assert call(M=0, G=0, lam=2.0, alpha=2.0, ids=None) == -2 and call(G=0, lam=2.0, alpha=2.0, ids=None) == -2
    assert call(lam=2.0, alpha=2.0, ids=None) == -1 and "lambda" in _lib.last_error()
    assert call(alpha=2.0, ids=None) == -1 and "alpha" in _lib.last_error()
    # nothing to do: no launch, no device pointer is looked at
    assert call(R=0) == 0 and call(R=0, ids=None, sc=None, lab=None, target=None) == 0
    assert call(K=0) == 0                                           # K = 0 and no out_kl
    assert call() == 0                                              # every output NULL
    for kw in (dict(R=0, G=0), dict(R=0, alpha=1.0), dict(K=0, lam=-1.0)):
        assert call(**kw) < 0                                       # an empty call is still checked


def test_check_calibration_args():
    check = engine_mod.check_calibration_args
    assert check(10, None, 0.3) == (10, 100, F32(0.3).item(), 0.01)
    assert check(10, 64, 1, 0.5, 1024) == (10, 64, 1.0, 0.5) and check(0, None, 0)[:2] == (0, 50)
    for bad in ((10, None, -0.1), (10, None, 1.5), (10, None, float("nan")), (10, None, True), (10, None, "0.5"), (10, None, None),
                (10, None, 0.5, 0.0), (10, None, 0.5, 1.0), (10, None, 0.5, float("nan")), (10, None, 0.5, False), (10, 9, 0.5),
                (10, 1025, 0.5), (1025, None, 0.5), (10, None, 0.5, 0.01, 0), (10, None, 0.5, 0.01, 1025)):
        with pytest.raises(ValueError):
            check(*bad)
    V = 12
    labels = np.arange(V) % 4
    lab, G, target = engine_mod.check_calibrate((labels, None, "history"), V)
    assert lab.dtype == torch.int32 and lab.tolist() == labels.tolist() and G == 4 and target == "history"
    mass = torch.ones((3, 4), dtype=torch.int64)
    assert engine_mod.check_calibrate((labels, 4, mass), V)[2] is mass and engine_mod.check_calibrate([labels, 2, "affinity"], V)[1] == 2
    for bad in ((labels, None), labels, (labels, None, "taste"), (labels, None, mass.to(torch.int32)), (labels, None, mass[:, :3]),
                (labels, None, mass[0]), (labels[:-1], None, "history"), (labels.astype(np.float32), None, "history"),
                (np.arange(V) * 100, None, "history"), (labels, 1025, "history"), (labels, 0, "history"), (labels, None, None)):
        with pytest.raises(ValueError):
            engine_mod.check_calibrate(bad, V)


def test_the_python_layers_refuse_before_any_work():
    """A model without an engine and an app without a dataloader: a call that got past its argument checks would fail on them with
    an AttributeError."""
    V = 40
    stub = types.SimpleNamespace(vocab_size=V)
    labels = np.arange(V) % 4
    cal = (labels, None, "history")
    batch = {"input_word_ids": torch.zeros((2, 8), dtype=torch.int64), "masked_lm_positions": torch.zeros((2, 1), dtype=torch.int64)}
    tensor = models.BERT4RecModel.recommend_tensor
    for bad in (dict(calibrate=cal, diversity=0.5), dict(calibrate=cal, max_per_group=engine_mod.pack_item_groups(labels, 2)),
                dict(calibrate=cal, sample_seed=3), dict(calibration=0.5), dict(return_calibration=True),
                dict(calibrate=cal, calibration=1.5), dict(calibrate=cal, calibration=float("nan")), dict(calibrate=cal, calibration_alpha=0.0),
                dict(calibrate=cal, calibration_alpha=1.0), dict(calibrate=cal, pool=5), dict(calibrate=cal, pool=2000),
                dict(calibrate=(labels, None, "taste")), dict(calibrate=(labels[:-1], None, "history")), dict(calibrate=labels),
                dict(calibrate=(labels, None, torch.ones((2, 3), dtype=torch.int64))), dict(calibrate=(np.arange(V) * 40, None, "history"))):
        with pytest.raises(ValueError):
            tensor(stub, batch, k=10, **bad)
    with pytest.raises(AttributeError):                             # a good call gets past the checks
        tensor(stub, batch, k=10, calibrate=cal, calibration=0.5)
    rec = Recommender(stub, None)
    for bad in (dict(calibrate_by=labels, diversity=0.5), dict(calibrate_by=labels, max_per_group=({}, 1)), dict(calibrate_by=labels, sample_seed=1),
                dict(calibration=0.5), dict(calibrate_by=labels, calibrate_to="taste"), dict(calibrate_by=labels, calibration=2.0),
                dict(calibrate_by=labels, candidate_pool=3)):
        with pytest.raises(ValueError):
            rec.recommend_batch([["a"]], 5, **bad)
    metrics = lambda: [evaluation.Counter(name="Valid Ranks"), evaluation.HR(5), evaluation.NDCG(10)]
    ok = evaluation.get(full_ranking=True, list_k=10, calibrate_by=labels, calibrate_to="affinity", calibration=0.3, metrics=metrics())
    assert ok.get_metrics_results()["Miscalibration@10"] == 0.0 and "Miscalibration@10" not in evaluation.get().get_metrics_results()
    for bad in (dict(calibrate_by=labels), dict(full_ranking=True, calibrate_by=labels), dict(full_ranking=True, list_k=10, calibration=0.5),
                dict(full_ranking=True, list_k=10, calibrate_by=labels, diversity=0.5),
                dict(full_ranking=True, list_k=10, calibrate_by=labels, max_per_group=engine_mod.pack_item_groups(labels, 2)),
                dict(full_ranking=True, list_k=10, calibrate_by=labels, sample_seed=1),
                dict(full_ranking=True, list_k=10, calibrate_by=labels, calibrate_to="taste"),
                dict(full_ranking=True, list_k=10, calibrate_by=labels, calibration=1.5),
                dict(full_ranking=True, list_k=10, calibrate_by=labels, calibration_alpha=1.0),
                dict(full_ranking=True, list_k=10, calibrate_by=(labels, 2000)),
                dict(full_ranking=True, list_k=10, calibrate_by=labels, candidate_pool=9),
                dict(full_ranking=True, list_k=10, calibrate_by=labels, metrics=[evaluation.HR(20)]),
                dict(full_ranking=True, list_k=10, calibrate_by=labels, metrics=[evaluation.MAP()])):
        with pytest.raises(ValueError):
            evaluation.get(**{"metrics": metrics(), **bad})
