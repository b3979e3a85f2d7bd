"""Sampled recommendations without a GPU: the noise's host probes against the numpy restatement (tests/sample_ref.py) over every
hash word, its distance from libm, the law of the restated sampler (chi-square of the first and second draws against the exact
Plackett-Luce probabilities), the scratch-size functions and the Python layers' argument checks."""
import numpy as np
import pytest

from bert4rec_amd import _lib, engine as engine_mod, evaluation, models
from bert4rec_amd.apps import Recommender
from tests import sample_ref as sr

F32 = np.float32
SEEDS = (0, 1, 0x0123456789ABCDEF)


@pytest.fixture(scope="module")
def all_words():
    """one word per distinct uniform: k << 9 for k < 2^23 (the low 9 bits do not count), and the restated noise of each"""
    words = (np.arange(1 << 23, dtype=np.uint64) << np.uint64(9)).astype(np.uint32)
    return words, sr.gumbel_from_word(words)


def test_gumbel_from_hash_equals_the_restatement_on_every_word(all_words):
    words, want = all_words
    f = _lib.load().b4r_gumbel_from_hash
    got = np.fromiter((f(w) for w in words.tolist()), dtype=F32, count=len(words))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert f(0x1FF) == f(0) and f(0xFFFFFFFF) == f(0xFFFFFE00)            # the low 9 bits do not count
    assert float(want.min()) == float(F32(sr.G_MIN)) and float(want.max()) == float(F32(sr.G_MAX))
    assert len(np.unique(want)) == 1 << 23                                # no two uniforms share a noise value


def test_noise_is_within_1e_12_of_libm(all_words):
    words, want = all_words
    u = sr.uniform(words)
    mine = 0.0 - sr.xln(0.0 - sr.xln(u))
    libm = -np.log(-np.log(u))
    worst = float(np.abs(mine - libm).max())
    differ = int((libm.astype(F32) != want).sum())
    print(f"largest |g - libm| = {worst:.3g}; fp32 values that differ from the rounded libm value: {differ} of {len(words)}")
    assert worst <= 1e-12
    assert differ <= 16                                                   # (ties of the rounding to fp32 only)


def test_sample_word_equals_the_restatement():
    f = _lib.load().b4r_sample_word
    rng = np.random.default_rng(5)
    seeds = [0, 1, 0x0123456789ABCDEF, (1 << 64) - 1, 5 << 32, (1 << 63) + 12345]
    streams = [0, 1, -1, -(1 << 63), (1 << 63) - 1, (7 << 32) + 1, -(3 << 32) - 9, 1 << 32]
    ids = [0, 1, 3, 1023, 1024, 335422, (1 << 31) - 1] + rng.integers(0, 1 << 31, 20).tolist()
    for seed in seeds:
        for stream in streams:
            want = sr.sample_word(seed, stream, ids)
            assert [f(seed, stream, i) for i in ids] == want.tolist()
            grid = sr.sample_word(seed, np.asarray([stream, stream + 1 if stream < (1 << 63) - 1 else 0], np.int64)[:, None],
                                  np.asarray(ids)[None, :])
            assert np.array_equal(grid[0], want)                          # the broadcast form the law test uses
    # the high words count: a seed or a stream that differs there gives other words
    assert f(1 << 32, 0, 5) != f(0, 0, 5) and f(0, 1 << 32, 5) != f(0, 0, 5) and f(0, -1, 5) != f(0, (1 << 32) - 1, 5)


# (items, streams, seed of the fixed N(0, 1.5^2) scores)
LAW = [(12, 40000, 11), (40, 100000, 40)]


@pytest.mark.parametrize("n,streams,score_seed", LAW, ids=[f"{n}x{s}" for n, s, _ in LAW])
def test_law_of_the_first_two_draws(n, streams, score_seed):
    """Chi-square of the first-draw and second-draw counts over streams 0 .. S-1 against the exact Plackett-Luce probabilities of
    softmax(t), t = fl32(score / T), at T = 1 and T = 2: p >= 0.01 in every configuration (fixed inputs: the p-values are
    recorded in DESIGN.md 6.6)."""
    scores = (np.random.default_rng(score_seed).standard_normal(n) * 1.5).astype(F32)
    for seed in SEEDS:
        g = sr.gumbel(seed, np.arange(streams, dtype=np.int64)[:, None], np.arange(n)[None, :])
        for inv_t in (1.0, 0.5):
            t = (scores * F32(inv_t)).astype(F32)
            key = (t[None, :] + g).astype(F32)
            order = np.argsort(-key.astype(np.float64), axis=1, kind="stable")
            p1, p2 = sr.plackett_luce_first_two(t.astype(np.float64))
            assert abs(p1.sum() - 1.0) < 1e-12 and abs(p2.sum() - 1.0) < 1e-12
            q1 = sr.chi_square_p(np.bincount(order[:, 0], minlength=n), p1)
            q2 = sr.chi_square_p(np.bincount(order[:, 1], minlength=n), p2)
            print(f"items {n} streams {streams} seed {seed:#x} T {1.0 / inv_t:g}: p(first) = {q1:.4f}, p(second) = {q2:.4f}")
            assert q1 >= 0.01 and q2 >= 0.01, (seed, inv_t, q1, q2)


def test_chi_square_p_value():
    """the p-value helper against closed forms: df = 2 gives exp(-x / 2); df = 1 gives erfc(sqrt(x / 2))"""
    import math
    for x in (0.1, 1.0, 5.0, 20.0):
        assert sr.gammaincc(1.0, x / 2) == pytest.approx(math.exp(-x / 2), rel=1e-12)
        assert sr.gammaincc(0.5, x / 2) == pytest.approx(math.erfc(math.sqrt(x / 2)), rel=1e-10)


def test_restated_sampler_orders_and_pads():
    scores = np.asarray([[1.0, 1.0, -2.0, 5.0, 0.5]], F32)
    ok = np.asarray([[True, True, False, True, True]])
    ids, sc, keys = sr.sample_full(scores, ok, 6, 1.0, 7, stream0=3)
    k = sr.keys_of(scores, 1.0, 7, [3])[0]
    live = [j for j in np.argsort(-k.astype(np.float64), kind="stable") if ok[0, j]]
    assert ids[0].tolist() == live + [-1, -1] and np.isneginf(sc[0, 4:]).all() and np.isneginf(keys[0, 4:]).all()
    assert (np.diff(keys[0, :4]) <= 0).all() and sc[0, :4].tolist() == scores[0, live].tolist()
    # a pool with every allowed item, in any order, dead entries and a duplicate aside: the same draw
    pool_ids = np.asarray([[4, 9, 3, 1, -1, 0, 3]], np.int64)
    pool_sc = np.asarray([[0.5, 1.0, 5.0, 1.0, 2.0, 1.0, np.nan]], F32)
    pids, psc, pk, pos = sr.sample_pool(pool_ids, pool_sc, 5, 4, 1.0, 7, stream0=3)
    assert pids.tolist() == ids[:, :4].tolist() and pk.tobytes() == keys[:, :4].tobytes() and psc.tobytes() == sc[:, :4].tobytes()
    assert all(pool_ids[0, p] == i for p, i in zip(pos[0], pids[0]))


def test_scratch_bytes():
    lib = _lib.load()
    f = lib.b4r_sample_full_scratch_bytes
    assert f(0, 1000, 10) == 0 and f(-1, 1000, 10) == 0 and f(4, 0, 10) == 0 and f(4, 1000, 1025) == 0 and f(4, 1000, -1) == 0
    for V in (4, 1024, 1025, 335423):
        last = 0
        for R in (1, 2, 16, 17, 256):
            assert f(R, V, 10) > last
            last = f(R, V, 10)
        assert f(16, V, 1) <= f(16, V, 10) <= f(16, V, 1024)
    assert f(16, 1024, 10) < f(16, 1025, 10)
    # (key, id) per kept candidate and one count per chunk: nothing the size of [R, V]
    assert f(256, 335423, 10) < 256 * 335423 * 4 // 10


def test_python_layers_refuse_bad_arguments_before_any_work():
    check = engine_mod.check_sample_seed
    assert check(0) == 0 and check((1 << 64) - 1) == (1 << 64) - 1 and check(np.int64(5)) == 5
    for bad in (-1, 1 << 64, 1.0, "3", None, True):
        with pytest.raises(ValueError, match="sample_seed"):
            check(bad)
    assert engine_mod.check_sample_streams(None) is None
    assert engine_mod.check_sample_streams([1, -2, 1 << 40], 3).tolist() == [1, -2, 1 << 40]
    for bad in ([1.0, 2.0], [[1, 2]], [True, False]):
        with pytest.raises(ValueError, match="streams"):
            engine_mod.check_sample_streams(bad)
    with pytest.raises(ValueError, match="streams"):
        engine_mod.check_sample_streams([1, 2], 3)
    assert engine_mod.check_stream0((1 << 63) + 1) == -(1 << 63) + 1 and engine_mod.check_stream0(-4) == -4
    assert engine_mod.check_sample_pool_args(10, 100) == (10, 100)
    for k, pool in ((11, 10), (1, 0), (1, 1025), (1, 2.5)):
        with pytest.raises(ValueError):
            engine_mod.check_sample_pool_args(k, pool)

    model = object.__new__(models.BERT4RecModel)            # the checks come before anything of the model is touched
    rt = models.BERT4RecModel.recommend_tensor
    for bad in (-1, 1 << 64, 1.5, "7", True):
        with pytest.raises(ValueError, match="sample_seed"):
            rt(model, {}, k=5, sample_seed=bad)
    with pytest.raises(ValueError, match="diversity"):
        rt(model, {}, k=5, sample_seed=1, diversity=0.5)
    with pytest.raises(ValueError, match="max_per_group"):
        rt(model, {}, k=5, sample_seed=1, max_per_group=object())
    with pytest.raises(ValueError, match="sample_seed"):
        rt(model, {}, k=5, sample_streams=[1, 2])
    with pytest.raises(ValueError, match="pool"):
        rt(model, {}, k=5, sample_seed=1, pool=4)
    for t in (0.0, float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            rt(model, {}, k=5, sample_seed=1, temperature=t)
    with pytest.raises(ValueError, match="return_distribution"):   # as before: a temperature alone scales nothing
        rt(model, {}, k=5, temperature=2.0)
    with pytest.raises(ValueError, match="pool"):                  # as before: a pool alone re-ranks nothing
        rt(model, {}, k=5, pool=50)

    rec = Recommender(None, None)
    with pytest.raises(ValueError, match="sample_seed"):
        rec.recommend_batch([[1, 2]], k=3, sample_seed=-1)
    with pytest.raises(ValueError, match="sample_seed"):
        rec.recommend_batch([[1, 2]], k=3, user_streams=[4])
    with pytest.raises(ValueError, match="diversity"):
        rec.recommend_batch([[1, 2]], k=3, sample_seed=1, diversity=0.2)
    with pytest.raises(ValueError, match="temperature"):
        rec.recommend_batch([[1, 2]], k=3, temperature=2.0)

    with pytest.raises(ValueError, match="list_k"):
        evaluation.get(full_ranking=True, sample_seed=1)
    with pytest.raises(ValueError, match="sample_seed"):
        evaluation.get(full_ranking=True, list_k=5, temperature=2.0)
    with pytest.raises(ValueError, match="diversity"):
        evaluation.get(full_ranking=True, list_k=5, sample_seed=1, diversity=0.3, metrics=[evaluation.HR(5)])
    with pytest.raises(ValueError, match="sample_seed"):
        evaluation.get(full_ranking=True, list_k=5, sample_seed=-3, metrics=[evaluation.HR(5)])
    with pytest.raises(ValueError, match="cut-off"):
        evaluation.get(full_ranking=True, list_k=5, sample_seed=1, metrics=[evaluation.HR(10)])
    with pytest.raises(ValueError):
        evaluation.get(full_ranking=True, list_k=5, sample_seed=1, candidate_pool=4, metrics=[evaluation.HR(5)])
    ev = evaluation.get(full_ranking=True, list_k=5, sample_seed=1, temperature=2.0, candidate_pool=50, item_counts=np.ones(10),
                        metrics=[evaluation.HR(5), evaluation.NDCG(5)])
    assert ev.sample_seed == 1 and ev.list_k == 5 and ev._sample_pool == 50
    plain = evaluation.get(full_ranking=True, list_k=5)
    assert plain.sample_seed is None and plain._list_pool == 5
