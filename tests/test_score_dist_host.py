"""Catalogue softmax (b4r_score_dist) without a GPU: the CPU restatement (tests/score_dist_ref.py) against closed forms, its blocked
arithmetic against plain fp64, the library's argument checks (they return before any launch) and the Python layers' own."""
import numpy as np
import pytest

from bert4rec_amd import _lib, evaluation, models
from bert4rec_amd import engine as engine_mod
from bert4rec_amd.apps import Recommender
from tests import catalogue_ref as ref
from tests import score_dist_ref as sref

F32 = np.float32


def test_equal_scores_give_the_uniform_distribution():
    for n, v in ((1, 0.0), (7, -3.25), (1024, 11.5), (1025, 0.0), (5000, 2000.0)):
        t = np.full((1, n + 3), v, F32)
        ok = np.ones((1, n + 3), bool)
        ok[0, :3] = False
        cnt, mx, lse, ent = sref.blocked(t, ok)
        assert cnt[0] == n and mx[0] == F32(v)
        assert lse[0] == pytest.approx(v + np.log(n), rel=1e-15, abs=1e-15)
        assert ent[0] == pytest.approx(np.log(n), rel=1e-15, abs=1e-15)
        _, lse_p, ent_p = sref.plain(t, ok)
        assert lse_p[0] == pytest.approx(lse[0], rel=1e-15, abs=1e-15) and ent_p[0] == pytest.approx(ent[0], rel=1e-15, abs=1e-15)


def test_one_allowed_item_and_the_empty_row():
    rng = np.random.default_rng(0)
    t = rng.standard_normal((2, 2049)).astype(F32) * 30
    ok = np.zeros((2, 2049), bool)
    ok[0, 1030] = True
    cnt, mx, lse, ent = sref.blocked(t, ok)
    assert cnt.tolist() == [1, 0]
    assert lse[0] == float(t[0, 1030]) and mx[0] == t[0, 1030] and ent[0] == 0.0
    assert mx[1] == -np.inf and lse[1] == -np.inf and ent[1] == 0.0
    lp = sref.query_logp(t, ok, lse, np.array([[1030, 5, -1, 2049, 1 << 40], [1030, 5, -1, 2049, -(1 << 40)]]))
    assert lp[0, 0] == 0.0 and np.isneginf(lp[0, 1:]).all() and np.isneginf(lp[1]).all()
    assert not np.isnan(lse).any() and not np.isnan(ent).any() and not np.isnan(lp).any()
    _, lse_p, ent_p = sref.plain(t, ok)
    assert lse_p[0] == lse[0] and ent_p.tolist() == [0.0, 0.0] and lse_p[1] == -np.inf


@pytest.mark.parametrize("V,H", [(3000, 64), (2049, 128)])
def test_blocked_arithmetic_against_fp64(V, H):
    rng = np.random.default_rng(V + H)
    table = (rng.standard_normal((V, H)) * 0.05).astype(F32)
    bias = (rng.standard_normal(V) * 0.01).astype(F32)
    base = rng.standard_normal((1, H)).astype(F32)
    hidden = np.concatenate([base * s for s in (1, 20, 200, 2000)]).astype(F32)
    ex = rng.integers(0, V, size=(4, 20)).astype(np.int64)
    ok = ref.allowed_mask(V, 3, ex, None, 4)
    for inv_t in (1.0, 0.25, 4.0):
        t = sref.scaled_scores(hidden, table, bias, None, inv_t)
        cnt, mx, lse, ent = sref.blocked(t, ok)
        cnt_p, lse_p, ent_p = sref.plain(t, ok)
        assert np.array_equal(cnt, cnt_p) and np.array_equal(mx, np.where(ok, t, -np.inf).max(axis=1).astype(F32))
        # numpy's fp32 exp is good to an ulp (2^-23 relative): the device's tolerances with 2^-23 in place of their 2^-21
        ln = np.log(cnt)
        assert (np.abs(lse - lse_p) <= 2.0 ** -23 + 2.0 ** -24 * ln).all(), np.abs(lse - lse_p).max()
        assert (np.abs(ent - ent_p) <= 2.0 ** -23 * (1 + 2 * ln) + 2.0 ** -24 * (ln + ln * ln)).all(), np.abs(ent - ent_p).max()
        assert (np.abs(lse - lse_p) <= sref.tol_lse(cnt)).all() and (np.abs(ent - ent_p) <= sref.tol_entropy(cnt)).all()
        assert (ent >= -1e-12).all() and (ent <= np.log(cnt) + 1e-9).all()
        # every allowed id queried: the probabilities sum to one
        lp = sref.query_logp(t, ok, lse, np.tile(np.arange(V), (4, 1)))
        total = np.exp(lp.astype(np.float64)).sum(axis=1)
        bound = sref.tol_lse(cnt) + 2.0 ** -24 * np.abs(np.where(ok, lp, 0.0)).max(axis=1)
        assert (np.abs(total - 1.0) <= bound).all()
        assert np.isneginf(lp[~ok]).all() and np.isfinite(lp[ok]).all()


def test_a_perturbed_exponential_stays_inside_the_tolerances():
    """The tolerances admit an fp32 exponential that is off by up to 3 ulp: 2 ulp of alternating sign stay inside them."""
    V, H = 3000, 64
    rng = np.random.default_rng(5)
    table = (rng.standard_normal((V, H)) * 0.05).astype(F32)
    hidden = np.concatenate([rng.standard_normal((1, H)).astype(F32) * s for s in (1, 20, 200)]).astype(F32)
    t = sref.scaled_scores(hidden, table)
    ok = np.ones((3, V), bool)
    _, lse_p, ent_p = sref.plain(t, ok)
    for r in range(3):
        S = W = 0.0
        m = float(t[r].max())
        for c0 in range(0, V, 1024):
            tc = t[r, c0:c0 + 1024]
            mc = F32(tc.max())
            x = (tc - mc).astype(F32)
            e = np.exp(x).astype(F32)
            sign = np.where(np.arange(e.size) % 2 == 0, 2, -2).astype(np.int32)
            e = np.where(e > 1e-30, (e.view(np.int32) + sign).view(F32), e)
            d = float(mc) - m
            f = np.exp(d)
            Sc, Wc = e.astype(np.float64).sum(), (e.astype(np.float64) * x.astype(np.float64)).sum()
            S += Sc * f
            W += (Wc + d * Sc) * f
        assert abs(m + np.log(S) - lse_p[r]) <= 2.4e-7 <= sref.tol_lse(V)
        assert abs(np.log(S) - W / S - ent_p[r]) <= sref.tol_entropy(V)


def test_check_temperature():
    check = engine_mod.check_temperature
    assert check(1.0) == 1.0 and check(4) == 0.25 and check(np.float32(0.25)) == 4.0
    assert check(3.0) == float(np.float32(1.0 / 3.0))
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), None, "1.0", True, 1e-60, 1e60):
        with pytest.raises(ValueError):
            check(bad)


def test_python_layers_refuse_bad_arguments_before_any_work():
    model = object.__new__(models.BERT4RecModel)            # the checks come before anything of the model is touched
    for t in (2.0, 0.5, 0.0, float("nan")):
        with pytest.raises(ValueError, match="return_distribution"):
            models.BERT4RecModel.recommend_tensor(model, {}, k=5, temperature=t)
    for t in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            models.BERT4RecModel.recommend_tensor(model, {}, k=5, return_distribution=True, temperature=t)
        with pytest.raises(ValueError, match="temperature"):
            models.BERT4RecModel.score_distribution_tensor(model, {}, temperature=t)
    rec = Recommender(None, None)
    with pytest.raises(ValueError, match="temperature"):
        rec.recommend_batch([[1, 2]], k=3, temperature=2.0)
    with pytest.raises(ValueError, match="temperature"):
        rec([1, 2], k=3, temperature=2.0)
    for p in (-0.1, 1.5, float("nan"), "0.1", True):
        with pytest.raises(ValueError, match="min_probability"):
            rec.recommend_batch([[1, 2]], k=3, min_probability=p)
    with pytest.raises(ValueError, match="full_ranking"):
        evaluation.get(distribution=True)
    ev = evaluation.get(full_ranking=True, distribution=True)
    assert ev.distribution and ev.distribution_results() == {"NLL": 0.0, "Perplexity": 1.0, "Entropy": 0.0}
    plain = evaluation.get(full_ranking=True)
    assert not plain.distribution and plain.distribution_results() == {}
    assert set(ev.get_metrics_results()) - set(plain.get_metrics_results()) == {"NLL", "Perplexity", "Entropy"}
    ev.reset_metrics()
    assert ev.distribution_results()["NLL"] == 0.0


def test_lib_binds_the_new_symbols():
    lib = _lib.load()
    for name in ("b4r_score_dist", "b4r_score_dist_scratch_bytes"):
        assert name in _lib.PROTOTYPES, name
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert lib.b4r_score_dist_scratch_bytes(0, 100) == 0 and lib.b4r_score_dist_scratch_bytes(4, 0) == 0
    # 24 bytes per row and chunk: it grows with R * ceil(V / 1024), not with R * V
    assert 256 * 328 * 24 <= lib.b4r_score_dist_scratch_bytes(256, 335423) < 256 * 335423 // 4
    assert lib.b4r_score_dist_scratch_bytes(16, 1024) < lib.b4r_score_dist_scratch_bytes(16, 1025)


def test_c_abi_refuses_bad_arguments_before_touching_the_device():
    lib = _lib.load()
    table = np.zeros(64 * 8 + 4, F32)
    tp = (table.ctypes.data + 15) & ~15                                 # (never read: every call below returns before a launch)

    def call(R=4, H=64, ld=None, V=1000, first=3, E=0, exclude=None, K=0, query=None, logp=None, inv_t=1.0, hidden=tp, tab=tp,
             allow=None, n_filters=0, scratch=None, scratch_bytes=0):
        return lib.b4r_score_dist(hidden, H if ld is None else ld, None, tab, None, H, V, first, R, exclude, E, None, allow, n_filters,
                                  None, None, inv_t, query, K, None, None, None, None, logp, scratch, scratch_bytes, None)
    for kw in (dict(K=1025), dict(K=-1), dict(R=-1), dict(E=-1), dict(first=-1), dict(H=30), dict(H=4100), dict(ld=60), dict(V=0),
               dict(allow=tp, n_filters=0)):
        assert call(**kw) == -2 and "b4r_score_dist" in _lib.last_error(), kw
    for inv_t in (0.0, -1.0, float("nan"), float("inf")):
        assert call(inv_t=inv_t) == -1 and "inv_temperature" in _lib.last_error()
    assert call(R=0) == 0                                              # nothing to do: no launch, no pointer is looked at
    assert call(hidden=None) == -1 and call(tab=None) == -1 and "null" in _lib.last_error()
    assert call(E=3) == -1 and call(K=3, logp=tp) == -1 and "query_ids" in _lib.last_error()
    assert call(tab=tp + 4) == -3
    assert call() == -5 and call(scratch=tp, scratch_bytes=16) == -5 and "scratch" in _lib.last_error()
