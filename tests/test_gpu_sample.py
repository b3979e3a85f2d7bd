"""Sampled recommendations on the GPU (b4r_gumbel_noise, b4r_sample_full, b4r_sample_pool): the ops against the CPU restatement
(tests/sample_ref.py), bit for bit in ids, scores and keys, and the model / app / evaluator layers built on them.

The shapes are the score-distribution tests' (tests/test_gpu_score_dist.py: 16 rows per group, 1024 ids per chunk, the 16-float
k-block and H % 4) with their planted rows -- an unfiltered row, a peaked row, a zero hidden row (all scores equal without a bias: the
order is the noise alone), a row with one allowed item, an empty row, a row whose first chunk holds nothing allowed -- plus a flat
unfiltered row (zero hidden, no filter).  make_case's twin table rows give equal scores: their keys differ by the noise alone."""
import functools

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, dataloaders, datasets, evaluation
from bert4rec_amd.apps import Recommender
from oracle import bert4rec_oracle as orc
from tests import catalogue_ref as ref
from tests import sample_ref as sr
from tests.b4r_testlib import P, stream
from tests.test_gpu_api import make_model
from tests.test_gpu_score_dist import FIRST, KINDS, SHAPES, dev, planted

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
HIGH_SEED = 0x0123456789ABCDEF


def test_gumbel_noise_equals_the_restatement_on_every_word():
    """The one test that pins the device's fp64 sequence, its two divisions included: all 2^23 distinct uniforms."""
    lib = _lib.load()
    words = (np.arange(1 << 23, dtype=np.uint64) << np.uint64(9)).astype(np.uint32)
    words[1::2] |= np.uint32(0x1FF)                                        # the low 9 bits do not count
    w = torch.from_numpy(words.view(np.int32)).to(DEV)
    out = torch.full((len(words),), 7.0, device=DEV)
    assert lib.b4r_gumbel_noise(P(w), len(words), P(out), stream()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = sr.gumbel_from_word(words)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (bad.size, [(hex(int(words[i])), float(got[i]), float(want[i])) for i in bad[:5]])
    assert lib.b4r_gumbel_noise(None, 0, None, stream()) == 0
    assert lib.b4r_gumbel_noise(None, 5, P(out), stream()) == -1


@functools.lru_cache(maxsize=None)
def case(R, H, V, offset):
    """planted()'s case, with the rows of kind 0 at every other occurrence turned into flat unfiltered rows (zero hidden)"""
    c = dict(planted(R, H, V, offset))
    hidden = c["hidden"].copy()
    flat = [r for r, kind in enumerate(c["kinds"].tolist()) if kind == 0][1::2]
    hidden[flat] = 0.0
    c["hidden"] = hidden
    c["flat"] = flat
    return c


@functools.lru_cache(maxsize=None)
def chain(R, H, V, offset, use_bias):
    c = case(R, H, V, offset)
    return ref.chain_scores(c["hidden"], c["table"], c["bias"] if use_bias else None)


def filter_words(c, filters):
    return {0: None, 1: c["one"], 3: c["words"]}[filters]


def run_sample(c, K, inv_t=1.0, use_bias=True, use_scale=False, filters=3, seed=1, row_stream=None, stream0=0, use_ex=True,
               scratch_bytes=None, hidden=None, hidden_row=None, hidden_ld=None, sync=True, outs=None, keep=None, null_out=()):
    """b4r_sample_full on the case; returns (rc, dict of numpy outputs).  The outputs start from sentinels."""
    lib = _lib.load()
    R, H = c["hidden"].shape
    V = c["table"].shape[0]
    words = filter_words(c, filters)
    if keep is None:
        d = dict(hidden=dev(c["hidden"] if hidden is None else hidden), table=dev(c["table"]), bias=dev(c["bias"]) if use_bias else None,
                 ex=dev(c["ex"]) if use_ex else None, gt=dev(c["gt"]) if use_ex else None,
                 words=None if words is None else dev(words.view(np.int32)), rf=dev(c["row_filter"]) if filters == 3 else None,
                 scale=dev(c["scale"]) if use_scale else None, hr=dev(hidden_row, torch.int64),
                 rs=None if row_stream is None else dev(np.asarray(row_stream, np.int64)))
        need = int(lib.b4r_sample_full_scratch_bytes(R, V, K))
        nbytes = need if scratch_bytes is None else scratch_bytes
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    else:
        d, scratch, nbytes = keep
    if outs is None:
        outs = dict(ids=torch.full((R, max(K, 1)), -7, dtype=torch.int64, device=DEV), scores=torch.full((R, max(K, 1)), 7.0, device=DEV),
                    keys=torch.full((R, max(K, 1)), 7.0, device=DEV))
    ptr = {k: (None if k in null_out else P(v)) for k, v in outs.items()}
    rc = lib.b4r_sample_full(P(d["hidden"]), hidden_ld or H, P(d["hr"]), P(d["table"]), P(d["bias"]), H, V, FIRST, R, P(d["ex"]),
                             c["ex"].shape[1] if use_ex else 0, P(d["gt"]), K, P(d["words"]), 0 if words is None else words.shape[0],
                             P(d["rf"]), P(d["scale"]), inv_t, seed, P(d["rs"]), stream0, ptr["ids"], ptr["scores"], ptr["keys"],
                             P(scratch), nbytes, stream())
    if not sync:
        return rc, outs, (d, scratch, nbytes)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in outs.items()}


def untouched(got):
    return (got["ids"] == -7).all() and (got["scores"] == 7.0).all() and (got["keys"] == 7.0).all()


def same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def restated(c, key, K, inv_t, use_bias, use_scale, filters, seed, row_stream, stream0, use_ex=True):
    """(ids, scores, keys) [R, K] of the restatement, and the allowed mask"""
    R, V = c["hidden"].shape[0], c["table"].shape[0]
    sc = ref.scaled(chain(*key, use_bias), c["scale"] if use_scale else None).astype(F32)
    ok = ref.allowed_mask(V, FIRST, c["ex"] if use_ex else None, c["gt"] if use_ex else None, R, filter_words(c, filters),
                          c["row_filter"] if filters == 3 else None)
    return sr.sample_full(sc, ok, K, inv_t, seed, row_stream, stream0), ok


def assert_same(got, want, K, what=""):
    ids, scores, keys = want
    assert np.array_equal(got["ids"][:, :K], ids), f"ids {what}"
    assert got["scores"][:, :K].tobytes() == scores.tobytes(), f"scores {what}"
    assert got["keys"][:, :K].tobytes() == keys.tobytes(), f"keys {what}"


def high_streams(R, salt):
    """row streams with their high words set, of both signs"""
    rng = np.random.default_rng(1000 + salt)
    s = rng.integers(-(1 << 62), 1 << 62, size=R).astype(np.int64)
    s[::3] = -s[::3] - 1
    return s


# (inv_temperature, bias, item_scale, filters, exclude and gt, seed, row_stream given, stream0)
CALLS = [(1.0, True, False, 3, True, HIGH_SEED, True, 0),
         (0.25, False, True, 3, True, 1, False, (1 << 63) - 5),           # stream0 + r wraps
         (4.0, False, False, 1, True, 0, False, 0),
         (1.0, True, True, 0, False, 1 << 40, True, 0)]
KS = (1, 10, 257, 1024)


@pytest.mark.parametrize("R,H,V", SHAPES, ids=[f"R{s[0]}_H{s[1]}_V{s[2]}" for s in SHAPES])
def test_sample_full_against_the_restatement(R, H, V):
    seen_short = seen_full = False
    for offset in (range(0, KINDS, R) if R < KINDS else (0,)):
        key = (R, H, V, offset)
        c = case(*key)
        for i, (inv_t, use_bias, use_scale, filters, use_ex, seed, with_rs, stream0) in enumerate(CALLS):
            rs = high_streams(R, i) if with_rs else None
            want_all, ok = restated(c, key, 1024, inv_t, use_bias, use_scale, filters, seed, rs, stream0, use_ex)
            n_allowed = ok.sum(axis=1)
            for K in KS:
                rc, got = run_sample(c, K, inv_t, use_bias, use_scale, filters, seed, rs, stream0, use_ex)
                assert rc == 0, _lib.last_error()
                assert_same(got, tuple(x[:, :K] for x in want_all), K, f"K={K} call {i}")
                seen_short |= bool((n_allowed < K).any())                  # K beyond |allowed|: the -1 / -inf / -inf tail
                seen_full |= bool((n_allowed >= K).any())
                live = got["ids"][:, :K] >= 0
                assert (live.sum(axis=1) == np.minimum(n_allowed, K)).all()
                assert np.isneginf(got["scores"][:, :K][~live]).all() and np.isneginf(got["keys"][:, :K][~live]).all()
                k64 = got["keys"][:, :K].astype(np.float64)
                assert (k64[:, :-1] >= k64[:, 1:]).all()                   # the draw order: keys descend
            if i == 0:
                rc, again = run_sample(c, 10, inv_t, use_bias, use_scale, filters, seed, rs, stream0, use_ex)
                rc2, first = run_sample(c, 10, inv_t, use_bias, use_scale, filters, seed, rs, stream0, use_ex)
                assert rc == 0 and rc2 == 0 and same_bits(first, again), "two calls differ"
                for skip in ("ids", "scores", "keys"):                     # any output may be NULL
                    rc, part = run_sample(c, 10, inv_t, use_bias, use_scale, filters, seed, rs, stream0, use_ex, null_out=(skip,))
                    assert rc == 0 and all(part[k].tobytes() == first[k].tobytes() for k in part if k != skip)
                    assert (part[skip] == (-7 if skip == "ids" else 7.0)).all()
            # the planted rows
            ids10 = want_all[0][:, :10]
            for r, kind in enumerate(c["kinds"].tolist()):
                if filters == 3 and kind == 3:
                    assert n_allowed[r] == 1 and ids10[r, 0] == c["gt"][r] and (ids10[r, 1:] == -1).all()
                if filters == 3 and kind == 4:
                    assert n_allowed[r] == 0 and (ids10[r] == -1).all()
    assert seen_short and seen_full


def test_flat_rows_are_ordered_by_the_noise_alone():
    """zero hidden, no bias: every score is +0.0, so the list is the order of the noise, and the scores returned are all +0.0"""
    key = (17, 64, 1023, 0)
    c = case(*key)
    assert c["flat"]
    rs = high_streams(17, 9)
    rc, got = run_sample(c, 257, 1.0, False, False, 3, 77, rs, 0)
    assert rc == 0, _lib.last_error()
    want, ok = restated(c, key, 257, 1.0, False, False, 3, 77, rs, 0)
    assert_same(got, want, 257)
    for r in c["flat"]:
        j = np.flatnonzero(ok[r])
        g = sr.gumbel(77, int(rs[r]), j)
        order = j[np.argsort(-g.astype(np.float64), kind="stable")][:257]
        assert np.array_equal(got["ids"][r], order) and (got["scores"][r].view(np.uint32) == 0).all()
        assert got["keys"][r].tobytes() == g[np.argsort(-g.astype(np.float64), kind="stable")][:257].tobytes()


def test_twin_table_rows_are_separated_by_the_noise():
    """make_case's duplicated table rows (7 and 4 copy 3; 1030 copies 1020): equal scores, so the noise alone orders them"""
    key = (3, 132, 2049, 0)
    c = case(*key)
    rc, got = run_sample(c, 1024, 1.0, True, False, 0, 5, None, 0, use_ex=False)
    assert rc == 0
    sc = chain(*key, True)
    assert sc[0, 7] == sc[0, 3] == sc[0, 4] and sc[0, 1030] == sc[0, 1020]
    keys = sr.keys_of(sc, 1.0, 5, [0, 1, 2])
    checked = 0
    for r in range(3):
        ids = got["ids"][r].tolist()
        for a, b in ((7, 3), (4, 3), (1030, 1020)):
            if a in ids and b in ids:
                ka, kb = float(keys[r, a]), float(keys[r, b])
                assert (ids.index(a) < ids.index(b)) == (ka > kb or (ka == kb and a < b))
                checked += 1
    assert checked >= 3


def test_grouped_rows_ld_and_hidden_row():
    """R = 40 with a scratch for 16 rows: three groups, the same bits (stream(r) is the row of the call); a hidden_ld > H with
    hidden_row: the same bits."""
    lib = _lib.load()
    key = (40, 64, 1500, 0)
    c = case(*key)
    K = 20
    for rs, stream0 in ((None, 12345678901234), (high_streams(40, 3), 0)):
        rc, full = run_sample(c, K, 0.5, True, False, 3, 9, rs, stream0)
        assert rc == 0, _lib.last_error()
        assert_same(full, restated(c, key, K, 0.5, True, False, 3, 9, rs, stream0)[0], K)
        small = int(lib.b4r_sample_full_scratch_bytes(16, 1500, K))
        assert small < int(lib.b4r_sample_full_scratch_bytes(40, 1500, K))
        rc, grouped = run_sample(c, K, 0.5, True, False, 3, 9, rs, stream0, scratch_bytes=small)
        assert rc == 0 and same_bits(full, grouped)
        rc, grouped = run_sample(c, K, 0.5, True, False, 3, 9, rs, stream0, scratch_bytes=small + small // 2)
        assert rc == 0 and same_bits(full, grouped)
        ld = 64 + 4
        wide = np.zeros((40 + 2, ld), F32)
        perm = np.random.default_rng(1).permutation(42)[:40]
        wide[perm, :64] = c["hidden"]
        rc, moved = run_sample(c, K, 0.5, True, False, 3, 9, rs, stream0, hidden=wide, hidden_row=perm, hidden_ld=ld)
        assert rc == 0 and same_bits(full, moved)


# ---- b4r_sample_pool ----------------------------------------------------------------------------------------------------------------
def run_pool(pool_ids, pool_scores, V, K, inv_t=1.0, seed=1, row_stream=None, stream0=0, null_out=()):
    lib = _lib.load()
    R, M = pool_ids.shape
    d_ids, d_sc = dev(np.ascontiguousarray(pool_ids, np.int64)), dev(np.ascontiguousarray(pool_scores, F32))
    rs = None if row_stream is None else dev(np.asarray(row_stream, np.int64))
    outs = dict(ids=torch.full((R, max(K, 1)), -7, dtype=torch.int64, device=DEV), scores=torch.full((R, max(K, 1)), 7.0, device=DEV),
                keys=torch.full((R, max(K, 1)), 7.0, device=DEV), pos=torch.full((R, max(K, 1)), -7, dtype=torch.int32, device=DEV))
    ptr = {k: (None if k in null_out else P(v)) for k, v in outs.items()}
    rc = lib.b4r_sample_pool(P(d_ids), P(d_sc), R, M, V, inv_t, seed, P(rs), stream0, K, ptr["ids"], ptr["scores"], ptr["keys"],
                             ptr["pos"], stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in outs.items()}


@pytest.mark.parametrize("M", [1, 63, 64, 65, 256, 257, 1024])
def test_sample_pool_against_the_restatement(M):
    V, R = 500, 5
    rng = np.random.default_rng(M)
    ids = rng.integers(-2, V + 2, size=(R, M)).astype(np.int64)           # dead ids on both sides, duplicates (M > V / 2)
    scores = (np.round(rng.standard_normal((R, M)) * 4) / 4).astype(F32)   # quantised: equal scores
    scores[rng.random((R, M)) < 0.05] = np.nan
    scores[rng.random((R, M)) < 0.03] = np.inf
    scores[rng.random((R, M)) < 0.03] = -np.inf
    if M > 1:
        ids[0, 1] = ids[0, 0] = 7; scores[0, 1] = scores[0, 0] = 1.0       # the same id twice with the same score: an exact key tie
        ids[1] = -1                                                        # a row without a live entry
    if M >= 63:
        ids[2, :] = rng.permutation(V)[:M] if M <= V else np.resize(rng.permutation(V), M)
        scores[2, :] = 0.0                                                 # a flat row
    rs = high_streams(R, M)
    for K, inv_t, seed, row_stream, stream0 in ((M, 1.0, HIGH_SEED, rs, 0), (max(1, M // 3), 4.0, 3, None, -7), (1, 0.25, 0, None, 0)):
        rc, got = run_pool(ids, scores, V, K, inv_t, seed, row_stream, stream0)
        assert rc == 0, _lib.last_error()
        w_ids, w_sc, w_keys, w_pos = sr.sample_pool(ids, scores, V, K, inv_t, seed, row_stream, stream0)
        assert np.array_equal(got["ids"], w_ids) and np.array_equal(got["pos"], w_pos)
        assert got["scores"].tobytes() == w_sc.tobytes() and got["keys"].tobytes() == w_keys.tobytes()
    if M > 1:
        assert got["ids"][1, 0] == -1 and got["pos"][1, 0] == -1 and np.isneginf(got["keys"][1, 0])
        rc, full = run_pool(ids, scores, V, M, 1.0, HIGH_SEED, rs, 0)
        first = full["pos"][0].tolist()
        assert first.index(0) + 1 == first.index(1)                        # the tie goes to the lower pool position


def test_sample_pool_of_everything_allowed_equals_sample_full():
    """the pool is b4r_rank_full_ex's top M with M >= |allowed(r)|: the same ids, scores and keys as b4r_sample_full"""
    lib = _lib.load()
    key = (17, 64, 1023, 0)
    c = case(*key)
    R, H, V, K, M = 17, 64, 1023, 50, 1024
    rs = high_streams(R, 4)
    for inv_t, seed in ((1.0, 11), (0.25, HIGH_SEED)):
        rc, full = run_sample(c, K, inv_t, True, False, 3, seed, rs, 0)
        assert rc == 0
        ids = torch.empty((R, M), dtype=torch.int64, device=DEV)
        scores = torch.empty((R, M), device=DEV)
        need = int(lib.b4r_rank_full_scratch_bytes(R, V, M))
        scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
        keep = [dev(c["hidden"]), dev(c["table"]), dev(c["bias"]), dev(c["ex"]), dev(c["gt"]), dev(c["words"].view(np.int32)), dev(c["row_filter"])]
        rc = lib.b4r_rank_full_ex(P(keep[0]), H, None, P(keep[1]), P(keep[2]), H, V, FIRST, R, P(keep[3]), c["ex"].shape[1], P(keep[4]), M,
                                  P(ids), P(scores), None, P(scratch), need, stream(), P(keep[5]), 3, P(keep[6]), None)
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert (ids[:, -1] == -1).all()                                    # every allowed item is in the pool
        rc, pooled = run_pool(ids.cpu().numpy(), scores.cpu().numpy(), V, K, inv_t, seed, rs, 0)
        assert rc == 0
        assert all(pooled[k].tobytes() == full[k].tobytes() for k in ("ids", "scores", "keys"))


# ---- behaviour ----------------------------------------------------------------------------------------------------------------------
def test_seed_and_stream_select_the_draw():
    key = (16, 64, 1024, 0)
    c = case(*key)
    base = run_sample(c, 10, 1.0, True, False, 0, 5, None, 0)[1]
    assert same_bits(base, run_sample(c, 10, 1.0, True, False, 0, 5, None, 0)[1])
    other_seed = run_sample(c, 10, 1.0, True, False, 0, 6, None, 0)[1]
    high_seed = run_sample(c, 10, 1.0, True, False, 0, 5 + (1 << 32), None, 0)[1]
    other_stream = run_sample(c, 10, 1.0, True, False, 0, 5, None, 1)[1]
    high_stream = run_sample(c, 10, 1.0, True, False, 0, 5, None, 1 << 32)[1]
    soft = c["kinds"] != 1                                                 # (a peaked row's score gaps exceed the noise)
    for other in (other_seed, high_seed, other_stream, high_stream):
        assert (other["ids"] != base["ids"]).any(axis=1)[soft].all()       # every such row draws another list
    # a row's list depends on its own stream alone: row_stream = stream0 + r restates the default
    rs = np.arange(16, dtype=np.int64) + 1
    assert same_bits(other_stream, run_sample(c, 10, 1.0, True, False, 0, 5, rs, 99)[1])


def test_a_small_temperature_reproduces_the_top_k():
    """score gaps of 1 at T = 0.01: t gaps of 100 exceed the noise's range of 19.5, so the draw is b4r_rank_full's top k"""
    lib = _lib.load()
    R, H, V, K = 3, 4, 1500, 40
    rng = np.random.default_rng(0)
    table = np.zeros((V, H), F32)
    table[:, 0] = rng.permutation(V).astype(F32)                           # distinct integer scores
    hidden = np.zeros((R, H), F32)
    hidden[:, 0] = (1.0, 2.0, -1.0)                                        # gaps 1, 2, 1 (the last row prefers the low values)
    c = dict(hidden=hidden, table=table, bias=np.zeros(V, F32), ex=np.full((R, 1), -1, np.int64), gt=np.full(R, -1, np.int64),
             one=None, words=None)
    rc, got = run_sample(c, K, 100.0, True, False, 0, 3, None, 0)
    assert rc == 0, _lib.last_error()
    ids = torch.empty((R, K), dtype=torch.int64, device=DEV)
    scores = torch.empty((R, K), device=DEV)
    need = int(lib.b4r_rank_full_scratch_bytes(R, V, K))
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    keep = [dev(hidden), dev(table), dev(c["bias"]), dev(c["ex"])]
    rc = lib.b4r_rank_full(P(keep[0]), H, None, P(keep[1]), P(keep[2]), H, V, FIRST, R, P(keep[3]), 1, None, K, P(ids), P(scores), None,
                           P(scratch), need, stream())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(got["ids"], ids.cpu().numpy()) and got["scores"].tobytes() == scores.cpu().numpy().tobytes()
    rc, warm = run_sample(c, K, 0.001, True, False, 0, 3, None, 0)        # a large temperature: the noise decides
    assert rc == 0 and (warm["ids"] != got["ids"]).any()


def test_argument_errors_leave_the_outputs_untouched():
    lib = _lib.load()
    c = case(20, 64, 1500, 0)
    for inv_t in (0.0, -1.0, float("nan"), float("inf")):
        rc, got = run_sample(c, 10, inv_t)
        assert rc == -1 and "inv_temperature" in _lib.last_error() and untouched(got)
    rc, got = run_sample(c, 1025)
    assert rc == -2 and untouched(got)
    small = int(lib.b4r_sample_full_scratch_bytes(16, 1500, 10))
    for nbytes in (small // 2, 0):
        rc, got = run_sample(c, 10, scratch_bytes=nbytes)
        assert rc == -5 and "b4r_sample_full" in _lib.last_error() and untouched(got)
    rc, got = run_sample(c, 0)                                             # K = 0 launches nothing
    assert rc == 0 and untouched(got)
    ids = np.zeros((2, 8), np.int64)
    sc = np.zeros((2, 8), F32)
    for K, inv_t, code in ((9, 1.0, -2), (-1, 1.0, -2), (4, 0.0, -1), (4, float("nan"), -1)):
        rc, got = run_pool(ids, sc, 100, K, inv_t)
        assert rc == code and (got["ids"] == -7).all() and (got["pos"] == -7).all() and (got["keys"] == 7.0).all()
    assert lib.b4r_sample_pool(None, None, 2, 0, 100, 1.0, 1, None, 0, 0, None, None, None, None, stream()) == -2      # M = 0
    assert lib.b4r_sample_pool(None, None, 2, 1025, 100, 1.0, 1, None, 0, 1, None, None, None, None, stream()) == -2   # M > 1024


def test_graph_capture_replays_the_eager_bits():
    c = case(20, 64, 1500, 0)
    rs = high_streams(20, 6)
    rc, eager = run_sample(c, 33, 0.25, True, True, 3, HIGH_SEED, rs, 0)
    assert rc == 0, _lib.last_error()
    pool_ids = np.random.default_rng(3).integers(-1, 1500, size=(20, 100)).astype(np.int64)
    pool_sc = np.random.default_rng(4).standard_normal((20, 100)).astype(F32)
    rc, eager_pool = run_pool(pool_ids, pool_sc, 1500, 10, 0.5, 7, rs, 0)
    assert rc == 0
    lib = _lib.load()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        rc, outs, keep = run_sample(c, 33, 0.25, True, True, 3, HIGH_SEED, rs, 0, sync=False)   # allocations and copies outside the capture
        assert rc == 0
        p_in = [dev(pool_ids), dev(pool_sc), dev(rs)]
        p_out = dict(ids=torch.full((20, 10), -7, dtype=torch.int64, device=DEV), scores=torch.full((20, 10), 7.0, device=DEV),
                     keys=torch.full((20, 10), 7.0, device=DEV), pos=torch.full((20, 10), -7, dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        outs["ids"].fill_(-7); outs["scores"].fill_(7.0); outs["keys"].fill_(7.0)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            rc, _, _ = run_sample(c, 33, 0.25, True, True, 3, HIGH_SEED, rs, 0, sync=False, outs=outs, keep=keep)
            assert rc == 0
            rc = lib.b4r_sample_pool(P(p_in[0]), P(p_in[1]), 20, 100, 1500, 0.5, 7, P(p_in[2]), 0, 10, P(p_out["ids"]), P(p_out["scores"]),
                                     P(p_out["keys"]), P(p_out["pos"]), stream())
            assert rc == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert (outs["ids"] == -7).all() and (p_out["ids"] == -7).all(), "a capture must not run the kernels"
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(eager, {k: v.cpu().numpy() for k, v in outs.items()})
    assert same_bits(eager_pool, {k: v.cpu().numpy() for k, v in p_out.items()})


# ---- layers ---------------------------------------------------------------------------------------------------------------------
def test_model_layers_against_the_op():
    V = 300
    model = make_model(V, seed=17)
    eng = model.engine
    batch = orc.synthetic_batch(48, 24, 6, V, seed=9, ragged=True)
    hidden, slots, _ = model._ranked_slot_hidden(batch)
    R = int(slots.numel())
    b_idx = (slots // 6).cpu()
    seen = batch["input_word_ids"][b_idx]
    rng = np.random.default_rng(2)
    allow = torch.as_tensor(rng.random(V) < 0.8)
    streams = torch.as_tensor(high_streams(R, 1))
    # every default call returns what it returned: the plain b4r_rank_full top k
    ids0, sc0, slots0 = model.recommend_tensor(batch, k=10)
    op_ids, op_sc, _ = eng.rank_full(hidden, None, seen, FIRST, None, 10)
    assert torch.equal(ids0, op_ids) and torch.equal(sc0.view(torch.int32), op_sc.view(torch.int32)) and torch.equal(slots0, slots)
    table, bias = eng.view("word_embeddings/embeddings").cpu().numpy(), eng.view("cls/predictions/output_bias/bias").cpu().numpy()
    sc_ref = ref.chain_scores(hidden.cpu().numpy(), table, bias)
    for kw, op_allow, temp, st in ((dict(), None, 1.0, None), (dict(allow=allow, temperature=2.0), allow, 2.0, streams)):
        ids, sc, slots1 = model.recommend_tensor(batch, k=10, sample_seed=HIGH_SEED, sample_streams=st, **kw)
        o_ids, o_sc, o_keys = eng.sample_full(hidden, None, seen, FIRST, None, 10, HIGH_SEED, op_allow, None, temp, st)
        assert torch.equal(ids, o_ids) and torch.equal(sc.view(torch.int32), o_sc.view(torch.int32)) and torch.equal(slots1, slots)
        # ... and the restatement on the transform's rows
        words = None if op_allow is None else ref.pack_bits(op_allow.numpy())
        ok = ref.allowed_mask(V, FIRST, seen.numpy(), None, R, words, None)
        w_ids, w_sc, w_keys = sr.sample_full(sc_ref, ok, 10, float(F32(1.0 / temp)), HIGH_SEED, None if st is None else st.numpy(), 0)
        assert np.array_equal(ids.cpu().numpy(), w_ids) and sc.cpu().numpy().tobytes() == w_sc.tobytes()
        assert o_keys.cpu().numpy().tobytes() == w_keys.tobytes()
        # the scores keep b4r_rank_full's bits: each drawn id's score in the full ranking of the row
        all_ids, all_sc, _ = eng.rank_full(hidden, None, seen, FIRST, None, 300, op_allow)
        look = {(r, int(i)): s for r in range(R) for i, s in zip(all_ids[r].cpu().tolist(), all_sc[r].cpu().view(torch.int32).tolist())}
        assert all(look[(r, int(i))] == s for r in range(R) for i, s in zip(ids[r].cpu().tolist(), sc[r].cpu().view(torch.int32).tolist()))
        # the pool variant: the best 40, then b4r_sample_pool
        p_ids, p_sc, _ = model.recommend_tensor(batch, k=10, sample_seed=HIGH_SEED, sample_streams=st, pool=40, **kw)
        top_ids, top_sc, _ = eng.rank_full(hidden, None, seen, FIRST, None, 40, op_allow)
        q_ids, q_sc, _, _ = eng.sample_pool(top_ids, top_sc, 10, HIGH_SEED, temp, st)
        assert torch.equal(p_ids, q_ids) and torch.equal(p_sc.view(torch.int32), q_sc.view(torch.int32))
        assert all(set(a) <= set(b) for a, b in zip(p_ids.cpu().tolist(), top_ids.cpu().tolist()))
        # return_distribution: b4r_score_dist's log probabilities of the drawn ids, over the full allowed set (also with a pool)
        for pool, want_ids in ((None, ids), (40, p_ids)):
            d_ids, d_sc, _, dist = model.recommend_tensor(batch, k=10, sample_seed=HIGH_SEED, sample_streams=st, pool=pool,
                                                          return_distribution=True, **kw)
            assert torch.equal(d_ids, want_ids)
            n, _, lse, _, logp = eng.score_distribution(hidden, None, seen, FIRST, None, op_allow, None, temp, want_ids)
            assert torch.equal(dist["logp"].view(torch.int32), logp.view(torch.int32)) and torch.equal(dist["lse"], lse)
            assert torch.equal(dist["n"], n) and torch.isfinite(dist["logp"]).all()
    # another seed, another list; the same seed, the same list
    again = model.recommend_tensor(batch, k=10, sample_seed=HIGH_SEED)[0]
    other = model.recommend_tensor(batch, k=10, sample_seed=HIGH_SEED + 1)[0]
    assert torch.equal(again, model.recommend_tensor(batch, k=10, sample_seed=HIGH_SEED)[0]) and (other != again).any(dim=1).all()
    lists = model.recommend(batch, k=10, sample_seed=HIGH_SEED)
    assert [pair[0] for row in lists for pair in row] == again.cpu().tolist()
    with pytest.raises(ValueError, match="diversity"):
        model.recommend_tensor(batch, k=10, sample_seed=1, diversity=0.5)


def test_recommend_batch_draws_per_user_streams():
    ds = datasets.synthetic_dataset(n_users=30, n_items=200, min_len=5, max_len=30, seed=4)
    dl = dataloaders.get_dataloader_factory("bert4rec").create_ml_1m_dataloader(data_source=ds, max_seq_len=24, max_predictions_per_seq=6)
    dl.generate_vocab()
    model = make_model(dl.tokenizer.get_vocab_size(), seed=5)
    items = dl.create_item_list()
    histories = [items[s:s + n] for s, n in ((0, 15), (40, 3), (90, 30), (120, 1), (7, 22))]
    users = [1 << 40, 17, -3, 99, 4]
    rec = Recommender(model, dl)
    plain = rec.recommend_batch(histories, 5)
    assert plain == rec.recommend_batch(histories, 5)                      # the default path, as before
    drawn = rec.recommend_batch(histories, 5, sample_seed=3, user_streams=users)
    assert drawn == rec.recommend_batch(histories, 5, sample_seed=3, user_streams=users) and drawn != plain
    assert all(len(row) == 5 and len(set(row)) == 5 and not set(row) & set(h) for row, h in zip(drawn, histories))
    # a user draws the same list whatever batch they ride in
    order = [3, 0, 4, 2, 1]
    moved = rec.recommend_batch([histories[i] for i in order], 5, sample_seed=3, user_streams=[users[i] for i in order])
    assert moved == [drawn[i] for i in order]
    pair = rec.recommend_batch([histories[2], histories[0]], 5, sample_seed=3, user_streams=[users[2], users[0]])
    assert pair == [drawn[2], drawn[0]]
    assert rec.recommend_batch(histories, 5, sample_seed=4, user_streams=users) != drawn
    # without user_streams the stream is the position in the batch
    assert rec.recommend_batch(histories, 5, sample_seed=3) == rec.recommend_batch(histories, 5, sample_seed=3, user_streams=[0, 1, 2, 3, 4])
    # probabilities of the drawn items, a temperature, a truncated draw
    pairs = rec.recommend_batch(histories, 5, sample_seed=3, user_streams=users, return_probabilities=True)
    assert [[item for item, _ in row] for row in pairs] == drawn and all(0.0 < p <= 1.0 for row in pairs for _, p in row)
    warm = rec.recommend_batch(histories, 5, sample_seed=3, user_streams=users, temperature=50.0)
    assert warm != drawn
    top = rec.recommend_batch(histories, 8)
    trunc = rec.recommend_batch(histories, 5, sample_seed=3, user_streams=users, candidate_pool=8, temperature=50.0)
    assert all(set(row) <= set(best) for row, best in zip(trunc, top))
    with pytest.raises(ValueError, match="user streams"):
        rec.recommend_batch(histories, 5, sample_seed=3, user_streams=[1, 2])


def test_evaluator_sampled_lists():
    V, K = 300, 10
    model = make_model(V, seed=19)
    eng = model.engine
    batches = [orc.synthetic_batch(32, 24, 6, V, seed=70 + i, ragged=True, finetune=True) for i in range(3)]
    counts = np.random.default_rng(5).integers(1, 50, size=V)
    metrics = lambda: [evaluation.Counter(name="Valid Ranks"), evaluation.HR(1), evaluation.HR(K), evaluation.NDCG(K)]
    for pool in (None, 60):
        ev = evaluation.get(full_ranking=True, list_k=K, sample_seed=21, temperature=0.5, candidate_pool=pool, item_counts=counts,
                            metrics=metrics())
        hits = {1: 0, K: 0}
        ndcg = 0.0
        valid = rows = 0
        lists = []
        for b in batches:
            ev.evaluate_batch(model, b)
            w = b["masked_lm_weights"] != 0
            b_idx, p_idx = torch.nonzero(w, as_tuple=True)
            slots = (b_idx * w.shape[1] + p_idx).cuda()
            hidden, _, _ = model._ranked_slot_hidden(b, slots)
            gt = b["masked_lm_ids"][b_idx, p_idx].to(torch.int64)
            ex = b["labels"][b_idx].to(torch.int64)
            if pool is None:
                ids = eng.sample_full(hidden, None, ex, FIRST, gt, K, 21, temperature=0.5, stream0=rows)[0]
            else:
                top_ids, top_sc, _ = eng.rank_full(hidden, None, ex, FIRST, gt, pool)
                ids = eng.sample_pool(top_ids, top_sc, K, 21, 0.5, stream0=rows)[0]
            rows += len(gt)                                                # stream0: the rows evaluated so far
            lists.append(ids.cpu().numpy())
            for row, g in zip(ids.cpu().tolist(), gt.tolist()):
                if not FIRST <= g < V:
                    continue
                valid += 1
                if g in row:
                    pos = row.index(g) + 1
                    hits[K] += 1
                    hits[1] += pos == 1
                    ndcg += 1.0 if pos == 1 else 1.0 / np.log2(pos + 1)
        res = ev.get_metrics_results()
        assert res["Valid Ranks"] == valid and valid > 0
        assert res["HR@1"] == pytest.approx(hits[1] / valid, abs=1e-12) and res[f"HR@{K}"] == pytest.approx(hits[K] / valid, abs=1e-12)
        assert res[f"NDCG@{K}"] == pytest.approx(ndcg / valid, abs=1e-9)
        assert {f"ILD@{K}", f"Novelty@{K}", f"Coverage@{K}", f"Gini@{K}"} <= set(res)
        shown = np.unique(np.concatenate(lists).reshape(-1))
        assert res[f"Coverage@{K}"] == pytest.approx((shown >= FIRST).sum() / (V - FIRST), abs=1e-12)
        ev.reset_metrics()                                                 # the streams start over: the same evaluation again
        for b in batches:
            ev.evaluate_batch(model, b)
        assert ev.get_metrics_results() == res
    # exploration buys coverage: the sampled lists at a high temperature cover more of the catalogue than the top-k lists
    plain = evaluation.get(full_ranking=True, list_k=K, item_counts=counts, metrics=metrics())
    hot = evaluation.get(full_ranking=True, list_k=K, sample_seed=1, temperature=100.0, item_counts=counts, metrics=metrics())
    for b in batches:
        plain.evaluate_batch(model, b)
        hot.evaluate_batch(model, b)
    assert hot.get_metrics_results()[f"Coverage@{K}"] >= plain.get_metrics_results()[f"Coverage@{K}"]
    # the default evaluator is untouched by the new keywords
    base = evaluation.get(full_ranking=True, list_k=K, item_counts=counts)
    for b in batches:
        base.evaluate_batch(model, b)
    assert base.get_metrics_results()[f"Coverage@{K}"] == plain.get_metrics_results()[f"Coverage@{K}"]
