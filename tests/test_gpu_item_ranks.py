"""Item ranks on the GPU (b4r_item_ranks, b4r_rank_metrics_multi): the ops against the CPU restatement (tests/item_ranks_ref.py), against
b4r_rank_full_ex and b4r_score_dist on the same inputs, and the model / app / evaluator layers built on them.

ranks, member, row_n and query_scores are bit-exact in the three modes.  The shapes reach the sweep's boundaries: 16 rows per tile
(R = 1, 16, 17, 33), 1024 ids per chunk (V = 4, 33, 1023, 1024, 1025, 2049, 70000), the 16-float k-block and H % 4 (H = 4, 32, 132), and
the query count's own (Q = 0, 1, 2, 15, 16, 17, 255, 256: the search's powers of two, one workgroup of 256 threads).  The rows are
test_gpu_score_dist's planted kinds (flat, peaked, zero hidden, one-bit filter, empty, empty first chunk) on make_case's twin table rows.
The double sums of b4r_rank_metrics_multi are held to 1e-12 relative, the bound tests/test_gpu_list_metrics.py derives for such sums
(R <= 300 rows, Q <= 16 terms each)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, evaluation
from tests import catalogue_ref as ref
from tests import item_ranks_ref as iref
from tests.b4r_testlib import P, stream
from tests.test_gpu_catalogue_filter import small_app
from tests.test_gpu_score_dist import FIRST, dev, one_bit_id, planted, run_dist

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
MODES = (iref.STRICT, iref.SELF, iref.JOINT)
SHAPES = [(1, 4, 4, 2), (16, 32, 33, 1), (17, 132, 1023, 15), (33, 32, 1024, 16), (17, 4, 1025, 17), (16, 132, 2049, 255),
          (33, 32, 2049, 256), (1, 32, 1025, 0), (2, 64, 70000, 17)]
# (bias, scale, filters: 3 = the three planted filters with row_filter, 1 = one filter for all rows, 0 = none)
VARIANTS = [(True, False, 3), (False, True, 3), (True, True, 0), (False, False, 1)]


def words_of(c, filters):
    return {0: None, 1: c["one"], 3: c["words"]}[filters]


@functools.lru_cache(maxsize=None)
def scores_of(R, H, V, use_bias, use_scale):
    c = planted(R, H, V, 0)
    return ref.scaled(ref.chain_scores(c["hidden"], c["table"], c["bias"] if use_bias else None), c["scale"] if use_scale else None)


def allowed_of(c, filters):
    R, V = c["hidden"].shape[0], c["table"].shape[0]
    return ref.allowed_mask(V, FIRST, c["ex"], None, R, words_of(c, filters), c["row_filter"] if filters == 3 else None)


@functools.lru_cache(maxsize=None)
def queries(R, H, V, Q):
    """Per row: the best and the worst allowed item, the twin rows' ids, a repeated id, padding, an id below first_item, an excluded id,
    a filtered id, the one-bit id, then random ids; cut to Q columns."""
    c = planted(R, H, V, 0)
    sc, ok = scores_of(R, H, V, True, False), allowed_of(c, 3)
    rng = np.random.default_rng(R + V + Q)
    out = np.zeros((R, max(Q, 1)), np.int64)
    filtered = np.flatnonzero(~c["masks"][2])
    for r in range(R):
        a = np.flatnonzero(ok[r])
        # (ties: the lowest id among the best stands first, the highest id among the worst stands last)
        best, worst = (int(a[np.argmax(sc[r, a])]), int(a[::-1][np.argmin(sc[r, a[::-1]])])) if a.size else (V - 1, FIRST)
        row = [best, worst, 7, 3, 4, best, -1, V, 1 << 40, -(1 << 40), 1, int(c["ex"][r, 0]), int(filtered[min(len(filtered) - 1, 5)]),
               one_bit_id(V), 1030, 1020, V - 1, V - 2, 11, 100, 200]
        row += rng.integers(0, V + 2, size=max(Q, 1)).tolist()
        if Q in (1, 2):
            row = [worst, best]
        out[r] = row[:max(Q, 1)]
    return out[:, :Q]


def run_ranks(c, query, mode, use_bias=True, use_scale=False, filters=3, scratch_bytes=None, hidden=None, hidden_row=None, hidden_ld=None,
              want=("ranks", "scores", "n", "member"), sync=True, outs=None, scratch=None, ex=None, row_filter=None, d=None):
    """b4r_item_ranks on the case; returns (rc, dict of numpy outputs incl. 8 sentinel elements behind each).  d: the inputs already
    on the device (a call inside a graph capture copies nothing)."""
    lib = _lib.load()
    R, H = c["hidden"].shape
    V = c["table"].shape[0]
    Q = query.shape[1]
    words = words_of(c, filters)
    ex = c["ex"] if ex is None else ex
    rf = (c["row_filter"] if row_filter is None else row_filter) if filters == 3 else None
    if d is None:
        d = dict(hidden=dev(c["hidden"] if hidden is None else hidden), table=dev(c["table"]), bias=dev(c["bias"]) if use_bias else None,
                 ex=dev(ex), words=None if words is None else dev(words.view(np.int32)), rf=dev(rf),
                 scale=dev(c["scale"]) if use_scale else None, q=dev(query), hr=dev(hidden_row, torch.int64))
    if outs is None:
        outs = dict(ranks=torch.full((R * Q + 8,), -7, dtype=torch.int32, device=DEV), scores=torch.full((R * Q + 8,), 7.0, device=DEV),
                    n=torch.full((R + 8,), -7, dtype=torch.int32, device=DEV), member=torch.full((R * Q + 8,), 9, dtype=torch.uint8, device=DEV))
    need = int(lib.b4r_item_ranks_scratch_bytes(R, V, Q))
    nbytes = need if scratch_bytes is None else scratch_bytes
    if scratch is None:
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    rc = lib.b4r_item_ranks(P(d["hidden"]), hidden_ld or H, P(d["hr"]), P(d["table"]), P(d["bias"]), H, V, FIRST, R, P(d["ex"]), ex.shape[1],
                            P(d["words"]), 0 if words is None else words.shape[0], P(d["rf"]), P(d["scale"]), P(d["q"]) if Q else None, Q, mode,
                            *(P(outs[k]) if k in want else None for k in ("ranks", "scores", "n", "member")), P(scratch), nbytes, stream())
    if not sync:
        return rc, outs, (d, scratch)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in outs.items()}


def split(got, R, Q):
    """(ranks [R, Q], scores, n [R], member) and whether the sentinels behind them stand"""
    tails = (got["ranks"][R * Q:] == -7).all() and (got["scores"][R * Q:] == 7.0).all() and (got["n"][R:] == -7).all() and \
        (got["member"][R * Q:] == 9).all()
    return got["ranks"][:R * Q].reshape(R, Q), got["scores"][:R * Q].reshape(R, Q), got["n"][:R], got["member"][:R * Q].reshape(R, Q), tails


def assert_equals_ref(c, query, mode, got, use_bias, use_scale, filters, what):
    R, H = c["hidden"].shape
    V, Q = c["table"].shape[0], query.shape[1]
    want = iref.item_ranks(scores_of(R, H, V, use_bias, use_scale), allowed_of(c, filters), query, FIRST, mode)
    ranks, scores, n, member, tails = split(got, R, Q)
    assert tails, what
    assert np.array_equal(ranks, want[0]), (what, "ranks")
    assert scores.tobytes() == want[1].tobytes(), (what, "query_scores")
    assert np.array_equal(n, want[2]), (what, "row_n")
    assert np.array_equal(member, want[3]), (what, "member")
    return want


@pytest.mark.parametrize("R,H,V,Q", SHAPES, ids=[f"R{s[0]}_H{s[1]}_V{s[2]}_Q{s[3]}" for s in SHAPES])
def test_item_ranks_bit_exact(R, H, V, Q):
    c = planted(R, H, V, 0)
    query = queries(R, H, V, Q)
    for use_bias, use_scale, filters in VARIANTS:
        for mode in MODES:
            rc, got = run_ranks(c, query, mode, use_bias, use_scale, filters)
            assert rc == 0, _lib.last_error()
            want = assert_equals_ref(c, query, mode, got, use_bias, use_scale, filters, (use_bias, use_scale, filters, mode))
            if mode == iref.STRICT and (use_bias, use_scale, filters) == (True, False, 3):
                kinds = c["kinds"]
                assert (want[2][kinds == 4] == 0).all() and (want[0][kinds == 4] == 0).all()          # the empty rows
                live = want[2] > 0
                b, w = (1, 0) if Q <= 2 else (0, 1)                                                    # the planted best and worst
                assert Q <= b or (want[0][live, b] == 1).all()
                assert Q <= w or (want[0][live, w] == want[2][live]).all()
    # hidden_row and hidden_ld > H: the rows live elsewhere in a padded buffer, in another order
    rng = np.random.default_rng(R)
    perm = rng.permutation(R) + 2
    wide = rng.standard_normal((R + 3, H + 8)).astype(F32)
    wide[perm, :H] = c["hidden"]
    for mode in MODES:
        rc, got = run_ranks(c, query, mode, hidden=wide, hidden_row=perm, hidden_ld=H + 8)
        assert rc == 0, _lib.last_error()
        assert_equals_ref(c, query, mode, got, True, False, 3, ("hidden_row", mode))


def rank_full_ex(c, gt, K, use_bias=True, use_scale=False, filters=3):
    lib = _lib.load()
    R, H = c["hidden"].shape
    V = c["table"].shape[0]
    words = words_of(c, filters)
    ids = torch.empty((R, max(K, 1)), dtype=torch.int64, device=DEV)
    scores = torch.empty((R, max(K, 1)), device=DEV)
    gt_rank = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    need = int(lib.b4r_rank_full_scratch_bytes(R, V, K))
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    keep = [dev(c["hidden"]), dev(c["table"]), dev(c["bias"]) if use_bias else None, dev(c["ex"]), dev(gt),
            None if words is None else dev(words.view(np.int32)), dev(c["row_filter"]) if filters == 3 else None,
            dev(c["scale"]) if use_scale else None]
    rc = lib.b4r_rank_full_ex(P(keep[0]), H, None, P(keep[1]), P(keep[2]), H, V, FIRST, R, P(keep[3]), c["ex"].shape[1], P(keep[4]), K,
                              P(ids) if K else None, P(scores) if K else None, P(gt_rank) if gt is not None else None, P(scratch), need,
                              stream(), P(keep[5]), 0 if words is None else words.shape[0], P(keep[6]), P(keep[7]))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return ids.cpu().numpy(), scores.cpu().numpy(), gt_rank.cpu().numpy()


@pytest.mark.parametrize("R,H,V,Q", [(17, 132, 1023, 15), (2, 64, 70000, 17)])
def test_self_mode_is_rank_full_ex_column_by_column(R, H, V, Q):
    c = planted(R, H, V, 0)
    query = queries(R, H, V, Q)
    for use_bias, use_scale, filters in ((True, False, 3), (False, True, 0)):
        rc, got = run_ranks(c, query, iref.SELF, use_bias, use_scale, filters)
        assert rc == 0, _lib.last_error()
        ranks = split(got, R, Q)[0]
        for i in range(Q):
            _, _, gt_rank = rank_full_ex(c, query[:, i].copy(), 0, use_bias, use_scale, filters)
            assert np.array_equal(ranks[:, i], gt_rank), (filters, i)


def test_top_k_fed_back_and_row_n_of_score_dist():
    R, H, V, K = 17, 132, 1023, 20
    c = planted(R, H, V, 0)
    for use_bias, use_scale, filters in VARIANTS[:2]:
        ids, top, _ = rank_full_ex(c, None, K, use_bias, use_scale, filters)
        rc, got = run_ranks(c, ids, iref.STRICT, use_bias, use_scale, filters)
        assert rc == 0, _lib.last_error()
        ranks, scores, n, member, tails = split(got, R, K)
        assert tails and np.array_equal(ranks, np.where(ids >= 0, np.arange(1, K + 1)[None, :], 0))
        assert scores.tobytes() == top.tobytes() and np.array_equal(member, (ids >= 0).astype(np.uint8))
        # b4r_score_dist without a ground truth counts the same allowed set
        rc, dist = run_dist(dict(c, gt=np.full(R, -1, np.int64)), 1.0, use_bias, use_scale, filters, query=None)
        assert rc == 0 and np.array_equal(n, dist["n"])


def test_one_joint_column_is_self():
    R, H, V = 16, 32, 33
    c = planted(R, H, V, 0)
    for col in range(12):
        query = c["query"][:, col:col + 1].copy()
        a = run_ranks(c, query, iref.JOINT)[1]
        b = run_ranks(c, query, iref.SELF)[1]
        assert np.array_equal(a["ranks"], b["ranks"]) and a["scores"].tobytes() == b["scores"].tobytes()
        assert np.array_equal(a["member"], b["member"])
        valid = (query[:, 0] >= FIRST) & (query[:, 0] < V)
        assert np.array_equal(a["n"][:R], b["n"][:R] + (valid & (a["member"][:R] == 0)))


def same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.mark.parametrize("mode", MODES)
def test_reproducible_graph_groups_and_row_order(mode):
    lib = _lib.load()
    R, H, V, Q = 33, 32, 2049, 256
    c = planted(R, H, V, 0)
    query = queries(R, H, V, Q)
    rc, first = run_ranks(c, query, mode)
    assert rc == 0 and same_bits(first, run_ranks(c, query, mode)[1])
    # a scratch for one group of 16 rows
    small = int(lib.b4r_item_ranks_scratch_bytes(16, V, Q))
    assert small < int(lib.b4r_item_ranks_scratch_bytes(R, V, Q))
    rc, grouped = run_ranks(c, query, mode, scratch_bytes=small)
    assert rc == 0 and same_bits(first, grouped)
    rc, untouched = run_ranks(c, query, mode, scratch_bytes=small // 2)
    assert rc == -5 and "b4r_item_ranks" in _lib.last_error()
    assert (untouched["ranks"] == -7).all() and (untouched["n"] == -7).all() and (untouched["member"] == 9).all()
    # the rows in another order
    perm = np.random.default_rng(5).permutation(R)
    rc, moved = run_ranks(c, query[perm], mode, hidden=c["hidden"][perm], ex=c["ex"][perm], row_filter=c["row_filter"][perm])
    assert rc == 0
    a, b = split(first, R, Q), split(moved, R, Q)
    for x, y in zip(a[:4], b[:4]):
        assert x[perm].tobytes() == y.tobytes()
    # NULL outputs: each alone, and the others untouched
    for only in ("ranks", "scores", "n", "member"):
        rc, got = run_ranks(c, query, mode, want=(only,))
        assert rc == 0 and got[only].tobytes() == first[only].tobytes()
        assert all((got[k] == s).all() for k, s in (("ranks", -7), ("scores", 7.0), ("n", -7), ("member", 9)) if k != only)
    # a captured graph, replayed twice
    rc, outs, keep = run_ranks(c, query, mode, sync=False)
    torch.cuda.synchronize()
    for t in outs.values():
        t.fill_(3)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            rc2, _, _ = run_ranks(c, query, mode, sync=False, outs=outs, scratch=keep[1], d=keep[0])
    torch.cuda.current_stream().wait_stream(side)
    assert rc2 == 0
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    replayed = {k: v.cpu().numpy() for k, v in outs.items()}
    for k in first:
        n = R if k == "n" else R * Q
        assert replayed[k][:n].tobytes() == first[k][:n].tobytes(), k


# ---- b4r_rank_metrics_multi -----------------------------------------------------------------------------------------------------------
TABLE = [(iref.COUNT, 0), (iref.MRR, 0), (iref.AUC, 0)] + [(f, k) for k in (1, 5, 10, 300) for f in (iref.HIT, iref.NDCG, iref.RECALL, iref.MAP)]


def metric_case(R, Q, seed):
    """distinct ranks per row in [1, 400], about a third of the entries 0, some rows without a target"""
    rng = np.random.default_rng(seed)
    ranks = np.stack([rng.permutation(400)[:Q] + 1 for _ in range(R)]).astype(np.int32)
    ranks[rng.random((R, Q)) < 0.35] = 0
    ranks[::7] = 0
    ranks[0, 0] = 1
    row_n = (rng.integers(0, 50, size=R) + 400).astype(np.int32)
    if R > 3:
        ranks[3] = 0; ranks[3, :min(Q, 2)] = [1, 2][:min(Q, 2)]; row_n[3] = min(Q, 2)      # nothing but targets: AUC = 1
    return ranks, row_n


def run_metrics(ranks, row_n, table, sums=None, users=None):
    lib = _lib.load()
    fam = (C.c_int32 * len(table))(*[f for f, _ in table])
    cut = (C.c_int32 * len(table))(*[k for _, k in table])
    sums = torch.zeros(len(table), dtype=torch.float64, device=DEV) if sums is None else sums
    users = torch.zeros(1, dtype=torch.int64, device=DEV) if users is None else users
    r_d, n_d = dev(ranks), dev(row_n)
    rc = lib.b4r_rank_metrics_multi(P(r_d), P(n_d), ranks.shape[0], ranks.shape[1], fam, cut, len(table), P(sums), P(users), stream())
    torch.cuda.synchronize()
    return rc, sums, users


@pytest.mark.parametrize("R,Q", [(1, 1), (5, 2), (256, 16), (257, 7), (300, 16)])
def test_rank_metrics_multi(R, Q):
    ranks, row_n = metric_case(R, Q, R + Q)
    rc, sums, users = run_metrics(ranks, row_n, TABLE)
    assert rc == 0, _lib.last_error()
    want, rows = iref.multi_metrics(ranks, row_n, TABLE)
    assert int(users[0]) == rows
    got = sums.cpu().tolist()
    for (fam, k), g, w in zip(TABLE, got, want):
        print(f"family {fam} @ {k}: {g!r} against {w!r}")
        assert g == pytest.approx(w, rel=1e-12, abs=0), (fam, k)
    # a second call accumulates; without row_n everything but AUC
    ranks2, row_n2 = metric_case(R, Q, R + Q + 1)
    rc, sums, users = run_metrics(ranks2, row_n2, TABLE, sums, users)
    want2, rows2 = iref.multi_metrics(ranks2, row_n2, TABLE)
    assert rc == 0 and int(users[0]) == rows + rows2
    for g, w, w2 in zip(sums.cpu().tolist(), want, want2):
        assert g == pytest.approx(w + w2, rel=1e-12, abs=0)
    no_auc = [t for t in TABLE if t[0] != iref.AUC]
    rc, s3, _ = run_metrics(ranks, None, no_auc)
    assert rc == 0 and s3.cpu().tolist() == [g for t, g in zip(TABLE, got) if t[0] != iref.AUC]      # the same order of additions
    rc, _, _ = run_metrics(ranks, None, TABLE)
    assert rc == -1 and "AUC" in _lib.last_error()


def test_rank_metrics_multi_with_one_column_is_rank_metrics():
    lib = _lib.load()
    R = 300
    ranks, _ = metric_case(R, 1, 11)
    single = [(0, 0), (1, 1), (1, 10), (2, 5), (2, 10), (3, 0)]                                       # b4r_rank_metrics' families
    rc, sums, users = run_metrics(ranks, None, single)
    assert rc == 0
    fam = (C.c_int32 * len(single))(*[f for f, _ in single])
    cut = (C.c_int32 * len(single))(*[k for _, k in single])
    s1 = torch.zeros(len(single), dtype=torch.float64, device=DEV)
    u1 = torch.zeros(1, dtype=torch.int64, device=DEV)
    r_d = dev(ranks.reshape(-1))
    assert lib.b4r_rank_metrics(P(r_d), R, fam, cut, len(single), P(s1), P(u1), stream()) == 0
    torch.cuda.synchronize()
    assert int(users[0]) == int(u1[0]) == int((ranks > 0).sum())
    for a, b in zip(sums.cpu().tolist(), s1.cpu().tolist()):
        assert a == pytest.approx(b, rel=1e-12, abs=0)


# ---- the model, the app and the evaluator -----------------------------------------------------------------------------------------------
def app_batch(rec, items, spans=((0, 15), (40, 3), (90, 30), (7, 22))):
    batches = [rec.dataloader.prepare_inference(list(items[s:s + n])) for s, n in spans]
    return {key: torch.from_numpy(np.concatenate([np.asarray(b[key]) for b in batches], axis=0)) for key in batches[0]}


@pytest.mark.parametrize("factorised", [False, True], ids=["hidden64", "hidden128"])
def test_item_ranks_tensor_is_the_position_in_recommend_tensor(factorised):
    rec, items = small_app(factorised)
    model, V = rec.model, rec.model.vocab_size
    assert V <= 1024
    batch = app_batch(rec, items)
    ids, scores, slots = model.recommend_tensor(batch, k=1024)[:3]
    ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
    R = ids.shape[0]
    query = np.tile(np.arange(-1, V + 1, dtype=np.int64), (R, 1))                     # every id, and one on each side
    got = model.item_ranks_tensor(batch, query)
    assert torch.equal(got["slot_index"], slots)
    ranks, sc, n, member = (got[k].cpu().numpy() for k in ("ranks", "scores", "n", "member"))
    seen = batch["input_word_ids"].numpy()
    for r in range(R):
        live = ids[r][ids[r] >= 0]
        assert n[r] == live.size
        want = np.zeros(V + 2, np.int64)
        want[live + 1] = np.arange(1, live.size + 1)
        assert np.array_equal(ranks[r], want)
        assert sc[r][live + 1].tobytes() == scores[r][:live.size].tobytes()
        assert np.array_equal(member[r], (want > 0).astype(np.uint8))
        assert (ranks[r][np.unique(seen[r]) + 1] == 0).all() and (member[r][np.unique(seen[r]) + 1] == 0).all()
    # [Q] for all slots; "self" ranks the seen items too; 300 columns = the composition of two blocks
    flat = model.item_ranks_tensor(batch, query[0])
    assert torch.equal(flat["ranks"], got["ranks"]) and torch.equal(flat["n"], got["n"])
    wide = np.random.default_rng(1).integers(-2, V + 2, size=(R, 300)).astype(np.int64)
    for members in ("strict", "self"):
        whole = model.item_ranks_tensor(batch, wide, members=members)
        parts = [model.item_ranks_tensor(batch, wide[:, a:b], members=members) for a, b in ((0, 256), (256, 300))]
        for k in ("ranks", "scores", "member"):
            assert torch.equal(whole[k], torch.cat([p[k] for p in parts], dim=1)), (members, k)
        assert torch.equal(whole["n"], parts[0]["n"]) and whole["ranks"].shape == (R, 300)
    own = model.item_ranks_tensor(batch, seen[:, :5], members="self")
    valid = torch.as_tensor(seen[:, :5] >= 3)
    assert bool((own["ranks"].cpu()[valid] > 0).all()) and int(own["member"].sum()) == 0
    with pytest.raises(ValueError):
        model.item_ranks_tensor(batch, wide, members="joint")
    with pytest.raises(ValueError):
        model.item_ranks_tensor(batch, query[:2])
    one = {k: v[:1] for k, v in batch.items()}
    ids1, scores1 = (t.cpu().numpy() for t in model.recommend_tensor(one, k=5)[:2])    # (a one-row forward of its own)
    listed = model.item_ranks(one, [int(ids1[0, 0]), int(ids1[0, 4]), int(seen[0, 0]), -1])
    assert [e["rank"] for e in listed] == [1, 5, None, None] and {e["of"] for e in listed} == {int(n[0])}
    assert listed[0]["score"] == float(scores1[0, 0]) and listed[3]["score"] == -np.inf


def test_recommender_item_ranks_agrees_with_recommend_batch():
    rec, items = small_app()
    V = rec.model.vocab_size
    histories = [items[s:s + n] for s, n in ((0, 15), (40, 3), (90, 30), (120, 1), (7, 22))]
    everything = rec.recommend_batch(histories, k=V - 3)
    asked = [everything[0][0], everything[0][9], histories[0][0], "no such item", everything[1][-1]]
    got = rec.item_ranks(histories, items=asked)
    assert rec.dataloader.get_tokenizer().get_vocab_size() == V                        # the unknown item was not added
    for full, hist, row in zip(everything, histories, got):
        assert [e["item"] for e in row] == asked and {e["of"] for e in row} == {len(full)}
        for e in row:
            if e["item"] == "no such item":
                assert e["rank"] is None and e["score"] is None
            elif e["item"] in hist:
                assert e["rank"] is None and np.isfinite(e["score"])
            else:
                assert e["rank"] == full.index(e["item"]) + 1
    per_user = [[full[2], full[0]] for full in everything]
    got = rec.item_ranks(histories, items_per_user=per_user)
    assert [[e["rank"] for e in row] for row in got] == [[3, 1]] * len(histories)
    allowed = items[::3]
    filtered = rec.recommend_batch(histories, k=V - 3, allowed_items=allowed)
    outside = next(i for i in items if i not in set(allowed))
    got = rec.item_ranks(histories, items=[filtered[0][1], outside], allowed_items=allowed)
    assert got[0][0]["rank"] == 2 and got[0][0]["of"] == len(filtered[0]) and all(row[1]["rank"] is None for row in got)
    assert rec.item_ranks([], items=asked) == []


def test_evaluator_multi_target():
    rec, items = small_app()
    model, dl = rec.model, rec.dataloader
    seqs = [items[s:s + n] for s, n in ((0, 15), (40, 3), (90, 30), (120, 2), (7, 22), (60, 6), (150, 9))]
    seqs.append(items[20:25] + [items[21], items[21], "no such item"])               # a repeated and an unknown target
    batches, skipped = evaluation.next_n_batches(dl, seqs, 3, batch_size=3)
    assert skipped == 2 and sum(b["target_ids"].shape[0] for b in batches) == 6
    ev = evaluation.get(full_ranking=True, multi_target=True)
    ev.evaluate(model, batches)
    got = ev.get_metrics_results()
    table, all_ranks, all_n = [(f, k) for _, f, k in ev._mt_table], [], []
    for b in batches:
        t = b["target_ids"].copy()
        for row in t:
            for j in range(len(row)):
                if row[j] in row[:j].tolist():
                    row[j] = -1
        out = model.item_ranks_tensor({k: torch.as_tensor(v) for k, v in b.items() if k != "target_ids"}, t, exclude_seen=False,
                                      exclude=torch.as_tensor(b["labels"]), members="joint")
        all_ranks.append(out["ranks"].cpu().numpy()); all_n.append(out["n"].cpu().numpy())
    ranks, row_n = np.concatenate(all_ranks), np.concatenate(all_n)
    assert (ranks[-1] > 0).sum() == 1                                                 # the repeated id once, the unknown one not at all
    want, rows = iref.multi_metrics(ranks, row_n, table)
    assert rows == 6
    for (name, fam, _), w in zip(ev._mt_table, want):
        assert got[name] == pytest.approx(w if fam == iref.COUNT else w / rows, rel=1e-12, abs=0), name
    assert got["Valid Ranks"] == int((ranks > 0).sum()) and 0.0 <= got["AUC"] <= 1.0 and got["Recall@10"] >= got["Recall@1"]
    ev.reset_metrics()
    assert ev.multi_target_results()["Valid Ranks"] == 0
    # n = 1: the single-target full-ranking evaluator on the same users
    long = [s for s in seqs[:-1] if len(s) > 1]
    one, _ = evaluation.next_n_batches(dl, long, 1, batch_size=4)
    ev.evaluate(model, one)
    multi = ev.get_metrics_results()
    dl._set_preprocessor_properties()
    rows = [dl.preprocessor.process_element(list(s), True, True) for s in long]
    loo = [{k: torch.as_tensor(np.stack([r[k] for r in rows[i:i + 4]])) for k in rows[0]} for i in range(0, len(rows), 4)]
    single = evaluation.get(full_ranking=True)
    single.evaluate(model, loo)
    base = single.get_metrics_results()
    for k in (1, 5, 10):
        assert multi[f"HR@{k}"] == pytest.approx(base[f"HR@{k}"], rel=1e-12, abs=0)
        assert multi[f"NDCG@{k}"] == pytest.approx(base[f"NDCG@{k}"], rel=1e-12, abs=0)
        assert multi[f"Recall@{k}"] == multi[f"HR@{k}"]
    assert multi["MRR"] == pytest.approx(base["MAP"], rel=1e-12, abs=0) and multi["Valid Ranks"] == base["Valid Ranks"] == len(long)
    bad = dict(one[0])
    bad["masked_lm_weights"] = np.ones_like(bad["masked_lm_weights"])
    with pytest.raises(ValueError, match="one ranked slot"):
        ev.evaluate_batch(model, bad)
    with pytest.raises(ValueError, match="target_ids"):
        ev.evaluate_batch(model, {k: v for k, v in one[0].items() if k != "target_ids"})
