"""Catalogue softmax on the GPU (b4r_score_dist): the op against the CPU restatement (tests/score_dist_ref.py) and the model /
app / evaluator layers built on it.

Bit-exact against the restatement: row_n, row_max (-0.0 taken as +0.0), the -inf entries of query_logp, and query_logp =
fl32((double) t - row_lse) given the device's own row_lse; row_max also equals fl32(top score * inv_temperature) of b4r_rank_full_ex
on the same inputs.  row_lse and row_entropy are held against the plain fp64 version within the derived tolerances (score_dist_ref:
tol_lse = 2^-21 + 2^-24 ln n, tol_entropy = 2^-21 (1 + 2 ln n) + 2^-24 (ln n + ln^2 n)); each test prints the largest distance it saw
as a share of the tolerance.

The shapes reach the sweep's boundaries: 16 rows per group (R = 1, 5, 16, 17, 33), 1024 ids per chunk (V = 4, 33, 1023, 1024, 1025,
2049, 3000, 70000), the 16-float k-block and H % 4 (H = 4, 32, 64, 128, 132, 1024).  Every shape plants, by row: a flat row, a peaked
row (hidden x 200: every other term underflows), a zero hidden row, a row under a one-bit filter, an empty row (a filter of zeros and
no ground truth), a row whose first chunk (or lower half, when V <= 1024) holds nothing allowed; twin table rows come with
make_case.  Shapes with fewer than 6 rows are run at several offsets of the row kinds so that each kind is met."""
import functools

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, dataloaders, datasets, evaluation
from bert4rec_amd.apps import Recommender, pack_item_groups
from oracle import bert4rec_oracle as orc
from tests import catalogue_ref as ref
from tests import score_dist_ref as sref
from tests.b4r_testlib import P, stream
from tests.test_gpu_api import make_model
from tests.test_gpu_full_rank import make_case

pytestmark = pytest.mark.gpu

DEV = "cuda"
FIRST = 3
F32 = np.float32
KINDS = 6   # flat, peaked, zero, one-bit, empty, empty chunk
SHAPES = [(1, 4, 4), (5, 32, 33), (17, 64, 1023), (16, 64, 1024), (33, 128, 1025), (3, 132, 2049), (2, 1024, 3000), (2, 64, 70000)]


def one_bit_id(V):
    return min(V - 1, 1030)


@functools.lru_cache(maxsize=None)
def planted(R, H, V, offset):
    """make_case's inputs with the planted rows: kind(r) = (r + offset) % 6.  Three filters: 0 = one bit, 1 = zeros, 2 = a random
    90 % with the first chunk (the lower half when V <= 1024) cleared; row_filter names them, or an index outside [0, 3)."""
    hidden, table, bias, ex, gt = make_case(R, H, V, seed=R * 31 + H + V % 97 + offset, E=12)
    hidden, table, bias = hidden.numpy().copy(), table.numpy().copy(), bias.numpy().copy()
    rng = np.random.default_rng(V + offset)
    cut = 1024 if V > 1024 else V // 2
    masks = np.zeros((3, V), bool)
    masks[0, one_bit_id(V)] = True
    masks[2] = rng.random(V) < 0.9
    masks[2, :cut] = False
    masks[2, V - 1] = True
    row_filter = np.zeros(R, np.int32)
    kinds = (np.arange(R) + offset) % KINDS
    for r, kind in enumerate(kinds.tolist()):
        if kind == 0:
            row_filter[r] = 3
        elif kind == 1:
            hidden[r] *= 200.0
            row_filter[r] = -1
        elif kind == 2:
            hidden[r] = 0.0
            row_filter[r] = 2
        elif kind == 3:
            row_filter[r] = 0
            gt[r] = one_bit_id(V)          # listed or not, the ground truth stays allowed: exactly one item
        elif kind == 4:
            row_filter[r] = 1
            gt[r] = -1
        else:
            row_filter[r] = 2
            gt[r] = V - 1
    scale = (0.5 + np.random.default_rng(V + 1).random(V)).astype(F32)
    query = np.zeros((R, 12), np.int64)
    for r in range(R):
        out = np.flatnonzero(~masks[2])
        query[r] = [gt[r], ex[r, 0], out[min(len(out) - 1, 5)], 1, -1, V, 1 << 40, -(1 << 40), one_bit_id(V), V - 1,
                    rng.integers(0, V), rng.integers(FIRST, V)]
    return dict(hidden=hidden, table=table, bias=bias, ex=ex, gt=gt, masks=masks, words=ref.pack_bits(masks), row_filter=row_filter,
                kinds=kinds, scale=scale, query=query, one=ref.pack_bits(masks[2:3]))


@functools.lru_cache(maxsize=None)
def chain(R, H, V, offset, use_bias):
    c = planted(R, H, V, offset)
    return ref.chain_scores(c["hidden"], c["table"], c["bias"] if use_bias else None)


def dev(x, dtype=None):
    if x is None:
        return None
    t = torch.as_tensor(x)
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def run_dist(c, inv_t=1.0, use_bias=True, use_scale=False, filters=3, query=True, scratch_bytes=None, hidden=None, hidden_row=None,
             hidden_ld=None, K=None, sync=True, outs=None, scratch=None):
    """b4r_score_dist on the case; returns (rc, dict of numpy outputs).  The outputs start from sentinels."""
    lib = _lib.load()
    R, H = c["hidden"].shape
    V = c["table"].shape[0]
    words = {0: None, 1: c["one"], 3: c["words"]}[filters]
    q = c["query"] if query is True else query
    K = (0 if q is None else q.shape[1]) if K is None else K
    d = dict(hidden=dev(c["hidden"] if hidden is None else hidden), table=dev(c["table"]), bias=dev(c["bias"]) if use_bias else None,
             ex=dev(c["ex"]), gt=dev(c["gt"]), words=None if words is None else dev(words.view(np.int32)),
             rf=dev(c["row_filter"]) if filters == 3 else None, scale=dev(c["scale"]) if use_scale else None, q=dev(q),
             hr=dev(hidden_row, torch.int64))
    if outs is None:
        outs = dict(n=torch.full((R,), -7, dtype=torch.int32, device=DEV), max=torch.full((R,), 7.0, device=DEV),
                    lse=torch.full((R,), 7.0, dtype=torch.float64, device=DEV), ent=torch.full((R,), 7.0, dtype=torch.float64, device=DEV),
                    logp=torch.full((R, max(K, 1)), 7.0, device=DEV))
    need = int(lib.b4r_score_dist_scratch_bytes(R, V))
    nbytes = need if scratch_bytes is None else scratch_bytes
    if scratch is None:
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    rc = lib.b4r_score_dist(P(d["hidden"]), hidden_ld or H, P(d["hr"]), P(d["table"]), P(d["bias"]), H, V, FIRST, R, P(d["ex"]),
                            c["ex"].shape[1], P(d["gt"]), P(d["words"]), 0 if words is None else words.shape[0], P(d["rf"]),
                            P(d["scale"]), inv_t, P(d["q"]), K, P(outs["n"]), P(outs["max"]), P(outs["lse"]), P(outs["ent"]),
                            P(outs["logp"]) if K > 0 else None, P(scratch), nbytes, stream())
    if not sync:
        return rc, outs, (d, scratch)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in outs.items()}


def untouched(got):
    return (got["n"] == -7).all() and all((got[k] == 7.0).all() for k in ("max", "lse", "ent", "logp"))


def same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def top_scores(c, use_bias, use_scale, filters):
    """topk_scores[:, 0] of b4r_rank_full_ex on the same inputs"""
    lib = _lib.load()
    R, H = c["hidden"].shape
    V = c["table"].shape[0]
    words = {0: None, 1: c["one"], 3: c["words"]}[filters]
    ids = torch.empty((R, 1), dtype=torch.int64, device=DEV)
    scores = torch.empty((R, 1), device=DEV)
    need = int(lib.b4r_rank_full_scratch_bytes(R, V, 1))
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    keep = [dev(c["hidden"]), dev(c["table"]), dev(c["bias"]) if use_bias else None, dev(c["ex"]), dev(c["gt"]),
            None if words is None else dev(words.view(np.int32)), dev(c["row_filter"]) if filters == 3 else None,
            dev(c["scale"]) if use_scale else None]
    rc = lib.b4r_rank_full_ex(P(keep[0]), H, None, P(keep[1]), P(keep[2]), H, V, FIRST, R, P(keep[3]), c["ex"].shape[1], P(keep[4]), 1,
                              P(ids), P(scores), None, P(scratch), need, stream(), P(keep[5]), 0 if words is None else words.shape[0],
                              P(keep[6]), P(keep[7]))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return scores[:, 0].cpu().numpy()


def check_against_ref(c, key, got, inv_t, use_bias, use_scale, filters, worst):
    """Every assertion on one call's outputs; worst: [lse, entropy] largest share of the tolerance so far."""
    R, H = c["hidden"].shape
    V = c["table"].shape[0]
    t = (ref.scaled(chain(*key, use_bias), c["scale"] if use_scale else None).astype(F32) * F32(inv_t)).astype(F32)
    words = {0: None, 1: c["one"], 3: c["words"]}[filters]
    ok = ref.allowed_mask(V, FIRST, c["ex"], c["gt"], R, words, c["row_filter"] if filters == 3 else None)
    n_b, max_b, lse_b, ent_b = sref.blocked(t, ok)
    n_p, lse_p, ent_p = sref.plain(t, ok)
    assert np.array_equal(got["n"], n_b) and np.array_equal(n_b, n_p), "row_n"
    assert np.array_equal((got["max"] + F32(0.0)).view(np.uint32), (max_b + F32(0.0)).view(np.uint32)), "row_max not bit-identical"
    live = n_p > 0
    assert (got["lse"][~live] == -np.inf).all() and (got["ent"][~live] == 0.0).all() and (got["max"][~live] == -np.inf).all()
    assert not np.isnan(got["lse"]).any() and not np.isnan(got["ent"]).any() and not np.isnan(got["logp"]).any()
    d_lse = np.abs(got["lse"][live] - lse_p[live]) / sref.tol_lse(n_p[live])
    d_ent = np.abs(got["ent"][live] - ent_p[live]) / sref.tol_entropy(n_p[live])
    if live.any():
        worst[0], worst[1] = max(worst[0], float(d_lse.max())), max(worst[1], float(d_ent.max()))
        if len(worst) > 2:
            worst[2] = max(worst[2], float(np.abs(got["lse"][live] - lse_p[live]).max()))
            worst[3] = max(worst[3], float(np.abs(got["ent"][live] - ent_p[live]).max()))
        assert d_lse.max() <= 1.0, f"row_lse: {d_lse.max()} of the tolerance"
        assert d_ent.max() <= 1.0, f"row_entropy: {d_ent.max()} of the tolerance"
    has_q = got["logp"].shape[1] == c["query"].shape[1]
    if has_q:
        want = sref.query_logp(t, ok, got["lse"], c["query"])
        assert np.array_equal(np.isneginf(got["logp"]), np.isneginf(want)), "-inf entries"
        assert np.array_equal(got["logp"].view(np.uint32), want.view(np.uint32)), "query_logp is not fl32(t - lse)"
        assert np.isneginf(got["logp"][:, 3:8]).all()                      # a special id, -1, V, 2^40, -2^40
    for r, kind in enumerate(c["kinds"].tolist()):
        if filters == 3 and kind == 3:                                     # one allowed item
            tq = float(t[r, one_bit_id(V)])
            assert got["n"][r] == 1 and got["lse"][r] == tq and got["ent"][r] == 0.0 and (not has_q or got["logp"][r, 8] == 0.0)
        if filters == 3 and kind == 4:
            assert got["n"][r] == 0 and (not has_q or np.isneginf(got["logp"][r]).all())
        if filters == 3 and kind == 5:
            cut = 1024 if V > 1024 else V // 2
            assert not ok[r, :cut].any()                                   # the chunk (or half) with nothing allowed
        if kind == 2 and not use_bias and live[r]:                         # zero hidden row, no bias: the uniform distribution
            ln = np.log(float(n_p[r]))
            assert got["lse"][r] == pytest.approx(ln, rel=1e-15, abs=1e-300) and got["ent"][r] == pytest.approx(ln, rel=1e-15, abs=1e-300)
    return t, ok


# (inv_temperature, bias, item_scale, filters): every value of each at least once; the planted filters in the first two
CALLS = [(1.0, True, False, 3), (0.25, False, True, 3), (4.0, False, False, 1), (1.0, True, True, 0)]


@pytest.mark.parametrize("R,H,V", SHAPES, ids=[f"R{s[0]}_H{s[1]}_V{s[2]}" for s in SHAPES])
def test_score_dist_against_the_restatement(R, H, V):
    worst = [0.0, 0.0, 0.0, 0.0]
    for offset in (range(0, KINDS, R) if R < KINDS else (0,)):
        key = (R, H, V, offset)
        c = planted(*key)
        for i, (inv_t, use_bias, use_scale, filters) in enumerate(CALLS):
            rc, got = run_dist(c, inv_t, use_bias, use_scale, filters)
            assert rc == 0, _lib.last_error()
            check_against_ref(c, key, got, inv_t, use_bias, use_scale, filters, worst)
            if i < 2:
                top = top_scores(c, use_bias, use_scale, filters)
                want = (top * F32(inv_t)).astype(F32)
                assert np.array_equal((got["max"] + F32(0.0)).view(np.uint32), (want + F32(0.0)).view(np.uint32)), "row_max vs the sweep's top score"
            if i == 0:
                rc, again = run_dist(c, inv_t, use_bias, use_scale, filters)
                assert rc == 0 and same_bits(got, again), "two calls differ"
            if i == 3:                                                     # K = 0 with query_ids NULL: the row outputs alone
                rc, bare = run_dist(c, inv_t, use_bias, use_scale, filters, query=None)
                assert rc == 0 and all(bare[k].tobytes() == got[k].tobytes() for k in ("n", "max", "lse", "ent"))
                assert (bare["logp"] == 7.0).all()
    print(f"R={R} H={H} V={V}: lse {worst[0]:.4f}, entropy {worst[1]:.4f} of the tolerance (largest distances {worst[2]:.3g}, {worst[3]:.3g})")


def test_grouped_rows_ld_and_hidden_row():
    """R = 40 with a scratch for 16 rows: three groups, the same bits; a hidden_ld > H with hidden_row: the same bits."""
    lib = _lib.load()
    key = (40, 64, 1500, 0)
    c = planted(*key)
    worst = [0.0, 0.0]
    rc, full = run_dist(c, 1.0, True, False, 3)
    assert rc == 0, _lib.last_error()
    check_against_ref(c, key, full, 1.0, True, False, 3, worst)
    small = int(lib.b4r_score_dist_scratch_bytes(16, 1500))
    assert small < int(lib.b4r_score_dist_scratch_bytes(40, 1500))
    rc, grouped = run_dist(c, 1.0, True, False, 3, scratch_bytes=small)
    assert rc == 0 and same_bits(full, grouped)
    rc, grouped = run_dist(c, 1.0, True, False, 3, scratch_bytes=small + int(lib.b4r_score_dist_scratch_bytes(16, 1500)) // 2)
    assert rc == 0 and same_bits(full, grouped)
    ld = 64 + 4
    wide = np.zeros((40 + 2, ld), F32)
    perm = np.random.default_rng(1).permutation(42)[:40]
    wide[perm, :64] = c["hidden"]
    rc, moved = run_dist(c, 1.0, True, False, 3, hidden=wide, hidden_row=perm, hidden_ld=ld)
    assert rc == 0 and same_bits(full, moved)
    print(f"R=40 H=64 V=1500: lse {worst[0]:.4f}, entropy {worst[1]:.4f} of the tolerance")


def test_all_ids_queried_sum_to_one():
    V = 300
    key = (7, 64, V, 0)
    c = planted(*key)
    query = np.tile(np.arange(V, dtype=np.int64), (7, 1))
    for inv_t, filters in ((1.0, 3), (4.0, 0)):
        rc, got = run_dist(c, inv_t, True, False, filters, query=query)
        assert rc == 0, _lib.last_error()
        t, ok = check_against_ref(c, key, got, inv_t, True, False, filters, [0.0, 0.0])
        lp = got["logp"]
        assert np.array_equal(np.isfinite(lp), ok)
        want = sref.query_logp(t, ok, got["lse"], query)
        assert np.array_equal(lp.view(np.uint32), want.view(np.uint32))
        live = got["n"] > 0
        total = np.exp(lp.astype(np.float64)).sum(axis=1)
        bound = sref.tol_lse(got["n"]) + 2.0 ** -24 * np.abs(np.where(ok, lp, 0.0)).max(axis=1)
        assert (np.abs(total[live] - 1.0) <= bound[live]).all(), np.abs(total[live] - 1.0).max()
        assert (total[~live] == 0.0).all()


def test_argument_errors_leave_the_outputs_untouched():
    lib = _lib.load()
    c = planted(20, 64, 1500, 0)
    for inv_t in (0.0, -1.0, float("nan"), float("inf")):
        rc, got = run_dist(c, inv_t)
        assert rc == -1 and "inv_temperature" in _lib.last_error() and untouched(got)
    rc, got = run_dist(c, K=1025)
    assert rc == -2 and untouched(got)
    small = int(lib.b4r_score_dist_scratch_bytes(16, 1500))
    for nbytes in (small // 2, 0):
        rc, got = run_dist(c, scratch_bytes=nbytes)
        assert rc == -5 and "b4r_score_dist" in _lib.last_error() and untouched(got)


def test_graph_capture_replays_the_eager_bits():
    c = planted(20, 64, 1500, 0)
    rc, eager = run_dist(c, 0.25, True, True, 3)
    assert rc == 0, _lib.last_error()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        rc, outs, keep = run_dist(c, 0.25, True, True, 3, sync=False)    # allocations and copies outside the capture
        assert rc == 0
        torch.cuda.synchronize()
        for v in outs.values():
            v.fill_(7)
        outs["n"].fill_(-7)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            lib = _lib.load()
            d, scratch = keep
            R, H = c["hidden"].shape
            V = c["table"].shape[0]
            rc = lib.b4r_score_dist(P(d["hidden"]), H, None, P(d["table"]), P(d["bias"]), H, V, FIRST, R, P(d["ex"]), c["ex"].shape[1],
                                    P(d["gt"]), P(d["words"]), 3, P(d["rf"]), P(d["scale"]), 0.25, P(d["q"]), c["query"].shape[1],
                                    P(outs["n"]), P(outs["max"]), P(outs["lse"]), P(outs["ent"]), P(outs["logp"]), P(scratch),
                                    scratch.numel(), stream())
            assert rc == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert (outs["n"] == -7).all(), "a capture must not run the kernels"
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(eager, {k: v.cpu().numpy() for k, v in outs.items()})


# ---- layers ---------------------------------------------------------------------------------------------------------------------
def test_model_layers_against_the_op():
    V = 300
    model = make_model(V, seed=17)
    batch = orc.synthetic_batch(48, 24, 6, V, seed=9, ragged=True)
    hidden, slots, _ = model._ranked_slot_hidden(batch)
    R = int(slots.numel())
    b_idx = (slots // 6).cpu()
    seen = batch["input_word_ids"][b_idx]
    rng = np.random.default_rng(2)
    query = torch.as_tensor(rng.integers(-2, V + 2, size=(R, 5)))
    allow = torch.as_tensor(rng.random(V) < 0.8)
    for kw, op_allow in ((dict(), None), (dict(allow=allow, temperature=2.0), allow)):
        got = model.score_distribution_tensor(batch, query_ids=query, **kw)
        assert set(got) == {"n", "lse", "entropy", "perplexity", "logp", "slot_index"} and torch.equal(got["slot_index"], slots)
        n, _, lse, ent, logp = model.engine.score_distribution(hidden, None, seen, FIRST, None, op_allow, None, kw.get("temperature", 1.0), query)
        assert torch.equal(got["n"], n) and torch.equal(got["lse"], lse) and torch.equal(got["entropy"], ent)
        assert torch.equal(got["logp"].view(torch.int32), logp.view(torch.int32)) and torch.equal(got["perplexity"], torch.exp(ent))
        # against the restatement on the transform's rows
        eng = model.engine
        t = sref.scaled_scores(hidden.cpu().numpy(), eng.view("word_embeddings/embeddings").cpu().numpy(),
                               eng.view("cls/predictions/output_bias/bias").cpu().numpy(), None, 1.0 / kw.get("temperature", 1.0))
        words = None if op_allow is None else ref.pack_bits(op_allow.numpy())
        ok = ref.allowed_mask(V, FIRST, seen.numpy(), None, R, words, None)
        n_p, lse_p, ent_p = sref.plain(t, ok)
        assert np.array_equal(n.cpu().numpy(), n_p)
        assert (np.abs(lse.cpu().numpy() - lse_p) <= sref.tol_lse(n_p)).all() and (np.abs(ent.cpu().numpy() - ent_p) <= sref.tol_entropy(n_p)).all()
        want = sref.query_logp(t, ok, lse.cpu().numpy(), query.numpy())
        assert np.array_equal(logp.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert model.score_distribution_tensor(batch)["logp"] is None
    # recommend_tensor: ids and scores keep their bits; logp is the op's, queried with the ids returned
    groups = pack_item_groups(np.arange(V) % 7, 2)
    for kw in (dict(), dict(allow=allow), dict(diversity=0.3), dict(max_per_group=groups), dict(allow=allow, diversity=0.5, max_per_group=groups)):
        ids0, sc0, slots0 = model.recommend_tensor(batch, k=10, **kw)
        for temp in (1.0, 0.5):
            ids, sc, slots1, dist = model.recommend_tensor(batch, k=10, return_distribution=True, temperature=temp, **kw)
            assert torch.equal(ids, ids0) and torch.equal(sc.view(torch.int32), sc0.view(torch.int32)) and torch.equal(slots1, slots0)
            _, _, lse, ent, logp = model.engine.score_distribution(hidden, None, seen, FIRST, None, kw.get("allow"), None, temp, ids)
            assert torch.equal(dist["logp"].view(torch.int32), logp.view(torch.int32)) and torch.equal(dist["lse"], lse)
            assert dist["logp"].shape == (R, 10) and torch.equal(torch.isfinite(dist["logp"]), ids >= 0)
            if not kw and temp == 1.0:                                     # the plain top k: log p falls with the score
                lp = dist["logp"].cpu().numpy().astype(np.float64)
                assert (np.diff(lp, axis=1) <= 0).all() and (np.exp(lp).sum(axis=1) <= 1.0 + 1e-6).all()
    lists, dist = model.recommend(batch, k=10, return_distribution=True)
    assert sum(len(x) for x in lists) == R and len(lists[int(b_idx[0])][0]) == 3
    assert lists[int(b_idx[0])][0][2] == dist["logp"][0].cpu().tolist()
    assert model.recommend(batch, k=10) == [[(i, s) for i, s, _ in row] for row in lists]
    with pytest.raises(ValueError, match="return_distribution"):
        model.recommend_tensor(batch, k=10, temperature=2.0)


def test_recommend_batch_probabilities():
    ds = datasets.synthetic_dataset(n_users=30, n_items=200, min_len=5, max_len=30, seed=4)
    dl = dataloaders.get_dataloader_factory("bert4rec").create_ml_1m_dataloader(data_source=ds, max_seq_len=24, max_predictions_per_seq=6)
    dl.generate_vocab()
    model = make_model(dl.tokenizer.get_vocab_size(), seed=5)
    items = dl.create_item_list()
    histories = [items[s:s + n] for s, n in ((0, 15), (40, 3), (90, 30), (120, 1), (7, 22))]
    rec = Recommender(model, dl)
    plain = rec.recommend_batch(histories, 5)
    pairs = rec.recommend_batch(histories, 5, return_probabilities=True)
    assert [[item for item, _ in row] for row in pairs] == plain
    probs = [p for row in pairs for _, p in row]
    assert all(0.0 < p <= 1.0 for p in probs) and all(sum(p for _, p in row) <= 1.0 + 1e-6 for row in pairs)
    cut = float(np.median(probs))
    kept = rec.recommend_batch(histories, 5, return_probabilities=True, min_probability=cut)
    assert kept == [[(item, p) for item, p in row if p >= cut] for row in pairs] and any(len(a) < len(b) for a, b in zip(kept, pairs))
    assert rec.recommend_batch(histories, 5, min_probability=cut) == [[item for item, _ in row] for row in kept]
    # k = 1: a pair, or None when the threshold leaves nothing; __call__ goes through the batch path
    one = rec.recommend_batch(histories, 1, return_probabilities=True)
    assert [x[0] for x in one] == rec.recommend_batch(histories, 1) and one == [row[0] for row in pairs]
    assert rec.recommend_batch(histories, 1, return_probabilities=True, min_probability=1.0) == [None] * len(histories)
    alone = rec(histories[0], 5, return_probabilities=True)
    assert [item for item, _ in alone] == plain[0] and [p for _, p in alone] == pytest.approx([p for _, p in pairs[0]], rel=1e-4)
    # a lower temperature sharpens: the best item's probability grows
    sharp = rec.recommend_batch(histories, 5, return_probabilities=True, temperature=0.5)
    assert [[item for item, _ in row] for row in sharp] == plain and all(s[0][1] > p[0][1] for s, p in zip(sharp, pairs))


def test_evaluator_distribution():
    V = 300
    model = make_model(V, seed=19)
    batches = [orc.synthetic_batch(32, 24, 6, V, seed=70 + i, ragged=True, finetune=True) for i in range(3)]
    ev = evaluation.get(full_ranking=True, distribution=True)
    plain = evaluation.get(full_ranking=True)
    nll, ent, tol_n, tol_e = [], [], [], []
    eng = model.engine
    table, bias = eng.view("word_embeddings/embeddings").cpu().numpy(), eng.view("cls/predictions/output_bias/bias").cpu().numpy()
    for b in batches:
        ev.evaluate_batch(model, b)
        plain.evaluate_batch(model, b)
        w = b["masked_lm_weights"] != 0
        b_idx, p_idx = torch.nonzero(w, as_tuple=True)
        slots = (b_idx * w.shape[1] + p_idx).cuda()
        hidden, _, _ = model._ranked_slot_hidden(b, slots)
        gt = b["masked_lm_ids"][b_idx, p_idx].numpy()
        t = sref.scaled_scores(hidden.cpu().numpy(), table, bias)
        ok = ref.allowed_mask(V, FIRST, b["labels"][b_idx].numpy(), gt, len(gt))
        n_p, lse_p, ent_p = sref.plain(t, ok)
        for r, g in enumerate(gt.tolist()):
            if FIRST <= g < V:
                nll.append(lse_p[r] - float(t[r, g]))
                ent.append(ent_p[r])
                tol_n.append(sref.tol_lse(n_p[r]) + 2.0 ** -24 * abs(nll[-1]))   # the row's lse, and the fp32 rounding of logp
                tol_e.append(sref.tol_entropy(n_p[r]))
    got, base = ev.get_metrics_results(), plain.get_metrics_results()
    assert {k: got[k] for k in base} == base and set(got) - set(base) == {"NLL", "Perplexity", "Entropy"}
    assert abs(got["NLL"] - np.mean(nll)) <= np.mean(tol_n) and abs(got["Entropy"] - np.mean(ent)) <= np.mean(tol_e)
    assert got["Perplexity"] == pytest.approx(np.exp(got["NLL"]), rel=1e-12)
    ev.reset_metrics()
    assert ev.get_metrics_results()["NLL"] == 0.0 and ev.get_metrics_results()["Entropy"] == 0.0
    ev.evaluate_batch(model, batches[0])
    again = ev.get_metrics_results()
    assert again["NLL"] > 0.0 and again["Entropy"] > 0.0
