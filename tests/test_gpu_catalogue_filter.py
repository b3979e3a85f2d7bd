"""Catalogue filters, the item scale and item-to-item neighbours on the GPU (b4r_rank_full_ex, b4r_item_neighbours): the ops against
the CPU restatement (tests/catalogue_ref.py) bit for bit, and the model / app layers built on them.

The shapes are the smallest that reach each boundary of the sweep: V = 33 (inside one 1024-id chunk, no multiple of 32), 1024 (one
whole chunk), 1025 (a 1-id tail chunk), 2051 (three chunks, a 3-id tail); R = 1, 16, 17 around the 16-row group; widths 64 and 128.

One statement of the specification is read by its own rule: under an all-zero filter "only gt is ranked", and gt is a member of
allowed(r), so the top K of such a row is gt followed by -1, and gt_rank is 1.  The top K is all -1 when no gt is given; both are
asserted below.

rnorm (1 / |row|, fp32, one fma per element in ascending k) against fp64: the kernel's worst error over these tables, measured on
an MI355X, is 4.867 ulp (V = 1024, width 128; 1.62 ... 4.86 ulp on the others), the figure a bit-level CPU restatement of its
arithmetic (fma chain, correctly rounded sqrt and divide) gives as well; the test prints the kernel's figure per table.  RNORM_ULP is
that figure rounded up to a power of two: 8, which is also the most allowed."""
import functools

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, dataloaders, datasets, models
from bert4rec_amd.apps import Recommender, pack_item_filter
from bert4rec_amd.models.components import networks
from tests import catalogue_ref as ref
from tests.b4r_testlib import P, stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
FIRST = 3
KS = (0, 1, 10, 1024)
VS = (33, 1024, 1025, 2051)
RNORM_ULP = 8.0   # 4.87 ulp rounded up to the next power of two


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@functools.lru_cache(maxsize=None)
def case(V, H):
    """17 rows against V items: hidden, table, bias, exclude, gt and the chain scores (with and without the bias), computed once.
    Planted ties: duplicated rows inside a chunk and across the chunk boundary (ids 1023 and 1024), lifted into every top 10; an
    all-zero row (id 5)."""
    R = 17
    g = torch.Generator().manual_seed(V * 7 + H)
    hidden = torch.randn(R, H, generator=g)
    table = torch.randn(V, H, generator=g) * 0.05
    bias = torch.randn(V, generator=g) * 0.01
    top = V - 1 if V != 1025 else 12                             # (at V = 1025 the last id is already half of the boundary pair)
    for a, b in ((7, 4), (1024, 1023), (top, 11)):
        if a < V and b < V and a != b:
            bias[b] = 6.0
            table[a] = table[b]; bias[a] = bias[b]
    table[5] = 0.0
    rng = np.random.default_rng(V + H)
    gt = rng.integers(FIRST, V, size=R).astype(np.int64)
    ex = rng.integers(0, V, size=(R, 8)).astype(np.int64)
    ex[:, 0] = -1
    ex[:, 1] = V + 5
    ex[::2, 2] = gt[::2]                     # gt listed: still ranked
    ex[1::2, 3] = 4                          # the lower id of a tie pair excluded
    hidden, table, bias = hidden.numpy(), table.numpy(), bias.numpy()
    return dict(hidden=hidden, table=table, bias=bias, gt=gt, ex=ex, sc=ref.chain_scores(hidden, table, bias),
                sc0=ref.chain_scores(hidden, table, None))


@functools.lru_cache(maxsize=None)
def on_device(V, H):
    c = case(V, H)
    return {k: torch.as_tensor(c[k]).to(DEV) for k in ("hidden", "table", "bias")}


def run_ex(V, H, R, K, words=None, row_filter=None, scale=None, use_bias=True, use_gt=True, use_ex=True):
    """b4r_rank_full_ex on the first R rows of case(V, H); returns (ids, scores, gt_rank) as numpy."""
    lib = _lib.load()
    c, d = case(V, H), on_device(V, H)
    ex_d = torch.as_tensor(c["ex"][:R]).to(DEV).contiguous() if use_ex else None
    gt_d = torch.as_tensor(c["gt"][:R]).to(DEV) if use_gt else None
    w_d = None if words is None else torch.as_tensor(words.view(np.int32)).to(DEV).contiguous()
    rf_d = None if row_filter is None else torch.as_tensor(np.asarray(row_filter, np.int32)).to(DEV)
    sc_d = None if scale is None else torch.as_tensor(scale).to(DEV)
    ids = torch.full((R, max(K, 1)), 7, dtype=torch.int64, device=DEV)
    scores = torch.full((R, max(K, 1)), 7.0, device=DEV)
    gt_rank = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    need = int(lib.b4r_rank_full_scratch_bytes(R, V, K))
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = lib.b4r_rank_full_ex(P(d["hidden"]), H, None, P(d["table"]), P(d["bias"]) if use_bias else None, H, V, FIRST, R, P(ex_d),
                              c["ex"].shape[1] if use_ex else 0, P(gt_d), K, P(ids), P(scores), P(gt_rank),   # (gt NULL: gt_rank is written 0)
                              P(scratch), need, stream(), P(w_d), 0 if words is None else words.shape[0], P(rf_d), P(sc_d))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return ids[:, :K].cpu().numpy(), scores[:, :K].cpu().numpy(), gt_rank.cpu().numpy().astype(np.int64)


def run_full(V, H, R, K):
    """b4r_rank_full itself on the first R rows of case(V, H), with the case's exclude and gt; returns (rc, ids, scores, gt_rank)."""
    lib = _lib.load()
    c, d = case(V, H), on_device(V, H)
    ex_d = torch.as_tensor(c["ex"][:R]).to(DEV).contiguous()
    gt_d = torch.as_tensor(c["gt"][:R]).to(DEV)
    ids = torch.full((R, max(K, 1)), 7, dtype=torch.int64, device=DEV)
    scores = torch.full((R, max(K, 1)), 7.0, device=DEV)
    gt_rank = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    need = int(lib.b4r_rank_full_scratch_bytes(R, V, K))
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = lib.b4r_rank_full(P(d["hidden"]), H, None, P(d["table"]), P(d["bias"]), H, V, FIRST, R, P(ex_d), c["ex"].shape[1], P(gt_d), K,
                           P(ids), P(scores), P(gt_rank), P(scratch), need, stream())
    torch.cuda.synchronize()
    return rc, ids[:, :K].cpu().numpy(), scores[:, :K].cpu().numpy(), gt_rank.cpu().numpy().astype(np.int64)


def want_ex(V, H, R, K, words=None, row_filter=None, scale=None, use_bias=True, use_gt=True, use_ex=True):
    c = case(V, H)
    sc = ref.scaled((c["sc"] if use_bias else c["sc0"])[:R], scale)
    gt = c["gt"][:R] if use_gt else None
    ok = ref.allowed_mask(V, FIRST, c["ex"][:R] if use_ex else None, gt, R, words, row_filter)
    return ref.expected(sc, ok, gt, K, FIRST)


def assert_same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), f"{what}: ids"
    assert bits_equal(got[1], want[1]), f"{what}: scores not bit-identical"
    assert np.array_equal(got[2], want[2]), f"{what}: gt_rank"


def filters_of(V, R, gt):
    """name -> (packed words [F, W], row_filter or None)"""
    rng = np.random.default_rng(V)
    W32 = ((V + 31) // 32) * 32
    out = {}
    out["ones"] = (ref.pack_bits(np.ones(V, bool)), None)
    out["zeros"] = (ref.pack_bits(np.zeros(V, bool)), None)
    one = np.zeros(V, bool); one[min(V - 1, 1030)] = True
    out["one_bit"] = (ref.pack_bits(one), None)
    low = np.zeros(V, bool); low[:FIRST] = True
    out["below_first"] = (ref.pack_bits(low), None)
    if W32 > V:
        past = np.zeros(W32, bool); past[V:] = True            # bits of ids >= V in the last word
        out["past_V"] = (ref.pack_bits(past), None)
    half = rng.random(V) < 0.5
    out["half"] = (ref.pack_bits(half), None)
    out["sparse"] = (ref.pack_bits(rng.random(V) < 1.0 / 64), None)
    three = rng.random((3, V)) < np.array([0.5, 0.1, 0.9])[:, None]
    rf = rng.integers(0, 3, size=R)
    rf[0] = 3                                                    # out of range: no filter for the row
    if R > 2:
        rf[2] = -1
    out["per_row"] = (ref.pack_bits(three), rf)
    no_gt = half.copy(); no_gt[gt] = False                       # every row's gt has its bit clear: still ranked
    out["gt_clear"] = (ref.pack_bits(no_gt), None)
    return out


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("R", [1, 16, 17])
@pytest.mark.parametrize("V", VS)
def test_rank_full_ex_filters_bit_exact(V, R, H):
    c, d = case(V, H), on_device(V, H)
    gt, ex = c["gt"][:R], c["ex"][:R]
    flt = filters_of(V, R, gt)
    for K in KS:
        rc, ids0, sc0, rk0 = run_full(V, H, R, K)
        assert rc == 0
        plain = want_ex(V, H, R, K)
        assert_same((ids0, sc0, rk0), plain, "b4r_rank_full")
        assert_same(run_ex(V, H, R, K), plain, "no filter")       # allow_bits NULL: b4r_rank_full
        for name, (words, rf) in flt.items():
            got = run_ex(V, H, R, K, words, rf)
            assert_same(got, want_ex(V, H, R, K, words, rf), f"{name} K={K}")
            if name == "ones":
                assert np.array_equal(got[0], ids0) and bits_equal(got[1], sc0) and np.array_equal(got[2], rk0)
            if name in ("zeros", "below_first", "past_V"):
                # only gt is ranked: first, then the -1 / -inf tail; without a gt nothing is
                assert (got[2] == 1).all()
                if K > 0:
                    assert np.array_equal(got[0][:, 0], gt) and (got[0][:, 1:] == -1).all() and (got[1][:, 1:] == -np.inf).all()
                    ids_n, sc_n, _ = run_ex(V, H, R, K, words, rf, use_gt=False)
                    assert (ids_n == -1).all() and (sc_n == -np.inf).all()
            if name == "one_bit" and K == 10:
                assert (got[0][:, 2:] == -1).all(), "K above the allowed count leaves a -1 / -inf tail"
            if name == "per_row":
                assert np.array_equal(got[0][0], ids0[0]) and bits_equal(got[1][0], sc0[0]) and got[2][0] == rk0[0]
    # the filter intersected with the exclude list: ids listed in both, ids only excluded, ids only filtered out
    both = np.ones(V, bool)
    both[ex[:, 4:6].reshape(-1)] = False
    words = ref.pack_bits(both)
    got = run_ex(V, H, R, 10, words)
    assert_same(got, want_ex(V, H, R, 10, words), "filter and exclude")
    for r in range(R):
        assert not (set(got[0][r].tolist()) - {int(gt[r])}) & set(ex[r].tolist())


def test_ties_across_the_chunk_boundary():
    V, H, R, K = 1025, 64, 16, 10
    ids, _, _ = run_ex(V, H, R, K, ref.pack_bits(np.ones(V, bool)), use_ex=False, use_gt=False)
    for r in range(R):                                            # ids 1023 / 1024 and 4 / 7 hold equal rows: the lower id first
        row = ids[r].tolist()
        assert row.index(1023) + 1 == row.index(1024) and row.index(4) + 1 == row.index(7)
    cut = np.ones(V, bool); cut[[1023, 4]] = False                # the filter removes the lower id of each pair
    words = ref.pack_bits(cut)
    got = run_ex(V, H, R, K, words, use_ex=False, use_gt=False)
    assert_same(got, want_ex(V, H, R, K, words, use_ex=False, use_gt=False), "ties")
    for r in range(R):
        row = got[0][r].tolist()
        assert 1024 in row and 7 in row and 1023 not in row and 4 not in row


@pytest.mark.parametrize("V,H", [(33, 64), (2051, 64), (1025, 128)])
def test_item_scale_and_null_bias(V, H):
    R = 17
    rng = np.random.default_rng(V)
    scale = rng.standard_normal(V).astype(np.float32)
    scale[[6, 8]] = (0.0, -0.0)
    scale[9] = 1.0
    words = ref.pack_bits(rng.random(V) < 0.5)
    for use_bias in (True, False):
        for sc in (None, scale):
            for w in (None, words):
                for K in (10, 1024):
                    kw = dict(words=w, scale=sc, use_bias=use_bias)
                    assert_same(run_ex(V, H, R, K, **kw), want_ex(V, H, R, K, **kw), f"bias={use_bias} scale={sc is not None} filter={w is not None}")
    lib = _lib.load()
    d = on_device(V, H)
    assert lib.b4r_rank_full(P(d["hidden"]), H, None, P(d["table"]), None, H, V, FIRST, R, None, 0, None, 10, None, None, None, None, 0,
                             stream()) == -1, "b4r_rank_full keeps refusing a NULL bias"


# ---- item neighbours ----------------------------------------------------------------------------------------------------------------
def run_nb(table_d, width, V, query, metric, K, words=None, row_filter=None):
    lib = _lib.load()
    R = len(query)
    q_d = torch.as_tensor(np.asarray(query, np.int64)).to(DEV)
    w_d = None if words is None else torch.as_tensor(words.view(np.int32)).to(DEV).contiguous()
    rf_d = None if row_filter is None else torch.as_tensor(np.asarray(row_filter, np.int32)).to(DEV)
    ids = torch.full((R, max(K, 1)), 7, dtype=torch.int64, device=DEV)
    scores = torch.full((R, max(K, 1)), 7.0, device=DEV)
    need = int(lib.b4r_item_neighbours_scratch_bytes(R, V, K, width))
    scratch = torch.zeros(need + 16, dtype=torch.uint8, device=DEV)
    off = (16 - scratch.data_ptr() % 16) % 16

    def call():
        rc = lib.b4r_item_neighbours(P(table_d), width, width, V, FIRST, P(q_d), R, metric, P(w_d), 0 if words is None else words.shape[0],
                                     P(rf_d), K, P(ids), P(scores), scratch.data_ptr() + off, need, stream())
        assert rc == 0, _lib.last_error()

    def read():
        torch.cuda.synchronize()
        return ids[:, :K].cpu().numpy(), scores[:, :K].cpu().numpy(), scratch[off:off + 4 * V].view(torch.float32).cpu().numpy()
    call()
    return read(), call, read


def ulp_error(got, want64):
    want32 = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want64) / np.spacing(np.abs(want32)).astype(np.float64)


@pytest.mark.parametrize("width", [64, 128])
@pytest.mark.parametrize("R", [1, 17])
@pytest.mark.parametrize("V", VS)
def test_item_neighbours(V, R, width):
    c, d = case(V, width), on_device(V, width)
    table = c["table"]
    rng = np.random.default_rng(V + R)
    query = rng.integers(FIRST, V, size=R).astype(np.int64)
    if R > 1:
        query[:7] = (1, V, 5, 4, min(V - 1, 1023), V - 1, -3)    # below first_item, >= V, the all-zero row, tie pairs, negative
    flt = filters_of(V, R, np.clip(query, 0, V - 1))
    rnorm64 = 1.0 / np.sqrt(np.maximum((table.astype(np.float64) ** 2).sum(axis=1), 1e-24))
    for metric in (0, 1):
        for K in KS:
            (ids, scores, rnorm), call, read = run_nb(d["table"], width, V, query, metric, K)
            if metric == 1:
                err = float(ulp_error(rnorm, rnorm64).max())
                if K == 0:
                    print(f"rnorm V={V} width={width}: worst error {err:.3f} ulp")
                assert err <= RNORM_ULP, f"rnorm is {err} ulp from fp64"
                assert np.isfinite(rnorm).all()                   # (the all-zero row 5 takes the clamp: 1e12)
            want = ref.neighbours(table, query, FIRST, metric, K, rnorm)
            assert np.array_equal(ids, want[0]) and bits_equal(scores, want[1]), f"metric {metric} K={K}"
            valid = ids >= 0
            assert np.isfinite(scores[valid]).all() and (scores[~valid] == -np.inf).all()
            for r in range(R):
                assert query[r] not in ids[r] and not ((ids[r] >= 0) & (ids[r] < FIRST)).any()
                if not FIRST <= query[r] < V:
                    assert (ids[r] == -1).all()
            if K == 1024 and V <= 1024:
                for r in range(R):                                # every other item is listed: the zero row scores exactly +-0.0
                    if FIRST <= query[r] < V and query[r] != 5:
                        assert (ids[r] == 5).sum() == 1 and (scores[r][ids[r] == 5] == 0.0).all()
                    if query[r] == 5:
                        assert (scores[r][ids[r] >= 0] == 0.0).all()
            call()                                                # the second run: bitwise the same
            again = read()
            assert np.array_equal(again[0], ids) and bits_equal(again[1], scores) and bits_equal(again[2], rnorm)
        for name in ("half", "sparse", "per_row", "zeros"):
            words, rf = flt[name]
            (ids, scores, rnorm), _, _ = run_nb(d["table"], width, V, query, metric, 10, words, rf)
            want = ref.neighbours(table, query, FIRST, metric, 10, rnorm, words, rf)
            assert np.array_equal(ids, want[0]) and bits_equal(scores, want[1]), f"metric {metric} filter {name}"
            if name == "zeros":
                assert (ids == -1).all()
        only5 = np.zeros(V, bool); only5[5] = True                # the all-zero row alone, at every V: exactly +-0.0
        ids, scores, _ = run_nb(d["table"], width, V, query, metric, 10, ref.pack_bits(only5))[0]
        for r in range(R):
            if FIRST <= query[r] < V and query[r] != 5:
                assert ids[r, 0] == 5 and (ids[r, 1:] == -1).all() and scores[r, 0] == 0.0


def test_item_neighbours_in_a_captured_graph():
    V, width, R, K = 2051, 64, 17, 10
    c, d = case(V, width), on_device(V, width)
    query = np.arange(FIRST, FIRST + R).astype(np.int64) * 100 % V
    words = ref.pack_bits(np.random.default_rng(1).random(V) < 0.5)
    (ids, scores, _), call, read = run_nb(d["table"], width, V, query, 1, K, words)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        graph.replay()
    got = read()
    assert np.array_equal(got[0], ids) and bits_equal(got[1], scores)


# ---- the model and the apps ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_app(factorised=False):
    ds = datasets.synthetic_dataset(n_users=30, n_items=200, min_len=5, max_len=30, seed=4)
    dl = dataloaders.get_dataloader_factory("bert4rec").create_ml_1m_dataloader(data_source=ds, max_seq_len=24, max_predictions_per_seq=6)
    dl.generate_vocab()
    V = dl.tokenizer.get_vocab_size()
    kw = dict(hidden_size=128, num_attention_heads=4, inner_dim=512, embedding_width=64) if factorised else \
        dict(hidden_size=64, num_attention_heads=2, inner_dim=256)
    enc = networks.Bert4RecEncoder(V, num_layers=1, max_sequence_length=24, output_dropout=0.0, attention_dropout=0.0, seed=5, **kw)
    model = models.BERT4RecModel(enc)
    return Recommender(model, dl), dl.create_item_list()


def test_recommend_batch_with_allowed_items():
    rec, items = small_app()
    V = rec.model.vocab_size
    histories = [items[s:s + n] for s, n in ((0, 15), (40, 3), (90, 30), (120, 1), (7, 22))]
    everything = rec.recommend_batch(histories, k=V - 3)
    allowed = items[::3] + ["no such item"]                        # unknown items are ignored
    for k in (1, 5):
        got = rec.recommend_batch(histories, k, allowed_items=allowed)
        want = [[i for i in full if i in set(allowed)][:k] for full in everything]
        assert got == [w[0] if k == 1 else w for w in want]
        assert rec(histories[0], k, allowed_items=allowed) == got[0]
    assert rec.dataloader.get_tokenizer().get_vocab_size() == V       # the unknown item was not added to the vocabulary
    # two users share a list, one differs, two more share another
    lists = [items[::2], items[1::2], list(reversed(items[::2])), items[5:60], items[5:60]]
    got = rec.recommend_batch(histories, 5, allowed_items_per_user=lists)
    assert got == [[i for i in full if i in set(lst)][:5] for full, lst in zip(everything, lists)]
    assert rec.recommend_batch(histories, 5, allowed_items=[]) == [[] for _ in histories]
    with pytest.raises(ValueError):
        rec.recommend_batch(histories, 5, allowed_items=allowed, allowed_items_per_user=lists)
    with pytest.raises(ValueError):
        rec.recommend_batch(histories, 5, allowed_items_per_user=lists[:2])


def test_recommend_tensor_allow_forms_agree():
    rec, items = small_app()
    model, V = rec.model, rec.model.vocab_size
    batches = [rec.dataloader.prepare_inference(list(items[s:s + 9])) for s in (0, 30, 60)]
    batch = {key: torch.from_numpy(np.concatenate([np.asarray(b[key]) for b in batches], axis=0)) for key in batches[0]}
    masks = torch.as_tensor(np.random.default_rng(2).random((2, V)) < 0.4)
    plain = model.recommend_tensor(batch, k=5)
    R = int(plain[2].numel())
    a = model.recommend_tensor(batch, k=5, allow=masks[0])
    for form in (masks[0].to(torch.uint8), masks[0].to(DEV), pack_item_filter(masks[0]), pack_item_filter(masks[0].to(DEV))):
        b = model.recommend_tensor(batch, k=5, allow=form)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(bool(masks[0][i]) for i in a[0].cpu().reshape(-1).tolist() if i >= 0) and not torch.equal(a[0], plain[0])
    rf = torch.tensor([1, 0, 2][:R] + [0] * max(0, R - 3))
    c = model.recommend_tensor(batch, k=5, allow=masks, row_filter=rf)
    b1 = model.recommend_tensor(batch, k=5, allow=masks[1])
    assert torch.equal(c[0][0], b1[0][0]) and torch.equal(c[0][1], a[0][1]) and torch.equal(c[0][2], plain[0][2])
    with pytest.raises(ValueError):
        model.recommend_tensor(batch, k=5, allow=masks)              # two filters, no row_filter
    with pytest.raises(ValueError):
        model.recommend_tensor(batch, k=5, allow=masks, row_filter=torch.zeros(R + 1, dtype=torch.int64))


@pytest.mark.parametrize("factorised", [False, True])
def test_similar_items(factorised):
    rec, items = small_app(factorised)
    model, V = rec.model, rec.model.vocab_size
    tok = rec.dataloader.get_tokenizer()
    table = model.engine.view("word_embeddings/embeddings")
    assert tuple(table.shape) == (V, 64)                             # the 64-wide table, also under hidden 128
    query_items = [items[3], "no such item", items[50]]
    query = [tok.tokenize(items[3]), -1, tok.tokenize(items[50])]
    allowed = items[::2]
    for metric in ("cosine", "dot"):
        ids, scores = model.similar_items_tensor(torch.tensor(query), k=7, metric=metric)
        assert ids.shape == (3, 7) and (ids[1] == -1).all() and bool(torch.isinf(scores[1]).all())
        lists = rec.similar_items(query_items, k=7, metric=metric)
        assert lists == [tok.detokenize([i for i in row if i >= 0]) for row in ids.cpu().tolist()]
        assert len(lists[0]) == 7 and lists[1] == [] and items[3] not in lists[0]
        # against the restatement on the table the model holds
        rnorm = None
        if metric == "cosine":
            (_, _, rnorm), _, _ = run_nb(table.contiguous(), 64, V, query, 1, 7)
        want = ref.neighbours(table.cpu().numpy(), query, FIRST, 1 if metric == "cosine" else 0, 7, rnorm)
        assert np.array_equal(ids.cpu().numpy(), want[0]) and bits_equal(scores.cpu().numpy(), want[1])
        if metric == "cosine":
            assert float(scores[0].max()) <= 1.0 + 1e-5
        only = rec.similar_items(query_items, k=7, metric=metric, allowed_items=allowed)
        assert all(i in set(allowed) for lst in only for i in lst) and len(only[0]) == 7
    with pytest.raises(ValueError):
        model.similar_items_tensor(torch.tensor(query), k=7, metric="euclid")
    with pytest.raises(ValueError):
        model.similar_items_tensor(torch.tensor([[3]]), k=7)
