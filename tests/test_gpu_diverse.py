"""Diversity-aware re-ranking on the GPU (b4r_rerank_diverse): the kernel against the CPU restatement (tests/diverse_ref.py) bit for
bit in out_ids, out_scores and out_mmr, and the model / app layers built on it.

The kernel is given an explicit fp32 rnorm wherever it is compared with the restatement, so the comparison does not depend on a
device reciprocal square root; the item_rnorm = NULL form is compared with a call that is given the rnorm b4r_item_neighbours
leaves in its scratch.

Shapes: a workgroup has 256 threads (4 waves) and a thread owns 1, 2 or 4 pool entries (M <= 256, <= 512, <= 1024), so M = 1, 2,
63, 64, 65, 256, 1023, 1024 cross the wave, workgroup and loop boundaries and 257, 512, 513 the boundaries between the three
instances; widths 4 (one 16-byte load), 64, 132 (no multiple of the 16-float unrolled step) and 256.  V = 40 with M up to 1024
fills a pool with repeated ids, and so with exact ties."""
import functools

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, dataloaders, datasets, models
from bert4rec_amd import engine as engine_mod
from bert4rec_amd.apps import Recommender
from bert4rec_amd.models.components import networks
from tests import diverse_ref as dref
from tests.b4r_testlib import P, stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
TABLES = ((40, 4), (300, 64), (1100, 132), (1100, 256))
MS = (1, 2, 63, 64, 65, 256, 257, 512, 513, 1023, 1024)
LAMBDAS = (0.0, 0.3, 1.0)
R_MAX = 17


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


@functools.lru_cache(maxsize=None)
def case(V, width):
    """An item table with two pairs of identical rows (ids 4 / 7 and 11 / V - 1), an fp32 rnorm, and the restatement's [V, V]
    similarities, computed once."""
    g = torch.Generator().manual_seed(V * 13 + width)
    table = (torch.randn(V, width, generator=g) * 0.05).numpy()
    table[7] = table[4]
    table[V - 1] = table[11]
    rnorm = (1.0 / np.sqrt(np.maximum((table.astype(np.float64) ** 2).sum(axis=1), 1e-24))).astype(F32)
    return dict(table=table, rnorm=rnorm, sim=dref.sim_matrix(table, rnorm), table_d=torch.as_tensor(table).to(DEV),
                rnorm_d=torch.as_tensor(rnorm).to(DEV))


def make_pool(V, M, R=R_MAX, seed=0):
    """R pool rows of M entries: distinct ids where V allows it (else repeats), scores descending with a few exact repeats."""
    rng = np.random.default_rng(seed + 31 * V + M)
    ids = np.stack([rng.permutation(V)[:M] if M <= V else rng.integers(0, V, size=M) for _ in range(R)]).astype(np.int64)
    sc = -np.sort(-rng.standard_normal((R, M)).astype(F32), axis=1)
    if M > 3:
        sc[:, 2] = sc[:, 1]
    return ids, sc


def run(c, width, V, ids, sc, lam, K, rnorm="given", outputs=(True, True, True)):
    """b4r_rerank_diverse; returns (rc, ids, scores, mmr, call) with the outputs as numpy ([R, K]; None where not asked for)."""
    lib = _lib.load()
    R, M = ids.shape
    ids_d, sc_d = torch.as_tensor(ids).to(DEV).contiguous(), torch.as_tensor(sc).to(DEV).contiguous()
    outs = [torch.full((R, max(K, 1)), 7, dtype=torch.int64, device=DEV) if outputs[0] else None,
            torch.full((R, max(K, 1)), 7.0, device=DEV) if outputs[1] else None,
            torch.full((R, max(K, 1)), 7.0, device=DEV) if outputs[2] else None]
    need = int(lib.b4r_rerank_diverse_scratch_bytes(R, M, V))
    scratch = torch.zeros(max(need, 16), dtype=torch.uint8, device=DEV) if rnorm is None else None
    rn = c["rnorm_d"] if isinstance(rnorm, str) else rnorm

    def call():
        return lib.b4r_rerank_diverse(P(c["table_d"]), width, width, V, P(rn), P(ids_d), P(sc_d), R, M, float(lam), K, P(outs[0]),
                                      P(outs[1]), P(outs[2]), P(scratch), need if scratch is not None else 0, stream())

    def read():
        torch.cuda.synchronize()
        return tuple(None if o is None else o[:, :K].cpu().numpy() for o in outs)
    rc = call()
    return (rc,) + read() + (call, read, scratch)


def cosine_neighbours(table_d, width, V, query, K, first_item=3):
    """b4r_item_neighbours(B4R_SIM_COSINE); returns (ids [R, K], scores [R, K], the rnorm [V] it left in its scratch) as numpy."""
    lib = _lib.load()
    R = len(query)
    q_d = torch.as_tensor(np.asarray(query, np.int64)).to(DEV)
    ids = torch.empty((R, K), dtype=torch.int64, device=DEV)
    scores = torch.empty((R, K), device=DEV)
    need = int(lib.b4r_item_neighbours_scratch_bytes(R, V, K, width))
    scratch = torch.zeros(need + 16, dtype=torch.uint8, device=DEV)
    off = (16 - scratch.data_ptr() % 16) % 16
    rc = lib.b4r_item_neighbours(P(table_d), width, width, V, first_item, P(q_d), R, _lib.SIM_COSINE, None, 0, None, K, P(ids), P(scores),
                                 scratch.data_ptr() + off, need, stream())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return ids.cpu().numpy(), scores.cpu().numpy(), scratch[off:off + 4 * V].view(torch.float32).cpu().numpy()


def assert_same(got, want, K, what):
    assert np.array_equal(got[0], want[0][:, :K]), f"{what}: ids"
    assert bits_equal(got[1], want[1][:, :K]), f"{what}: scores not bit-identical"
    assert bits_equal(got[2], want[2][:, :K]), f"{what}: mmr not bit-identical"


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("V,width", TABLES)
def test_grid_bit_exact(V, width, M):
    c = case(V, width)
    ids, sc = make_pool(V, M)
    for lam in LAMBDAS:
        want = dref.rerank(c["table"], c["rnorm"], ids, sc, lam, M, c["sim"])    # K = M once: a smaller K is its prefix
        for R in (1, R_MAX):
            for K in sorted({0, 1, min(M, 10), M}):
                rc, g_ids, g_sc, g_mmr = run(c, width, V, ids[:R], sc[:R], lam, K)[:4]
                assert rc == 0, _lib.last_error()
                assert_same((g_ids, g_sc, g_mmr), tuple(w[:R] for w in want), K, f"lambda={lam} R={R} K={K}")
        if lam == 1.0:
            assert np.array_equal(want[0], ids) or M > V               # distinct ids, descending scores: the pool's own order


@pytest.mark.parametrize("M", [65, 300, 1024])
def test_dead_entries(M):
    V, width = 300, 64
    c = case(V, width)
    ids, sc = make_pool(V, M, R=10, seed=5)
    ids[0, :] = -1; sc[0, :] = -np.inf                                # the -1 / -inf tail from 0 live entries,
    ids[1, 1:] = -1; sc[1, 1:] = -np.inf                              # from 1 (a pool with one live entry),
    ids[2, M - 1:] = -1; sc[2, M - 1:] = -np.inf                      # from M - 1
    ids[3, [0, 5, M // 2, M - 2]] = -1                                # -1 in the middle, scores left finite
    ids[4, 3] = V; ids[4, 7] = 2 ** 40; ids[4, 9] = -2 ** 40          # ids past V and outside 32 bits
    sc[5, 2] = np.inf; sc[5, 4] = np.nan; sc[5, 6] = -np.inf          # scores that are not finite on good ids
    sc[6, :] = F32(0.75)                                              # all live scores equal: rel = 1
    sc[7, :] = F32(-0.0); sc[7, ::2] = F32(0.0)                       # ... equal as +-0.0
    ids[8, : M - 1] = -1                                              # only the last entry is live
    sc[9, 1::2] = -np.inf                                             # every other entry dead
    for lam in LAMBDAS:
        want = dref.rerank(c["table"], c["rnorm"], ids, sc, lam, M, c["sim"])
        for K in (1, min(M, 10), M):
            rc, g_ids, g_sc, g_mmr = run(c, width, V, ids, sc, lam, K)[:4]
            assert rc == 0, _lib.last_error()
            assert_same((g_ids, g_sc, g_mmr), want, K, f"lambda={lam} K={K}")
        assert (g_ids[0] == -1).all() and (g_sc[0] == -np.inf).all() and (g_mmr[0] == -np.inf).all()
        assert g_ids[1, 0] == ids[1, 0] and (g_ids[1, 1:] == -1).all() and g_mmr[1, 0] == F32(lam)
        assert (g_ids[2, : M - 1] >= 0).all() and g_ids[2, M - 1] == -1
        assert g_ids[8, 0] == ids[8, M - 1] and (g_ids[8, 1:] == -1).all()
        for r in (3, 4, 5, 9):                                        # a dead entry is never picked; the live ones all are
            live = (ids[r] >= 0) & (ids[r] < V) & np.isfinite(sc[r])
            n = int(live.sum())
            assert sorted(g_ids[r, :n].tolist()) == sorted(ids[r, live].tolist()) and (g_ids[r, n:] == -1).all()
        if lam == 1.0:
            assert np.array_equal(g_ids[6], ids[6]) and (g_mmr[6] == 1.0).all() and np.array_equal(g_ids[7], ids[7])


@pytest.mark.parametrize("where,M,p1,p2", [("one thread's two loop turns", 300, 5, 261), ("two lanes", 300, 5, 6), ("two waves", 300, 5, 70),
                                           ("turns 0 and 3 of one thread", 1000, 9, 777), ("two waves, one turn apart", 1000, 200, 300)])
def test_ties_go_to_the_lower_position(where, M, p1, p2):
    """ids 4 / 7 and 11 / V - 1 hold identical table rows (and so identical rnorm): given equal scores, two such entries have the
    same rel and the same sim to every pick, so the same mmr at every step, until one of them is picked."""
    V, width = 1100, 132
    c = case(V, width)
    rng = np.random.default_rng(M + p1)
    rest = np.setdiff1d(np.arange(V), [4, 7, 11, V - 1])
    ids = np.stack([rng.permutation(rest)[:M] for _ in range(4)]).astype(np.int64)
    sc = -np.sort(-rng.standard_normal((4, M)).astype(F32), axis=1)
    ids[0::2, p1], ids[0::2, p2] = 4, 7                                # the higher id first as well: the position decides, not the id
    ids[1::2, p1], ids[1::2, p2] = V - 1, 11
    sc[:, p2] = sc[:, p1]
    for lam in (0.3, 1.0):
        want = dref.rerank(c["table"], c["rnorm"], ids, sc, lam, M, c["sim"])
        rc, g_ids, g_sc, g_mmr = run(c, width, V, ids, sc, lam, M)[:4]
        assert rc == 0, _lib.last_error()
        assert_same((g_ids, g_sc, g_mmr), want, M, f"{where}, lambda={lam}")
        for r in range(4):
            row = g_ids[r].tolist()
            assert row.index(ids[r, p1]) < row.index(ids[r, p2]), f"{where}: row {r}"
            if lam == 1.0:
                assert g_mmr[r, row.index(ids[r, p1])] == g_mmr[r, row.index(ids[r, p2])]


def test_lambda_one_is_the_sweeps_own_order():
    """The pool comes from a real b4r_rank_full call; rows 0 and 1 exclude most of the catalogue, so their pools end in -1 / -inf."""
    lib = _lib.load()
    V, width, R, M, K = 300, 64, R_MAX, 100, 10
    c = case(V, width)
    g = torch.Generator().manual_seed(9)
    hidden = torch.randn(R, width, generator=g).to(DEV)
    bias = (torch.randn(V, generator=g) * 0.01).to(DEV)
    ex = torch.full((R, V), -1, dtype=torch.int64)
    ex[0, :] = torch.arange(V); ex[0, :5] = -1                         # ids 0 .. 4 are left, and 0 .. 2 lie below first_item: 2 items
    ex[1, : V - 50] = torch.arange(V - 50)
    ex = ex.to(DEV)
    pool_ids = torch.empty((R, M), dtype=torch.int64, device=DEV)
    pool_sc = torch.empty((R, M), device=DEV)
    need = int(lib.b4r_rank_full_scratch_bytes(R, V, M))
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert lib.b4r_rank_full(P(hidden), width, None, P(c["table_d"]), P(bias), width, V, 3, R, P(ex), V, None, M, P(pool_ids), P(pool_sc),
                             None, P(scratch), need, stream()) == 0, _lib.last_error()
    out_ids = torch.full((R, K), 7, dtype=torch.int64, device=DEV)
    out_sc = torch.full((R, K), 7.0, device=DEV)
    assert lib.b4r_rerank_diverse(P(c["table_d"]), width, width, V, P(c["rnorm_d"]), P(pool_ids), P(pool_sc), R, M, 1.0, K, P(out_ids),
                                  P(out_sc), None, None, 0, stream()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(out_ids, pool_ids[:, :K]) and torch.equal(out_sc, pool_sc[:, :K])
    assert int((pool_ids[0] >= 0).sum()) == 2 and int((out_ids[0] >= 0).sum()) == 2 and int((pool_ids[1] >= 0).sum()) == 50


def test_similarity_is_the_item_neighbours_cosine():
    """Pools of two entries (q, c) at lambda = 0: step 0 picks q (every mmr is 0: the lower position), step 1 picks c with
    mmr = 0 - sim(c, q).  That sim is b4r_item_neighbours' cosine score of (query q, item c), bit for bit, with the rnorm that call
    left in its scratch; and the item_rnorm = NULL form computes the same rnorm."""
    V, width = 300, 64
    c = case(V, width)
    query = np.array([4, 11, 150], np.int64)
    nb_ids, nb_sc, rnorm_dev = cosine_neighbours(c["table_d"], width, V, query, V - 1)      # first_item = 3: ids 3 .. V-1 but q
    cands = np.arange(3, V)
    for qi, q in enumerate(query):
        cs = cands[cands != q]
        ids = np.stack([np.full(len(cs), q), cs], axis=1).astype(np.int64)
        sc = np.tile(np.array([2.0, 1.0], F32), (len(cs), 1))
        rn_d = torch.as_tensor(rnorm_dev).to(DEV)
        rc, g_ids, _, g_mmr = run(c, width, V, ids, sc, 0.0, 2, rnorm=rn_d)[:4]
        assert rc == 0, _lib.last_error()
        assert (g_ids[:, 0] == q).all() and np.array_equal(g_ids[:, 1], cs) and (g_mmr[:, 0] == 0.0).all()
        score_of = dict(zip(nb_ids[qi].tolist(), nb_sc[qi].tolist()))
        want = np.array([score_of[int(j)] for j in cs], F32)
        assert bits_equal(-g_mmr[:, 1] + F32(0.0), want + F32(0.0))      # (+ 0.0: a zero's sign is lost in 0 - sim)
        assert not (want == 0.0).any()
        rc, n_ids, n_sc, n_mmr, _, _, scratch = run(c, width, V, ids, sc, 0.0, 2, rnorm=None)
        assert rc == 0, _lib.last_error()
        assert np.array_equal(n_ids, g_ids) and bits_equal(n_mmr, g_mmr)
        off = (16 - scratch.data_ptr() % 16) % 16
        assert bits_equal(scratch[off:off + 4 * V].view(torch.float32).cpu().numpy(), rnorm_dev)
    # and against the restatement with that rnorm, on a full pool
    ids, sc = make_pool(V, 100, R=5, seed=3)
    want = dref.rerank(c["table"], rnorm_dev, ids, sc, 0.3, 100)
    for form in (torch.as_tensor(rnorm_dev).to(DEV), None):
        rc, g_ids, g_sc, g_mmr = run(c, width, V, ids, sc, 0.3, 100, rnorm=form)[:4]
        assert rc == 0, _lib.last_error()
        assert_same((g_ids, g_sc, g_mmr), want, 100, "device rnorm")


def test_errors_and_null_outputs():
    V, width = 300, 64
    c = case(V, width)
    lib = _lib.load()
    ids, sc = make_pool(V, 100, R=3)
    ids_d, sc_d = torch.as_tensor(ids).to(DEV), torch.as_tensor(sc).to(DEV)
    out = torch.full((300,), 7, dtype=torch.int64, device=DEV)

    def call(M=100, K=10, lam=0.5, ld=width, w=width, rnorm=c["rnorm_d"], scratch=None, nbytes=0):
        return lib.b4r_rerank_diverse(P(c["table_d"]), ld, w, V, P(rnorm), P(ids_d), P(sc_d), 3, M, lam, K, P(out), None, None, P(scratch),
                                      nbytes, stream())
    for kw, code in ((dict(M=0), -2), (dict(M=1025), -2), (dict(K=101), -2), (dict(lam=-0.1), -1), (dict(lam=1.5), -1),
                     (dict(lam=float("nan")), -1), (dict(ld=width + 4), -2), (dict(w=6, ld=6), -2)):
        assert call(**kw) == code, kw
        assert "b4r_rerank_diverse" in _lib.last_error()
    need = int(lib.b4r_rerank_diverse_scratch_bytes(3, 100, V))
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert call(rnorm=None, scratch=scratch, nbytes=4 * V - 1) == -5 and "scratch" in _lib.last_error()    # B4R_E_NOMEM
    assert call(rnorm=None, scratch=None, nbytes=0) == -5
    assert call(rnorm=None, scratch=scratch, nbytes=need) == 0
    assert call(K=0) == 0 and lib.b4r_rerank_diverse(None, width, width, V, None, None, None, 0, 100, 0.5, 10, None, None, None, None, 0,
                                                     stream()) == 0
    torch.cuda.synchronize()
    assert (out[30:] == 7).all() and (out[:30] >= 0).all()            # nothing faulted; only [R, K] = [3, 10] was written
    # any output may be NULL: each alone gives what all three give
    full = run(c, width, V, ids, sc, 0.3, 10)
    for i in range(3):
        only = run(c, width, V, ids, sc, 0.3, 10, outputs=tuple(j == i for j in range(3)))
        assert only[0] == 0 and all(only[1 + j] is None for j in range(3) if j != i)
        assert np.array_equal(only[1 + i].view(np.uint32 if i else np.int64), full[1 + i].view(np.uint32 if i else np.int64))


def test_reproducible_and_in_a_captured_graph():
    V, width, M, K = 1100, 132, 513, 100
    c = case(V, width)
    ids, sc = make_pool(V, M, seed=11)
    for rnorm in ("given", None):
        rc, a_ids, a_sc, a_mmr, call, read, _ = run(c, width, V, ids, sc, 0.3, K, rnorm=rnorm)
        assert rc == 0, _lib.last_error()
        assert call() == 0
        b = read()
        assert np.array_equal(b[0], a_ids) and bits_equal(b[1], a_sc) and bits_equal(b[2], a_mmr)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                assert call() == 0
        torch.cuda.current_stream().wait_stream(side)
        for _ in range(2):
            graph.replay()
        g = read()
        assert np.array_equal(g[0], a_ids) and bits_equal(g[1], a_sc) and bits_equal(g[2], a_mmr)


# ---- the model and the apps ---------------------------------------------------------------------------------------------------------
def build_small_app(factorised=False):
    """A Recommender on a one-layer model over about 200 items (V about 200 + 3), plain (hidden 64) or factorised (hidden 128, table
    width 64), and its item list.  Built anew per call: an engine sizes its workspaces under the arithmetic mode it first runs in."""
    ds = datasets.synthetic_dataset(n_users=30, n_items=200, min_len=5, max_len=30, seed=4)
    dl = dataloaders.get_dataloader_factory("bert4rec").create_ml_1m_dataloader(data_source=ds, max_seq_len=24, max_predictions_per_seq=6)
    dl.generate_vocab()
    V = dl.tokenizer.get_vocab_size()
    kw = dict(hidden_size=128, num_attention_heads=4, inner_dim=512, embedding_width=64) if factorised else \
        dict(hidden_size=64, num_attention_heads=2, inner_dim=256)
    enc = networks.Bert4RecEncoder(V, num_layers=1, max_sequence_length=24, output_dropout=0.0, attention_dropout=0.0, seed=5, **kw)
    return Recommender(models.BERT4RecModel(enc), dl), dl.create_item_list()


def device_rnorm(model):
    """The rnorm b4r_rerank_diverse computes for the model's item table when it is given none (read from its scratch)."""
    lib = _lib.load()
    table = model.engine.view("word_embeddings/embeddings")
    V, width = (int(x) for x in table.shape)
    need = int(lib.b4r_rerank_diverse_scratch_bytes(1, 1, V))
    scratch = torch.zeros(need, dtype=torch.uint8, device=DEV)
    ids, sc = torch.zeros((1, 1), dtype=torch.int64, device=DEV), torch.zeros((1, 1), device=DEV)
    out = torch.empty((1, 1), dtype=torch.int64, device=DEV)
    assert lib.b4r_rerank_diverse(P(table), width, width, V, None, P(ids), P(sc), 1, 1, 0.5, 1, P(out), None, None, P(scratch), need,
                                  stream()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    off = (16 - scratch.data_ptr() % 16) % 16
    return scratch[off:off + 4 * V].view(torch.float32).cpu().numpy()


def mean_pairwise_cosine(table64, rows):
    total, n = 0.0, 0
    for row in rows:
        e = table64[[i for i in row if i >= 0]]
        e = e / np.linalg.norm(e, axis=1, keepdims=True)
        cos = e @ e.T
        k = len(e)
        total += (cos.sum() - np.trace(cos)) / (k * (k - 1))
        n += 1
    return total / n


@pytest.mark.parametrize("factorised", [False, True])
def test_recommend_tensor_diversity(factorised, gemm_mode):
    rec, items = build_small_app(factorised)
    model, V = rec.model, rec.model.vocab_size
    batches = [rec.dataloader.prepare_inference(list(items[s:s + 9])) for s in (0, 30, 60, 95, 140)]
    batch = {key: torch.from_numpy(np.concatenate([np.asarray(b[key]) for b in batches], axis=0)) for key in batches[0]}
    k, pool = 8, 60
    plain = model.recommend_tensor(batch, k=k)
    same = model.recommend_tensor(batch, k=k, diversity=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, same))
    zero = model.recommend_tensor(batch, k=k, diversity=0.0)
    assert torch.equal(zero[0], plain[0]) and torch.equal(zero[1], plain[1]) and torch.equal(zero[2], plain[2])
    div = model.recommend_tensor(batch, k=k, diversity=0.7, pool=pool)
    cand = model.recommend_tensor(batch, k=pool)
    assert div[0].shape == (plain[0].shape[0], k) and torch.equal(div[2], plain[2])
    for row, c_row in zip(div[0].cpu().tolist(), cand[0].cpu().tolist()):
        assert set(row) <= set(c_row) and len(set(row)) == k
    table = model.engine.view("word_embeddings/embeddings").cpu().numpy()
    assert table.shape == (V, 64)
    lam = engine_mod.check_rerank_args(k, pool, 0.7)[2]
    want = dref.rerank(table, device_rnorm(model), cand[0].cpu().numpy(), cand[1].cpu().numpy(), lam, k)
    assert np.array_equal(div[0].cpu().numpy(), want[0]) and bits_equal(div[1].cpu().numpy(), want[1])
    assert not torch.equal(div[0], plain[0])
    t64 = table.astype(np.float64)
    assert mean_pairwise_cosine(t64, div[0].cpu().tolist()) <= mean_pairwise_cosine(t64, plain[0].cpu().tolist())
    # the default pool: min(1024, max(10 k, 50)) = 80 candidates
    d80 = model.recommend_tensor(batch, k=k, diversity=0.7)
    c80 = model.recommend_tensor(batch, k=80)
    assert np.array_equal(d80[0].cpu().numpy(), dref.rerank(table, device_rnorm(model), c80[0].cpu().numpy(), c80[1].cpu().numpy(), lam, k)[0])
    lists = model.recommend(batch, k=k, diversity=0.7, pool=pool)
    assert [ids for per_row in lists for ids, _ in per_row] == div[0].cpu().tolist()
    for bad in (dict(diversity=1.5), dict(diversity=-0.1), dict(diversity=0.5, pool=k - 1), dict(diversity=0.5, pool=1025), dict(pool=50)):
        with pytest.raises(ValueError):
            model.recommend_tensor(batch, k=k, **bad)


def test_recommend_batch_with_diversity_and_allowed_items():
    rec, items = build_small_app()
    histories = [items[s:s + n] for s, n in ((0, 15), (40, 3), (90, 30), (120, 1), (7, 22))]
    allowed = items[::3]
    plain = rec.recommend_batch(histories, 5, allowed_items=allowed)
    assert rec.recommend_batch(histories, 5, allowed_items=allowed, diversity=0.0) == plain
    got = rec.recommend_batch(histories, 5, allowed_items=allowed, diversity=0.5)
    assert all(len(lst) == 5 and len(set(lst)) == 5 and set(lst) <= set(allowed) for lst in got)
    assert all(not set(lst) & set(h) for lst, h in zip(got, histories))          # and nothing the user has seen
    small = rec.recommend_batch(histories, 5, allowed_items=allowed, diversity=0.5, candidate_pool=5)
    assert [sorted(lst) for lst in small] == [sorted(lst) for lst in plain]       # a pool of k: the same items, in MMR order
    assert rec(histories[0], 5, allowed_items=allowed, diversity=0.5) == got[0]
    assert rec(histories[0], 5, diversity=0.5) == rec.recommend_batch(histories[:1], 5, diversity=0.5)[0]
    with pytest.raises(ValueError):
        rec.recommend_batch(histories, 5, diversity=0.5, candidate_pool=4)
