"""Full-catalogue top K and held-out rank (b4r_rank_full) on the GPU: the op against the C oracle and numpy, its edges, and the
model / evaluator / app layers built on it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, dataloaders, datasets, evaluation
from bert4rec_amd.apps import Recommender
from oracle import bert4rec_oracle as orc
from tests.b4r_testlib import P, stream
from tests.test_gpu_api import make_model, oracle_of

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32P, I64P = C.POINTER(C.c_float), C.POINTER(C.c_int64)


def c_oracle():
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
    so = os.path.join(here, "librank_oracle.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", here])
    return C.CDLL(so)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.float32)


def oracle_scores(hidden, table, bias):
    """rank_oracle_scores of every row against every item: [R, V] float32."""
    hidden, table, bias = (np.ascontiguousarray(x, dtype=np.float32) for x in (hidden, table, bias))
    R, H = hidden.shape
    V = table.shape[0]
    cand = np.ascontiguousarray(np.tile(np.arange(V, dtype=np.int64), (R, 1)))
    out = np.zeros((R, V), np.float32)
    c_oracle().rank_oracle_scores(hidden.ctypes.data_as(F32P), table.ctypes.data_as(F32P), bias.ctypes.data_as(F32P),
                                  cand.ctypes.data_as(I64P), C.c_int64(R), C.c_int64(V), C.c_int64(H), out.ctypes.data_as(F32P))
    return out


def allowed_mask(V, first, exclude, gt):
    R = exclude.shape[0]
    ok = np.ones((R, V), bool)
    ok[:, :first] = False
    for r in range(R):
        ex = exclude[r]
        ex = ex[(ex >= 0) & (ex < V)]
        ok[r, ex] = False
        if gt is not None and first <= gt[r] < V:
            ok[r, gt[r]] = True
    return ok


def expected(sc, ok, gt, K):
    """numpy: stable descending order over the allowed ids, truncated / padded to K; gt_rank by the counting formula."""
    R, V = sc.shape
    ids = np.full((R, K), -1, np.int64)
    ranks = np.zeros(R, np.int64)
    for r in range(R):
        order = np.argsort(-sc[r].astype(np.float64), kind="stable")
        order = order[ok[r, order]][:K]
        ids[r, :len(order)] = order
        if gt is not None and ok[r].any() and 0 <= gt[r] < V and ok[r, gt[r]]:
            s, g = sc[r], gt[r]
            j = np.arange(V)
            ranks[r] = 1 + int((ok[r] & (s > s[g])).sum()) + int((ok[r] & (s == s[g]) & (j < g)).sum())
    return ids, ranks


def run_full(hidden_d, H, table_d, bias_d, V, first, exclude, gt, K, R=None, hidden_row=None, hidden_ld=None, scratch_bytes=None,
             outputs=True):
    lib = _lib.load()
    R = exclude.shape[0] if R is None else R
    E = exclude.shape[1] if exclude is not None else 0
    ex_d = torch.as_tensor(exclude).to(DEV).contiguous() if exclude is not None and E > 0 else None
    gt_d = torch.as_tensor(gt).to(DEV) if gt is not None else None
    hr_d = torch.as_tensor(hidden_row).to(DEV) if hidden_row is not None else None
    ids = torch.full((max(R, 1), max(K, 1)), 7, dtype=torch.int64, device=DEV)
    scores = torch.full((max(R, 1), max(K, 1)), 7.0, device=DEV)
    gt_rank = torch.full((max(R, 1),), -7, dtype=torch.int32, device=DEV)
    need = int(lib.b4r_rank_full_scratch_bytes(R, V, K))
    nbytes = need if scratch_bytes is None else scratch_bytes
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    rc = lib.b4r_rank_full(P(hidden_d), hidden_ld or H, P(hr_d), P(table_d), P(bias_d), H, V, first, R, P(ex_d), E if ex_d is not None else 0,
                           P(gt_d), K, P(ids) if outputs else None, P(scores) if outputs else None,
                           P(gt_rank) if gt is not None else None, P(scratch), nbytes, stream())
    torch.cuda.synchronize()
    return rc, ids[:R, :K].cpu().numpy(), scores[:R, :K].cpu().numpy(), gt_rank[:R].cpu().numpy().astype(np.int64)


def make_case(R, H, V, seed, E=40, first=3):
    hidden, table, bias = rnd(R, H, seed=seed), rnd(V, H, seed=seed + 1, scale=0.05), rnd(V, seed=seed + 2, scale=0.01)
    # planted exact ties: duplicated rows (inside a chunk, across the 1024-id chunk boundary, at the top ids), zeros of both signs
    for a, b in ((7, 3), (4, 3), (1030, 1020), (V - 1, 11), (V - 2, 11)):
        if a < V and b < V and a != b:
            bias[b] = 3.0                     # lifted into every row's top K
            table[a] = table[b]; bias[a] = bias[b]
    if V > 200:
        table[100] = 0.0; bias[100] = 0.0
        table[200] = 0.0; bias[200] = -0.0
    rng = np.random.default_rng(seed)
    gt = rng.integers(first, V, size=R).astype(np.int64)
    ex = rng.integers(0, V, size=(R, E)).astype(np.int64)
    ex[:, 1] = ex[:, 0]                       # duplicates
    ex[:, 2] = -1                             # padding
    ex[:, 3] = V + 5                          # out of range
    ex[:, 4] = -9
    ex[::2, 5] = gt[::2]                      # gt listed: still ranked
    ex[:, 6] = 1                              # a special id listed
    if R > 1:
        ex[1, 7] = 11                         # one of a tie pair excluded
    return hidden, table, bias, ex, gt


CASES = [  # (R, H, V, K)
    (4, 32, 5, 10),
    (24, 64, 3709, 100),
    (20, 128, 8193, 1024),
    (17, 256, 26732, 10),
    (3, 1024, 3709, 1),
    (2, 128, 335423, 100),
    (2, 64, 335423, 1024),
]


@pytest.mark.parametrize("R,H,V,K", CASES, ids=[f"R{c[0]}_H{c[1]}_V{c[2]}_K{c[3]}" for c in CASES])
def test_rank_full_bit_exact(R, H, V, K):
    hidden, table, bias, ex, gt = make_case(R, H, V, seed=R * 31 + H + V % 97)
    if V == 5:
        ex[:, 7:] = -1
    sc = oracle_scores(hidden.numpy(), table.numpy(), bias.numpy())
    ok = allowed_mask(V, 3, ex, gt)
    want_ids, want_rank = expected(sc, ok, gt, K)
    hd, td, bd = hidden.to(DEV), table.to(DEV), bias.to(DEV)
    rc, ids, scores, ranks = run_full(hd, H, td, bd, V, 3, ex, gt, K)
    assert rc == 0, _lib.last_error()
    assert np.array_equal(ids, want_ids)
    valid = ids >= 0
    rows = np.nonzero(valid)[0]
    assert np.array_equal(scores[valid].view(np.uint32), sc[rows, ids[valid]].view(np.uint32)), "scores not bit-identical"
    assert (scores[~valid] == -np.inf).all()
    assert np.array_equal(ranks, want_rank)
    if V == 5:
        assert (~valid).any(), "K > |allowed| must leave a -1 / -inf tail"
    # the whole-vocabulary ranking of b4r_rank_candidates, filtered, gives the same list
    if V <= 26732:
        lib = _lib.load()
        ranking = torch.empty(R, V, dtype=torch.int64, device=DEV)
        need = int(lib.b4r_rank_scratch_bytes(R, V))
        scr = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=DEV)
        _lib.check(lib.b4r_rank_candidates(P(hd), H, None, P(td), P(bd), H, V, None, R, V, None, P(ranking), None, None,
                                           P(scr), need, stream()))
        full = ranking.cpu().numpy()
        for r in range(R):
            f = full[r][ok[r, full[r]]][:K]
            assert np.array_equal(ids[r, :len(f)], f)
    # hidden rows by index, with a leading dimension > H: the same answer
    ld = H + 4
    wide = torch.zeros(R + 2, ld)
    perm = np.random.default_rng(1).permutation(R + 2)[:R]
    wide[perm, :H] = hidden
    rc, ids2, scores2, ranks2 = run_full(wide.to(DEV), H, td, bd, V, 3, ex, gt, K, hidden_row=torch.as_tensor(perm, dtype=torch.int64),
                                         hidden_ld=ld)
    assert rc == 0 and np.array_equal(ids2, ids) and np.array_equal(scores2.view(np.uint32), scores.view(np.uint32))
    assert np.array_equal(ranks2, ranks)


def test_rank_full_edges():
    lib = _lib.load()
    R, H, V, K = 40, 64, 5000, 10
    hidden, table, bias, ex, gt = make_case(R, H, V, seed=5)
    hd, td, bd = hidden.to(DEV), table.to(DEV), bias.to(DEV)
    # a row that excludes every item (and has no ranked gt), a row whose gt is a special id
    ex_all = np.full((R, V + 10), -1, np.int64)
    ex_all[:, :ex.shape[1]] = ex
    ex_all[0, :V] = np.arange(V)
    gt2 = gt.copy()
    gt2[0] = -1
    gt2[1] = 2
    sc = oracle_scores(hidden.numpy(), table.numpy(), bias.numpy())
    ok = allowed_mask(V, 3, ex_all, gt2)
    want_ids, want_rank = expected(sc, ok, gt2, K)
    rc, ids, scores, ranks = run_full(hd, H, td, bd, V, 3, ex_all, gt2, K)
    assert rc == 0, _lib.last_error()
    assert (ids[0] == -1).all() and (scores[0] == -np.inf).all() and ranks[0] == 0 and ranks[1] == 0
    assert np.array_equal(ids, want_ids) and np.array_equal(ranks, want_rank)
    # a scratch for 16 rows: the rows go in groups, same answer; two calls: bitwise the same
    small = int(lib.b4r_rank_full_scratch_bytes(16, V, K))
    rc, ids_g, scores_g, ranks_g = run_full(hd, H, td, bd, V, 3, ex_all, gt2, K, scratch_bytes=small)
    assert rc == 0 and np.array_equal(ids_g, ids) and np.array_equal(scores_g.view(np.uint32), scores.view(np.uint32))
    assert np.array_equal(ranks_g, ranks)
    rc, ids_b, scores_b, ranks_b = run_full(hd, H, td, bd, V, 3, ex_all, gt2, K)
    assert rc == 0 and np.array_equal(ids_b, ids) and np.array_equal(scores_b.view(np.uint32), scores.view(np.uint32))
    assert np.array_equal(ranks_b, ranks)
    # K = 0: only the ranks; no exclude list; R = 0
    rc, _, _, ranks0 = run_full(hd, H, td, bd, V, 3, ex_all, gt2, 0)
    assert rc == 0 and np.array_equal(ranks0, ranks)
    rc, ids_n, _, ranks_n = run_full(hd, H, td, bd, V, 3, None, gt2, K, R=R)
    okn = allowed_mask(V, 3, np.full((R, 1), -1, np.int64), gt2)
    wn_ids, wn_rank = expected(sc, okn, gt2, K)
    assert rc == 0 and np.array_equal(ids_n, wn_ids) and np.array_equal(ranks_n, wn_rank)
    rc, _, _, _ = run_full(hd, H, td, bd, V, 3, ex_all[:0], gt2[:0], K)
    assert rc == 0
    # errors, not faults
    rc, _, _, _ = run_full(hd, H, td, bd, V, 3, ex_all, gt2, K, scratch_bytes=small // 2)
    assert rc == -5
    rc, *_ = run_full(hd, H, td, bd, V, 3, ex_all, gt2, K, scratch_bytes=0)
    assert rc == -5
    rc, *_ = run_full(None, H, td, bd, V, 3, ex_all, gt2, K)
    assert rc == -1
    rc, *_ = run_full(hd, H, td, bd, V, 3, ex_all, gt2, 1025)
    assert rc == -2
    rc, *_ = run_full(hd, 30, td, bd, V, 3, ex_all, gt2, K)
    assert rc == -2
    rc, *_ = run_full(hd, H, td, bd, V, 3, ex_all, gt2, K, hidden_ld=H - 4)
    assert rc == -2
    assert lib.b4r_rank_full(P(hd), H, None, P(td), P(bd), H, V, 3, R, None, 5, None, K, None, None, None, None, 0, stream()) == -1
    assert "b4r_rank_full" in _lib.last_error()
    assert lib.b4r_rank_full_scratch_bytes(256, 335423, 100) < 256 * 335423 * 4 // 4


@pytest.mark.parametrize("K", (100, 1024))
def test_rank_full_rows_of_equal_scores(K):
    """A zero hidden row under a constant bias: every score of the row is the bias, so the 32 score bits are resolved at once
    (kmin == kmax) and the id bits alone decide: the sweep's two 8-bit passes over the local id (K = 100: each chunk holds more than
    K) and the merge's four over the id (K = 1024).  17 rows (a
    second, partly filled tile), three chunks with the last partly beyond V; one row keeps five ids (K beyond the allowed set), one
    none."""
    R, H, V = 17, 8, 2049 + 3
    hidden, table, bias, ex, gt = make_case(R, H, V, seed=77)
    bias[:] = 0.5
    hidden[0] = 0.0
    hidden[16] = 0.0
    ex_all = np.full((R, V), -1, np.int64)
    ex_all[:, :ex.shape[1]] = ex
    ex_all[2, :V - 5] = np.arange(5, V)          # row 2: ids 3 and 4 (of 0 .. 4) are left, and gt
    ex_all[3] = np.arange(V)                     # row 3: nothing but gt
    gt[3] = -1
    sc = oracle_scores(hidden.numpy(), table.numpy(), bias.numpy())
    assert (sc[0].view(np.uint32) == np.float32(0.5).view(np.uint32)).all() and (sc[16] == sc[0]).all()
    ok = allowed_mask(V, 3, ex_all, gt)
    want_ids, want_rank = expected(sc, ok, gt, K)
    rc, ids, scores, ranks = run_full(hidden.to(DEV), H, table.to(DEV), bias.to(DEV), V, 3, ex_all, gt, K)
    assert rc == 0, _lib.last_error()
    assert np.array_equal(ids, want_ids) and np.array_equal(ranks, want_rank)
    valid = ids >= 0
    assert np.array_equal(scores[valid].view(np.uint32), sc[np.nonzero(valid)[0], ids[valid]].view(np.uint32))
    assert (scores[~valid] == -np.inf).all()
    assert (np.diff(ids[0]) > 0).all() and valid[0].all()          # equal scores: ascending ids
    assert valid[2].sum() == ok[2].sum() <= 3 and not valid[3].any()


def test_recommend_tensor_against_op_and_oracle():
    V = 300
    model = make_model(V, seed=17)
    batch = orc.synthetic_batch(128, 24, 6, V, seed=9, ragged=True)
    ids, scores, slots = model.recommend_tensor(batch, k=10)
    R = int(slots.numel())
    assert ids.shape == (R, 10) and scores.shape == (R, 10) and R == int(batch["masked_lm_weights"].sum())
    # bit-exact against the op on the transformed hidden states the model formed
    hidden, slots2, _ = model._ranked_slot_hidden(batch)
    assert torch.equal(slots2, slots)
    b_idx = (slots // 6).cpu()
    seen = batch["input_word_ids"][b_idx]
    ids_op, scores_op, _ = model.engine.rank_full(hidden, None, seen, 3, None, 10)
    assert torch.equal(ids_op, ids) and torch.equal(scores_op.view(torch.int32), scores.view(torch.int32))
    ids_h = ids.cpu().numpy()
    for r in range(R):
        assert not set(ids_h[r].tolist()) & (set(seen[r].tolist()) | {0, 1, 2})
    # end to end against the oracle's forward: identical top 10 up to logit ties within 2e-4
    cfg_o, params = oracle_of(model)
    logits = orc.model_forward(params, batch, cfg_o)["mlm_logits"].reshape(-1, V)[slots.cpu()].numpy()
    same = []
    for r in range(R):
        ok = np.ones(V, bool)
        ok[:3] = False
        ok[seen[r].numpy()] = False
        order = np.argsort(-logits[r].astype(np.float64), kind="stable")
        order = order[ok[order]][:10]
        eq = np.array_equal(order, ids_h[r])
        same.append(eq)
        if not eq:
            top = logits[r][order]
            assert float(np.min(top[:-1] - top[1:])) < 2e-4, f"slot {r}: top-10 differs without a tie"
    assert np.mean(same) >= 0.999, np.mean(same)
    # extra exclusions and the list form
    extra = torch.full((128, 2), -1, dtype=torch.int64)
    extra[:, 0] = torch.as_tensor(ids_h[np.searchsorted(b_idx.numpy(), np.arange(128)).clip(0, R - 1), 0])
    ids_x, _, _ = model.recommend_tensor(batch, k=10, exclude=extra)
    for r in range(R):
        assert int(extra[b_idx[r], 0]) not in ids_x[r].tolist()
    lists = model.recommend(batch, k=10)
    assert sum(len(x) for x in lists) == R and lists[int(b_idx[0])][0][0] == ids_h[0].tolist()


def _eval_batches(V, n=3, labels_gt_only=False):
    out = []
    for i in range(n):
        b = orc.synthetic_batch(32, 24, 6, V, seed=70 + i, ragged=True, finetune=True)
        if labels_gt_only:
            w = b["masked_lm_weights"].bool()
            lab = torch.zeros_like(b["labels"])
            for r in range(lab.shape[0]):
                lab[r, 0] = b["masked_lm_ids"][r][w[r]][0]
            b["labels"] = lab
        out.append(b)
    return out


def test_evaluator_full_ranking():
    V = 300
    model = make_model(V, seed=19)
    batches = _eval_batches(V)
    ev = evaluation.get(full_ranking=True)
    om = orc.EvalMetrics()
    for b in batches:
        ranks = ev.evaluate_batch(model, b).cpu().numpy().astype(np.int64)
        w = b["masked_lm_weights"] != 0
        b_idx, p_idx = torch.nonzero(w, as_tuple=True)
        slots = (b_idx * w.shape[1] + p_idx).cuda()
        hidden, _, _ = model._ranked_slot_hidden(b, slots)
        sc = oracle_scores(hidden.cpu().numpy(), model.engine.view("word_embeddings/embeddings").cpu().numpy(),
                           model.engine.view("cls/predictions/output_bias/bias").cpu().numpy())
        gt = b["masked_lm_ids"][b_idx, p_idx].numpy()
        ok = allowed_mask(V, 3, b["labels"][b_idx].numpy(), gt)
        _, want = expected(sc, ok, gt, 0)
        assert np.array_equal(ranks, want)
        for r in want.tolist():
            om.update(int(r))
    got = ev.get_metrics_results()
    for key, v in om.results().items():
        assert got[key] == pytest.approx(v, abs=1e-12), key
    # labels = gt and PAD only: the rank is gt's place in rank_items(items=None) with the special ids removed
    ev2 = evaluation.get(full_ranking=True)
    for b in _eval_batches(V, n=1, labels_gt_only=True):
        ranks = ev2.evaluate_batch(model, b).cpu().numpy()
        full = model.rank_items(b)
        w = b["masked_lm_weights"] != 0
        i = 0
        for row, lists in enumerate(full):
            gts = b["masked_lm_ids"][row][w[row]].tolist()
            for lst, g in zip(lists, gts):
                order = [x for x in lst.cpu().tolist() if x >= 3]
                assert ranks[i] == 1 + order.index(g)
                i += 1
    # the sampled protocol is untouched by the new switch
    pop = (np.random.default_rng(3).zipf(1.3, size=5000) % (V - 3) + 3).tolist()
    smp = dataloaders.samplers.get("pop_random", source=pop, vocab=list(range(V)), sample_size=100)
    a = evaluation.get(sampler=smp, seed=4)
    c = evaluation.get(sampler=smp, seed=4, full_ranking=False)
    assert a._device_sampler_ready(model) and c._device_sampler_ready(model)
    for b in batches:
        a.evaluate_batch(model, b)
        c.evaluate_batch(model, b)
    assert a.get_metrics_results() == c.get_metrics_results()


def test_recommend_batch_equals_single_calls():
    ds = datasets.synthetic_dataset(n_users=30, n_items=200, min_len=5, max_len=30, seed=4)
    dl = dataloaders.get_dataloader_factory("bert4rec").create_ml_1m_dataloader(data_source=ds, max_seq_len=24, max_predictions_per_seq=6)
    dl.generate_vocab()
    model = make_model(dl.tokenizer.get_vocab_size(), seed=5)
    items = dl.create_item_list()
    histories = [items[s:s + n] for s, n in ((0, 15), (40, 3), (90, 30), (120, 1), (7, 22))]
    rec = Recommender(model, dl)
    for k in (1, 5):
        got = rec.recommend_batch(histories, k)
        assert got == [rec(h, k) for h in histories]
