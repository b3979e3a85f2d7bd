"""Item ranks (b4r_item_ranks, b4r_rank_metrics_multi) without a GPU: the CPU restatement (tests/item_ranks_ref.py) against a
brute-force comparison sort and hand-worked metric cases, the library's argument checks (they return before any launch), the Python
layers' own, and next_n_batches on a small log."""
import functools
import math

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, dataloaders, datasets, evaluation, models
from bert4rec_amd import engine as engine_mod
from bert4rec_amd.apps import Recommender
from bert4rec_amd.evaluation import evaluation_metrics as em
from tests import catalogue_ref as ref
from tests import item_ranks_ref as iref

F32 = np.float32
FIRST = 3


def small_case(seed=0, R=5, H=8, V=70, Q=14):
    rng = np.random.default_rng(seed)
    table = (rng.standard_normal((V, H)) * 0.5).astype(F32)
    table[9] = table[5]; table[40] = table[5]          # exact ties between items
    table[20] = 0.0; table[21] = -0.0
    hidden = rng.standard_normal((R, H)).astype(F32)
    hidden[2] = 0.0                                    # every score ties: only the ids order
    sc = ref.chain_scores(hidden, table)
    sc[3, 30] = -0.0; sc[3, 31] = 0.0                  # signed zeros compare equal
    ex = rng.integers(0, V, size=(R, 6)).astype(np.int64)
    mask = rng.random(V) < 0.7
    words = ref.pack_bits(mask)
    row_filter = np.array([0, -1, 0, 5, 0][:R], np.int32)
    ok = ref.allowed_mask(V, FIRST, ex, None, R, words, row_filter)
    ok[4] = False                                      # an empty row
    query = rng.integers(FIRST, V, size=(R, Q)).astype(np.int64)
    query[:, 0] = 5; query[:, 1] = 9; query[:, 2] = 40; query[:, 3] = query[:, 0]        # ties, and a repeated id
    query[:, 4:9] = [-1, V, 1 << 40, -(1 << 40), 1]                                     # padding and an id below first_item
    query[:, 9] = ex[:, 0]                                                              # an excluded id
    query[:, 10] = np.flatnonzero(~mask)[3]                                             # a filtered id
    query[3, 11] = 30; query[3, 12] = 31
    return sc, ok, query


def brute_force(sc_row, ok_row, query_row, mode):
    """ranks by a comparison sort of the ranked items: a stands before b iff s_a > s_b, or s_a == s_b and a < b"""
    V = sc_row.shape[0]
    valid = [FIRST <= int(q) < V for q in query_row]
    ranked = set(np.flatnonzero(ok_row).tolist())
    if mode == iref.JOINT:
        ranked |= {int(q) for q, v in zip(query_row, valid) if v}

    def before(a, b):
        sa, sb = float(sc_row[a]), float(sc_row[b])
        return sa > sb or (sa == sb and a < b)
    order = sorted(ranked, key=functools.cmp_to_key(lambda a, b: -1 if before(a, b) else (1 if before(b, a) else 0)))
    out = []
    for q, v in zip(query_row, valid):
        q = int(q)
        if not v or (mode == iref.STRICT and not ok_row[q]):
            out.append(0)
        elif q in ranked:
            out.append(order.index(q) + 1)
        else:
            out.append(1 + sum(1 for j in order if before(j, q)))
    return out, len(order)


@pytest.mark.parametrize("mode", [iref.STRICT, iref.SELF, iref.JOINT])
def test_restatement_equals_a_comparison_sort(mode):
    for seed in (0, 1):
        sc, ok, query = small_case(seed)
        ranks, scores, row_n, member = iref.item_ranks(sc, ok, query, FIRST, mode)
        for r in range(sc.shape[0]):
            want, n = brute_force(sc[r], ok[r], query[r], mode)
            assert ranks[r].tolist() == want and row_n[r] == n, (seed, r)
        V = sc.shape[1]
        valid = (query >= FIRST) & (query < V)
        assert np.isneginf(scores[~valid]).all() and (member[~valid] == 0).all() and (ranks[~valid] == 0).all()
        safe = np.where(valid, query, 0)
        assert np.array_equal(scores[valid], np.take_along_axis(sc, safe, 1)[valid])
        assert np.array_equal(member[valid], np.take_along_axis(ok, safe, 1)[valid].astype(np.uint8))
        assert np.array_equal(ranks[:, 0], ranks[:, 3])                           # a repeated id: the same rank
        if mode == iref.STRICT:
            assert (ranks[4] == 0).all() and row_n[4] == 0                          # the empty row
            assert ((ranks > 0) == (member == 1)).all()
        elif mode == iref.SELF:
            assert (ranks[4][valid[4]] == 1).all() and row_n[4] == 0
        else:
            distinct = [len({int(q) for q, v in zip(query[r], valid[r]) if v}) for r in range(len(query))]
            assert row_n[4] == distinct[4]
            for r in range(len(query)):                                             # distinct ids have distinct joint ranks
                got = {int(q): int(k) for q, k, v in zip(query[r], ranks[r], valid[r]) if v}
                assert len(set(got.values())) == len(got)
            assert ranks[3, 12] == ranks[3, 11] + 1                                 # -0.0 and +0.0 tie: the lower id stands first


def test_self_mode_is_rank_full_gt_rank():
    sc, ok, query = small_case(2)
    R, V = sc.shape
    ranks, _, _, _ = iref.item_ranks(sc, ok, query, FIRST, iref.SELF)
    for i in range(query.shape[1]):
        gt = query[:, i]
        ok_gt = ok.copy()
        for r in range(R):
            if FIRST <= gt[r] < V:
                ok_gt[r, gt[r]] = True
        _, _, want = ref.expected(sc, ok_gt, gt, 0, FIRST)
        assert np.array_equal(ranks[:, i], want), i


def test_metric_restatement_on_hand_worked_rows():
    l2 = math.log2
    rho = [1, 3]
    assert iref.row_gain(rho, iref.COUNT, 0) == 2.0
    assert iref.row_gain(rho, iref.HIT, 1) == 1.0 and iref.row_gain([2, 3], iref.HIT, 1) == 0.0
    assert iref.row_gain(rho, iref.RECALL, 2) == 0.5 and iref.row_gain(rho, iref.RECALL, 3) == 1.0
    assert iref.row_gain(rho, iref.NDCG, 2) == pytest.approx(1.0 / (1.0 + 1.0 / l2(3)), rel=1e-15)
    assert iref.row_gain(rho, iref.NDCG, 3) == pytest.approx((1.0 + 1.0 / l2(4)) / (1.0 + 1.0 / l2(3)), rel=1e-15)
    assert iref.row_gain([1, 2], iref.NDCG, 5) == 1.0                                  # the ideal list
    assert iref.row_gain(rho, iref.MAP, 2) == 0.5                                      # (1 / min(2, 2)) * (1 / 1)
    assert iref.row_gain(rho, iref.MAP, 3) == pytest.approx((1.0 + 2.0 / 3.0) / 2.0, rel=1e-15)
    assert iref.row_gain([2, 5, 9], iref.MAP, 1) == 0.0 and iref.row_gain([2, 5, 9], iref.MAP, 5) == pytest.approx((0.5 + 0.4) / 3, rel=1e-15)
    assert iref.row_gain(rho, iref.MRR, 0) == 1.0 and iref.row_gain([4, 2], iref.MRR, 0) == 0.5
    assert iref.row_gain(rho, iref.AUC, 0, 10) == (1.0 + (1.0 - 1.0 / 8.0)) / 2.0       # one wrong item before the second target
    assert iref.row_gain([1, 2], iref.AUC, 0, 10) == 1.0 and iref.row_gain([9, 10], iref.AUC, 0, 10) == 0.0
    assert iref.row_gain([1, 2], iref.AUC, 0, 2) == 1.0                                # nothing but targets
    table = [(iref.COUNT, 0), (iref.HIT, 2), (iref.RECALL, 2), (iref.MRR, 0)]
    sums, users = iref.multi_metrics(np.array([[1, 3, 0], [0, 0, 0], [0, 4, 2]]), np.array([10, 10, 10]), table)
    assert users == 2 and sums == [4.0, 2.0, 1.0, 1.5]


def test_one_target_gives_the_single_target_metrics():
    ranks = np.array([1, 2, 3, 5, 6, 10, 11, 40, 1000], np.int64)
    for k in (1, 5, 10):
        assert [iref.row_gain([int(v)], iref.HIT, k) for v in ranks] == em.HR(k).gain(ranks).tolist()
        assert np.allclose([iref.row_gain([int(v)], iref.NDCG, k) for v in ranks], em.NDCG(k).gain(ranks), rtol=1e-15, atol=0)
        assert [iref.row_gain([int(v)], iref.RECALL, k) for v in ranks] == em.HR(k).gain(ranks).tolist()
    assert np.allclose([iref.row_gain([int(v)], iref.MRR, 0) for v in ranks], em.MAP().gain(ranks), rtol=1e-15, atol=0)
    assert np.allclose([iref.row_gain([int(v)], iref.MAP, 2000) for v in ranks], em.MAP().gain(ranks), rtol=1e-15, atol=0)
    assert (iref.COUNT, iref.HIT, iref.NDCG, iref.MRR) == (em.GAIN_COUNT, em.GAIN_HIT, em.GAIN_NDCG, em.GAIN_RECIPROCAL)


def test_lib_binds_the_new_symbols():
    lib = _lib.load()
    for name in ("b4r_item_ranks", "b4r_item_ranks_scratch_bytes", "b4r_rank_metrics_multi"):
        assert name in _lib.PROTOTYPES, name
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    size = lib.b4r_item_ranks_scratch_bytes
    assert size(0, 100, 4) == 0 and size(4, 0, 4) == 0 and size(4, 100, 257) == 0 and size(4, 100, -1) == 0
    assert 0 < size(16, 1000, 0) < size(16, 1000, 1) < size(16, 1000, 256) < size(17, 1000, 256)
    assert size(256, 335423, 256) == size(256, 3709, 256) < 256 * 335423 // 4          # it does not grow with the catalogue
    assert (engine_mod.MGAIN_COUNT, engine_mod.MGAIN_HIT, engine_mod.MGAIN_NDCG, engine_mod.MGAIN_MRR, engine_mod.MGAIN_RECALL,
            engine_mod.MGAIN_MAP, engine_mod.MGAIN_AUC) == (iref.COUNT, iref.HIT, iref.NDCG, iref.MRR, iref.RECALL, iref.MAP, iref.AUC)


def test_c_abi_refuses_bad_arguments_before_touching_the_device():
    import ctypes as C
    lib = _lib.load()
    table = np.zeros(64 * 8 + 4, F32)
    tp = (table.ctypes.data + 15) & ~15                                 # (never read: every call below returns before a launch)

    def call(R=4, H=64, ld=None, V=1000, first=3, E=0, exclude=None, Q=2, query=tp, members=0, hidden=tp, tab=tp, allow=None,
             n_filters=0, scratch=None, scratch_bytes=0):
        return lib.b4r_item_ranks(hidden, H if ld is None else ld, None, tab, None, H, V, first, R, exclude, E, allow, n_filters, None,
                                  None, query, Q, members, tp, None, tp, None, scratch, scratch_bytes, None)
    for kw in (dict(Q=257), dict(Q=-1), dict(R=-1), dict(E=-1), dict(first=-1), dict(H=30), dict(H=4100), dict(ld=60), dict(V=0),
               dict(allow=tp, n_filters=0)):
        assert call(**kw) == -2 and "b4r_item_ranks" in _lib.last_error(), kw
    for m in (3, -1, 100):
        assert call(members=m) == -1 and "members" in _lib.last_error()
    assert call(R=0) == 0 and call(R=0, members=2, Q=256) == 0          # nothing to do: no launch, no pointer is looked at
    assert call(R=0, members=3) == -1                                   # (the mode is checked whatever R is)
    assert call(hidden=None) == -1 and call(tab=None) == -1 and "null" in _lib.last_error()
    assert call(query=None) == -1 and "query_ids" in _lib.last_error()
    assert call(E=3) == -1 and "exclude" in _lib.last_error()
    assert call(tab=tp + 4) == -3
    need = lib.b4r_item_ranks_scratch_bytes(16, 1000, 2)
    assert call() == -5 and call(scratch=tp, scratch_bytes=16) == -5 and "scratch" in _lib.last_error()
    assert call(R=40, scratch=tp, scratch_bytes=need - 65) == -5         # below one group of 16 rows

    fam = lambda *f: (C.c_int32 * len(f))(*f)

    def metrics(ranks=tp, row_n=tp, R=4, Q=3, families=(0, 1), n=None, sums=tp, users=tp):
        f = fam(*families)
        return lib.b4r_rank_metrics_multi(ranks, row_n, R, Q, f, fam(*([5] * len(families))), len(families) if n is None else n, sums, users,
                                          None)
    assert metrics(families=(0, 6), row_n=None) == -1 and "AUC" in _lib.last_error()
    assert metrics(ranks=None) == -1 and metrics(sums=None) == -1 and metrics(users=None) == -1
    assert metrics(families=(7,)) == -1 and metrics(families=(-1,)) == -1 and "family" in _lib.last_error()
    for kw in (dict(R=0), dict(Q=0), dict(Q=257), dict(n=0), dict(families=tuple([0] * 33))):
        assert metrics(**kw) == -2 and "b4r_rank_metrics_multi" in _lib.last_error(), kw


def test_check_item_ranks_args():
    check = engine_mod.check_item_ranks_args
    q, Q, mode = check(np.array([[5, -1, 7]], np.int32), 1, "joint")
    assert q.dtype == torch.int64 and Q == 3 and mode == 2
    assert check(torch.zeros((4, 0), dtype=torch.int64))[1:] == (0, 0) and check(torch.zeros((2, 256), dtype=torch.int64), 2, "self")[1:] == (256, 1)
    assert check(torch.zeros((2, 300), dtype=torch.int64), 2, "self", None)[1] == 300
    for bad in (dict(query_ids=torch.zeros((2, 257), dtype=torch.int64)), dict(query_ids=torch.zeros(3, dtype=torch.int64)),
                dict(query_ids=torch.zeros((2, 3))), dict(query_ids=torch.zeros((2, 3), dtype=torch.bool)),
                dict(query_ids=torch.zeros((2, 3), dtype=torch.int64), n_rows=3),
                dict(query_ids=torch.zeros((2, 3), dtype=torch.int64), members="all"),
                dict(query_ids=torch.zeros((2, 3), dtype=torch.int64), members=2)):
        with pytest.raises(ValueError):
            check(**bad)


def test_python_layers_refuse_bad_arguments_before_any_work():
    model = object.__new__(models.BERT4RecModel)            # the checks come before anything of the model is touched
    ids = torch.zeros((2, 300), dtype=torch.int64)
    with pytest.raises(ValueError, match="joint"):
        models.BERT4RecModel.item_ranks_tensor(model, {}, ids, members="joint")
    with pytest.raises(ValueError, match="members"):
        models.BERT4RecModel.item_ranks_tensor(model, {}, ids, members="every")
    with pytest.raises(ValueError, match="query_ids"):
        models.BERT4RecModel.item_ranks_tensor(model, {}, torch.zeros((2, 3)))
    rec = Recommender(None, None)
    with pytest.raises(ValueError, match="items"):
        rec.item_ranks([[1, 2]])
    with pytest.raises(ValueError, match="items"):
        rec.item_ranks([[1, 2]], items=[1], items_per_user=[[1]])
    with pytest.raises(ValueError, match="item lists"):
        rec.item_ranks([[1, 2]], items_per_user=[[1], [2]])
    with pytest.raises(ValueError, match="not both"):
        rec.item_ranks([[1, 2]], items=[1], allowed_items=[1], allowed_items_per_user=[[1]])
    with pytest.raises(ValueError, match="full_ranking"):
        evaluation.get(multi_target=True)
    for kw in (dict(list_k=5), dict(distribution=True), dict(list_k=5, sample_seed=1), dict(list_k=5, calibrate_by=np.zeros(10, np.int64)),
               dict(list_k=5, diversity=0.5), dict(list_k=5, max_per_group=(np.zeros(10, np.int64), 1))):
        with pytest.raises(ValueError, match="multi_target"):
            evaluation.get(full_ranking=True, multi_target=True, **kw)
    with pytest.raises(ValueError, match="cut-offs"):
        evaluation.get(full_ranking=True, multi_target=True, metrics=[em.HR(k) for k in range(1, 9)])
    ev = evaluation.get(full_ranking=True, multi_target=True)
    names = [f"{m}@{k}" for k in (1, 5, 10) for m in ("Recall", "HR", "NDCG", "MAP")] + ["MRR", "AUC", "Valid Ranks"]
    assert list(ev.multi_target_results()) == names and set(ev.multi_target_results().values()) == {0.0}
    assert set(names) <= set(ev.get_metrics_results())
    assert list(evaluation.get(full_ranking=True, multi_target=True, metrics=[em.HR(3), em.NDCG(20)]).multi_target_results())[:8] == \
        [f"{m}@{k}" for k in (3, 20) for m in ("Recall", "HR", "NDCG", "MAP")]
    plain = evaluation.get(full_ranking=True)
    assert not plain.multi_target and plain.multi_target_results() == {} and "Recall@5" not in plain.get_metrics_results()
    ev.reset_metrics()
    assert ev.multi_target_results()["MRR"] == 0.0

    class Cpu:                                               # a model without a GPU engine
        engine = None
    with pytest.raises(ValueError, match="GPU"):
        ev.evaluate_batch(Cpu(), {})


def small_loader():
    ds = datasets.synthetic_dataset(n_users=12, n_items=60, min_len=2, max_len=14, seed=3)
    dl = dataloaders.get_dataloader_factory("bert4rec").create_ml_1m_dataloader(data_source=ds, max_seq_len=8, max_predictions_per_seq=3)
    dl.generate_vocab()
    return dl


def test_next_n_batches():
    dl = small_loader()
    tok = dl.get_tokenizer()
    items = dl.create_item_list()
    V = tok.get_vocab_size()
    seqs = [items[0:9], items[10:13], items[20:22], items[30:36] + ["no such item", items[40]], items[50:53] + [items[50]] * 2, [items[5]]]
    n = 3
    batches, skipped = evaluation.next_n_batches(dl, seqs, n, batch_size=2)
    assert skipped == 3 and [b["target_ids"].shape for b in batches] == [(2, n), (1, n)]      # 3, 2 and 1 items: left out
    assert tok.get_vocab_size() == V                                                          # the unknown target was not added
    kept = [seqs[0], seqs[3], seqs[4]]
    rows = {key: np.concatenate([b[key] for b in batches]) for key in batches[0]}
    assert rows["target_ids"].dtype == np.int64
    for i, seq in enumerate(kept):
        want = dl.prepare_inference(list(seq[:-n]))
        for key, v in want.items():
            assert np.array_equal(rows[key][i], np.asarray(v)[0]), key
        assert (rows["masked_lm_weights"][i] != 0).sum() == 1
        targets = [tok.tokenize(x) if x != "no such item" else -1 for x in seq[-n:]]
        assert rows["target_ids"][i].tolist() == targets
    assert rows["target_ids"][1].tolist()[1] == -1
    assert evaluation.next_n_batches(dl, [], 2) == ([], 0) and evaluation.next_n_batches(dl, [items[:2]], 2) == ([], 1)
    for bad in (dict(n=0), dict(n=1.5), dict(n=True), dict(n=2, batch_size=0)):
        with pytest.raises(ValueError):
            evaluation.next_n_batches(dl, seqs, **bad)
