"""The evaluation path at every cell of both matrices (tests/inference_matrix.py) and in every mode the cell runs in, against the
restatement in float64 (tests/activation_ref.py with the parameters cast to double; tests/inference_checks.py):

Engine.encoder_forward(ranked_rows_only=True) -> mlm_transform_rows -> rank_full / rank_candidates -> rank_metrics,

on an evaluation-shaped batch: fine-tune rows (one valid slot, every other slot (position 0, id 0)) with a row of length 1, a row of
full length, a row whose slot is not its last token and a row with two slots.  Per cell and mode, in this order:

1. forms: the forward's launch labels parse to the cell's inference record; where the last layer runs the attention block, whether
   it swept every query is read from the rows of its context the forward wrote;
2. no stale reads: over a workspace filled with NaN every ranked row of sequence_output and every transformed row is finite, and the
   result is bitwise that of a run over a workspace filled with another constant;
3. hidden rows: sequence_output at the ranked rows and mlm_transform_rows's output against the fp64 rows;
4. scores: rank_full's and rank_candidates's scores against the fp64 logits of the same ids;
5. rankings, every row judged (tol = twice check 4's bound): returned ids allowed and distinct, their fp64 scores never rising by
   more than tol, the last one within tol of the k-th best allowed, gt_rank inside the interval of ranks the ground truth takes
   when its fp64 score moves by +-tol; and bit-exact against oracle/rank_oracle.c on the hidden rows this test formed;
6. the public surface on the same cell and batch: rank_items_tensor handed the rows (the evaluator's resident batches) is bitwise
   the op-level chain above.  recommend_tensor, rank_items_tensor without rows and the evaluator's evaluate_batch run the dense
   encoder forward (workspace key (B, L, 0)): that chain is held to checks 3 - 5 op by op with the same bounds, and the public
   results must equal it bitwise; get_metrics_results() equals orc.EvalMetrics fed those ranks to 1e-12;
7. (test_shape_changes_on_one_engine) L changes from batch to batch on one engine: every result bitwise that of a fresh engine.

Bounds of checks 3 and 4: tests/inference_checks.py (16 e32 exact fp32, min(512 e32, 1e-3) bf16x3, 5e-2 mode 2; e32 the fp32
restatement's own error against fp64 at that cell and quantity).  Every figure is printed before it is asserted.

Measured on an MI355X, worst over the cells, the same for both chains (the bound of that cell in brackets; DESIGN.md section 4.6
has the table and mode 2 per cell; the test prints "MEASURED cell [mode] chain quantity: err, e32, bound" for every case):

* exact fp32: hidden rows 7.6e-6 (h1024hd32 [3.2e-5]), scores 2.9e-6 (h1024hd32 [1.7e-5]) -- at most 30 % of a bound;
* bf16x3: hidden rows 2.9e-5 (b128_L225 [1e-3]), scores 1.2e-5 (h1024hd32 [5.4e-4]) -- at most 5 % of a bound;
* bf16: hidden rows 8.3e-3, scores 1.9e-3 (both h1024hd64_e256 [5e-2]); hidden 64 1e-6, hidden 128 / 256 3e-4 ... 5e-3.

90 cell cases and 5 shape-change cases, about 10 s."""
import functools

import numpy as np
import pytest
import torch

from bert4rec_amd import evaluation, models
from bert4rec_amd.models.components import networks
from oracle import bert4rec_oracle as orc
from tests import feature_matrix as fm
from tests import geometry_matrix as gm
from tests import inference_checks as ic
from tests import inference_matrix as im
from tests import test_gpu_feature_matrix as tfm
from tests import test_gpu_geometry as tgm
from tests.test_gpu_feature_matrix import matrix_mode, parse_forward  # noqa: F401 (matrix_mode: a fixture)
from tests.test_gpu_full_rank import expected, oracle_scores
from tests.test_gpu_train_step import launch_labels

pytestmark = pytest.mark.gpu

DEV = "cuda"
K = ic.TOP_K
NAN = float("nan")
OTHER_FILL = -7.5


def build_cell(c):
    """the cell's model from its own matrix's build_cell, dropout 0: (oracle config, engine, parameters)"""
    if c.matrix == "feature":
        return tfm.build_cell(fm.CELLS[c.name], od=0.0, ad=0.0)
    return tgm.build_cell(gm.CELLS[c.name], od=0.0, ad=0.0)


@functools.lru_cache(maxsize=None)
def cell_reference(name):
    """per cell, shared by its modes: the batch, its ranked slots, the fp64 restatement on them and e32 per quantity (CPU)"""
    c = im.CELLS[name]
    cfg_o, params = ic.cell_params(c)
    batch = ic.eval_batch(im.BATCH, c.L, c.P, c.V)
    ref64 = ic.restatement(params, batch, cfg_o, c.acts, torch.float64)
    e32 = ic.e32_of(ic.restatement(params, batch, cfg_o, c.acts, torch.float32), ref64)
    return params, batch, ic.ranked_slots(batch), ref64, e32


def run_forward(eng, batch, rk, ranked_rows_only, fill=None, labels_cap=0):
    """the encoder forward of the evaluation path and the transform on the ranked rows; fill: the whole workspace tensor first"""
    cb, keep = eng.prepare_batch(batch)
    B, L, P = cb.B, cb.L, cb.P
    key_p = P if ranked_rows_only else 0
    ws = eng.workspace(B, L, key_p, encoder_only=ranked_rows_only)
    if fill is not None:
        ws.fill_(fill)
    labels = None
    if labels_cap:
        labels = launch_labels(lambda: eng.encoder_forward(cb, ranked_rows_only=ranked_rows_only), cap=labels_cap)
    else:
        eng.encoder_forward(cb, ranked_rows_only=ranked_rows_only)
    assert eng.workspace(B, L, key_p, encoder_only=ranked_rows_only) is ws
    seq = eng.region("sequence_output", B, L, key_p, encoder_only=ranked_rows_only)
    rows = rk.rows.to(DEV)
    hidden = eng.mlm_transform_rows(seq, rows)
    torch.cuda.synchronize()
    return {"labels": labels, "sequence_output": seq[rows].clone(), "mlm_hidden": hidden, "shape": (B, L, key_p)}


def rank_ops(eng, hidden, rk, ex_eval, ex_rec, cand):
    ids_e, sc_e, rank_e = eng.rank_full(hidden, None, ex_eval, ic.FIRST_ITEM, rk.gt, K)
    ids_r, sc_r, _ = eng.rank_full(hidden, None, ex_rec, ic.FIRST_ITEM, None, K)
    ranking, rank_c, sc_c = eng.rank_candidates(hidden, None, torch.from_numpy(cand), rk.gt, want_ranking=True, want_scores=True)
    torch.cuda.synchronize()
    return {"ids_e": ids_e, "sc_e": sc_e, "rank_e": rank_e, "ids_r": ids_r, "sc_r": sc_r, "ranking": ranking, "rank_c": rank_c,
            "sc_c": sc_c}


def assert_forms(labels, c, mode):
    attn, ffn, emb_proj, emb_fused, slotq_rows = parse_forward(labels, c, im.BATCH)
    want = c.forms(mode)
    got = im.InferenceForms(tuple(attn), tuple(ffn), emb_proj, emb_fused, want.slot_only_last, slotq_rows)
    print(f"forms [{mode}]: {got}")
    assert got == want, f"forms of the {mode} encoder-only forward: {got}, expected {want}\n{labels}"
    assert not any(l.startswith(("masked-LM head", "zero fill")) for l in labels), labels


def check_against_fp64(tag, mode, c, eng, fwd, ops, rk, ref64, e32, ex_eval, ex_rec, cand):
    """checks 3 - 5 on one chain's results"""
    V = c.V
    # 3. hidden rows
    err = {q: float((fwd[q].cpu().double() - ref64[q]).abs().max()) for q in ("sequence_output", "mlm_hidden")}
    # 4. scores of the returned ids
    s64 = ref64["scores"].numpy()
    c64 = np.take_along_axis(s64, cand, 1)
    score_errs = []
    for key_ids, key_sc in (("ids_e", "sc_e"), ("ids_r", "sc_r")):
        ids, sc = ops[key_ids].cpu().numpy(), ops[key_sc].cpu().numpy().astype(np.float64)
        valid = ids >= 0
        assert np.isneginf(sc[~valid]).all() and np.isfinite(sc[valid]).all(), f"{tag}: rank_full scores"
        r_idx = np.nonzero(valid)[0]
        if valid.any():
            score_errs.append(float(np.abs(sc[valid] - s64[r_idx, ids[valid]]).max()))
    score_errs.append(float(np.abs(ops["sc_c"].cpu().numpy().astype(np.float64) - c64).max()))
    err["scores"] = max(score_errs)
    bounds = {q: ic.bound(mode, e32[q]) for q in ic.QUANTITIES}
    for q in ic.QUANTITIES:
        print(f"MEASURED {c.name} [{mode}] {tag} {q}: err {err[q]:.3e} e32 {e32[q]:.3e} bound {bounds[q]:.3e} "
              f"ratio-to-e32 {err[q] / e32[q]:.1f}")
    for q in ic.QUANTITIES:
        assert bounds[q] <= (ic.BF16_BOUND if mode == "bf16" else ic.CONTRACT), (q, bounds[q])
        assert err[q] <= bounds[q], f"{tag} {q}: {err[q]:.3e} > {bounds[q]:.3e} (e32 {e32[q]:.3e})"
    # 5. rankings, every row
    tol = 2 * bounds["scores"]
    gt = rk.gt.numpy()
    ok_e, ok_r = ic.allowed(V, ex_eval.numpy(), gt), ic.allowed(V, ex_rec.numpy())
    ic.check_top_k(ops["ids_e"].cpu().numpy(), s64, ok_e, K, tol, f"{tag} rank_full (evaluator's exclusions)")
    ic.check_top_k(ops["ids_r"].cpu().numpy(), s64, ok_r, K, tol, f"{tag} rank_full (recommend's exclusions)")
    ic.check_gt_ranks(ops["rank_e"].cpu().numpy(), s64, gt, tol, ok_e, f"{tag} rank_full")
    g = cand.shape[1] - 1
    ic.check_gt_ranks(ops["rank_c"].cpu().numpy(), c64, [g] * len(cand), tol, None, f"{tag} rank_candidates")
    ranking = ops["ranking"].cpu().numpy()
    for r in range(len(cand)):
        assert sorted(ranking[r].tolist()) == sorted(cand[r].tolist()), f"{tag} row {r}: the ranking is not the candidates"
        s = s64[r, ranking[r]]
        assert (s[1:] - s[:-1] <= tol).all(), f"{tag} row {r}: candidate ranking rises by {float((s[1:] - s[:-1]).max()):.2e}"
    # ... and the ranking kernels themselves, bit-exact on these hidden rows against oracle/rank_oracle.c
    sc = oracle_scores(fwd["mlm_hidden"].cpu().numpy(), eng.view("word_embeddings/embeddings").cpu().numpy(),
                       eng.view("cls/predictions/output_bias/bias").cpu().numpy())
    want_ids, want_rank = expected(sc, ok_e, gt, K)
    ids = ops["ids_e"].cpu().numpy()
    assert np.array_equal(ids, want_ids) and np.array_equal(ops["rank_e"].cpu().numpy().astype(np.int64), want_rank), tag
    valid = ids >= 0
    assert np.array_equal(ops["sc_e"].cpu().numpy()[valid].view(np.uint32), sc[np.nonzero(valid)[0], ids[valid]].view(np.uint32)), tag
    csc = np.take_along_axis(sc, cand, 1)
    assert np.array_equal(ops["sc_c"].cpu().numpy().view(np.uint32), csc.view(np.uint32)), f"{tag}: candidate scores not bit-identical"
    want_ranking, _ = orc.rank_candidates(csc, cand)
    assert np.array_equal(ranking, want_ranking), tag
    assert np.array_equal(ops["rank_c"].cpu().numpy().astype(np.int64), orc.rank_of_ground_truth(want_ranking, gt)), tag


def public_model(c, params):
    enc = networks.Bert4RecEncoder(c.V, c.H, c.layers, c.heads, c.L, c.inner, inner_activation=c.acts[0], output_dropout=0.0,
                                   attention_dropout=0.0, embedding_width=c.E, device=DEV)
    model = models.BERT4RecModel(enc, mlm_activation=c.acts[1])
    model.engine.load_named(params)
    return model


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


def metrics_of(ranks):
    om = orc.EvalMetrics()
    for r in ranks:
        om.update(int(r))
    return om.results()


CASES = [pytest.param(name, mode, id=f"{name}-{mode}") for name, c in im.CELLS.items() for mode in c.modes]


@pytest.mark.parametrize("name,matrix_mode", CASES, indirect=["matrix_mode"])
def test_evaluation_path_of_every_cell_follows_the_fp64_restatement(name, matrix_mode):
    c, mode = im.CELLS[name], matrix_mode
    params, batch, rk, ref64, e32 = cell_reference(name)
    cfg_o, eng, built = build_cell(c)
    assert set(built) == set(params) and all(torch.equal(built[n], params[n]) for n in params), "build_cell's parameters"
    ex_eval, ex_rec, extra = ic.exclusion_lists(batch, rk, c.V)
    cand = ic.draw_candidates(c.V, rk.gt.numpy())
    R = int(rk.rows.numel())
    assert R == im.BATCH + 1

    # 1. forms (over a workspace of NaN, which check 2 reads) -------------------------------------------------------------------
    fwd = run_forward(eng, batch, rk, True, fill=NAN, labels_cap=64 + 24 * c.layers)
    assert_forms(fwd["labels"], c, mode)
    if c.forms(mode).attn_fwd[-1] == "Block":
        ctx = eng.region(f"attention_context_{c.layers - 1}", im.BATCH, c.L, c.P, encoder_only=True)
        dense = bool(torch.isfinite(ctx).all())
        assert dense == c.sweeps_every_query(mode), f"dense sweep of the last block forward: {dense}"
    # 2. no stale reads -----------------------------------------------------------------------------------------------------------
    for q in ("sequence_output", "mlm_hidden"):
        assert bool(torch.isfinite(fwd[q]).all()), f"{q}: a ranked row read the workspace's fill"
    again = run_forward(eng, batch, rk, True, fill=OTHER_FILL)
    for q in ("sequence_output", "mlm_hidden"):
        assert same_bits(fwd[q], again[q]), f"{q} depends on what the workspace held"
    # 3 - 5 -------------------------------------------------------------------------------------------------------------------------
    ops = rank_ops(eng, fwd["mlm_hidden"], rk, ex_eval, ex_rec, cand)
    check_against_fp64("ranked-rows", mode, c, eng, fwd, ops, rk, ref64, e32, ex_eval, ex_rec, cand)

    # 6. the public surface ---------------------------------------------------------------------------------------------------------
    model = public_model(c, params)
    gt_d, cand_t = rk.gt.to(DEV), torch.from_numpy(cand)
    ranking, gt_rank, slots, _ = model.rank_items_tensor(batch, cand_t, gt_d, slots=rk.slots.to(DEV), rows=rk.rows.to(DEV))
    assert same_bits(ranking, ops["ranking"]) and same_bits(gt_rank, ops["rank_c"]), "rank_items_tensor on the ranked rows"
    # ... and what runs the dense encoder forward: op by op within the same bounds, then bitwise through the public calls
    dense_fwd = run_forward(eng, batch, rk, False, fill=NAN)
    for q in ("sequence_output", "mlm_hidden"):
        assert bool(torch.isfinite(dense_fwd[q]).all()), f"dense forward, {q}"
    dops = rank_ops(eng, dense_fwd["mlm_hidden"], rk, ex_eval, ex_rec, cand)
    check_against_fp64("dense", mode, c, eng, dense_fwd, dops, rk, ref64, e32, ex_eval, ex_rec, cand)
    ids, scores, slots = model.recommend_tensor(batch, k=K, exclude_seen=True, exclude=extra)
    assert torch.equal(slots.cpu(), rk.slots)
    assert same_bits(ids, dops["ids_r"]) and same_bits(scores, dops["sc_r"]), "recommend_tensor"
    ranking, gt_rank, slots, counts = model.rank_items_tensor(batch, cand_t, gt_d)
    assert torch.equal(slots.cpu(), rk.slots) and counts == batch["masked_lm_weights"].sum(dim=1).tolist()
    assert same_bits(ranking, dops["ranking"]) and same_bits(gt_rank, dops["rank_c"]), "rank_items_tensor"
    ev = evaluation.get(full_ranking=True)
    ranks = ev.evaluate_batch(model, batch)
    assert same_bits(ranks, dops["rank_e"]), "full-ranking evaluate_batch"
    got = ev.get_metrics_results()
    for key, v in metrics_of(dops["rank_e"].cpu().tolist()).items():
        assert got[key] == pytest.approx(v, abs=1e-12), key
    ev = evaluation.get()
    ranks = ev.evaluate_batch(model, batch, cand, rk.gt.numpy())
    assert same_bits(torch.as_tensor(ranks).to(DEV), dops["rank_c"]), "sampled-protocol evaluate_batch with given candidates"
    got = ev.get_metrics_results()
    for key, v in metrics_of(dops["rank_c"].cpu().tolist()).items():
        assert got[key] == pytest.approx(v, abs=1e-12), key


# ---- 7. shape changes on one engine ------------------------------------------------------------------------------------------------------
def chain_at(eng, c, L, P, fill=None):
    """the op-level chain at (BATCH, L, P): forms from the labels, hidden rows, top k"""
    batch = ic.eval_batch(im.BATCH, L, P, c.V)
    rk = ic.ranked_slots(batch)
    fwd = run_forward(eng, batch, rk, True, fill=fill, labels_cap=64 + 24 * c.layers)
    ids, sc, rank = eng.rank_full(fwd["mlm_hidden"], None, batch["labels"][rk.b_idx], ic.FIRST_ITEM, rk.gt, K)
    torch.cuda.synchronize()
    forms = parse_forward(fwd["labels"], c._replace(L=L, P=P), im.BATCH)
    swept = None   # over a workspace of NaN: whether the last layer's attention block swept every query (no label tells)
    if fill is not None and forms[0][-1] == "Block":
        swept = bool(torch.isfinite(eng.region(f"attention_context_{c.layers - 1}", im.BATCH, L, P, encoder_only=True)).all())
    return forms, swept, (fwd["sequence_output"], fwd["mlm_hidden"], ids, sc, rank)


SHAPE_CASES = [pytest.param(name, mode, id=f"{name}-{mode}") for name, mode in im.SHAPE_CHANGES]


@pytest.mark.parametrize("name,matrix_mode", SHAPE_CASES, indirect=["matrix_mode"])
def test_shape_changes_on_one_engine_give_a_fresh_engines_results(name, matrix_mode):
    """the evaluator's trim_padding: (B, L, P), then a shorter or longer L' that takes other forms, then (B, L, P) again, all in the
    one workspace buffer the engine keeps for the largest shape -- each bitwise the result of a fresh engine at that shape"""
    c = im.CELLS[name]
    (L, P), (L2, P2) = im.SHAPE_CHANGES[(name, matrix_mode)]
    _, eng, _ = build_cell(c)
    seen = []
    for step, (l, p) in enumerate(((L, P), (L2, P2), (L, P))):
        forms, _, got = chain_at(eng, c, l, p)
        _, fresh_eng, _ = build_cell(c)
        fresh_forms, swept, want = chain_at(fresh_eng, c, l, p, fill=NAN)
        print(f"{name} [{matrix_mode}] step {step} (L {l}, P {p}): {forms}, last block swept every query: {swept}")
        assert forms == fresh_forms
        for a, b, what in zip(got, want, ("sequence_output rows", "transformed rows", "top-k ids", "top-k scores", "gt_rank")):
            assert same_bits(a, b), f"step {step} (L {l}, P {p}): {what} differ from a fresh engine's"
        seen.append((forms, swept))
    assert seen[0] == seen[2] and seen[0] != seen[1], "the shape in between must take other forms"
    assert len({id(w) for w in eng._ws.values()}) <= 2   # (the shapes share the buffer of the largest one)
