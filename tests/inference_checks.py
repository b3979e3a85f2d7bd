"""What tests/test_gpu_inference_matrix.py asks of the evaluation path, as functions that need no GPU: the evaluation-shaped batch
with its edge rows, the float64 restatement on the ranked rows, the bounds derived from the restatement's own fp32 error, and the
interval criteria that judge every ranked row.  tests/test_inference_matrix_host.py runs the fp32 restatement through the same
functions: the reference has to pass its own criteria.

Bounds (e32 = the largest absolute difference between the fp32 and the fp64 restatement of the same quantity at that cell):

* exact fp32: 16 e32 -- the same arithmetic in another summation order;
* bf16x3: 512 e32, never above the 1e-3 contract -- three-term products carry 2^-17 relative against fp32's 2^-24 (a ratio of 128),
  margin 4;
* bf16 (mode 2): DESIGN.md section 4.6's eval-logits bound, 5e-2 absolute; the hidden rows (LayerNorm outputs of unit scale, larger
  than the logits) are held to the same absolute figure, which is relatively the tighter of the two."""
from typing import Dict, NamedTuple

import numpy as np
import torch

from oracle import bert4rec_oracle as orc
from tests import activation_ref as ar
from tests.b4r_testlib import set_row_slots

FIRST_ITEM = 3          # [PAD] 0, [MASK] 1, [UNK] 2 are never ranked
TOP_K = 10
NEGATIVES = 100
CONTRACT = 1e-3
BF16_BOUND = 5e-2
QUANTITIES = ("sequence_output", "mlm_hidden", "scores")


def eval_batch(B, L, P, V, seed=31):
    """fine-tune rows (one valid slot on the last real token, every other slot (position 0, id 0)) of ragged lengths, and by hand:
    row 0 of length 1 (its slot at position 0, shared with the padding slots), row 1 of full length, row 2 with its valid slot not on
    its last token, row 3 with two valid slots"""
    assert B >= 8 and P >= 2 and L >= 8
    batch = orc.synthetic_batch(B, L, P, V, seed=seed + L, ragged=True, finetune=True)
    rng = np.random.default_rng(seed)

    def resize(row, n):
        seq = torch.from_numpy(rng.integers(FIRST_ITEM, V, size=n).astype(np.int64))
        batch["labels"][row] = 0
        batch["labels"][row, :n] = seq
        batch["input_mask"][row] = 0
        batch["input_mask"][row, :n] = 1

    resize(0, 1)
    set_row_slots(batch, 0, [0], orc.MASK_TOKEN_ID)
    resize(1, L)
    set_row_slots(batch, 1, [L - 1], orc.MASK_TOKEN_ID)
    n2 = int(batch["input_mask"][2].sum())
    set_row_slots(batch, 2, [n2 // 2 - 1], orc.MASK_TOKEN_ID)
    n3 = int(batch["input_mask"][3].sum())
    set_row_slots(batch, 3, [1, n3 - 1], orc.MASK_TOKEN_ID)
    return batch


class Ranked(NamedTuple):
    b_idx: torch.Tensor    # [R] batch row of every ranked slot, batch order then slot order
    slots: torch.Tensor    # [R] b * P + p
    rows: torch.Tensor     # [R] b * L + position: the row of sequence_output the slot reads
    gt: torch.Tensor       # [R] the slot's ground truth


def ranked_slots(batch) -> Ranked:
    w = batch["masked_lm_weights"] != 0
    assert bool((w == (batch["masked_lm_ids"] != 0)).all())
    b_idx, p_idx = torch.nonzero(w, as_tuple=True)
    L, P = batch["input_word_ids"].shape[1], w.shape[1]
    rows = b_idx * L + batch["masked_lm_positions"][b_idx, p_idx]
    assert int(torch.unique(rows).numel()) == int(rows.numel())
    return Ranked(b_idx, b_idx * P + p_idx, rows, batch["masked_lm_ids"][b_idx, p_idx])


def restatement(params, batch, cfg_o, acts, dtype) -> Dict[str, torch.Tensor]:
    """tests/activation_ref.model_forward in `dtype`, on the ranked slots: sequence_output [R, H], mlm_hidden [R, E], scores [R, V]"""
    rk = ranked_slots(batch)
    out = ar.model_forward({n: p.to(dtype) for n, p in params.items()}, batch, cfg_o, *acts)
    B, L, H = out["sequence_output"].shape
    assert out["mlm_logits"].dtype == dtype
    return {"sequence_output": out["sequence_output"].reshape(B * L, H)[rk.rows],
            "mlm_hidden": out["mlm_hidden"].reshape(-1, out["mlm_hidden"].shape[-1])[rk.slots],
            "scores": out["mlm_logits"].reshape(-1, out["mlm_logits"].shape[-1])[rk.slots]}


def e32_of(ref32, ref64) -> Dict[str, float]:
    return {q: float((ref32[q].double() - ref64[q]).abs().max()) for q in QUANTITIES}


def bound(mode: str, e32: float) -> float:
    if mode == "f32":
        return 16.0 * e32
    if mode == "bf16x3":
        return min(512.0 * e32, CONTRACT)
    assert mode == "bf16"
    return BF16_BOUND


def exclusion_lists(batch, rk: Ranked, V, seed=5):
    """what the two full-catalogue protocols exclude per ranked row: the evaluator the user's whole sequence (`labels`; the ground truth
    stays ranked), recommend_tensor the row's input_word_ids and a caller's list (here: two drawn ids and the -1 padding)"""
    extra = torch.full((batch["labels"].shape[0], 3), -1, dtype=torch.int64)
    extra[:, :2] = torch.from_numpy(np.random.default_rng(seed).integers(FIRST_ITEM, V, size=(extra.shape[0], 2)))
    return batch["labels"][rk.b_idx], torch.cat([batch["input_word_ids"][rk.b_idx], extra[rk.b_idx]], dim=1), extra


def allowed(V, exclude, gt=None) -> np.ndarray:
    """[R, V] bool: ids a full-catalogue ranking may return (b4r_rank_full: not below FIRST_ITEM, not excluded; the ground truth always)"""
    exclude = np.asarray(exclude)
    ok = np.ones((exclude.shape[0], V), bool)
    ok[:, :FIRST_ITEM] = False
    for r in range(exclude.shape[0]):
        ex = exclude[r]
        ok[r, ex[(ex >= 0) & (ex < V)]] = False
        if gt is not None and FIRST_ITEM <= int(gt[r]) < V:
            ok[r, int(gt[r])] = True
    return ok


def draw_candidates(V, gt, seed=7) -> np.ndarray:
    """[R, C]: NEGATIVES distinct items other than the ground truth (fewer where the vocabulary has fewer), the ground truth last"""
    rng = np.random.default_rng(seed)
    n = min(NEGATIVES, V - FIRST_ITEM - 1)
    out = np.zeros((len(gt), n + 1), np.int64)
    for r, g in enumerate(np.asarray(gt)):
        pool = np.setdiff1d(np.arange(FIRST_ITEM, V), [g])
        out[r, :n] = rng.permutation(pool)[:n]
        out[r, n] = g
    return out


def rank_interval(scores64: np.ndarray, g: int, tol: float, ok=None):
    """the closed interval of 1-based ranks entry g takes among the (allowed) entries when its fp64 score is moved by +-tol"""
    ok = np.ones(scores64.shape, bool) if ok is None else ok.copy()
    ok[g] = False
    s = scores64[g]
    return 1 + int((ok & (scores64 > s + tol)).sum()), 1 + int((ok & (scores64 >= s - tol)).sum())


def check_top_k(ids, ref64, ok, k, tol, what=""):
    """every row of a returned top-k list [R, k] (-1 where fewer than k ids are allowed) against the fp64 scores [R, V]"""
    ids, ref64 = np.asarray(ids), np.asarray(ref64)
    for r in range(ids.shape[0]):
        n_ok = int(ok[r].sum())
        got = ids[r]
        n = min(k, n_ok)
        assert (got[:n] >= 0).all() and (got[n:] == -1).all(), f"{what} row {r}: {got} for {n_ok} allowed ids"
        got = got[:n]
        assert ok[r, got].all(), f"{what} row {r}: an id that is not allowed in {got}"
        assert len(set(got.tolist())) == n, f"{what} row {r}: duplicates in {got}"
        if n == 0:
            continue
        s = ref64[r, got]
        assert (s[1:] - s[:-1] <= tol).all(), f"{what} row {r}: fp64 scores rise by {float((s[1:] - s[:-1]).max()):.2e} > {tol:.2e}"
        kth = np.sort(ref64[r, ok[r]])[::-1][n - 1]
        assert s[-1] >= kth - tol, f"{what} row {r}: the last id scores {s[-1]:.6f}, the {n}-th best allowed {kth:.6f} (tol {tol:.2e})"


def check_gt_ranks(ranks, ref64, gt_index, tol, ok=None, what=""):
    """ranks [R] against the interval of every row; ref64 [R, C] the fp64 scores of the ranked entries, gt_index [R] the ground truth's"""
    ranks = np.asarray(ranks)
    for r in range(ranks.shape[0]):
        lo, hi = rank_interval(np.asarray(ref64[r]), int(gt_index[r]), tol, None if ok is None else ok[r])
        assert lo <= int(ranks[r]) <= hi, f"{what} row {r}: gt_rank {int(ranks[r])} outside [{lo}, {hi}] (tol {tol:.2e})"


def stable_top_k(scores, ok, k):
    """ids [R, k] by descending score over the allowed ids, ties to the lower id, -1 padded; and the counting-formula rank helper"""
    scores = np.asarray(scores)
    ids = np.full((scores.shape[0], k), -1, np.int64)
    for r in range(scores.shape[0]):
        order = np.argsort(-scores[r].astype(np.float64), kind="stable")
        order = order[ok[r, order]][:k]
        ids[r, :len(order)] = order
    return ids


def counted_rank(scores, g, ok=None):
    scores = np.asarray(scores)
    ok = np.ones(scores.shape, bool) if ok is None else ok
    j = np.arange(scores.shape[0])
    return 1 + int((ok & (scores > scores[g])).sum()) + int((ok & (scores == scores[g]) & (j < g)).sum())


def cell_params(c, seed=3):
    """the oracle config (dropout 0) and the parameters build_cell of either matrix loads: the oracle's initialisers (the factorised
    ones with a table of width E) with biases, betas and gammas made non-trivial"""
    from tests import factorized_ref as fr
    cfg_o = orc.OracleConfig(vocab_size=c.V, hidden_size=c.H, num_layers=c.layers, num_attention_heads=c.heads,
                             max_sequence_length=c.L, inner_dim=c.inner, output_dropout=0.0, attention_dropout=0.0)
    if c.E:
        return cfg_o, fr.init_params(cfg_o, c.E, seed)
    params = orc.init_params(cfg_o, seed)
    g = torch.Generator().manual_seed(seed + 1)
    for n, p in params.items():
        if n.endswith(("bias", "beta")):
            p.copy_(torch.randn(p.shape, generator=g) * 0.02)
        elif n.endswith("gamma"):
            p.copy_(1.0 + torch.randn(p.shape, generator=g) * 0.05)
    return cfg_o, params
