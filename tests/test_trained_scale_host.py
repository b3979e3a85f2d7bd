"""tests/trained_scale.py is what it claims to be, without a GPU: the six cells cover every launch form of a train step, the planted
rows of the batch are there, the two levels are as sharp as stated on the fp64 reference at every cell, and the fp32 restatement
passes the criteria the device is held to (tests/test_gpu_trained_scale.py) -- with room, so that no bound is vacuous:

* forward quantities and the loss: 16 e32 below the contract term 1e-3 max(1, max |ref64|);
* gradients, per tensor: e32g below the gradient contract G (2e-3 without dropout, 5e-3 in training mode).  16 e32g may exceed G at
  the sharp level (the key-bias gradients, analytically zero and measured against the floor): the exact-fp32 bound is then 16 e32g
  and the bf16x3 bound G;
* accuracy: the fp32 argmax is the fp64 one at every weighted slot whose two best fp64 logits lie further apart than the logits
  bound, and fewer than 5 % of the slots lie closer."""
import pytest
import torch

from tests import feature_matrix as fm
from tests import inference_checks as ic
from tests import inference_matrix as im
from tests import trained_scale as ts
from tests.test_feature_matrix_host import SPLIT_FORMS, pairs

CASES = [pytest.param(name, level, id=f"{name}-{level}") for name in ts.CELLS for level in ts.LEVELS]


def test_cells_cover_every_form_of_a_train_step():
    """between their split and exact-fp32 records: attention forward Block, Core, SlotQuery, Core64; backward Block, BlockFolded,
    Core16, Core32, SlotQuery, Core64; feed-forward Block, Wide, CompactRows, TileProducts; emb_fused, emb_proj, slot_only_last,
    slotq_rows (and the gathered compact rows)"""
    got = set()
    for name in ts.CELLS:
        modes = ts.modes_of(name)
        assert "bf16x3" in modes, name
        for mode in modes:
            got |= pairs(fm.CELLS[name].forms(mode))
    assert got == SPLIT_FORMS, (sorted(SPLIT_FORMS - got), sorted(got - SPLIT_FORMS))
    assert any("f32" in ts.modes_of(n) for n in ts.CELLS)
    assert set(ts.EVAL_PATH_CELLS) <= set(ts.CELLS)
    assert {fm.CELLS[n].head_dim for n in ts.EVAL_PATH_CELLS} == {32, 64}


@pytest.mark.parametrize("name", ts.CELLS)
def test_batch_holds_every_planted_row(name):
    c = fm.CELLS[name]
    b = ts.cell_batch(name)
    assert b["input_word_ids"].shape == (ts.BATCH, c.L) and b["masked_lm_ids"].shape == (ts.BATCH, c.P)
    lens = b["input_mask"].sum(dim=1)
    for r in range(ts.BATCH):   # masks are prefixes; valid slots lie on [MASK] tokens inside them and carry the label
        n = int(lens[r])
        assert bool(b["input_mask"][r, :n].all()) and n >= 1
        w = b["masked_lm_weights"][r] != 0
        assert bool((w == (b["masked_lm_ids"][r] != 0)).all())
        pos = b["masked_lm_positions"][r][w]
        assert bool((pos < n).all()) and pos.unique().numel() == pos.numel()
        assert bool((b["input_word_ids"][r, pos] == 1).all()) and bool((b["labels"][r, pos] == b["masked_lm_ids"][r][w]).all())
        assert bool((b["masked_lm_positions"][r][~w] == 0).all())
    weights = b["masked_lm_weights"].sum(dim=1)
    assert int(lens[ts.ROW_SINGLE]) == 1 and int(weights[ts.ROW_SINGLE]) == 1
    assert int(lens[ts.ROW_FULL]) == c.L and int(weights[ts.ROW_FULL]) >= min(c.P, 2)
    if c.L >= 65:
        assert int(lens[ts.ROW_SHORT]) <= 32 and int(weights[ts.ROW_SHORT]) >= 1
    n = int(lens[ts.ROW_REPEAT])
    item, count = torch.unique(b["labels"][ts.ROW_REPEAT, :n], return_counts=True)
    top = int(item[count.argmax()])
    assert 2 * int(count.max()) >= n and top >= ic.FIRST_ITEM
    assert int((b["input_word_ids"][ts.ROW_REPEAT, :n] == top).sum()) >= n // 3          # many contributions to that item's row
    assert int((b["masked_lm_ids"][ts.ROW_REPEAT] == top).sum()) >= 1                    # and its label on masked slots
    assert int((b["input_word_ids"] == 1).sum()) >= 10                                   # ... and to the [MASK] row
    assert int(weights[ts.ROW_UNWEIGHTED]) == 0 and int(lens[ts.ROW_UNWEIGHTED]) >= 5
    assert not bool((b["input_word_ids"][ts.ROW_UNWEIGHTED] == 1).any())
    assert int(weights.sum()) == int(ic.ranked_slots(b).rows.numel()) >= 20


def test_sharpen_rescales_one_draw():
    name = "h128hd64_L200"      # factorised: the projection is among the kernels
    _, params = ic.cell_params(im.CELLS[name])
    mod, sharp = ts.sharpen(params, "moderate"), ts.sharpen(params, "sharp")
    assert set(mod) == set(params) == set(sharp)
    t_m, qk_m, k_m, b_m, g_m = ts.LEVELS["moderate"]
    t_s, qk_s, k_s, b_s, g_s = ts.LEVELS["sharp"]
    for n, p in params.items():
        assert mod[n].dtype == torch.float32 and mod[n].shape == p.shape
        if n == ts.TRANSFORM_KERNEL:
            assert torch.equal(mod[n], p) and torch.equal(sharp[n], p)
            continue
        if n.endswith("gamma"):
            a, b, ratio = mod[n] - 1.0, sharp[n] - 1.0, g_s / g_m
        elif n.endswith(("bias", "beta")):
            a, b, ratio = mod[n], sharp[n], b_s / b_m
        elif n.endswith("embeddings"):
            a, b, ratio = mod[n], sharp[n], t_s / t_m
        elif n.endswith(("query/kernel", "key/kernel")):
            a, b, ratio = mod[n], sharp[n], qk_s / qk_m
        else:
            a, b, ratio = mod[n], sharp[n], k_s / k_m
        assert torch.allclose(b, a * ratio, rtol=1e-5, atol=1e-6), n      # the same draw at both levels
    std = lambda t: float(t.double().std())
    # truncated at two sigma: the std of the draw is 0.88 of the nominal one
    assert 0.8 * t_s < std(sharp["word_embeddings/embeddings"]) < 1.05 * t_s
    assert 0.8 * qk_s < std(sharp["transformer/layer_0/self_attention/query/kernel"]) < 1.05 * qk_s
    assert 0.8 * k_s < std(sharp["embedding_projection/kernel"]) < 1.05 * k_s
    # parameters the initialisers left trivial are drawn from the seed
    raw = {"x/bias": torch.zeros(64), "x/gamma": torch.ones(64)}
    drawn = ts.sharpen(raw, "sharp", seed=5)
    assert 0.5 * b_s < std(drawn["x/bias"]) < 1.5 * b_s and 0.5 * g_s < std(drawn["x/gamma"]) < 1.5 * g_s
    assert torch.equal(drawn["x/bias"], ts.sharpen(raw, "sharp", seed=5)["x/bias"])


@pytest.mark.parametrize("name,level", CASES)
def test_no_relu_of_the_reference_sits_on_its_kink(name, level):
    """every relu pre-activation that carries a gradient is further than RELU_CLEARANCE from zero in fp64, in the eval and in the
    training-mode forward, and the clearance moved the biases by a few 1e-3 at the most"""
    c = fm.CELLS[name]
    w = ts.cell_weights(name, level)
    z = ts.relu_preactivations(w, name)
    assert len(z) == (2 if c.acts[0] == "relu" else 0) + (1 if c.acts[1] == "relu" else 0)
    for n, t in z.items():
        assert float(t.abs().min()) >= ts.RELU_CLEARANCE, n
    _, params = ic.cell_params(im.CELLS[name])
    raw = ts.sharpen(params, level)
    for n in w:
        if n in z:
            assert float((w[n] - raw[n]).abs().max()) <= 5e-3, n
        else:
            assert torch.equal(w[n], raw[n]), n


@pytest.mark.parametrize("name,level", CASES)
def test_level_is_as_sharp_as_it_claims(name, level):
    st = ts.level_statistics(name, level)
    print(f"LEVEL {name} [{level}]: " + ", ".join(f"{k} {v:.3g}" for k, v in st.items()))
    std_min, pmax_min, span_min = ts.CONDITIONS[level]
    assert st["score_std"] >= std_min
    assert st["logit_span"] >= span_min
    if level == "moderate":
        assert st["pmax_over_uniform_median"] >= pmax_min
    else:
        assert st["pmax_median"] >= pmax_min
        assert st["pmax_max"] >= 0.999                                   # a query that attends to one key
        assert st["top_prob_max"] >= 0.3 and st["gt_prob_min"] <= 1e-4   # a confident slot and a long-tail slot


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name,level", CASES)
def test_fp32_restatement_meets_what_the_device_is_held_to(name, level, training):
    batch = ts.cell_batch(name)
    r64 = ts.reference(name, level, torch.float64, training)
    e32, e32g = ts.fp32_errors(name, level, training)
    for q in ts.FORWARD + ("loss",):
        contract = ts.contract_of(batch, q, r64[q])
        print(f"E32 {name} [{level}, training {training}] {q}: e32 {e32[q]:.3e} contract {contract:.3e}")
        assert 0.0 < 16.0 * e32[q] < contract, q
        for mode in ts.MODES:       # the fp32 restatement passes either mode's bound, and no bound is above the contract
            assert e32[q] <= ts.forward_bound(mode, e32[q], contract) <= contract, (q, mode)
    G = ts.GRAD_CONTRACT[training]
    assert set(e32g) == {n for n in ts.cell_weights(name, level) if ts.orc.is_trainable(n)}
    for n, e in sorted(e32g.items(), key=lambda kv: -kv[1])[:3]:
        print(f"E32G {name} [{level}, training {training}] {n}: {e:.3e} (G {G:.0e})")
    for n, e in e32g.items():
        assert e < G, (n, e)
        assert e <= ts.grad_bound("f32", e, training) and ts.grad_bound("bf16x3", e, training) <= G, n
        assert float(r64["grads"][n].abs().max()) > 0.0 or n.endswith("key/bias"), n
    # the key-bias gradients are zero in fp64 (to its own rounding), so they are measured against the floor
    floor = 1e-4 * max(float(g.abs().max()) for g in r64["grads"].values()) + 1e-7
    for n in e32g:
        if n.endswith("key/bias"):
            assert float(r64["grads"][n].abs().max()) <= 1e-9 * floor, n
    if training:                    # the masks were applied: another loss than in eval mode
        assert abs(float(r64["loss"]) - float(ts.reference(name, level, torch.float64, False)["loss"])) > 1e-3
        return
    # accuracy: argmax agreement outside the slots whose fp64 top-two gap is below the (wider, bf16x3) logits bound
    width = ts.forward_bound("bf16x3", e32["logits"], ts.contract_of(batch, "logits", r64["logits"]))
    best, tie = ts.tie_slots(batch, r64["logits"], width)
    got = ts.on_slots(batch, "logits", ts.reference(name, level, torch.float32, False)["logits"]).argmax(dim=-1)
    assert float(tie.double().mean()) < ts.TIE_CAP, (int(tie.sum()), tie.numel())
    assert bool((got == best)[~tie].all())
