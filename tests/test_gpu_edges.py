"""GPU edge cases of the hot path against the oracle: minimum and maximum sequence lengths, single rows, slots that are
all ignored but one, the length limit, bad arguments.  Both arithmetic modes.  Every loss / gradient case runs twice: on the
materialising head over all rows, and under the flags b4r_train_step sets (the logits-free head where the mode has it, the last
layer on the head's rows only: compact dense products and the slot-query attention at hidden 128 / 256, the slot mode of the
feed-forward block and the compact-query attention at hidden 64)."""
import ctypes as C

import pytest
import torch

from bert4rec_amd import _lib
from bert4rec_amd.engine import Engine, make_model_config
from oracle import bert4rec_oracle as orc
from tests.b4r_testlib import set_row_slots

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gemm_mode")]


def build(V, L, layers=1, heads=2, inner=64, hidden=None):
    hidden = hidden or 32 * heads
    cfg_o = orc.OracleConfig(vocab_size=V, hidden_size=hidden, num_layers=layers, num_attention_heads=heads,
                             max_sequence_length=L, inner_dim=inner)
    eng = Engine(make_model_config(V, hidden, layers, heads, L, inner, 0.0, 0.0), "cuda")
    params = orc.init_params(cfg_o, 5)
    eng.load_named(params)
    return eng, params, cfg_o


def check(eng, params, cfg_o, batch, grads=True, train_step_flags=True):
    """train_step_flags=False: only where B4R_FLAG_HEAD_ROWS_ONLY's precondition (valid slots distinct) does not hold"""
    loss_ref, grads_ref, out_ref = orc.loss_and_grads(params, batch, cfg_o, training=False)
    cb, keep = eng.prepare_batch(batch)
    eng.begin_step()
    eng.forward(cb, training=False, pooler=True)
    B, L, P = cb.B, cb.L, cb.P
    logits = eng.region("mlm_logits", B, L, P).view(B, P, -1).cpu()
    assert float((logits - out_ref["mlm_logits"]).abs().max()) < 1e-3
    assert float((eng.region("pooled_output", B, L, P).cpu() - out_ref["pooled_output"]).abs().max()) < 1e-3
    if not grads:
        return
    floor = 1e-4 * max(float(g.abs().max()) for g in grads_ref.values()) + 1e-7   # key bias: analytically zero

    def check_loss_and_grads(path):
        torch.cuda.synchronize()
        st = eng.read_state()
        assert st["valid_count"] == float((batch["masked_lm_ids"] != 0).sum()), path
        assert abs(st["loss_sum"] / st["valid_count"] - float(loss_ref)) < 1e-3, path
        got = eng.export_named(eng.grads)
        for n, g in grads_ref.items():
            a = got[n].double() / st["valid_count"]
            b = g.double().reshape(a.shape)
            assert float((a - b).abs().max()) <= 2e-3 * max(float(b.abs().max()), floor), (path, n)

    eng.loss(cb, want_grad=True)
    eng.backward(cb, training=False)
    check_loss_and_grads("materialising head, all rows")
    if train_step_flags:
        fused = eng.fused_head_supported()
        eng.begin_step()
        eng.forward(cb, training=False, pooler=False, fused_head=fused, head_rows_only=True)
        eng.loss(cb, want_grad=True, fused_head=fused)
        eng.backward(cb, training=False, fused_head=fused, head_rows_only=True)
        check_loss_and_grads("train-step flags")


def edge_batch(B, L, P, V, seed, n_valid=None):
    """ragged rows plus: row 0 of length 1 (its valid slot at position 0, padding slots (0, 0) beside it), row 1 with a single valid
    slot at its last token, row 2 with every key masked, row 3 whose ignored slots repeat its valid slots' positions"""
    assert B >= 5
    batch = orc.synthetic_batch(B, L, P, V, seed=seed, ragged=True, rate=0.3)
    batch["labels"][0, 1:] = 0
    batch["input_mask"][0] = 0
    batch["input_mask"][0, 0] = 1
    set_row_slots(batch, 0, [0], orc.MASK_TOKEN_ID)
    set_row_slots(batch, 1, [int(batch["input_mask"][1].sum()) - 1], orc.MASK_TOKEN_ID)
    batch["input_mask"][2] = 0
    n3 = int(batch["input_mask"][3].sum())
    k = min(P // 2, n3 - 1, 6)
    set_row_slots(batch, 3, list(range(1, n3, max(1, n3 // k)))[:k], orc.MASK_TOKEN_ID)
    k = int((batch["masked_lm_ids"][3] != 0).sum())
    batch["masked_lm_positions"][3, k:] = batch["masked_lm_positions"][3, :k].repeat(P // k + 1)[:P - k]
    return batch


@pytest.mark.parametrize("B,L,P", [(1, 1, 1), (1, 2, 1), (2, 3, 2), (1, 64, 4), (2, 65, 3), (1, 256, 8), (32, 16, 4)])
def test_sequence_length_extremes(B, L, P):
    eng, params, cfg_o = build(53, L)
    batch = orc.synthetic_batch(B, L, P, 53, seed=B + L, ragged=(L > 4), rate=0.5)
    check(eng, params, cfg_o, batch)


def test_rows_with_a_single_valid_slot_and_repeated_padding_positions():
    """finetune / validation rows: slot 0 valid, every other slot is (position 0, id 0) (bert4rec_preprocessor.py:95-99)"""
    eng, params, cfg_o = build(71, 24, layers=2)
    batch = orc.synthetic_batch(6, 24, 5, 71, seed=3, ragged=True, finetune=True)
    assert int((batch["masked_lm_ids"] != 0).sum()) == 6 and int(batch["masked_lm_positions"][:, 1:].abs().sum()) == 0
    check(eng, params, cfg_o, batch)


def test_masked_positions_may_repeat():
    """the kernels scatter-add: duplicated positions (not produced by the reference's preprocessor) still sum correctly.  Materialising
    path only: valid slots that share a position break B4R_FLAG_HEAD_ROWS_ONLY's precondition (include/b4r.h: valid slots distinct,
    ignored ones may collide), so the train step's flags are not run on this batch."""
    eng, params, cfg_o = build(40, 12)
    batch = orc.synthetic_batch(3, 12, 4, 40, seed=9)
    batch["masked_lm_positions"][0] = torch.tensor([5, 5, 5, 7])
    batch["masked_lm_ids"][0] = torch.tensor([9, 9, 11, 12])
    check(eng, params, cfg_o, batch, train_step_flags=False)


@pytest.mark.parametrize("L", [65, 96, 224])
@pytest.mark.parametrize("hidden,inner", [(128, 512), (256, 1024)])
def test_wide_last_layer_on_the_heads_rows_at_edge_rows(hidden, inner, L):
    """hidden 128 / 256 with inner >= 3 hidden + 8 and 64 < L <= 224, P <= 64: under the train-step flags the last layer runs on the
    compact slot rows with the slots as its attention's only queries (slot-query attention); rows of length 1, single valid slots,
    a row with every key masked and ignored slots on valid slots' positions"""
    P = {65: 24, 96: 40, 224: 64}[L]
    eng, params, cfg_o = build(301, L, layers=2, heads=hidden // 32, inner=inner)
    check(eng, params, cfg_o, edge_batch(6 if L < 224 else 5, L, P, 301, seed=L + hidden))


def test_dense_last_layer_fallback_at_hidden_256_inner_512():
    """ml-1m_256's geometry (inner 512 < 3 * 256 + 8): the last layer stays dense under the train-step flags"""
    eng, params, cfg_o = build(301, 96, layers=2, heads=8, inner=512)
    check(eng, params, cfg_o, edge_batch(6, 96, 40, 301, seed=7))


@pytest.mark.parametrize("P,inner", [(48, 392), (49, 392), (48, 384)], ids=["compact", "P_above_half_L", "inner_below_3H_plus_8"])
def test_compact_last_layer_boundaries(P, inner):
    """head_rows_dense_ok's edges at hidden 128, L = 96: P = L / 2 with inner = 3 H + 8 takes the compact rows, one slot more or
    inner = 3 H keeps the dense products"""
    eng, params, cfg_o = build(211, 96, layers=2, heads=4, inner=inner)
    check(eng, params, cfg_o, edge_batch(6, 96, P, 211, seed=P + inner))


@pytest.mark.parametrize("L,P", [(65, 24), (200, 64)])
def test_hidden_64_last_layer_on_the_heads_rows_at_edge_rows(L, P):
    """hidden 64: the slot mode of the feed-forward block and the compact-query attention of the last layer"""
    eng, params, cfg_o = build(211, L, layers=2, heads=2, inner=256)
    check(eng, params, cfg_o, edge_batch(8, L, P, 211, seed=L))


def test_limits_are_reported():
    lib = _lib.load()
    eng, params, cfg_o = build(30, 300)
    batch = orc.synthetic_batch(1, 257, 2, 30, seed=1)
    cb, keep = eng.prepare_batch(batch)
    with pytest.raises(_lib.B4RError, match="256"):
        eng.forward(cb)
    eng2, _, _ = build(30, 16)
    long_batch = orc.synthetic_batch(2, 20, 2, 30, seed=1)
    cb2, keep2 = eng2.prepare_batch(long_batch)
    with pytest.raises(_lib.B4RError, match="max_sequence_length"):
        eng2.forward(cb2)
    with pytest.raises(ValueError):
        eng2.prepare_batch({"input_word_ids": torch.zeros(2, 4, dtype=torch.int64)})
    with pytest.raises(ValueError):
        eng2.prepare_batch({"input_word_ids": torch.zeros(4, dtype=torch.int64), "input_mask": torch.zeros(4, dtype=torch.int64)})
    # workspace too small is an error code, not a fault
    cb3, keep3 = eng2.prepare_batch(orc.synthetic_batch(2, 16, 2, 30, seed=2))
    small = torch.empty(1024, device="cuda")
    rc = lib.b4r_forward(C.byref(eng2.cfg), C.byref(cb3), eng2.params.data_ptr(), eng2.pooler.data_ptr(), small.data_ptr(),
                         small.numel() * 4, eng2.state.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    assert rc == -5 and "workspace too small" in _lib.last_error()


def test_out_of_range_ids_read_the_pad_row_instead_of_faulting():
    eng, params, cfg_o = build(30, 8)
    batch = orc.synthetic_batch(2, 8, 2, 30, seed=4)
    bad = {k: v.clone() for k, v in batch.items()}
    bad["input_word_ids"][0, 0] = 999
    ref = {k: v.clone() for k, v in batch.items()}
    ref["input_word_ids"][0, 0] = 0
    cb, keep = eng.prepare_batch(bad)
    eng.forward(cb)
    got = eng.region("mlm_logits", 2, 8, 2).view(2, 2, -1).cpu().clone()
    want = orc.model_forward(params, ref, cfg_o)["mlm_logits"]
    assert float((got - want).abs().max()) < 1e-3
