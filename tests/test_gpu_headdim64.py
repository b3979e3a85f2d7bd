"""GPU tests of attention heads of width 64 (hidden_size = 64 * num_attention_heads, b4r_attn64.hip), both arithmetic modes:
the attention core through the C ABI against fp64 autograd, the model's forward / loss / gradients against the oracle, b4r_train_step
with the benchmark's flags, reproducibility, and the trainer end to end."""
import math

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, dataloaders, evaluation, models, trainers
from bert4rec_amd.models.components import networks
from bert4rec_amd.trainers import optimizers
from oracle import bert4rec_oracle as orc
from tests import b4r_testlib as T
from tests.b4r_testlib import P, set_row_slots, stream
from tests.test_gpu_model import LOGIT_TOL, build, compare_grads, outputs, run_loss_and_grads
from tests.test_gpu_train_step import VOCAB, two_steps

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gemm_mode")]

DEV = "cuda"


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the attention core through the ABI
# ---------------------------------------------------------------------------------------------------------------------------
def attention_reference(q, k, v, mask, rate=0.0, keep=None):
    """q, k, v [B, L, h, 64] fp64 (q already scaled); mask [B, L].  A sequence without a valid key attends uniformly (Keras' -1e9
    absorbs the scores in fp32): its probabilities are 1/L, and its gradients those of a softmax taken at that point."""
    s = torch.einsum("bqhd,bkhd->bhqk", q, k)
    s = s + (1.0 - mask.double())[:, None, None, :] * -1e9
    dead = (mask.sum(1) == 0)[:, None, None, None]
    raw = torch.einsum("bqhd,bkhd->bhqk", q, k)
    s = torch.where(dead, raw - raw.detach(), s)
    a = torch.softmax(s, dim=-1)
    if keep is not None:
        a = a * keep.double() / (1 - rate)
    return torch.einsum("bhqk,bkhd->bqhd", a, v)


def core_case(B, L, heads, seed=22):
    H = 64 * heads
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * L, 3 * H, generator=g)
    qkv[:, :H] *= math.sqrt(0.5)   # scores distributed as those of the width-32 tests (q.k over 64 columns instead of 32)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.int64)
    if L > 1:
        mask[1, 0] = 0                        # an interior hole: the mask is per key, not a length
    mask[2] = 0                               # a sequence without a valid key
    mask[3] = 0
    mask[3, int(torch.randint(0, L, (1,), generator=g))] = 1   # a single valid key
    qkv.view(B, L, 3 * H)[2, :, :H] *= 0.25   # |score| < 32: fp32 rounds every (score - 1e9) of that sequence to -1e9
    dctx = torch.randn(B * L, H, generator=g)
    return qkv, mask, dctx


@pytest.mark.parametrize("heads", [1, 2, 4])
@pytest.mark.parametrize("L", [1, 7, 16, 33, 50, 64, 65, 96, 200, 224, 256])
def test_attention_core_matches_fp64_autograd(L, heads):
    lib = _lib.load()
    B, H, seed, step, sid, qscale = 4, 64 * heads, 21, 4, 9, 0.125
    qkv, mask, dctx = core_case(B, L, heads)
    x3 = lib.b4r_get_gemm_mode() == _lib.GEMM_BF16X3
    qd, md, dcd = qkv.to(DEV), mask.to(DEV), dctx.to(DEV)
    for rate in (0.0, 0.2):
        x = qkv.double().view(B, L, 3, heads, 64).clone().requires_grad_(True)
        keep = orc.dropout_keep_mask((B, heads, L, L), rate, seed, step, sid, orc.ATTN_PITCH) if rate > 0 else None
        ctx_ref = attention_reference(x[:, :, 0], x[:, :, 1], x[:, :, 2], mask, rate, keep)
        ctx_ref.backward(dctx.double().view(B, L, heads, 64))
        st = T.new_state(seed, step)
        ctx = torch.full((B * L, H), float("nan"), device=DEV)
        lse = torch.full((B * heads * L,), float("nan"), device=DEV)
        bits = torch.zeros(lib.b4r_attn_keep_words(B, L, heads), dtype=torch.int32, device=DEV)
        _lib.check(lib.b4r_attn_fwd_hd(P(qd), P(md), B, L, heads, 64, P(ctx), P(lse), P(st), sid, rate, P(bits), stream()))
        assert not bool(bits.any())           # nothing stored: the backward hashes the decisions again
        d = T.maxdiff(ctx.view(B, L, heads, 64), ctx_ref)
        assert d < (3e-4 if x3 else 5e-5), (rate, d)
        dqkv = torch.full((B * L, 3 * H), float("nan"), device=DEV)
        _lib.check(lib.b4r_attn_bwd_hd(P(qd), P(md), P(ctx), P(lse), P(dcd), B, L, heads, 64, qscale, P(dqkv), P(st), sid, rate,
                                       P(bits), stream()))
        gref = x.grad.view(B * L, 3, H).clone()
        gref[:, 0] *= qscale
        d = T.maxdiff(dqkv.view(B * L, 3, H), gref)
        assert d < (4e-4 * max(2.5, float(gref.abs().max())) if x3 else 2e-4), (rate, d)


def test_attention_core_head_width_dispatch():
    """head_dim 32 is b4r_attn_fwd / b4r_attn_bwd bit for bit; any width but 32 and 64 is refused with a message"""
    lib = _lib.load()
    B, L, heads = 2, 40, 4
    H = 32 * heads
    qkv = torch.randn(B * L, 3 * H, generator=torch.Generator().manual_seed(1)).to(DEV)
    mask = torch.ones(B, L, dtype=torch.int64, device=DEV)
    outs = []
    for fn in ("b4r_attn_fwd", "b4r_attn_fwd_hd"):
        ctx, lse = torch.empty(B * L, H, device=DEV), torch.empty(B * heads * L, device=DEV)
        args = (P(qkv), P(mask), B, L, heads) + ((32,) if fn.endswith("_hd") else ()) + (P(ctx), P(lse), None, 0, 0.0, None, stream())
        _lib.check(getattr(lib, fn)(*args))
        outs.append((ctx.clone(), lse.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for hd in (16, 48, 128):
        ctx, lse = torch.empty(B * L, H, device=DEV), torch.empty(B * heads * L, device=DEV)
        rc = lib.b4r_attn_fwd_hd(P(qkv), P(mask), B, L, 1, hd, P(ctx), P(lse), None, 0, 0.0, None, stream())
        assert rc == -2 and "32, 64" in _lib.last_error()
        rc = lib.b4r_attn_bwd_hd(P(qkv), P(mask), P(ctx), P(lse), P(ctx), B, L, 1, hd, 1.0, P(qkv), None, 0, 0.0, None, stream())
        assert rc == -2


# ---------------------------------------------------------------------------------------------------------------------------
# 2.-3. the model against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def oracle_cfg(H, heads, L, layers=2, dropout=0.0, vocab=None):
    return orc.OracleConfig(vocab_size=vocab or 3 * H + 11, hidden_size=H, num_layers=layers, num_attention_heads=heads,
                            max_sequence_length=L, inner_dim=4 * H, output_dropout=dropout, attention_dropout=dropout)


@pytest.mark.parametrize("H,heads,L", [(64, 1, 50), (64, 1, 200), (128, 2, 50), (128, 2, 200), (256, 4, 50), (256, 4, 200),
                                       (512, 8, 50)])
def test_forward_logits_and_top10_match_oracle(H, heads, L):
    cfg_o = oracle_cfg(H, heads, L)
    eng, params = build(cfg_o)
    B, Pn = (4, 40) if L == 200 else (6, 10)
    batch = orc.synthetic_batch(B, L, Pn, cfg_o.vocab_size, seed=1, ragged=True)
    ref = orc.model_forward(params, batch, cfg_o, training=False)
    cb, keep = eng.prepare_batch(batch)
    eng.forward(cb, training=False, pooler=True)
    got = outputs(eng, cb)
    assert T.maxdiff(got["sequence_output"], ref["sequence_output"]) < LOGIT_TOL
    assert T.maxdiff(got["mlm_logits"], ref["mlm_logits"]) < LOGIT_TOL
    # top 10: the oracle's logits at the device's top-10 items are the oracle's own top-10 values (ties may swap places)
    gl, rl = got["mlm_logits"].cpu().double(), ref["mlm_logits"].double()
    at = rl.gather(-1, gl.topk(10, dim=-1).indices)
    assert float((at - rl.topk(10, dim=-1).values).abs().max()) < 2 * LOGIT_TOL


@pytest.mark.parametrize("H,heads,L", [(64, 1, 200), (128, 2, 50), (256, 4, 64)])
def test_loss_and_gradients_match_autograd_eval_mode(H, heads, L):
    cfg_o = oracle_cfg(H, heads, L)
    eng, params = build(cfg_o)
    batch = orc.synthetic_batch(6, L, max(4, L // 5), cfg_o.vocab_size, seed=2, ragged=True)
    loss_ref, grads_ref, _ = orc.loss_and_grads(params, batch, cfg_o, training=False)
    st, grads = run_loss_and_grads(eng, batch, training=False)
    assert abs(st["loss_sum"] / st["valid_count"] - float(loss_ref)) < LOGIT_TOL
    compare_grads(grads, grads_ref, st["valid_count"], rel=2e-3)


@pytest.mark.parametrize("H,heads,L", [(64, 1, 100), (128, 2, 50), (256, 4, 200)])
def test_train_mode_matches_oracle_mask_for_mask(H, heads, L):
    cfg_o = oracle_cfg(H, heads, L, dropout=0.2)
    eng, params = build(cfg_o)
    batch = orc.synthetic_batch(5, L, max(4, L // 5), cfg_o.vocab_size, seed=3, ragged=True)
    seed, step = 4242, 17
    loss_ref, grads_ref, _ = orc.loss_and_grads(params, batch, cfg_o, training=True, rng=(seed, step))
    st, grads = run_loss_and_grads(eng, batch, training=True, seed=seed, step=step)
    assert abs(st["loss_sum"] / st["valid_count"] - float(loss_ref)) < LOGIT_TOL
    compare_grads(grads, grads_ref, st["valid_count"], rel=5e-3)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. b4r_train_step with the benchmark's flags (the logits-free head, the last layer on the head's rows)
# ---------------------------------------------------------------------------------------------------------------------------
def step_case(H, heads, L, vocab):
    cfg_o = oracle_cfg(H, heads, L, layers=2, dropout=0.1, vocab=vocab)
    B, Pn = (8, 40) if L == 200 else (24, 10)
    batch = orc.synthetic_batch(B, L, Pn, vocab, seed=H + L, ragged=True)
    n0 = int(batch["input_mask"][0].sum())
    set_row_slots(batch, 0, [0] + list(range(2, n0, max(1, n0 // 4)))[:3], orc.MASK_TOKEN_ID)
    set_row_slots(batch, 1, [int(batch["input_mask"][1].sum()) - 1], orc.MASK_TOKEN_ID)
    hp_o = orc.AdamWConfig(num_warmup_steps=0, num_train_steps=100, gradient_clip_norm=5.0)
    return cfg_o, batch, hp_o


@pytest.mark.parametrize("H,heads,L,vocab", [(128, 2, 200, VOCAB["ml-1m"]), (256, 4, 50, VOCAB["steam"]), (64, 1, 200, 1001)],
                         ids=["ml1m_128x2", "steam_256x4", "h64x1"])
def test_train_step_matches_oracle(H, heads, L, vocab):
    cfg_o, batch, hp_o = step_case(H, heads, L, vocab)
    clipped, labels = two_steps(cfg_o, batch, hp_o, rel=5e-3)
    assert labels.count("b4r_attn_fwd_hd") == 2 and labels.count("b4r_attn_bwd_hd") == 2, labels
    assert not any("32-token tiles" in l or "head's slots" in l or l.startswith("b4r_attn_block") for l in labels), labels


# ---------------------------------------------------------------------------------------------------------------------------
# 5. reproducibility
# ---------------------------------------------------------------------------------------------------------------------------
def test_graph_replayed_steps_equal_eager_steps_and_runs_are_bitwise_reproducible():
    from bert4rec_amd.engine import make_adamw_config
    cfg_o = oracle_cfg(128, 2, 50, dropout=0.1, vocab=301)
    batch = orc.synthetic_batch(16, 50, 10, cfg_o.vocab_size, seed=21, ragged=True)
    hp = make_adamw_config(num_warmup_steps=2, num_train_steps=100)
    runs = []
    for graphed, n in ((False, 20), (False, 20), (True, 20)):
        eng, _ = build(cfg_o)
        eng.set_seed(1234)
        cb, keep = eng.prepare_batch(batch)
        losses = []
        for it in range(n):
            (eng.train_step_graphed if graphed else eng.train_step)(hp, cb)
            torch.cuda.synchronize()
            losses.append(eng.read_state()["loss_sum"])
        runs.append((losses, eng.params.clone()))
    (l0, p0), (l1, p1), (l2, p2) = runs
    assert l0 == l1 and torch.equal(p0, p1)
    assert np.isfinite(l0[-1]) and l0[-1] != l0[0]
    for a, b in zip(l0, l2):
        assert abs(a - b) <= 1e-4 * abs(a)
    assert float((p0 - p2).abs().max()) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------------
# 6. end to end
# ---------------------------------------------------------------------------------------------------------------------------
def test_train_evaluate_save_load_at_128x2(tmp_path, gemm_mode):
    if gemm_mode == "f32":
        pytest.skip("end to end in the default mode only")
    from bert4rec_amd import datasets
    ds = datasets.synthetic_dataset(n_users=120, n_items=300, min_len=4, max_len=40, seed=1)
    dl = dataloaders.get_dataloader_factory("bert4rec").create_ml_1m_dataloader(data_source=ds, max_seq_len=24,
                                                                                max_predictions_per_seq=6, input_duplication_factor=2)
    train, val, test = dl.prepare_training()
    enc = networks.Bert4RecEncoder(dl.tokenizer.get_vocab_size(), hidden_size=128, num_layers=2, num_attention_heads=2,
                                   max_sequence_length=24, inner_dim=512, output_dropout=0.1, attention_dropout=0.1, seed=3)
    model = models.BERT4RecModel(enc)
    trainer = trainers.get(model=model)
    trainer.initialize_model(optimizer=optimizers.get("adamw", init_lr=1e-3, num_warmup_steps=5, num_train_steps=2000))
    tb = dataloaders.make_batches(train, batch_size=64, seed=1)
    vb = dataloaders.make_batches(val, batch_size=64, seed=1)
    hist = trainer.train(tb, vb, epochs=1).history
    assert all(np.isfinite(v).all() for v in hist.values())
    assert model.engine.read_state()["step"] == len(tb)
    evaluator = evaluation.get(dataloader=dl)
    testb = dataloaders.make_batches(test, batch_size=64, seed=1)
    evaluator.evaluate(model, testb)
    res = evaluator.get_metrics_results()
    assert res["Valid Ranks"] == len(test) and all(0 <= v <= 1 for k, v in res.items() if k != "Valid Ranks")
    wrapper = models.BERT4RecModelWrapper(model)
    trainer.update_wrapper_meta_info(wrapper, dl)
    wrapper.save(tmp_path / "model", dl.get_tokenizer(), mode=2)
    loaded = models.BERT4RecModelWrapper.load(tmp_path / "model", mode=2)
    m2 = loaded["model_wrapper"].model
    assert m2.encoder.get_config()["num_attention_heads"] == 2
    b0 = testb.batches[0]
    assert torch.equal(model(b0)["mlm_logits"].cpu(), m2(b0)["mlm_logits"].cpu())
