"""The geometry matrix (tests/geometry_matrix.py): the models check_cfg accepts beyond the shipped configurations -- hidden 32, 512 and
1024, 16 and 32 heads, inner sizes off the tile grid, one layer, 8 and 32 layers, tiny vocabularies -- each cell one Engine.train_step
with the benchmark's flags, checked against tests/activation_ref.py mask for mask as tests/test_gpu_feature_matrix.py checks its
cells:

* the step's launch labels, parsed into forms per layer, equal the cell's expected forms (a moved plan_step threshold fails here);
* f32 / bf16x3: run_and_check_train_step -- the gradient buffer, the gradient AdamW consumed, AdamW to fp32 rounding, loss, gradient
  norm, counts and accuracy sums (1e-3 on the loss, relative 5e-3 on the gradients);
* bf16 (mode 2): the mode-2 bounds of the feature matrix;
* where the last layer runs the attention block: whether its forward swept every query (the labels do not tell), from the rows of
  its context the step wrote.

Plus the evaluation forward (logits, top-10 and the encoder-only forward on the ranked rows) at EVAL_CELLS, and the attention cores
at 16 and 32 heads of both widths against fp64 autograd."""
import math

import pytest
import torch

from bert4rec_amd import _lib, activations
from bert4rec_amd.engine import Engine, make_model_config
from oracle import bert4rec_oracle as orc
from tests import activation_ref as ar
from tests import b4r_testlib as T
from tests import factorized_ref as fr
from tests.b4r_testlib import P, maxdiff, stream
from tests.geometry_matrix import CELLS, EVAL_CELLS, MODES, last_block_sweeps_every_query
from tests.test_gpu_feature_matrix import SEED, check_bf16_step, matrix_mode, parse_forms  # noqa: F401 (matrix_mode: a fixture)
from tests.test_gpu_headdim64 import attention_reference
from tests.test_gpu_train_step import launch_labels, run_and_check_train_step, set_edge_rows

pytestmark = pytest.mark.gpu

DROPOUT = 0.1
DEV = "cuda"


def build_cell(c, od=DROPOUT, ad=DROPOUT, seed=3):
    cfg_o = orc.OracleConfig(vocab_size=c.V, hidden_size=c.H, num_layers=c.layers, num_attention_heads=c.heads,
                             max_sequence_length=c.L, inner_dim=c.inner, output_dropout=od, attention_dropout=ad)
    eng = Engine(make_model_config(c.V, c.H, c.layers, c.heads, c.L, c.inner, od, ad), "cuda", embedding_width=c.E,
                 inner_activation=activations.IDS[c.acts[0]], mlm_activation=activations.IDS[c.acts[1]])
    if c.E:
        params = fr.init_params(cfg_o, c.E, seed)
    else:   # the oracle's initialisers with biases, betas and gammas made non-trivial (as fr.init_params does)
        params = orc.init_params(cfg_o, seed)
        g = torch.Generator().manual_seed(seed + 1)
        for n, p in params.items():
            if n.endswith(("bias", "beta")):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            elif n.endswith("gamma"):
                p.copy_(1.0 + torch.randn(p.shape, generator=g) * 0.05)
    eng.load_named(params)
    return cfg_o, eng, params


def cell_batch(c, seed=11):
    return set_edge_rows(orc.synthetic_batch(c.B, c.L, c.P, c.V, seed=seed + c.L, ragged=True))


def label_cap(c):
    return 64 + 24 * c.layers   # (the exact-fp32 step runs about 14 launches per layer)


# ---- the train step ---------------------------------------------------------------------------------------------------------------
CASES = [pytest.param(name, mode, id=f"{name}-{mode}") for name, c in CELLS.items() for mode in c.modes]


@pytest.mark.parametrize("name,matrix_mode", CASES, indirect=["matrix_mode"])
def test_train_step_of_every_geometry_follows_the_restatement_in_its_forms(name, matrix_mode):
    c = CELLS[name]
    cfg_o, eng, _ = build_cell(c)
    batch = cell_batch(c)
    hp_o = orc.AdamWConfig(num_warmup_steps=0, num_train_steps=100, gradient_clip_norm=5.0)
    eng.set_seed(SEED)
    cb, _ = eng.prepare_batch(batch)
    want = c.forms(matrix_mode)
    # the last layer's block forward: a dense sweep writes every row of its context, the slots-only sweep the slots' rows alone
    ctx = eng.region(f"attention_context_{c.layers - 1}", c.B, c.L, c.P) if want.attn_fwd[-1] == "Block" else None
    if ctx is not None:
        ctx.fill_(float("nan"))
    labels = []
    if matrix_mode == "bf16":
        check_bf16_step(eng, cfg_o, batch, cb, hp_o, c, labels, name)
    else:
        ref = lambda *a, **k: ar.loss_and_grads(*a, inner=c.acts[0], mlm=c.acts[1], **k)   # noqa: E731
        run_and_check_train_step(eng, cfg_o, batch, cb, hp_o, 0, SEED, rel=5e-3, labels=labels, ref=ref, label_cap=label_cap(c))
    got = parse_forms(labels, c, c.B)
    print(f"forms [{matrix_mode}]: {got}")
    assert got == want, f"forms of the {matrix_mode} step: {got}, expected {want}\n{labels}"
    assert len(got.attn_fwd) == len(got.attn_bwd) == len(got.ffn) == c.layers
    if ctx is not None:
        dense = bool(torch.isfinite(ctx).all())
        assert dense == last_block_sweeps_every_query(c, matrix_mode), f"dense sweep of the last block forward: {dense}"


# ---- the evaluation forward -------------------------------------------------------------------------------------------------------------
EVAL_CASES = [pytest.param(name, mode, id=f"{name}-{mode}") for name in EVAL_CELLS for mode in MODES]
TOP = 10


@pytest.mark.parametrize("name,matrix_mode", EVAL_CASES, indirect=["matrix_mode"])
def test_eval_forward_at_the_new_widths_follows_the_restatement(name, matrix_mode):
    """the full eval forward's logits against the restatement (1e-3; mode 2: 5e-2, as in the feature matrix) and its top-10 items
    (each of them within twice that of the restatement's 10th best logit); in f32 and bf16x3 the encoder-only forward on the ranked
    rows must give the full forward's rows there"""
    c = CELLS[name]
    cfg_o, eng, params = build_cell(c, od=0.0, ad=0.0)
    batch = cell_batch(c, seed=21)
    cb, _ = eng.prepare_batch(batch)
    B, L, P_ = cb.B, cb.L, cb.P
    eng.forward(cb, training=False, pooler=False)
    torch.cuda.synchronize()
    ref = ar.model_forward(params, batch, cfg_o, *c.acts)["mlm_logits"].reshape(B * P_, c.V).double()
    logits = eng.region("mlm_logits", B, L, P_)[:, :c.V].cpu().double()
    tol = 5e-2 if matrix_mode == "bf16" else 1e-3
    err = maxdiff(logits, ref)
    print(f"{name} [{matrix_mode}]: eval logits max-abs {err:.2e}")
    assert err <= tol
    got_top = logits.topk(TOP, dim=-1).indices
    floor = ref.topk(TOP, dim=-1).values[:, -1:]
    assert bool((ref.gather(1, got_top) >= floor - 2 * tol).all()), "top-10 items"
    if matrix_mode == "bf16":   # (the two forwards then differ in term count: the slot-query attention keeps three)
        return
    full = eng.region("sequence_output", B, L, P_).clone()
    eng.region("sequence_output", B, L, P_).fill_(float("nan"))
    labels = launch_labels(lambda: eng.forward(cb, training=False, pooler=False, head_rows_only=True, encoder_only=True))
    torch.cuda.synchronize()
    got = eng.region("sequence_output", B, L, P_)
    valid = batch["masked_lm_ids"] != 0
    rows = (torch.arange(B)[:, None] * L + batch["masked_lm_positions"].clamp(0, L - 1))[valid].to(got.device)
    assert rows.numel() > 0
    d = maxdiff(got[rows], full[rows])
    print(f"{name}: encoder-only rows max-abs {d:.2e}; launches {labels}")
    assert d < 2e-5
    if matrix_mode == "bf16x3":   # the last layer with the slots as its only queries
        assert "attention core forward, queries = the head's slots" in labels, labels


# ---- the attention cores at 16 and 32 heads ----------------------------------------------------------------------------------------
def core_case(B, L, heads, width, seed=22):
    """tests/test_gpu_headdim64.py's core_case at either width: a full-length sequence, an interior hole, a sequence without a valid
    key and one with a single valid key"""
    H = width * heads
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * L, 3 * H, generator=g)
    qkv[:, :H] *= math.sqrt(32 / width)   # scores distributed as those of the width-32 tests
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.int64)
    if L > 1:
        mask[1, 0] = 0
    mask[2] = 0
    mask[3] = 0
    mask[3, int(torch.randint(0, L, (1,), generator=g))] = 1
    qkv.view(B, L, 3 * H)[2, :, :H] *= 0.25
    dctx = torch.randn(B * L, H, generator=g)
    return qkv, mask, dctx


@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("heads", [16, 32])
@pytest.mark.parametrize("L", [1, 65, 200, 256])
def test_attention_core_at_16_and_32_heads_matches_fp64_autograd(L, heads, width, gemm_mode):
    """b4r_attn_fwd_hd / b4r_attn_bwd_hd at the head counts of hidden 512 and 1024, with and without dropout; the bounds of
    test_gpu_headdim64.py::test_attention_core_matches_fp64_autograd"""
    lib = _lib.load()
    B, H, seed, step, sid, qscale = 4, width * heads, 21, 4, 9, 0.125
    qkv, mask, dctx = core_case(B, L, heads, width)
    x3 = gemm_mode == "bf16x3"
    qd, md, dcd = qkv.to(DEV), mask.to(DEV), dctx.to(DEV)
    for rate in (0.0, 0.2):
        x = qkv.double().view(B, L, 3, heads, width).clone().requires_grad_(True)
        keep = orc.dropout_keep_mask((B, heads, L, L), rate, seed, step, sid, orc.ATTN_PITCH) if rate > 0 else None
        ctx_ref = attention_reference(x[:, :, 0], x[:, :, 1], x[:, :, 2], mask, rate, keep)
        ctx_ref.backward(dctx.double().view(B, L, heads, width))
        st = T.new_state(seed, step)
        ctx = torch.full((B * L, H), float("nan"), device=DEV)
        lse = torch.full((B * heads * L,), float("nan"), device=DEV)
        bits = torch.zeros(lib.b4r_attn_keep_words(B, L, heads), dtype=torch.int32, device=DEV)
        _lib.check(lib.b4r_attn_fwd_hd(P(qd), P(md), B, L, heads, width, P(ctx), P(lse), P(st), sid, rate, P(bits), stream()))
        d = maxdiff(ctx.view(B, L, heads, width), ctx_ref)
        assert d < (3e-4 if x3 else 5e-5), (rate, d)
        dqkv = torch.full((B * L, 3 * H), float("nan"), device=DEV)
        _lib.check(lib.b4r_attn_bwd_hd(P(qd), P(md), P(ctx), P(lse), P(dcd), B, L, heads, width, qscale, P(dqkv), P(st), sid, rate,
                                       P(bits), stream()))
        gref = x.grad.view(B * L, 3, H).clone()
        gref[:, 0] *= qscale
        d = maxdiff(dqkv.view(B * L, 3, H), gref)
        assert d < (4e-4 * max(2.5, float(gref.abs().max())) if x3 else 2e-4), (rate, d)
