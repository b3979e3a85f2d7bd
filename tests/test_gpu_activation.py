"""inner_activation / mlm_activation on the GPU: the activation epilogues and the transform LayerNorm backward against fp64 for every id,
then the model's logits, loss and every gradient, train steps and the Python surface against tests/activation_ref.py.

Tolerances as in test_gpu_factorized.py: 1e-3 on logits and loss, relative 2e-3 on gradients without dropout and 5e-3 with it."""
import ctypes as C

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, activations
from bert4rec_amd.engine import Engine, make_adamw_config, make_model_config
from oracle import bert4rec_oracle as orc
from tests import activation_ref as ar
from tests import factorized_ref as fr
from tests.b4r_testlib import P, stream
from tests.test_gpu_model import compare_grads

pytestmark = [pytest.mark.gpu]

IDS = list(range(9))


def act64(i, x):
    return ar.value_and_grad64(ar.NAMES[i], x.double().cpu().numpy())


# ---- op level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.usefixtures("gemm_mode")
@pytest.mark.parametrize("act", IDS)
def test_bias_activation_and_backward_epilogues_match_fp64(act):
    lib = _lib.load()
    g = torch.Generator().manual_seed(40 + act)
    M, N, K = 96, 256, 64
    A = (torch.randn(M, K, generator=g) * 0.6).cuda()
    B = (torch.randn(K, N, generator=g) * 0.3).cuda()
    bias = (torch.randn(N, generator=g) * 0.5).cuda()
    Cm = torch.full((M, N), float("nan"), device="cuda")
    C2 = torch.full((M, N), float("nan"), device="cuda")
    d = _lib.GemmDesc()
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.M, d.N, d.K = P(A), K, P(B), N, P(Cm), N, M, N, K
    d.epilogue, d.bias, d.C2, d.ldc2, d.qscale, d.activation = _lib.EPI_BIAS_GELU, P(bias), P(C2), N, 1.0, act
    _lib.check(lib.b4r_gemm_f32(C.byref(d), stream()), "b4r_gemm_f32")
    torch.cuda.synchronize()
    pre = A.double() @ B.double() + bias.double()
    f, fd = act64(act, pre)
    assert float((C2.double() - pre).abs().max()) < 1e-4
    assert np.abs(Cm.double().cpu().numpy() - f).max() < 1e-4 * max(1.0, np.abs(f).max())
    # backward: C = (dY . W^T) * f'(R), B as [N, K]
    dY = (torch.randn(M, K, generator=g)).cuda()
    W = (torch.randn(N, K, generator=g) * 0.3).cuda()
    R = pre.float().contiguous()
    Cb = torch.full((M, N), float("nan"), device="cuda")
    d = _lib.GemmDesc()
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.M, d.N, d.K, d.b_is_nk = P(dY), K, P(W), K, P(Cb), N, M, N, K, 1
    d.epilogue, d.R, d.ldr, d.qscale, d.activation = _lib.EPI_GELU_BWD, P(R), N, 1.0, act
    _lib.check(lib.b4r_gemm_f32(C.byref(d), stream()), "b4r_gemm_f32")
    torch.cuda.synchronize()
    _, fr64 = act64(act, R)
    want = (dY.double() @ W.double().t()).cpu().numpy() * fr64
    assert np.abs(Cb.double().cpu().numpy() - want).max() < 1e-4 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("act", IDS)
def test_dgrad_tail_of_the_weight_gradient_product_matches_fp64(act):
    """b4r_gemm_tn_f32 with dgrad_out and dgrad_gelu_pre (bf16x3 mode, No = 64): dX = (B . W^T) * f'(G)"""
    lib = _lib.load()
    prev = lib.b4r_get_gemm_mode()
    lib.b4r_set_gemm_mode(_lib.GEMM_BF16X3)
    try:
        g = torch.Generator().manual_seed(70 + act)
        Rr, Mo, No = 200, 256, 64
        A = torch.randn(Rr, Mo, generator=g).cuda()
        Bm = torch.randn(Rr, No, generator=g).cuda()
        W = (torch.randn(Mo, No, generator=g) * 0.3).cuda()
        G = torch.randn(Rr, Mo, generator=g).cuda() * 2
        out = torch.empty(Mo, No, device="cuda")
        dX = torch.full((Rr, Mo), float("nan"), device="cuda")
        sc = torch.empty(lib.b4r_gemm_tn_scratch_floats(Rr, Mo, No), device="cuda")
        d = _lib.GemmTnDesc()
        d.A, d.lda, d.B, d.ldb, d.out, d.ldo, d.R, d.Mo, d.No = P(A), Mo, P(Bm), No, P(out), No, Rr, Mo, No
        d.dgrad_w, d.dgrad_ldw, d.dgrad_out, d.dgrad_ldo, d.dgrad_gelu_pre, d.dgrad_ldg, d.activation = P(W), No, P(dX), Mo, P(G), Mo, act
        assert lib.b4r_gemm_tn_dgrad_supported(C.byref(d)) == 1
        _lib.check(lib.b4r_gemm_tn_f32(C.byref(d), P(sc), stream()), "b4r_gemm_tn_f32")
        torch.cuda.synchronize()
        _, fg = act64(act, G)
        want = (Bm.double() @ W.double().t()).cpu().numpy() * fg
        assert np.abs(dX.double().cpu().numpy() - want).max() < 1e-4 * max(1.0, np.abs(want).max())
        assert float((out.double() - A.double().t() @ Bm.double()).abs().max()) < 1e-3
    finally:
        lib.b4r_set_gemm_mode(prev)


@pytest.mark.parametrize("act", IDS)
@pytest.mark.parametrize("H", [64, 256])
def test_transform_layer_norm_backward_matches_fp64(act, H):
    lib = _lib.load()
    g = torch.Generator().manual_seed(act * 7 + H)
    rows = 77
    z = torch.randn(rows, H, generator=g, dtype=torch.float64)
    gam = 1 + 0.1 * torch.randn(H, generator=g, dtype=torch.float64)
    bet = 0.1 * torch.randn(H, generator=g, dtype=torch.float64)
    dy = torch.randn(rows, H, generator=g, dtype=torch.float64)
    pre = torch.randn(rows, H, generator=g, dtype=torch.float64) * 2
    mean = z.mean(-1)
    rstd = 1.0 / torch.sqrt(((z - mean[:, None]) ** 2).mean(-1) + 1e-12)
    zl = z.clone().requires_grad_()
    gl = gam.clone().requires_grad_()
    bl = bet.clone().requires_grad_()
    y = (zl - zl.mean(-1, keepdim=True)) / torch.sqrt(((zl - zl.mean(-1, keepdim=True)) ** 2).mean(-1, keepdim=True) + 1e-12) * gl + bl
    dz_ref, dg_ref, db_ref = torch.autograd.grad(y, [zl, gl, bl], dy)
    _, fp = act64(act, pre)
    dz_ref = dz_ref.numpy() * fp
    cu = lambda t: t.float().cuda().contiguous()
    dz = torch.empty(rows, H, device="cuda")
    dgb = torch.empty(2 * H, device="cuda")
    sc = torch.empty(lib.b4r_ln_bwd_scratch_floats(rows, H), device="cuda")
    args = [cu(dy), cu(z), cu(mean), cu(rstd), cu(gam)]
    _lib.check(lib.b4r_ln_bwd_act(*[P(t) for t in args], rows, H, P(dz), P(dgb), P(dgb[H:]), P(sc), P(cu(pre)), act, stream()),
               "b4r_ln_bwd_act")
    torch.cuda.synchronize()
    assert np.abs(dz.double().cpu().numpy() - dz_ref).max() < 1e-4 * max(1.0, np.abs(dz_ref).max())
    assert float((dgb[:H].double().cpu() - dg_ref).abs().max()) < 1e-3 and float((dgb[H:].double().cpu() - db_ref).abs().max()) < 1e-3


def test_unknown_activation_ids_are_refused():
    lib = _lib.load()
    A = torch.zeros(32, 64, device="cuda")
    d = _lib.GemmDesc()
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.M, d.N, d.K = P(A), 64, P(A), 64, P(A), 64, 32, 64, 64
    d.epilogue, d.bias, d.C2, d.ldc2, d.activation = _lib.EPI_BIAS_GELU, P(A), P(A), 64, 9
    assert lib.b4r_gemm_f32(C.byref(d), stream()) == -1 and "activation" in _lib.last_error()


# ---- model level ----------------------------------------------------------------------------------------------------------------------
# (H, heads, E): Block (64 x 2), Wide at head width 64 (128 x 2), TileProducts + CompactRows (256 x 8), factorised E = 64 at H = 128
CASES = {"h64": (64, 2, None), "h128_hd64": (128, 2, None), "h256": (256, 8, None), "h128_e64": (128, 4, 64)}
PAIRS = [("relu", "relu"), ("swish", "sigmoid"), ("tanh", "gelu")]


def build(H, heads, E, inner, mlm, V=307, layers=2, L=48, od=0.0, ad=0.0, seed=3):
    cfg_o = orc.OracleConfig(vocab_size=V, hidden_size=H, num_layers=layers, num_attention_heads=heads, max_sequence_length=L,
                             inner_dim=4 * H, output_dropout=od, attention_dropout=ad)
    eng = Engine(make_model_config(V, H, layers, heads, L, 4 * H, od, ad), "cuda", embedding_width=E,
                 inner_activation=activations.IDS[inner], mlm_activation=activations.IDS[mlm])
    params = fr.init_params(cfg_o, E, seed) if E else orc.init_params(cfg_o, seed)
    eng.load_named(params)
    return cfg_o, eng, params


def run_grads(eng, batch, training, fused_head, seed=5, step=2):
    cb, keep = eng.prepare_batch(batch)
    eng.set_seed(seed)
    eng.set_step(step)
    eng.begin_step()
    eng.forward(cb, training=training, pooler=False, fused_head=fused_head, head_rows_only=fused_head)
    eng.loss(cb, want_grad=True, fused_head=fused_head)
    eng.backward(cb, training=training, fused_head=fused_head, head_rows_only=fused_head)
    torch.cuda.synchronize()
    return eng.read_state(), eng.export_named(eng.grads)


@pytest.mark.usefixtures("gemm_mode")
@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(p) for p in PAIRS])
@pytest.mark.parametrize("name", list(CASES))
def test_logits_match_the_restatement(name, pair):
    H, heads, E = CASES[name]
    cfg_o, eng, params = build(H, heads, E, *pair)
    batch = orc.synthetic_batch(6, 48, 8, cfg_o.vocab_size, seed=4, ragged=True)
    cb, keep = eng.prepare_batch(batch)
    eng.forward(cb, training=False, pooler=False)
    torch.cuda.synchronize()
    ref = ar.model_forward(params, batch, cfg_o, *pair)
    logits = eng.region("mlm_logits", cb.B, cb.L, cb.P)[:, :cfg_o.vocab_size].cpu()
    assert float((logits - ref["mlm_logits"].reshape(logits.shape)).abs().max()) < 1e-3
    # ... and they are not the GELU model's
    gelu = orc.model_forward(params, batch, cfg_o)["mlm_logits"] if not E else fr.model_forward(params, batch, cfg_o)["mlm_logits"]
    assert float((logits - gelu.reshape(logits.shape)).abs().max()) > 1e-2


@pytest.mark.usefixtures("gemm_mode")
@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(p) for p in PAIRS])
@pytest.mark.parametrize("name", list(CASES))
def test_loss_and_every_gradient_match_the_restatement(name, pair, training, gemm_mode):
    H, heads, E = CASES[name]
    od, ad = (0.1, 0.1) if training else (0.0, 0.0)
    cfg_o, eng, params = build(H, heads, E, *pair, od=od, ad=ad)
    batch = orc.synthetic_batch(6, 48, 8, cfg_o.vocab_size, seed=6, ragged=True)
    loss_ref, grads_ref, _ = ar.loss_and_grads(params, batch, cfg_o, *pair, training=training, rng=(5, 2))
    heads_modes = [False] + ([True] if eng.fused_head_supported() else [])
    for fused in heads_modes:
        st, g = run_grads(eng, batch, training, fused)
        assert abs(st["loss_sum"] / st["valid_count"] - float(loss_ref)) < 1e-3
        compare_grads(g, grads_ref, st["valid_count"], rel=5e-3 if training else 2e-3)


def hip_hp(hp_o):
    return make_adamw_config(hp_o.init_lr, hp_o.num_train_steps, hp_o.num_warmup_steps, hp_o.end_lr, hp_o.weight_decay_rate,
                             hp_o.beta_1, hp_o.beta_2, hp_o.epsilon, hp_o.gradient_clip_norm)


@pytest.mark.parametrize("H,heads,inner", [(64, 2, "swish"), (128, 4, "relu")])
def test_train_step_ex_follows_the_restatement(H, heads, inner):
    """b4r_train_step_ex with the benchmark's flags (fused head, head rows only): the gradient the optimizer consumed and the updated
    weights, three steps with dropout"""
    cfg_o, eng, params = build(H, heads, None, inner, "relu", od=0.1, ad=0.1)
    batch = orc.synthetic_batch(6, 48, 8, cfg_o.vocab_size, seed=8, ragged=True)
    hp_o = orc.AdamWConfig(num_warmup_steps=0, num_train_steps=100, gradient_clip_norm=5.0)
    hp = hip_hp(hp_o)
    cb, keep = eng.prepare_batch(batch)
    eng.set_seed(21)
    eng.ensure_training_buffers()
    for step in range(3):
        p_now = eng.export_named()
        m_now, v_now = eng.export_named(eng.adam_m), eng.export_named(eng.adam_v)
        loss_ref, grads_ref, _ = ar.loss_and_grads(p_now, batch, cfg_o, inner, "relu", training=True, rng=(21, step))
        eng.train_step(hp, cb)
        torch.cuda.synchronize()
        st = eng.read_state()
        assert abs(st["loss_sum"] / st["valid_count"] - float(loss_ref)) < 1e-3
        g = eng.export_named(eng.grads)
        compare_grads(g, grads_ref, st["valid_count"], rel=5e-3)
        trainable = list(grads_ref)
        p_o = {n: p_now[n].clone() for n in trainable}
        m_o = {n: m_now[n].clone() for n in trainable}
        v_o = {n: v_now[n].clone() for n in trainable}
        orc.adamw_apply(p_o, {n: g[n] / st["valid_count"] for n in trainable}, m_o, v_o, step, hp_o)
        after = eng.export_named()
        for n in trainable:
            err = float((after[n] - p_o[n]).abs().max())
            assert err < 1e-6 + 1e-5 * float(p_o[n].abs().max()), (n, err)


def steps(eng, batch, n, graphed=False):
    hp = make_adamw_config(num_warmup_steps=0)
    cb, keep = eng.prepare_batch(batch)
    eng.set_seed(9)
    for _ in range(n):
        (eng.train_step_graphed if graphed else eng.train_step)(hp, cb)
    torch.cuda.synchronize()
    return eng.params.clone()


@pytest.mark.parametrize("H,heads", [(64, 2), (128, 2)])
def test_steps_are_reproducible_and_graph_replay_equals_eager(H, heads):
    batch = orc.synthetic_batch(8, 48, 8, 307, seed=2, ragged=True)
    runs = [steps(build(H, heads, None, "swish", "tanh", od=0.2, ad=0.1)[1], batch, 3, graphed=gr) for gr in (False, False, True)]
    assert torch.equal(runs[0], runs[1])
    assert torch.equal(runs[0], runs[2])


@pytest.mark.parametrize("H,heads", [(64, 2), (256, 8)])
def test_zero_activations_word_through_ex_is_bitwise_the_classic_model(H, heads):
    """b4r_train_step_ex with the activations word 0 against b4r_train_step"""
    batch = orc.synthetic_batch(8, 48, 8, 307, seed=2, ragged=True)
    a = build(H, heads, None, "gelu", "gelu", od=0.1, ad=0.1)[1]
    b = build(H, heads, None, "gelu", "gelu", od=0.1, ad=0.1)[1]
    ex = C.pointer(_lib.ModelConfigEx(b.cfg, 0, (0, 0, 0)))
    b._api = lambda name: (lambda *args: getattr(b.lib, name + "_ex")(ex, *args))
    assert torch.equal(steps(a, batch, 2), steps(b, batch, 2))


# ---- Python surface --------------------------------------------------------------------------------------------------------------------
def test_api_model_follows_the_restatement_and_ranks_like_it():
    from bert4rec_amd.models.bert4rec_model import BERT4RecModel
    from bert4rec_amd.models.components.networks import Bert4RecEncoder
    V, H, L = 307, 64, 32
    enc = Bert4RecEncoder(vocab_size=V, hidden_size=H, num_layers=2, num_attention_heads=2, max_sequence_length=L, inner_dim=4 * H,
                          inner_activation="relu", output_dropout=0.0, attention_dropout=0.0, seed=5)
    model = BERT4RecModel(enc, mlm_activation="tanh")
    assert model.get_config()["mlm_activation"] == "tanh" and enc.get_config()["inner_activation"] == "relu"
    cfg_o = orc.OracleConfig(vocab_size=V, hidden_size=H, num_layers=2, num_attention_heads=2, max_sequence_length=L, inner_dim=4 * H)
    params = enc.engine.export_named()
    batch = orc.synthetic_batch(6, L, 5, V, seed=3, ragged=True)
    ref = ar.model_forward(params, batch, cfg_o, "relu", "tanh")["mlm_logits"]
    cb, keep = enc.engine.prepare_batch(batch)
    enc.engine.forward(cb, training=False, pooler=False)
    torch.cuda.synchronize()
    got = enc.engine.region("mlm_logits", cb.B, cb.L, cb.P)[:, :V].cpu().reshape(ref.shape)
    assert float((got - ref).abs().max()) < 1e-3
    # the rows the rankers transform (b4r_mlm_transform_rows) carry the MLM activation too
    seq = ar.encoder_forward(params, batch["input_word_ids"], batch["input_mask"], cfg_o, "relu")["sequence_output"]
    t_ref = ar.mlm_transform(params, seq, batch["masked_lm_positions"], cfg_o, "tanh").reshape(-1, H)
    rows = (torch.arange(6)[:, None] * L + batch["masked_lm_positions"]).reshape(-1).cuda()
    t = enc.engine.mlm_transform_rows(seq.reshape(-1, H).cuda().contiguous(), rows)
    torch.cuda.synchronize()
    assert float((t.cpu() - t_ref).abs().max()) < 1e-4
    top_ref = torch.topk(t_ref @ params["word_embeddings/embeddings"].t() + params["cls/predictions/output_bias/bias"], 10).indices
    top = torch.topk(t.cpu() @ params["word_embeddings/embeddings"].t() + params["cls/predictions/output_bias/bias"], 10).indices
    assert float((top == top_ref).float().mean()) >= 0.999


# ---- device math on a grid: the 1e-6 max(1, |f|) bound on [-30, 30] and finite values at +-88 -------------------------------------
GRID = np.concatenate([np.linspace(-30, 30, 6001), [-88.0, -50.0, -1e-3, -1e-6, 0.0, 1e-6, 1e-3, 50.0, 88.0]]).astype(np.float32)


@pytest.mark.usefixtures("gemm_mode")
@pytest.mark.parametrize("act", IDS)
def test_device_activation_math_meets_its_bound_on_a_grid(act):
    """the BIAS_GELU epilogue with a zero product (pre = bias: the grid exactly) and the GELU_BWD epilogue with a product of exactly 1
    (ones . (1/64)^T over K = 64) give f and f' at the grid points"""
    lib = _lib.load()
    x = torch.tensor(GRID)
    N = ((x.numel() + 3) // 4) * 4
    xs = torch.zeros(N)
    xs[:x.numel()] = x
    M, K = 32, 64
    zeros = torch.zeros(M, K, device="cuda")
    B = torch.zeros(K, N, device="cuda")
    bias = xs.cuda()
    Cm, C2 = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
    d = _lib.GemmDesc()
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.M, d.N, d.K = P(zeros), K, P(B), N, P(Cm), N, M, N, K
    d.epilogue, d.bias, d.C2, d.ldc2, d.qscale, d.activation = _lib.EPI_BIAS_GELU, P(bias), P(C2), N, 1.0, act
    _lib.check(lib.b4r_gemm_f32(C.byref(d), stream()), "b4r_gemm_f32")
    ones = torch.ones(M, K, device="cuda")
    W = torch.full((N, K), 1.0 / 64, device="cuda")
    R = xs.cuda().expand(M, N).contiguous()
    Cb = torch.empty(M, N, device="cuda")
    d = _lib.GemmDesc()
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.M, d.N, d.K, d.b_is_nk = P(ones), K, P(W), K, P(Cb), N, M, N, K, 1
    d.epilogue, d.R, d.ldr, d.qscale, d.activation = _lib.EPI_GELU_BWD, P(R), N, 1.0, act
    _lib.check(lib.b4r_gemm_f32(C.byref(d), stream()), "b4r_gemm_f32")
    torch.cuda.synchronize()
    n = x.numel()
    f64, d64 = ar.value_and_grad64(ar.NAMES[act], GRID.astype(np.float64))
    for got, want, what in ((Cm[0, :n], f64, "f"), (Cb[0, :n], d64, "f'")):
        g = got.double().cpu().numpy()
        assert np.all(np.isfinite(g)), (ar.NAMES[act], what)
        inside = np.abs(GRID) <= 30
        err = np.abs(g - want)[inside] / np.maximum(1.0, np.abs(want[inside]))
        assert err.max() <= 1e-6, (ar.NAMES[act], what, float(err.max()), float(GRID[inside][err.argmax()]))
    assert torch.equal(Cm, Cm[0].expand(M, N)) and torch.equal(Cb, Cb[0].expand(M, N))


# ---- the LayerNorm transform epilogue (hidden 64, bf16x3) ------------------------------------------------------------------------------
@pytest.mark.parametrize("act", IDS)
def test_bias_activation_layer_norm_epilogue_matches_fp64(act):
    lib = _lib.load()
    prev = lib.b4r_get_gemm_mode()
    lib.b4r_set_gemm_mode(_lib.GEMM_BF16X3)
    try:
        g = torch.Generator().manual_seed(90 + act)
        M, N, K = 160, 64, 128
        A = (torch.randn(M, K, generator=g) * 0.5).cuda()
        B = (torch.randn(K, N, generator=g) * 0.2).cuda()
        bias = (torch.randn(N, generator=g) * 0.3).cuda()
        gam = (1 + 0.1 * torch.randn(N, generator=g)).cuda()
        bet = (0.1 * torch.randn(N, generator=g)).cuda()
        Cm, C2, C3 = (torch.full((M, N), float("nan"), device="cuda") for _ in range(3))
        mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
        d = _lib.GemmDesc()
        d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.M, d.N, d.K = P(A), K, P(B), N, P(Cm), N, M, N, K
        d.epilogue, d.bias, d.C2, d.ldc2, d.C3, d.ldc3, d.qscale = _lib.EPI_BIAS_GELU_LN, P(bias), P(C2), N, P(C3), N, 1.0
        d.ln_gamma, d.ln_beta, d.ln_mean, d.ln_rstd, d.ln_eps, d.activation = P(gam), P(bet), P(mean), P(rstd), 1e-12, act
        assert lib.b4r_gemm_ln_supported(C.byref(d)) == 1
        _lib.check(lib.b4r_gemm_f32(C.byref(d), stream()), "b4r_gemm_f32")
        torch.cuda.synchronize()
        pre = A.double() @ B.double() + bias.double()
        f = torch.tensor(act64(act, pre)[0])
        mu = f.mean(-1, keepdim=True)
        var = ((f - mu) ** 2).mean(-1, keepdim=True)
        y = (f - mu) / torch.sqrt(var + 1e-12) * gam.double().cpu() + bet.double().cpu()
        assert float((C3.double().cpu() - pre.cpu()).abs().max()) < 1e-4
        assert float((Cm.double().cpu() - f).abs().max()) < 1e-4 * max(1.0, float(f.abs().max()))
        # the LayerNorm amplifies by rstd: rows whose activation is nearly constant (sigmoid, tanh saturated) have a large one
        tol = 1e-4 * max(1.0, float((1.0 / torch.sqrt(var + 1e-12)).max()))
        assert float((C2.double().cpu() - y).abs().max()) < tol
    finally:
        lib.b4r_set_gemm_mode(prev)


# ---- the hidden-64 feed-forward block and the wide pair at 128 / 256, every id --------------------------------------------------------
def ffn_act_reference(t, N, H, act, rate, seed, step, site, x1_from_z1, eps=1e-12):
    """fp64: x1 = LN1(z1) (or given); x2 = LN2(x1 + drop(f(x1 W1 + b1) W2 + b2)); loss = sum(x2 * dx2); autograd"""
    from tests.test_gpu_blocks import ln64
    d = {k: v.double().requires_grad_(k != "dx2") for k, v in t.items()}
    if x1_from_z1:
        x1, mean1, rstd1 = ln64(d["z1"], d["g1"], d["be1"], eps)
    else:
        x1, mean1, rstd1 = d["x1"], None, None
    x1.retain_grad()
    fpre = x1 @ d["W1"] + d["b1"]
    fpre.retain_grad()
    y = ar.ACT[ar.NAMES[act]](fpre) @ d["W2"] + d["b2"]
    if rate > 0:
        y = y * orc.dropout_keep_mask((N, H), rate, seed, step, site).double() / (1.0 - rate)
    z2 = x1 + y
    z2.retain_grad()
    x2, mean2, rstd2 = ln64(z2, d["g2"], d["be2"], eps)
    (x2 * d["dx2"]).sum().backward()
    out = dict(x1=x1.detach(), z2=z2.detach(), x2=x2.detach(), mean2=mean2.detach(), rstd2=rstd2.detach(), dz2=z2.grad, df=fpre.grad,
               fpre=fpre.detach(), dx1=x1.grad)
    if x1_from_z1:
        out.update(mean1=mean1.detach(), rstd1=rstd1.detach(), dz1=d["z1"].grad, dW1=d["W1"].grad, db1=d["b1"].grad, dW2=d["W2"].grad,
                   db2=d["b2"].grad, dg1=d["g1"].grad, dbe1=d["be1"].grad)
    return out


@pytest.mark.parametrize("rate", [0.0, 0.2])
@pytest.mark.parametrize("act", IDS)
def test_ffn_block_matches_fp64_autograd_for_every_activation(act, rate):
    """b4r_ffn_block_fwd / _bwd (hidden 64, full mode); the row-list and slot modes run in the model tests below (head rows only)"""
    from tests import b4r_testlib as T
    from tests.test_gpu_blocks import ffn_inputs
    lib = _lib.load()
    prev = lib.b4r_get_gemm_mode()
    lib.b4r_set_gemm_mode(_lib.GEMM_BF16X3)
    try:
        N, seed, step, site = 333, 4242, 3, 7
        t = ffn_inputs(N, seed=N + act)
        ref = ffn_act_reference(t, N, 64, act, rate, seed, step, site, True)
        g = {k: v.cuda() for k, v in t.items()}
        x1 = ref["x1"].float().cuda()
        st = T.new_state(seed, step) if rate > 0 else None
        out = {k: torch.full(s, float("nan"), device="cuda") for k, s in
               dict(z2=(N, 64), x2=(N, 64), mean2=(N,), rstd2=(N,), dz1=(N, 64), dW1=(64, 256), db1=(256,), dW2=(256, 64), db2=(64,),
                    dln=(128,)).items()}
        d = _lib.FfnDesc()
        d.N, d.H, d.I, d.activation = N, 64, 256, act
        d.x1, d.W1, d.b1, d.W2, d.b2 = P(x1), P(g["W1"]), P(g["b1"]), P(g["W2"]), P(g["b2"])
        d.ln_gamma, d.ln_beta, d.ln_eps = P(g["g2"]), P(g["be2"]), 1e-12
        d.rng, d.drop_stream, d.drop_rate = P(st), site, rate
        d.z2, d.x2, d.mean2, d.rstd2 = P(out["z2"]), P(out["x2"]), P(out["mean2"]), P(out["rstd2"])
        _lib.check(lib.b4r_ffn_block_fwd(C.byref(d), stream()), "b4r_ffn_block_fwd")
        torch.cuda.synchronize()
        for k in ("z2", "x2"):
            assert T.maxdiff(out[k], ref[k]) < 1e-4 * max(1.0, float(ref[k].abs().max())), k
        dz2 = ref["dz2"].float().cuda()
        mean1, rstd1 = ref["mean1"].float().cuda(), ref["rstd1"].float().cuda()
        scratch = torch.empty(lib.b4r_ffn_block_bwd_scratch_floats(N), device="cuda")
        d.dz2, d.z1, d.mean1, d.rstd1, d.ln1_gamma = P(dz2), P(g["z1"]), P(mean1), P(rstd1), P(g["g1"])
        d.dz1, d.dW1, d.db1, d.dW2, d.db2, d.dln1_gamma = (P(out["dz1"]), P(out["dW1"]), P(out["db1"]), P(out["dW2"]), P(out["db2"]),
                                                           P(out["dln"]))
        d.scratch = P(scratch)
        _lib.check(lib.b4r_ffn_block_bwd(C.byref(d), stream()), "b4r_ffn_block_bwd")
        torch.cuda.synchronize()
        assert T.maxdiff(out["dz1"], ref["dz1"]) < 1e-4 * max(1.0, float(ref["dz1"].abs().max()))
        for k, r in (("dW1", "dW1"), ("db1", "db1"), ("dW2", "dW2"), ("db2", "db2")):
            assert T.maxdiff(out[k], ref[r]) < 2e-5 * max(1.0, float(ref[r].abs().max())), k
        assert T.maxdiff(out["dln"][:64], ref["dg1"]) < 2e-5 * max(1.0, float(ref["dg1"].abs().max()))
        assert T.maxdiff(out["dln"][64:], ref["dbe1"]) < 2e-5 * max(1.0, float(ref["dbe1"].abs().max()))
    finally:
        lib.b4r_set_gemm_mode(prev)


@pytest.mark.parametrize("rate", [0.0, 0.2])
@pytest.mark.parametrize("act", IDS)
@pytest.mark.parametrize("H", [128, 256])
def test_wide_ffn_pair_matches_fp64_autograd_for_every_activation(H, act, rate):
    """b4r_ffn_wide_fwd (with f / fpre and in the inference form the encoder-only forwards use) and b4r_ffn_wide_bwd"""
    from tests import b4r_testlib as T
    from tests.test_gpu_blocks import wide_ffn_inputs
    lib = _lib.load()
    prev = lib.b4r_get_gemm_mode()
    lib.b4r_set_gemm_mode(_lib.GEMM_BF16X3)
    try:
        I, N, seed, step, site = 4 * H, 219, 977, 5, 9
        t = wide_ffn_inputs(N, H, I, seed=N + H + act)
        ref = ffn_act_reference(t, N, H, act, rate, seed, step, site, False)
        g = {k: v.cuda() for k, v in t.items()}
        st = T.new_state(seed, step) if rate > 0 else None
        out = {k: torch.full(s, float("nan"), device="cuda") for k, s in
               dict(z2=(N, H), x2=(N, H), mean2=(N,), rstd2=(N,), f=(N, I), fpre=(N, I), df=(N, I), dx1=(N, H)).items()}
        scratch = torch.empty(lib.b4r_ffn_wide_scratch_floats(H, I), device="cuda")
        d = _lib.FfnDesc()
        d.N, d.H, d.I, d.activation = N, H, I, act
        d.x1, d.W1, d.b1, d.W2, d.b2 = P(g["x1"]), P(g["W1"]), P(g["b1"]), P(g["W2"]), P(g["b2"])
        d.ln_gamma, d.ln_beta, d.ln_eps = P(g["g2"]), P(g["be2"]), 1e-12
        d.rng, d.drop_stream, d.drop_rate = P(st), site, rate
        d.z2, d.x2, d.mean2, d.rstd2 = P(out["z2"]), P(out["x2"]), P(out["mean2"]), P(out["rstd2"])
        d.scratch = P(scratch)
        _lib.check(lib.b4r_ffn_wide_fwd(C.byref(d), P(out["f"]), P(out["fpre"]), stream()), "b4r_ffn_wide_fwd")
        torch.cuda.synchronize()
        for k in ("fpre", "z2", "x2"):
            assert T.maxdiff(out[k], ref[k]) < max(1e-4, 2e-5 * float(ref[k].abs().max())), k
        x2_keep = out["x2"].clone()
        out["x2"].fill_(float("nan"))
        _lib.check(lib.b4r_ffn_wide_fwd(C.byref(d), None, None, stream()), "b4r_ffn_wide_fwd")
        torch.cuda.synchronize()
        assert torch.equal(out["x2"], x2_keep)
        d.dz2 = P(ref["dz2"].float().cuda())
        _lib.check(lib.b4r_ffn_wide_bwd(C.byref(d), P(out["fpre"]), P(out["df"]), P(out["dx1"]), 1, stream()), "b4r_ffn_wide_bwd")
        torch.cuda.synchronize()
        assert T.maxdiff(out["df"], ref["df"]) < 1e-4 * max(1.0, float(ref["df"].abs().max())), "df"
        assert T.maxdiff(out["dx1"], ref["dx1"]) < 1e-4 * max(1.0, float(ref["dx1"].abs().max())), "dx1"
    finally:
        lib.b4r_set_gemm_mode(prev)


# ---- every feed-forward id through the model (hidden 64: Block, its slot mode under head rows only) -----------------------------------
@pytest.mark.parametrize("inner", list(ar.NAMES))
def test_every_inner_activation_through_the_hidden64_model(inner):
    cfg_o, eng, params = build(64, 2, None, inner, "softplus", od=0.1, ad=0.1)
    batch = orc.synthetic_batch(6, 48, 8, cfg_o.vocab_size, seed=6, ragged=True)
    loss_ref, grads_ref, _ = ar.loss_and_grads(params, batch, cfg_o, inner, "softplus", training=True, rng=(5, 2))
    for fused in (False, True):
        st, g = run_grads(eng, batch, True, fused)
        assert abs(st["loss_sum"] / st["valid_count"] - float(loss_ref)) < 1e-3
        compare_grads(g, grads_ref, st["valid_count"], rel=5e-3)


# ---- the launch forms --------------------------------------------------------------------------------------------------------------
def step_labels(eng, batch):
    lib = _lib.load()
    hp = make_adamw_config(num_warmup_steps=0)
    cb, keep = eng.prepare_batch(batch)
    eng.ensure_training_buffers()
    n = C.c_int32(0)
    us = (C.c_float * 512)()
    names = C.create_string_buffer(512 * 128)
    _lib.check(lib.b4r_timing_begin(stream(), 512), "b4r_timing_begin")
    eng.train_step(hp, cb)
    _lib.check(lib.b4r_timing_end(C.byref(n), us, names, 128, 512), "b4r_timing_end")
    return [names.raw[j * 128:(j + 1) * 128].split(b"\0", 1)[0].decode() for j in range(n.value)]


@pytest.mark.parametrize("name", ["h64", "h128_hd64", "h256"])
def test_forms_and_launch_count_do_not_depend_on_the_activation(name):
    """the train step (fused head, head rows only) launches the same kernels for every activation pair; the forms are the expected
    ones: Block at 64; Wide, then CompactRows on the last layer at 128; TileProducts, then CompactRows at 256"""
    H, heads, E = CASES[name]
    batch = orc.synthetic_batch(8, 64, 12, 307, seed=2, ragged=True)
    runs = {pair: step_labels(build(H, heads, E, *pair, L=64, od=0.1, ad=0.1)[1], batch) for pair in [("gelu", "gelu")] + PAIRS}
    base = runs[("gelu", "gelu")]
    for pair, labels in runs.items():
        assert labels == base, (pair, labels, base)
    if H == 64:
        assert base.count("b4r_ffn_block_fwd") == 2 and base.count("b4r_ffn_block_bwd (dw)") == 2, base
    elif H == 128:   # layer 0 Wide, the last layer CompactRows
        assert base.count("wide feed-forward block forward") == 1 and base.count("wide feed-forward block backward (df, dx1)") == 1, base
        assert any(l.startswith("last layer on the head's rows") for l in base), base
    else:
        assert not any("wide feed-forward" in l or l.startswith("b4r_ffn_block") for l in base), base
        assert any(l.startswith("last layer on the head's rows") for l in base), base


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_trainer_fit_evaluate_save_load_with_relu_and_tanh(tmp_path):
    from bert4rec_amd import dataloaders, datasets, evaluation, models, trainers
    from bert4rec_amd.models.components import networks
    from bert4rec_amd.trainers import optimizers
    ds = datasets.synthetic_dataset(n_users=120, n_items=300, min_len=4, max_len=40, seed=1)
    dl = dataloaders.get_dataloader_factory("bert4rec").create_ml_1m_dataloader(data_source=ds, max_seq_len=24,
                                                                                max_predictions_per_seq=6, input_duplication_factor=2)
    train, val, test = dl.prepare_training()
    enc = networks.Bert4RecEncoder(dl.tokenizer.get_vocab_size(), hidden_size=64, num_layers=2, num_attention_heads=2,
                                   max_sequence_length=24, inner_dim=256, output_dropout=0.1, attention_dropout=0.1, seed=3,
                                   inner_activation="relu")
    model = models.BERT4RecModel(enc, mlm_activation="tanh")
    trainer = trainers.get(model=model)
    trainer.initialize_model(optimizer=optimizers.get("adamw", init_lr=1e-3, num_warmup_steps=5, num_train_steps=2000))
    tb = dataloaders.make_batches(train, batch_size=64, seed=1)
    vb = dataloaders.make_batches(val, batch_size=64, seed=1)
    hist = trainer.train(tb, vb, epochs=1).history
    assert all(np.isfinite(v).all() for v in hist.values())
    evaluator = evaluation.get(dataloader=dl)
    testb = dataloaders.make_batches(test, batch_size=64, seed=1)
    evaluator.evaluate(model, testb)
    res = evaluator.get_metrics_results()
    assert res["Valid Ranks"] == len(test) and all(0 <= v <= 1 for k, v in res.items() if k != "Valid Ranks")
    # the trained model against the restatement
    cfg_o = orc.OracleConfig(vocab_size=enc.get_config()["vocab_size"], hidden_size=64, num_layers=2, num_attention_heads=2,
                             max_sequence_length=24, inner_dim=256)
    b0 = testb.batches[0]
    params = {k: v.clone() for k, v in model.get_weights().items()}
    ref = ar.model_forward(params, {k: torch.as_tensor(v) for k, v in b0.items()}, cfg_o, "relu", "tanh")["mlm_logits"]
    got = model(b0)["mlm_logits"].cpu()
    assert float((got - ref.reshape(got.shape)).abs().max()) < 1e-3
    wrapper = models.BERT4RecModelWrapper(model)
    trainer.update_wrapper_meta_info(wrapper, dl)
    wrapper.save(tmp_path / "model", dl.get_tokenizer(), mode=2)
    loaded = models.BERT4RecModelWrapper.load(tmp_path / "model", mode=2)
    m2 = loaded["model_wrapper"].model
    # inner_activation round-trips through encoder_config.json; mlm_activation is not persisted (as in the reference)
    assert m2.encoder.get_config()["inner_activation"] == "relu" and m2.encoder.engine.inner_activation == activations.RELU
    assert torch.equal(model.encoder(b0)["sequence_output"].cpu(), m2.encoder(b0)["sequence_output"].cpu())


def test_recommend_tensor_top10_follows_the_restatement():
    from bert4rec_amd.models.bert4rec_model import BERT4RecModel
    from bert4rec_amd.models.components.networks import Bert4RecEncoder
    V, L = 300, 24
    model = BERT4RecModel(Bert4RecEncoder(V, hidden_size=256, num_layers=2, num_attention_heads=8, max_sequence_length=L, inner_dim=1024,
                                          output_dropout=0.0, attention_dropout=0.0, seed=17, inner_activation="swish"),
                          mlm_activation="sigmoid")
    batch = orc.synthetic_batch(128, L, 6, V, seed=9, ragged=True)
    ids, scores, slots = model.recommend_tensor(batch, k=10)
    cfg_o = orc.OracleConfig(vocab_size=V, hidden_size=256, num_layers=2, num_attention_heads=8, max_sequence_length=L, inner_dim=1024)
    params = {k: v.clone() for k, v in model.get_weights().items()}
    logits = ar.model_forward(params, batch, cfg_o, "swish", "sigmoid")["mlm_logits"].reshape(-1, V)[slots.cpu()].numpy()
    b_idx = (slots // 6).cpu()
    seen = batch["input_word_ids"][b_idx]
    ids_h = ids.cpu().numpy()
    same = []
    for r in range(int(slots.numel())):
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


def test_explicit_gelu_is_bitwise_the_default():
    from bert4rec_amd.models.bert4rec_model import BERT4RecModel
    from bert4rec_amd.models.components.networks import Bert4RecEncoder
    batch = orc.synthetic_batch(8, 32, 6, 211, seed=2, ragged=True)
    hp = make_adamw_config(num_warmup_steps=0)
    out = []
    for kw in ({}, {"inner_activation": "gelu"}):
        enc = Bert4RecEncoder(211, hidden_size=64, num_layers=2, num_attention_heads=2, max_sequence_length=32, inner_dim=256, seed=4,
                              **kw)
        model = BERT4RecModel(enc, **({"mlm_activation": "gelu"} if kw else {}))
        cb, keep = enc.engine.prepare_batch(batch)
        enc.engine.set_seed(3)
        for _ in range(2):
            enc.engine.train_step(hp, cb)
        torch.cuda.synchronize()
        out.append((enc.engine.params.clone(), model(batch)["mlm_logits"].cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
