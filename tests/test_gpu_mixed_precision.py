"""Mixed precision (B4R_GEMM_BF16, policy "mixed_bfloat16") on the GPU: the one-term kernel instances against fp64 references of
bf16-rounded operands, the model against the oracle within bf16 bounds, the launch plan of mode 1, reproducibility and graphs.

Measured errors and the bounds asserted here: DESIGN.md, "Mixed precision"."""
import ctypes as C
import math

import pytest
import torch

from bert4rec_amd import _lib
from bert4rec_amd import mixed_precision as mp
from oracle import bert4rec_oracle as orc
from tests import b4r_testlib as T
from tests.b4r_testlib import P, stream
from tests.test_gpu_model import build
from tests.test_gpu_train_step import hip_adamw_config, launch_labels, shipped_case

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture
def bf16_mode():
    lib = _lib.load()
    prev = lib.b4r_get_gemm_mode()
    _lib.check(lib.b4r_set_gemm_mode(_lib.GEMM_BF16))
    yield lib
    lib.b4r_set_gemm_mode(prev)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.float32)


def bf(x):
    """round to bf16 (nearest even) and back: the operand a one-term product multiplies"""
    return x.to(torch.bfloat16).to(torch.float64)


def in_mode(lib, mode, fn):
    prev = lib.b4r_get_gemm_mode()
    _lib.check(lib.b4r_set_gemm_mode(mode))
    try:
        return fn()
    finally:
        lib.b4r_set_gemm_mode(prev)


def check_one_term(got, A, B):
    """got = A.B from the one-term path: close to the fp64 product of the bf16-rounded operands, and at least 10x closer to it
    than to the unrounded product (which proves that no lo term ran)"""
    scale = float((A.double().abs() @ B.double().abs()).max())
    err_r = T.maxdiff(got, bf(A) @ bf(B))
    err_x = T.maxdiff(got, A.double() @ B.double())
    assert err_r <= 1e-4 * scale, (err_r, scale)
    assert 10 * err_r < err_x, (err_r, err_x)


# the shapes of tests/test_gpu_ops.py that the bf16 tile kernels take (b4r_gemm_rx_supported): [K,N] and [N,K] register kernels
# (K = 32, 64), the K loop (K > 64), the 64 x 64 and 128 x 128 LDS tiles
@pytest.mark.parametrize("M,N,K", [(128, 64, 32), (512, 192, 64), (1024, 64, 64), (256, 64, 256), (128, 64, 192),
                                   (160, 128, 512), (384, 320, 256), (96, 1024, 128)])
@pytest.mark.parametrize("b_is_nk", [0, 1])
def test_tile_products_are_one_term(bf16_mode, M, N, K, b_is_nk):
    A, B = rnd(M, K, seed=1), rnd(K, N, seed=2, scale=0.3)
    Bop = B.t().contiguous() if b_is_nk else B
    c, _ = T.gemm(A.to(DEV), Bop.to(DEV), M, N, K, b_is_nk=b_is_nk)
    check_one_term(c, A, B)
    # an epilogue instance: the pre-activation copy of the bias + GELU epilogue is the product plus the bias
    bias = rnd(N, seed=3)
    c, c2 = T.gemm(A.to(DEV), Bop.to(DEV), M, N, K, b_is_nk=b_is_nk, epi=_lib.EPI_BIAS_GELU, bias=bias.to(DEV), want_c2=True)
    check_one_term(c2 - bias.to(DEV), A, B)


@pytest.mark.parametrize("R,Mo,No", [(1000, 64, 192), (517, 300, 64), (4096, 64, 64), (3000, 256, 1024), (70, 128, 128)])
def test_weight_gradient_products_are_one_term(bf16_mode, R, Mo, No):
    A, B = rnd(R, Mo, seed=10), rnd(R, No, seed=11)
    out, _, _ = T.gemm_tn(A.to(DEV), B.to(DEV), R, Mo, No)
    check_one_term(out, A.t(), B)


def attention_reference(q, k, v, mask, rate=0.0, keep=None):
    """q, k, v [B, L, h, d] fp64 (q already scaled, as the library's QKV product leaves it); mask [B, L]"""
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) + (1.0 - mask.double())[:, None, None, :] * -1e9
    a = torch.softmax(s, dim=-1)
    if keep is not None:
        a = a * keep.double() / (1 - rate)
    return torch.einsum("bhqk,bkhd->bqhd", a, v)


SEED, STEP, SID = 21, 4, 9


def attention_case(B, L, heads, d, rate, seed=22):
    H = heads * d
    qkv = rnd(B * L, 3 * H, seed=seed)
    qkv[:, :H] *= math.sqrt(32 / d)   # scores distributed alike at both widths
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.int64)
    dctx = rnd(B * L, H, seed=seed + 1)
    keep = orc.dropout_keep_mask((B, heads, L, L), rate, SEED, STEP, SID, orc.ATTN_PITCH) if rate > 0 else None
    x = qkv.double().view(B, L, 3, heads, d).clone().requires_grad_(True)
    ctx_ref = attention_reference(x[:, :, 0], x[:, :, 1], x[:, :, 2], mask, rate, keep)
    ctx_ref.backward(dctx.double().view(B, L, heads, d))
    return qkv, mask, dctx, ctx_ref.detach().reshape(B * L, H), x.grad.reshape(B * L, 3 * H)


def attention_fwd(lib, qd, md, B, L, heads, d, rate):
    H = heads * d
    st = T.new_state(SEED, STEP)
    ctx = torch.full((B * L, H), float("nan"), device=DEV)
    lse = torch.empty(B * heads * L, device=DEV)
    bits = torch.zeros(lib.b4r_attn_keep_words(B, L, heads), dtype=torch.int32, device=DEV)
    _lib.check(lib.b4r_attn_fwd_hd(P(qd), P(md), B, L, heads, d, P(ctx), P(lse), P(st), SID, rate, P(bits), stream()))
    torch.cuda.synchronize()
    return ctx, lse, bits, st


def attention_bwd(lib, qd, md, fwd, dcd, B, L, heads, d, rate):
    ctx, lse, bits, st = fwd
    dqkv = torch.full((B * L, 3 * heads * d), float("nan"), device=DEV)
    _lib.check(lib.b4r_attn_bwd_hd(P(qd), P(md), P(ctx), P(lse), P(dcd), B, L, heads, d, 1.0, P(dqkv), P(st), SID, rate, P(bits),
                                   stream()))
    torch.cuda.synchronize()
    return dqkv.cpu().double()


# width 32 at L = 50 and 240 runs the 16-token-tile core, at L = 200 the backward on 32-token tiles; width 64 is one core at every
# length.  Each backward is fed the SAME forward (mode 1's ctx, lse and dropout words), so its own arithmetic is what differs.
@pytest.mark.parametrize("d,L", [(32, 50), (32, 200), (32, 240), (64, 50), (64, 200), (64, 240)])
@pytest.mark.parametrize("rate", [0.0, 0.2])
def test_attention_cores_are_one_term(bf16_mode, d, L, rate):
    lib = bf16_mode
    B, heads = 2, 2
    qkv, mask, dctx, ctx_ref, g_ref = attention_case(B, L, heads, d, rate)
    qd, md, dcd = qkv.to(DEV), mask.to(DEV), dctx.to(DEV)
    fwd2 = attention_fwd(lib, qd, md, B, L, heads, d, rate)
    fwd1 = in_mode(lib, _lib.GEMM_BF16X3, lambda: attention_fwd(lib, qd, md, B, L, heads, d, rate))
    g2 = attention_bwd(lib, qd, md, fwd1, dcd, B, L, heads, d, rate)
    g1 = in_mode(lib, _lib.GEMM_BF16X3, lambda: attention_bwd(lib, qd, md, fwd1, dcd, B, L, heads, d, rate))
    ctx2, ctx1 = fwd2[0].cpu().double(), fwd1[0].cpu().double()
    gs = max(1.0, float(g_ref.abs().max()))
    e2_ctx, e2_g = float((ctx2 - ctx_ref).abs().max()), float((g2 - g_ref).abs().max()) / gs
    e1_ctx, e1_g = float((ctx1 - ctx_ref).abs().max()), float((g1 - g_ref).abs().max()) / gs
    print(f"d={d} L={L} rate={rate}: ctx err mode2 {e2_ctx:.2e} mode1 {e1_ctx:.2e}; grad err mode2 {e2_g:.2e} mode1 {e1_g:.2e}")
    assert e2_ctx < 1.2e-1 and e2_g < 8e-2        # measured up to 5.6e-2 and 3.8e-2 (bf16: 2^-9 relative per operand)
    assert float((ctx2 - ctx1).abs().max()) > 10 * e1_ctx
    assert float((g2 - g1).abs().max()) / gs > 10 * e1_g


def train_step_labels(lib, name, mode):
    cfg_o, batch, hp_o = shipped_case(name)

    def run():
        eng, _ = build(cfg_o)
        eng.set_seed(4321)
        cb, _ = eng.prepare_batch(batch)
        eng.ensure_training_buffers()
        return launch_labels(lambda: eng.train_step(hip_adamw_config(hp_o), cb))
    return in_mode(lib, mode, run)


def strip(name):
    """the launch's entry point: template arguments and the arithmetic tag of the label ("(bf16x3)" / "(bf16)") removed"""
    return name.split("<", 1)[0].replace("bf16x3", "bf16").replace(", bf16)", ")")


@pytest.mark.parametrize("name", ["ml-1m_64", "steam_64", "ml-1m_128"])
def test_mode_two_plans_the_launches_of_mode_one(bf16_mode, name):
    lib = bf16_mode
    l1 = [strip(n) for n in train_step_labels(lib, name, _lib.GEMM_BF16X3)]
    l2 = [strip(n) for n in train_step_labels(lib, name, _lib.GEMM_BF16)]
    assert len(l1) > 10
    assert l1 == l2


def cosine(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(a @ b) / max(float(a.norm() * b.norm()), 1e-300)


# loss relative error and, per gradient tensor, cosine and relative norm error of one mode-2 train step against the oracle's fp32
# step on the same dropout masks (bounds: DESIGN.md "Mixed precision", about 2-3x the measured errors)
@pytest.mark.parametrize("name", ["ml-1m_64", "steam_64", "ml-1m_128", "ml-20m_256"])
def test_train_step_matches_oracle_within_bf16_bounds(bf16_mode, name):
    cfg_o, batch, hp_o = shipped_case(name, num_layers=1 if name == "ml-20m_256" else None)
    eng, _ = build(cfg_o)
    seed = 4321
    eng.set_seed(seed)
    cb, _ = eng.prepare_batch(batch)
    eng.ensure_training_buffers()
    params_now = eng.export_named()
    loss_ref, grads_ref, _ = orc.loss_and_grads(params_now, batch, cfg_o, training=True, rng=(seed, 0))
    eng.train_step(hip_adamw_config(hp_o), cb)
    torch.cuda.synchronize()
    st = eng.read_state()
    cnt = st["valid_count"]
    loss_err = abs(st["loss_sum"] / cnt - float(loss_ref)) / abs(float(loss_ref))
    grads = eng.export_named(eng.grads)
    big = max(float(g.norm()) for g in grads_ref.values())
    worst_cos, worst_norm = 1.0, 0.0
    for n, g in grads_ref.items():
        if float(g.norm()) < 1e-3 * big:   # the key-bias gradient is analytically zero: rounding noise on both sides
            continue
        a = grads[n].double() / cnt
        worst_cos = min(worst_cos, cosine(a, g))
        worst_norm = max(worst_norm, float((a - g.double()).norm() / g.double().norm()))
    print(f"{name}: loss rel err {loss_err:.2e}, worst cosine {worst_cos:.6f}, worst rel norm err {worst_norm:.2e}")
    # measured: loss <= 5e-6, cosine >= 0.999987, norm error <= 5.2e-3 (the masked-LM head keeps its three terms)
    assert loss_err <= 2e-5
    assert worst_cos >= 0.99996
    assert worst_norm <= 1.5e-2


def run_steps(cfg_o, batch, hp_o, n, graphed=False, switch_after_capture=False):
    lib = _lib.load()
    eng, _ = build(cfg_o)
    eng.set_seed(77)
    cb, _ = eng.prepare_batch(batch)
    eng.ensure_training_buffers()
    hp = hip_adamw_config(hp_o)
    for i in range(n):
        if switch_after_capture and i == 2:   # steps 0 (eager) and 1 (captured) ran in mode 1
            _lib.check(lib.b4r_set_gemm_mode(_lib.GEMM_BF16))
        (eng.train_step_graphed if graphed else eng.train_step)(hp, cb)
    torch.cuda.synchronize()
    return eng.params.clone(), eng.read_state()["loss_sum"]


def test_mode_two_steps_are_reproducible_and_graphs_replay_them(bf16_mode):
    cfg_o, batch, hp_o = shipped_case("steam_64")
    p1, l1 = run_steps(cfg_o, batch, hp_o, 20)
    p2, l2 = run_steps(cfg_o, batch, hp_o, 20)
    assert torch.equal(p1, p2) and l1 == l2
    pg, lg = run_steps(cfg_o, batch, hp_o, 20, graphed=True)
    assert torch.equal(p1, pg) and l1 == lg


def test_graph_captured_in_mode_one_is_not_replayed_in_mode_two(bf16_mode):
    lib = bf16_mode
    cfg_o, batch, hp_o = shipped_case("steam_64")
    _lib.check(lib.b4r_set_gemm_mode(_lib.GEMM_BF16X3))
    pg, lg = run_steps(cfg_o, batch, hp_o, 3, graphed=True, switch_after_capture=True)
    # the same sequence eagerly: two mode-1 steps, then one mode-2 step
    eng, _ = build(cfg_o)
    eng.set_seed(77)
    cb, _ = eng.prepare_batch(batch)
    eng.ensure_training_buffers()
    hp = hip_adamw_config(hp_o)
    _lib.check(lib.b4r_set_gemm_mode(_lib.GEMM_BF16X3))
    eng.train_step(hp, cb)
    eng.train_step(hp, cb)
    _lib.check(lib.b4r_set_gemm_mode(_lib.GEMM_BF16))
    eng.train_step(hp, cb)
    torch.cuda.synchronize()
    assert torch.equal(eng.params, pg) and eng.read_state()["loss_sum"] == lg


def test_policy_reports_and_selects_mode_two(bf16_mode):
    assert mp.global_policy().name == "mixed_bfloat16"
    mp.set_global_policy("float32")
    assert bf16_mode.b4r_get_gemm_mode() == _lib.GEMM_BF16X3


# eval-mode logits of the materialising forward against the oracle, at a shipped hidden-64 shape and at width-64 heads (H 128,
# 2 heads), and the train step of the width-64 model against the oracle mask for mask
@pytest.mark.parametrize("H,heads,L", [(64, 2, 200), (64, 2, 50), (128, 2, 200)])
def test_eval_logits_match_oracle_within_bf16_bounds(bf16_mode, H, heads, L):
    from tests.test_gpu_headdim64 import oracle_cfg
    from tests.test_gpu_model import outputs
    cfg_o = oracle_cfg(H, heads, L)
    eng, params = build(cfg_o)
    batch = orc.synthetic_batch(4, L, 10, cfg_o.vocab_size, seed=1, ragged=True)
    ref = orc.model_forward(params, batch, cfg_o, training=False)
    cb, _ = eng.prepare_batch(batch)
    eng.forward(cb, training=False, pooler=True)
    got = outputs(eng, cb)
    err = T.maxdiff(got["mlm_logits"], ref["mlm_logits"])
    print(f"H={H} heads={heads} L={L}: logits max-abs {err:.2e}")
    assert err <= 5e-2


def test_width64_train_mode_matches_oracle_within_bf16_bounds(bf16_mode):
    from tests.test_gpu_headdim64 import oracle_cfg
    from tests.test_gpu_model import run_loss_and_grads
    cfg_o = oracle_cfg(128, 2, 100, dropout=0.2)
    eng, params = build(cfg_o)
    batch = orc.synthetic_batch(5, 100, 20, cfg_o.vocab_size, seed=3, ragged=True)
    loss_ref, grads_ref, _ = orc.loss_and_grads(params, batch, cfg_o, training=True, rng=(4242, 17))
    st, grads = run_loss_and_grads(eng, batch, training=True, seed=4242, step=17)
    loss_err = abs(st["loss_sum"] / st["valid_count"] - float(loss_ref)) / abs(float(loss_ref))
    big = max(float(g.norm()) for g in grads_ref.values())
    worst_cos, worst_norm = 1.0, 0.0
    for n, g in grads_ref.items():
        if float(g.norm()) < 1e-3 * big:
            continue
        a = grads[n].double() / st["valid_count"]
        worst_cos = min(worst_cos, cosine(a, g))
        worst_norm = max(worst_norm, float((a - g.double()).norm() / g.double().norm()))
    print(f"width 64: loss rel err {loss_err:.2e}, worst cosine {worst_cos:.6f}, worst rel norm err {worst_norm:.2e}")
    assert loss_err <= 1e-3
    assert worst_cos >= 0.9999
    assert worst_norm <= 2e-2


def train_and_evaluate(policy):
    from bert4rec_amd import dataloaders, evaluation, trainers
    from bert4rec_amd.trainers import optimizers
    from tests.test_gpu_api import make_loader, make_model
    prev = mp.global_policy().name
    mp.set_global_policy(policy)
    try:
        dl = make_loader()
        train, val, test = dl.prepare_training()
        model = make_model(dl.tokenizer.get_vocab_size(), dropout=0.1)
        trainer = trainers.get(model=model)
        trainer.initialize_model(optimizer=optimizers.get("adamw", init_lr=2e-3, num_warmup_steps=5, num_train_steps=2000))
        trainer.train(dataloaders.make_batches(train, batch_size=64, seed=1), dataloaders.make_batches(val, batch_size=64, seed=1),
                      epochs=6)
        evaluator = evaluation.get(dataloader=dl)
        evaluator.evaluate(model, dataloaders.make_batches(test, batch_size=64, seed=1))
        return evaluator.get_metrics_results()
    finally:
        mp.set_global_policy(prev)


def test_policy_end_to_end_training_and_evaluation():
    """trainer.train + evaluation.get on the labelled synthetic log of tests/test_gpu_api.py: mixed_bfloat16 against float32"""
    want = train_and_evaluate("float32")
    got = train_and_evaluate("mixed_bfloat16")
    print("float32", {k: round(want[k], 4) for k in ("NDCG@10", "HR@10")}, "mixed_bfloat16",
          {k: round(got[k], 4) for k in ("NDCG@10", "HR@10")})
    assert got["HR@10"] > 0.12
    # two training runs whose arithmetic differs diverge in trajectory, so the metrics differ by the sampling noise of this log's
    # 120 test users: two standard deviations of a rate near HR@10 (measured: NDCG@10 0.125 / 0.175, HR@10 0.258 / 0.308)
    n = got["Valid Ranks"]
    for k in ("NDCG@10", "HR@10"):
        p = want["HR@10"]
        assert abs(got[k] - want[k]) <= 2 * math.sqrt(2 * p * (1 - p) / n), (k, got[k], want[k])


# ---- the runtime-activation epilogues and the activation-gradient tail at one term, every id -----------------------------------------
def act64(act, x):
    from tests import activation_ref as ar
    f, d = ar.value_and_grad64(ar.NAMES[act], x.double().cpu().numpy())
    return torch.from_numpy(f), torch.from_numpy(d)


def check_one_term_scaled(got, A, B, s):
    """got = (A.B) * s (s elementwise, fp64) from the one-term path: as check_one_term, with the factor on every side"""
    scale = float(((A.double().abs() @ B.double().abs()) * s.abs()).max())
    err_r = T.maxdiff(got, (bf(A) @ bf(B)) * s)
    err_x = T.maxdiff(got, (A.double() @ B.double()) * s)
    assert err_r <= 1e-4 * scale, (err_r, scale)
    assert 10 * err_r < err_x, (err_r, err_x)


# the register kernel, and the shapes of the compact-row feed-forward products at hidden 128 (B*P = 960 rows) and 256
@pytest.mark.parametrize("M,N,K", [(96, 256, 64), (960, 512, 128), (384, 1024, 256)])
@pytest.mark.parametrize("act", range(9))
def test_activation_epilogues_are_one_term(bf16_mode, act, M, N, K):
    """B4R_EPI_BIAS_GELU / B4R_EPI_GELU_BWD with activation `act` in mode 2: the product one term, the activation (its derivative)
    the requested one, applied to the pre-activation the launch wrote"""
    g = torch.Generator().manual_seed(140 + act)
    A, B = torch.randn(M, K, generator=g) * 0.6, torch.randn(K, N, generator=g) * 0.3
    bias = torch.randn(N, generator=g) * 0.5
    c, c2 = T.gemm(A.to(DEV), B.to(DEV), M, N, K, epi=_lib.EPI_BIAS_GELU, bias=bias.to(DEV), want_c2=True, activation=act)
    torch.cuda.synchronize()
    check_one_term(c2 - bias.to(DEV), A, B)
    f, _ = act64(act, c2)
    assert float((c.cpu().double() - f).abs().max()) < 1e-4 * max(1.0, float(f.abs().max()))
    # backward: C = (dY . W^T) * f'(R), W as [N, K]
    dY, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.3
    R = torch.randn(M, N, generator=g) * 2
    cb, _ = T.gemm(dY.to(DEV), W.to(DEV), M, N, K, b_is_nk=1, epi=_lib.EPI_GELU_BWD, R=R.to(DEV), activation=act)
    torch.cuda.synchronize()
    _, fd = act64(act, R)
    check_one_term_scaled(cb, dY, W.t(), fd)


@pytest.mark.parametrize("act", range(9))
def test_activation_layer_norm_epilogue_is_one_term(bf16_mode, act):
    """B4R_EPI_BIAS_GELU_LN (hidden 64: the masked-LM transform) in mode 2: the pre-activation one term, then `act` and the LayerNorm
    in fp32 on it"""
    lib = bf16_mode
    g = torch.Generator().manual_seed(190 + act)
    M, N, K = 160, 64, 128
    A, B = torch.randn(M, K, generator=g) * 0.5, torch.randn(K, N, generator=g) * 0.2
    bias, gam, bet = torch.randn(N, generator=g) * 0.3, 1 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    Ad, Bd, bd, gd, btd = (t.to(DEV) for t in (A, B, bias, gam, bet))
    Cm, C2, C3 = (torch.full((M, N), float("nan"), device=DEV) for _ in range(3))
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    d = _lib.GemmDesc()
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.M, d.N, d.K = P(Ad), K, P(Bd), N, P(Cm), N, M, N, K
    d.epilogue, d.bias, d.C2, d.ldc2, d.C3, d.ldc3, d.qscale = _lib.EPI_BIAS_GELU_LN, P(bd), P(C2), N, P(C3), N, 1.0
    d.ln_gamma, d.ln_beta, d.ln_mean, d.ln_rstd, d.ln_eps, d.activation = P(gd), P(btd), P(mean), P(rstd), 1e-12, act
    assert lib.b4r_gemm_ln_supported(C.byref(d)) == 1
    _lib.check(lib.b4r_gemm_f32(C.byref(d), stream()), "b4r_gemm_f32")
    torch.cuda.synchronize()
    check_one_term(C3 - bd, A, B)
    f, _ = act64(act, C3)
    assert float((Cm.cpu().double() - f).abs().max()) < 1e-4 * max(1.0, float(f.abs().max()))
    mu = f.mean(-1, keepdim=True)
    var = ((f - mu) ** 2).mean(-1, keepdim=True)
    y = (f - mu) / torch.sqrt(var + 1e-12) * gam.double() + bet.double()
    tol = 1e-4 * max(1.0, float((1.0 / torch.sqrt(var + 1e-12)).max()))
    assert float((C2.cpu().double() - y).abs().max()) < tol


@pytest.mark.parametrize("act", range(9))
def test_weight_gradient_with_activation_gradient_tail_is_one_term(bf16_mode, act):
    """b4r_gemm_tn_f32 with dgrad_out / dgrad_gelu_pre (No = 64) in mode 2: out = A^T.B and dX = (B . W^T) * f'(G), one term each"""
    lib = bf16_mode
    g = torch.Generator().manual_seed(170 + act)
    Rr, Mo, No = 200, 256, 64
    A, Bm = torch.randn(Rr, Mo, generator=g), torch.randn(Rr, No, generator=g)
    W, G = torch.randn(Mo, No, generator=g) * 0.3, torch.randn(Rr, Mo, generator=g) * 2
    Ad, Bd, Wd, Gd = (t.to(DEV) for t in (A, Bm, W, G))
    out = torch.empty(Mo, No, device=DEV)
    dX = torch.full((Rr, Mo), float("nan"), device=DEV)
    sc = torch.empty(lib.b4r_gemm_tn_scratch_floats(Rr, Mo, No), device=DEV)
    d = _lib.GemmTnDesc()
    d.A, d.lda, d.B, d.ldb, d.out, d.ldo, d.R, d.Mo, d.No = P(Ad), Mo, P(Bd), No, P(out), No, Rr, Mo, No
    d.dgrad_w, d.dgrad_ldw, d.dgrad_out, d.dgrad_ldo, d.dgrad_gelu_pre, d.dgrad_ldg, d.activation = P(Wd), No, P(dX), Mo, P(Gd), Mo, act
    assert lib.b4r_gemm_tn_dgrad_supported(C.byref(d)) == 1
    _lib.check(lib.b4r_gemm_tn_f32(C.byref(d), P(sc), stream()), "b4r_gemm_tn_f32")
    torch.cuda.synchronize()
    check_one_term(out, A.t(), Bm)
    _, fg = act64(act, G)
    check_one_term_scaled(dX, Bm, W.t(), fg)
