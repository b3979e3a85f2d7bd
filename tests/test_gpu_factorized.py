"""Factorised item embeddings (embedding_width E < hidden_size H) on the GPU: the two new launches against fp64 autograd, the model's
forward, gradients and train steps against the restatement in tests/factorized_ref.py, reproducibility, the unfactorised _ex route
against the classic one, and the evaluation / app paths on a factorised model.

Tolerances as in test_gpu_model.py: 1e-3 on logits, relative 2e-3 on gradients without dropout and 5e-3 with it."""
import ctypes as C

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib
from bert4rec_amd.engine import Engine, make_adamw_config, make_model_config
from oracle import bert4rec_oracle as orc
from tests import factorized_ref as fr
from tests.test_gpu_model import compare_grads

pytestmark = [pytest.mark.gpu]

LOGIT_TOL = 1e-3


def build(H, E, heads=None, V=307, layers=2, L=48, od=0.0, ad=0.0, seed=3):
    heads = heads or H // 32
    cfg_o = orc.OracleConfig(vocab_size=V, hidden_size=H, num_layers=layers, num_attention_heads=heads, max_sequence_length=L,
                             inner_dim=4 * H, output_dropout=od, attention_dropout=ad)
    eng = Engine(make_model_config(V, H, layers, heads, L, 4 * H, od, ad), "cuda", embedding_width=E)
    params = fr.init_params(cfg_o, E, seed)
    eng.load_named(params)
    return cfg_o, eng, params


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- the two launches on their own ----------------------------------------------------------------------------------------------
@pytest.mark.usefixtures("gemm_mode")
@pytest.mark.parametrize("E,H,rate", [(64, 128, 0.0), (64, 256, 0.2), (128, 256, 0.0), (256, 512, 0.15)])
def test_embed_proj_ops_match_fp64_autograd(E, H, rate):
    """ragged ids with out-of-range entries (they read row 0), N = 3 * 37 (not a multiple of any tile), dropout with the exact mask"""
    lib = _lib.load()
    B, L, V = 3, 37, 53
    g = torch.Generator().manual_seed(E + H)
    ids = torch.randint(0, V, (B, L), generator=g)
    ids[0, 5], ids[1, 0], ids[2, 36] = -4, V, V + 100
    T = torch.randn(V, E, generator=g) * 0.5
    Pos = torch.randn(L, E, generator=g) * 0.5
    gam = 1 + 0.1 * torch.randn(E, generator=g)
    bet = 0.1 * torch.randn(E, generator=g)
    Wp = torch.randn(E, H, generator=g) * 0.05
    bp = 0.1 * torch.randn(H, generator=g)
    dx0 = torch.randn(B * L, H, generator=g)
    seed, step = 11, 4
    # fp64 reference
    leaf = [t.double().requires_grad_() for t in (T, Pos, gam, bet, Wp, bp)]
    safe = torch.where((ids >= 0) & (ids < V), ids, torch.zeros_like(ids))
    z = leaf[0][safe] + leaf[1][:L].unsqueeze(0)
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    y = (z - mean) / torch.sqrt(var + 1e-12) * leaf[2] + leaf[3]
    if rate > 0:
        keep = orc.dropout_keep_mask((B, L, E), rate, seed, step, orc.STREAM_EMB)
        y = torch.where(keep, y / (1 - rate), torch.zeros((), dtype=y.dtype))
    x0 = (y @ leaf[4] + leaf[5]).reshape(B * L, H)
    grads = torch.autograd.grad(x0, leaf, dx0.double())
    # d(item row + position row): autograd through z
    zl = z.detach().requires_grad_()
    m2 = zl.mean(-1, keepdim=True)
    y2 = (zl - m2) / torch.sqrt(((zl - m2) ** 2).mean(-1, keepdim=True) + 1e-12) * gam.double() + bet.double()
    if rate > 0:
        y2 = torch.where(keep, y2 / (1 - rate), torch.zeros((), dtype=y2.dtype))
    (drows_ref,) = torch.autograd.grad((y2 @ Wp.double() + bp.double()).reshape(B * L, H), zl, dx0.double())

    d = lambda t: t.float().contiguous().cuda()   # noqa: E731
    ids_d, T_d, P_d, g_d, b_d, W_d, bp_d, dx_d = d(ids).long(), d(T), d(Pos), d(gam), d(bet), d(Wp), d(bp), d(dx0)
    rng = torch.tensor([seed, step], dtype=torch.int32, device="cuda")
    x0_d = torch.empty(B * L, H, device="cuda")
    mean_d, rstd_d = torch.empty(B * L, device="cuda"), torch.empty(B * L, device="cuda")
    _lib.check(lib.b4r_embed_proj_fwd(ids_d.data_ptr(), B, L, T_d.data_ptr(), V, P_d.data_ptr(), g_d.data_ptr(), b_d.data_ptr(), E,
                                      1e-12, W_d.data_ptr(), bp_d.data_ptr(), H, x0_d.data_ptr(), mean_d.data_ptr(), rstd_d.data_ptr(),
                                      rng.data_ptr(), rate, stream()), "b4r_embed_proj_fwd")
    n_sc = lib.b4r_embed_proj_bwd_scratch_floats(B * L, E, H)
    assert n_sc > 0
    sc = torch.empty(n_sc, device="cuda")
    drows = torch.empty(B * L, E, device="cuda")
    dWp, dbp, dln = torch.empty(E, H, device="cuda"), torch.empty(H, device="cuda"), torch.empty(2 * E, device="cuda")
    _lib.check(lib.b4r_embed_proj_bwd(dx_d.data_ptr(), ids_d.data_ptr(), B, L, T_d.data_ptr(), V, P_d.data_ptr(), g_d.data_ptr(),
                                      b_d.data_ptr(), E, mean_d.data_ptr(), rstd_d.data_ptr(), W_d.data_ptr(), H, rng.data_ptr(), rate,
                                      drows.data_ptr(), dWp.data_ptr(), dbp.data_ptr(), dln.data_ptr(), sc.data_ptr(), stream()),
               "b4r_embed_proj_bwd")
    torch.cuda.synchronize()

    def rel(a, b):
        return float((a.double().cpu() - b).abs().max()) / max(float(b.abs().max()), 1e-30)
    assert rel(x0_d, x0.detach()) < 1e-5
    assert rel(dWp, grads[4]) < 1e-5 and rel(dbp, grads[5]) < 1e-5
    assert rel(dln[:E], grads[2]) < 1e-5 and rel(dln[E:], grads[3]) < 1e-5
    assert rel(drows.reshape(B, L, E), drows_ref) < 1e-4


@pytest.mark.parametrize("E", [32, 96, 512])
def test_embed_proj_ops_refuse_bad_widths(E):
    lib = _lib.load()
    assert lib.b4r_embed_proj_bwd_scratch_floats(64, E, 256) == -1
    x = torch.zeros(16, device="cuda")
    rc = lib.b4r_embed_proj_fwd(x.data_ptr(), 1, 2, x.data_ptr(), 2, x.data_ptr(), x.data_ptr(), x.data_ptr(), E, 1e-12, x.data_ptr(),
                                x.data_ptr(), 256, x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 0.0, stream())
    assert rc == -2


# ---- the model ---------------------------------------------------------------------------------------------------------------------
CASES = {"h128_e64": (128, 64, None), "h256_e64": (256, 64, None), "h256_e128": (256, 128, None), "h256_e64_hd64": (256, 64, 4)}


@pytest.mark.usefixtures("gemm_mode")
@pytest.mark.parametrize("name", list(CASES))
def test_forward_logits_match_the_restatement(name):
    H, E, heads = CASES[name]
    cfg_o, eng, params = build(H, E, heads)
    batch = orc.synthetic_batch(6, 48, 8, cfg_o.vocab_size, seed=4, ragged=True)
    cb, keep = eng.prepare_batch(batch)
    eng.forward(cb, training=False, pooler=False)
    torch.cuda.synchronize()
    ref = fr.model_forward(params, batch, cfg_o)
    logits = eng.region("mlm_logits", cb.B, cb.L, cb.P)[:, :cfg_o.vocab_size].cpu()
    assert float((logits - ref["mlm_logits"].reshape(logits.shape)).abs().max()) < LOGIT_TOL
    hid = eng.region("mlm_hidden", cb.B, cb.L, cb.P).cpu()
    assert hid.shape[1] == E
    assert float((hid - ref["mlm_hidden"].reshape(hid.shape)).abs().max()) < LOGIT_TOL


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
@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name", ["h128_e64", "h256_e128", "h256_e64_hd64"])
def test_every_gradient_matches_autograd(name, training, gemm_mode):
    H, E, heads = CASES[name]
    od, ad = (0.1, 0.1) if training else (0.0, 0.0)
    cfg_o, eng, params = build(H, E, heads, od=od, ad=ad)
    batch = orc.synthetic_batch(6, 48, 8, cfg_o.vocab_size, seed=6, ragged=True)
    loss_ref, grads_ref, _ = fr.loss_and_grads(params, batch, cfg_o, training=training, rng=(5, 2))
    heads_modes = [False] + ([True] if eng.fused_head_supported() else [])
    assert gemm_mode == "f32" or heads_modes == [False, True]
    for fused in heads_modes:
        st, g = run_grads(eng, batch, training, fused)
        assert abs(st["loss_sum"] / st["valid_count"] - float(loss_ref)) < 1e-3
        assert set(grads_ref) <= set(g) and "embedding_projection/kernel" in grads_ref
        assert tuple(g["word_embeddings/embeddings"].shape) == (cfg_o.vocab_size, E)
        compare_grads(g, grads_ref, st["valid_count"], rel=5e-3 if training else 2e-3)


def hip_hp(hp_o):
    return make_adamw_config(hp_o.init_lr, hp_o.num_train_steps, hp_o.num_warmup_steps, hp_o.end_lr, hp_o.weight_decay_rate,
                             hp_o.beta_1, hp_o.beta_2, hp_o.epsilon, hp_o.gradient_clip_norm)


@pytest.mark.usefixtures("gemm_mode")
@pytest.mark.parametrize("name", ["h128_e64", "h256_e128"])
def test_train_step_ex_follows_the_restatement_and_the_reference_optimizer(name):
    """three b4r_train_step_ex calls with dropout: each step's gradient (re-derived from the device's parameters) fed to
    oracle.adamw_apply must give the parameters the device holds"""
    H, E, heads = CASES[name]
    cfg_o, eng, params = build(H, E, heads, od=0.1, ad=0.1)
    batch = orc.synthetic_batch(6, 48, 8, cfg_o.vocab_size, seed=8, ragged=True)
    hp_o = orc.AdamWConfig(num_warmup_steps=0, num_train_steps=100, gradient_clip_norm=5.0)
    hp = hip_hp(hp_o)
    cb, keep = eng.prepare_batch(batch)
    eng.set_seed(21)
    eng.ensure_training_buffers()
    for step in range(3):
        p_now = eng.export_named()
        m_now, v_now = eng.export_named(eng.adam_m), eng.export_named(eng.adam_v)
        loss_ref, grads_ref, _ = fr.loss_and_grads(p_now, batch, cfg_o, training=True, rng=(21, step))
        eng.train_step(hp, cb)
        torch.cuda.synchronize()
        st = eng.read_state()
        assert st["step"] == step + 1
        assert abs(st["loss_sum"] / st["valid_count"] - float(loss_ref)) < 1e-3
        g = eng.export_named(eng.grads)
        compare_grads(g, grads_ref, st["valid_count"], rel=5e-3)
        # the optimizer on the step's own gradient
        trainable = [n for n in grads_ref]
        p_o = {n: p_now[n].clone() for n in trainable}
        m_o = {n: m_now[n].clone() for n in trainable}
        v_o = {n: v_now[n].clone() for n in trainable}
        mine = {n: g[n] / st["valid_count"] for n in trainable}
        orc.adamw_apply(p_o, mine, m_o, v_o, step, hp_o)
        after = eng.export_named()
        for n in trainable:
            err = float((after[n] - p_o[n]).abs().max())
            assert err < 1e-6 + 1e-5 * float(p_o[n].abs().max()), (n, err)


@pytest.mark.usefixtures("gemm_mode")
def test_two_identical_steps_are_bitwise_equal():
    outs = []
    for _ in range(2):
        cfg_o, eng, params = build(256, 64, od=0.2, ad=0.1)
        batch = orc.synthetic_batch(16, 48, 8, cfg_o.vocab_size, seed=9, ragged=True)
        cb, keep = eng.prepare_batch(batch)
        eng.set_seed(77)
        hp = make_adamw_config(num_warmup_steps=0, num_train_steps=10)
        eng.train_step(hp, cb)
        eng.train_step(hp, cb)
        torch.cuda.synchronize()
        outs.append((eng.params.clone(), eng.grads.clone(), eng.read_state()["loss_sum"]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]


@pytest.mark.usefixtures("gemm_mode")
@pytest.mark.parametrize("H", [64, 128])
def test_ex_at_full_width_is_bitwise_the_classic_step(H):
    """b4r_train_step_ex with embedding_width = hidden_size and b4r_train_step: the same bits"""
    lib = _lib.load()
    cfg_o = orc.OracleConfig(vocab_size=211, hidden_size=H, num_layers=2, num_attention_heads=H // 32, max_sequence_length=48,
                             inner_dim=4 * H, output_dropout=0.1, attention_dropout=0.1)
    params = orc.init_params(cfg_o, 3)
    batch = orc.synthetic_batch(8, 48, 8, 211, seed=10, ragged=True)
    hp = make_adamw_config(num_warmup_steps=0, num_train_steps=10)
    res = []
    for ex in (False, True):
        eng = Engine(make_model_config(211, H, 2, H // 32, 48, 4 * H, 0.1, 0.1), "cuda")
        eng.load_named(params)
        eng.set_seed(5)
        eng.ensure_training_buffers()
        cb, keep = eng.prepare_batch(batch)
        ws = eng.workspace(cb.B, cb.L, cb.P)
        args = (C.byref(hp), C.byref(cb), eng.params.data_ptr(), eng.grads.data_ptr(), eng.adam_m.data_ptr(), eng.adam_v.data_ptr(),
                ws.data_ptr(), ws.numel() * 4, eng.state.data_ptr(), stream())
        if ex:
            x = _lib.ModelConfigEx(eng.cfg, H, (0, 0, 0))
            _lib.check(lib.b4r_train_step_ex(C.byref(x), *args), "b4r_train_step_ex")
        else:
            _lib.check(lib.b4r_train_step(C.byref(eng.cfg), *args), "b4r_train_step")
        torch.cuda.synchronize()
        res.append((eng.params.clone(), eng.grads.clone(), eng.state.clone()))
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))


def test_grad_norm_of_a_factorised_step_is_the_norm_of_its_gradient_buffer():
    cfg_o, eng, params = build(256, 64, od=0.1, ad=0.1)
    if not eng.fused_head_supported():
        pytest.skip("needs the bf16x3 mode")
    batch = orc.synthetic_batch(8, 48, 8, cfg_o.vocab_size, seed=12, ragged=True)
    cb, keep = eng.prepare_batch(batch)
    hp = make_adamw_config(num_warmup_steps=0, num_train_steps=10, gradient_clip_norm=0.05)
    eng.set_seed(3)
    for _ in range(2):
        eng.train_step(hp, cb)
    torch.cuda.synchronize()
    st = eng.read_state()
    g = eng.grads[:eng.n_params].double()
    want = float(g.pow(2).sum().sqrt()) / st["valid_count"]
    assert want > 0 and abs(st["grad_norm"] - want) <= 2e-6 * want
    # ... and it came from the closing reduce launch: the count of the layout's trainable entries matched what that launch wrote, so
    # no separate norm launch ran (a mismatch would fall back to one and give the same norm)
    lib = _lib.load()
    n = C.c_int32(0)
    us = (C.c_float * 256)()
    names = C.create_string_buffer(256 * 128)
    _lib.check(lib.b4r_timing_begin(stream(), 256), "b4r_timing_begin")
    eng.train_step(hp, cb)
    _lib.check(lib.b4r_timing_end(C.byref(n), us, names, 128, 256), "b4r_timing_end")
    labels = [names.raw[j * 128:(j + 1) * 128].split(b"\0", 1)[0].decode() for j in range(n.value)]
    assert "global norm" not in labels and labels.count("multi_slab_reduce") == 1, labels
    assert "embed_proj_fwd" in labels and "embed_proj_bwd" in labels, labels


def test_item_table_scatter_at_width_e_poisons_out_of_range_contributions():
    cfg_o, eng, params = build(128, 64)
    batch = orc.synthetic_batch(4, 48, 8, cfg_o.vocab_size, seed=2, ragged=True)
    for scale in (1.0, 1e12):
        eng.load_named(params)
        cb, keep = eng.prepare_batch(batch)
        eng.ensure_training_buffers()
        eng.begin_step()
        eng.forward(cb, training=False, pooler=False)
        eng.loss(cb, want_grad=True)
        eng.region("mlm_logits", cb.B, cb.L, cb.P).mul_(scale)
        eng.backward(cb, training=False)
        torch.cuda.synchronize()
        g = eng.export_named(eng.grads)
        table, other = g["word_embeddings/embeddings"], g["transformer/layer_1/intermediate/kernel"]
        assert bool(torch.isfinite(other).all())
        if scale == 1.0:
            assert bool(torch.isfinite(table).all()) and float(table.abs().max()) > 0
        else:
            assert bool(torch.isnan(table).all())


# ---- evaluation and apps ----------------------------------------------------------------------------------------------------------
def factorised_model(H=256, E=64, V=307):
    from bert4rec_amd.models.bert4rec_model import BERT4RecModel
    from bert4rec_amd.models.components.networks import Bert4RecEncoder
    enc = Bert4RecEncoder(vocab_size=V, hidden_size=H, num_layers=2, num_attention_heads=H // 32, max_sequence_length=48,
                          inner_dim=4 * H, embedding_width=E, output_dropout=0.0, attention_dropout=0.0, device="cuda")
    return BERT4RecModel(enc)


def test_rank_items_and_full_ranking_on_a_factorised_model():
    model = factorised_model()
    cfg_o = orc.OracleConfig(vocab_size=307, hidden_size=256, num_layers=2, num_attention_heads=8, max_sequence_length=48,
                             inner_dim=1024)
    params = {n: t for n, t in model.get_weights().items()}
    batch = orc.synthetic_batch(8, 48, 4, 307, seed=13, ragged=True)
    ref = fr.model_forward(params, batch, cfg_o)["mlm_logits"].reshape(-1, 307)
    ranking, _, slots, _ = model.rank_items_tensor(batch)
    got = ranking[:, :10].cpu()
    want = ref[slots.cpu()].topk(10, dim=-1).indices
    agree = float((got == want).float().mean())
    if agree < 0.999:   # differences only between near-ties
        vals = ref[slots.cpu()]
        for r in range(got.shape[0]):
            a, b = vals[r, got[r]], vals[r, want[r]]
            assert float((a - b).abs().max()) < 1e-4
    # recommend_tensor (b4r_rank_full) against b4r_rank_candidates over the same hidden rows
    ids, scores, slots2 = model.recommend_tensor(batch, k=10, exclude_seen=False)
    hidden, _, _ = model._ranked_slot_hidden(batch)
    assert hidden.shape[1] == 64
    full, _, _ = model.engine.rank_candidates(hidden, None, None, None, n_candidates=307, n_rows=hidden.shape[0])
    full = full.cpu()
    for r in range(full.shape[0]):
        allowed = [int(i) for i in full[r] if int(i) >= 3][:10]
        assert ids[r].cpu().tolist() == allowed


def test_short_training_evaluation_and_save_load_round_trip(tmp_path):
    from bert4rec_amd.models.bert4rec_model import BERT4RecModel
    from bert4rec_amd.models.components.networks import Bert4RecEncoder
    from bert4rec_amd.trainers.optimizers import get as get_optimizer
    model = factorised_model(H=128, E=64)
    model.compile(optimizer=get_optimizer("adamw", num_train_steps=10, num_warmup_steps=1))
    batches = [orc.synthetic_batch(8, 48, 6, 307, seed=30 + i, ragged=True) for i in range(3)]
    for b in batches:
        model.train_step(b)
    res = model.evaluate(batches)
    assert np.isfinite(res["loss"])
    path = tmp_path / "w.safetensors"
    model.save_weights(path)
    w0 = model.get_weights()
    enc2 = Bert4RecEncoder(**{k: v for k, v in model.encoder.get_config().items()}, device="cuda")
    other = BERT4RecModel(enc2)
    other.load_weights(path)
    w1 = other.get_weights()
    assert set(w0) == set(w1) and all(torch.equal(w0[n], w1[n]) for n in w0)
    o0 = model(batches[0])["mlm_logits"]
    o1 = other(batches[0])["mlm_logits"]
    assert torch.equal(o0, o1)
    # a checkpoint of another width is refused with a clear error
    plain = BERT4RecModel(Bert4RecEncoder(vocab_size=307, hidden_size=128, num_layers=2, num_attention_heads=4,
                                          max_sequence_length=48, inner_dim=512, device="cuda"))
    with pytest.raises(ValueError, match="embedding_width"):
        plain.load_weights(path)


def test_trainer_and_full_ranking_evaluator_on_a_factorised_model(tmp_path):
    """the product surface end to end: trainers.get(...).train, evaluation.get(...) with sampled negatives and with full_ranking=True,
    and a wrapper save / load that round-trips embedding_width"""
    from bert4rec_amd import dataloaders, datasets, evaluation, models, trainers
    from bert4rec_amd.models.components import networks
    from bert4rec_amd.trainers import optimizers
    ds = datasets.synthetic_dataset(n_users=120, n_items=300, min_len=4, max_len=40, seed=1)
    dl = dataloaders.get_dataloader_factory("bert4rec").create_ml_1m_dataloader(data_source=ds, max_seq_len=24,
                                                                                max_predictions_per_seq=6, input_duplication_factor=2)
    train, val, test = dl.prepare_training()
    enc = networks.Bert4RecEncoder(dl.tokenizer.get_vocab_size(), hidden_size=128, num_layers=2, num_attention_heads=4,
                                   max_sequence_length=24, inner_dim=512, output_dropout=0.1, attention_dropout=0.1,
                                   embedding_width=64, seed=3)
    model = models.BERT4RecModel(enc)
    trainer = trainers.get(model=model)
    trainer.initialize_model(optimizer=optimizers.get("adamw", init_lr=1e-3, num_warmup_steps=5, num_train_steps=2000))
    tb = dataloaders.make_batches(train, batch_size=64, seed=1)
    vb = dataloaders.make_batches(val, batch_size=64, seed=1)
    hist = trainer.train(tb, vb, epochs=1).history
    assert all(np.isfinite(v).all() for v in hist.values())
    assert model.engine.read_state()["step"] == len(tb)
    testb = dataloaders.make_batches(test, batch_size=64, seed=1)
    for ev in (evaluation.get(dataloader=dl), evaluation.get(full_ranking=True)):
        ev.evaluate(model, testb)
        res = ev.get_metrics_results()
        assert res["Valid Ranks"] == len(test) and all(0 <= v <= 1 for k, v in res.items() if k != "Valid Ranks")
    wrapper = models.BERT4RecModelWrapper(model)
    trainer.update_wrapper_meta_info(wrapper, dl)
    wrapper.save(tmp_path / "model", dl.get_tokenizer(), mode=2)
    m2 = models.BERT4RecModelWrapper.load(tmp_path / "model", mode=2)["model_wrapper"].model
    assert m2.encoder.get_config()["embedding_width"] == 64
    b0 = testb.batches[0]
    assert torch.equal(model(b0)["mlm_logits"].cpu(), m2(b0)["mlm_logits"].cpu())
