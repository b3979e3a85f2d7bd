"""GPU parity tests of b4r_train_step itself -- what bench.py times and what single-GPU training runs -- at every shipped encoder
configuration (bert4rec_amd/config) against the oracle.

The step combines pieces no other entry point uses together: the head merge folded into the transform's LayerNorm backward (hidden
64), the loss sums formed in the backward, the gradient norm from the closing reduce launch, the fused AdamW and the last layer on the
head's rows only (compact dense products, the slot-query attention).  A weight check after AdamW only confirms the sign of each
gradient at step 1 (the update is about lr * sign(g)), so every step here is checked through what it leaves behind:

* the gradient buffer against the oracle's autograd with the same dropout masks (parameters re-read from the device before each
  step, so nothing drifts between steps);
* the gradient the optimizer consumed, recovered from the first moment, against the oracle's clipped gradient;
* the optimizer itself: orc.adamw_apply fed the step's own gradient must give the parameters and moments the device holds, to fp32
  rounding (bias correction, schedule, decay mask and clip included);
* loss, gradient norm, counts and accuracy sums.

Tolerances: 1e-3 on the loss, relative 5e-3 on train-mode gradients and 2e-3 without dropout (as in test_gpu_model.py)."""
import ctypes as C

import pytest
import torch

from bert4rec_amd import _lib
from bert4rec_amd.config import available_configs, get_encoder_config
from bert4rec_amd.engine import make_adamw_config
from oracle import bert4rec_oracle as orc
from tests.b4r_testlib import set_row_slots
from tests.test_gpu_model import LOGIT_TOL, build, compare_grads

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gemm_mode")]

# item vocabulary of each dataset (items + PAD / MASK / UNK)
VOCAB = {"ml-1m": 3709, "ml-20m": 26732, "steam": 13047, "beauty": 54545, "reddit": 335423}
# configurations whose steps run with the clip active (gradient_clip_norm far below the gradient norm)
CLIPPED = {"ml-1m_64", "steam_128", "beauty_256", "ml-20m_256", "reddit_128"}
TIE = 1e-4        # top-2 oracle logits closer than this: the argmax may differ between two float implementations
# in the exact-fp32 mode (the materialising head, no slot-query attention) one configuration per hidden size: the rest of that half
# of the matrix doubled the file's time for the same kernels at other sizes
F32_CASES = {"ml-1m_64", "ml-1m_128", "steam_256"}


def set_edge_rows(batch):
    """row 0: a valid slot at position 0 and fewer than P masks, so that the padding slots (position 0, id 0) collide with it (what
    the reference's preprocessor produces whenever it masks position 0); row 1: a single valid slot"""
    n0 = int(batch["input_mask"][0].sum())
    set_row_slots(batch, 0, [0] + list(range(2, n0, max(1, n0 // 4)))[:3], orc.MASK_TOKEN_ID)
    set_row_slots(batch, 1, [int(batch["input_mask"][1].sum()) - 1], orc.MASK_TOKEN_ID)
    return batch


def shipped_case(name, num_layers=None, dropout=True):
    """oracle config, batch and Adam hyper-parameters of one train step at a shipped configuration (small batch)"""
    c = get_encoder_config(name)
    L = c["max_sequence_length"]
    V = VOCAB[name.rsplit("_", 1)[0]]
    B, P = (8, 40) if L == 200 else (24, 20)
    if V > 100000:
        B = 4      # the oracle's fp32 logits alone are B * P x V
    cfg_o = orc.OracleConfig(vocab_size=V, hidden_size=c["hidden_size"], num_layers=num_layers or c["num_layers"],
                             num_attention_heads=c["num_attention_heads"], max_sequence_length=L, inner_dim=c["inner_dim"],
                             output_dropout=c["output_dropout"] if dropout else 0.0,
                             attention_dropout=c["attention_dropout"] if dropout else 0.0)
    batch = set_edge_rows(orc.synthetic_batch(B, L, P, V, seed=len(name) + L, ragged=True))
    clip = 1e-3 if name in CLIPPED else 5.0
    hp_o = orc.AdamWConfig(num_warmup_steps=0, num_train_steps=100, gradient_clip_norm=clip)   # lr > 0 at step 0, decays at step 1
    return cfg_o, batch, hp_o


def hip_adamw_config(hp_o):
    return make_adamw_config(hp_o.init_lr, hp_o.num_train_steps, hp_o.num_warmup_steps, hp_o.end_lr, hp_o.weight_decay_rate,
                             hp_o.beta_1, hp_o.beta_2, hp_o.epsilon, hp_o.gradient_clip_norm)


def assert_counts_match(st, batch, logits, tie_width=TIE):
    """valid / slot counts exactly; argmax hits exactly but for slots whose two best oracle logits (nearly) tie"""
    y = batch["masked_lm_ids"]
    assert st["valid_count"] == float((y != 0).sum())
    assert st["slots_all"] == float(y.numel())
    top = logits.topk(2, dim=-1)
    hit = top.indices[..., 0] == y
    tie = (top.values[..., 0] - top.values[..., 1]) < tie_width
    valid = y != 0
    assert abs(st["correct_masked"] - float((hit & valid).sum())) <= float((tie & valid).sum()), "masked accuracy"
    assert abs(st["correct_all"] - float(hit.sum())) <= float(tie.sum()), "sparse categorical accuracy"


def relative_error(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def launch_labels(fn, cap=256):
    """run fn() under the launch timer (b4r_timing_begin / b4r_timing_end): the labels of its launches in enqueue order.  The timer
    records at most cap launches; a full record may have dropped some, so it fails rather than return a truncated list"""
    lib = _lib.load()
    stride = 128
    n = C.c_int32(0)
    us = (C.c_float * cap)()
    names = C.create_string_buffer(cap * stride)
    _lib.check(lib.b4r_timing_begin(torch.cuda.current_stream().cuda_stream, cap), "b4r_timing_begin")
    fn()
    _lib.check(lib.b4r_timing_end(C.byref(n), us, names, stride, cap), "b4r_timing_end")
    assert n.value < cap, f"launch timer full ({cap} launches): pass a larger cap"
    return [names.raw[j * stride:(j + 1) * stride].split(b"\0", 1)[0].decode() for j in range(n.value)]


def run_and_check_train_step(eng, cfg_o, batch, cb, hp_o, step, seed, rel, labels=None, ref=orc.loss_and_grads, label_cap=256,
                             step_fn=None):
    """one Engine.train_step (the engine's state holds `step`), checked against the oracle as the module docstring says; returns the
    state it left and the oracle's gradient norm.  labels (a list): filled with the step's launches (launch timer, at most label_cap
    of them).  ref: the restatement the step is checked against (ref(params, batch, cfg_o, training=, rng=) -> loss, gradients,
    outputs).  step_fn(hp, cb): the step under test (default eng.train_step; tests/test_gpu_dp_matrix.py: the data-parallel step)"""
    step_fn = step_fn or eng.train_step
    hp = hip_adamw_config(hp_o)
    eng.ensure_training_buffers()
    names = [n for n in eng.variable_names() if orc.is_trainable(n)]
    params_now = eng.export_named()
    m_now, v_now = eng.export_named(eng.adam_m), eng.export_named(eng.adam_v)
    loss_ref, grads_ref, out_ref = ref(params_now, batch, cfg_o, training=True, rng=(seed, step))
    if labels is None:
        step_fn(hp, cb)
    else:
        labels[:] = launch_labels(lambda: step_fn(hp, cb), label_cap)
    torch.cuda.synchronize()
    st = eng.read_state()
    assert st["step"] == step + 1
    grads = eng.export_named(eng.grads)
    params_after, m_after, v_after = eng.export_named(), eng.export_named(eng.adam_m), eng.export_named(eng.adam_v)
    cnt = st["valid_count"]

    # scalars
    assert_counts_match(st, batch, out_ref["mlm_logits"])
    gnorm_ref = float(sum(g.double().pow(2).sum() for g in grads_ref.values()).sqrt())
    print(f"MEASURED step {step}: loss err {abs(st['loss_sum'] / cnt - float(loss_ref)):.2e}, "
          f"gradient norm rel err {abs(st['grad_norm'] - gnorm_ref) / gnorm_ref:.2e}")
    assert abs(st["loss_sum"] / cnt - float(loss_ref)) < LOGIT_TOL
    assert abs(st["grad_norm"] - gnorm_ref) <= 2e-3 * gnorm_ref, (st["grad_norm"], gnorm_ref)

    # the gradient buffer
    worst = compare_grads(grads, grads_ref, cnt, rel=rel)
    print(f"MEASURED step {step}: worst gradient tensor rel err {worst[1]:.2e} ({worst[0]})")

    # what the optimizer consumed: m = b1 m_before + (1 - b1) clip_scale g
    clip_scale = min(1.0, hp_o.gradient_clip_norm / gnorm_ref)
    b1 = hp_o.beta_1
    consumed = {n: (m_after[n].double() - b1 * m_now[n].double()) / (1.0 - b1) for n in names}
    compare_grads(consumed, {n: grads_ref[n] * clip_scale for n in names}, 1.0, rel=rel)

    assert_adamw_exact(st, names, grads, (params_now, m_now, v_now), (params_after, m_after, v_after), step, hp_o)
    return st, gnorm_ref


def assert_adamw_exact(st, names, grads, before, after, step, hp_o):
    """the optimizer, exactly: the oracle's AdamW from the pre-step state (params, m, v), fed the step's own gradient (the buffer over
    the valid count), must give the state the device holds after it"""
    params_now, m_now, v_now = before
    params_after, m_after, v_after = after
    inv = torch.tensor(1.0 / st["valid_count"], dtype=torch.float32)
    p_o = {n: params_now[n].clone() for n in names}
    m_o = {n: m_now[n].clone() for n in names}
    v_o = {n: v_now[n].clone() for n in names}
    orc.adamw_apply(p_o, {n: grads[n] * inv for n in names}, m_o, v_o, step, hp_o)
    for n in names:
        for what, got, want in (("param", params_after, p_o), ("m", m_after, m_o), ("v", v_after, v_o)):
            err = relative_error(got[n], want[n])
            assert err <= 1e-6, f"AdamW {what} of {n} at step {step}: relative error {err:.2e}"
    assert abs(st["lr"] - float(orc.learning_rate(step, hp_o))) <= 1e-6 * hp_o.init_lr


def two_steps(cfg_o, batch, hp_o, rel, seed=4321):
    eng, _ = build(cfg_o)
    eng.set_seed(seed)
    cb, keep = eng.prepare_batch(batch)
    clipped, labels = [], []
    for step in range(2):
        st, gnorm = run_and_check_train_step(eng, cfg_o, batch, cb, hp_o, step, seed, rel, labels=labels if step == 0 else None)
        clipped.append(gnorm > hp_o.gradient_clip_norm)
    return clipped, labels


def assert_train_step_paths(cfg_o, labels):
    """the logits-free step takes the paths this matrix is meant to check (launch timer labels): hidden 64 folds the head's merge
    into the transform's LayerNorm backward (no combine launch); the wider sizes with inner >= 3 hidden + 8 (here P <= L / 2) run the
    last layer on the head's compact rows, with the slots as the attention's only queries where L > 64; inner below that (ml-1m_256)
    keeps it dense"""
    H, I, L = cfg_o.hidden_size, cfg_o.inner_dim, cfg_o.max_sequence_length
    rows = any(l.startswith("last layer on the head's rows") for l in labels)
    slotq = any(l.endswith("queries = the head's slots") for l in labels)
    assert labels.count("masked-LM head forward (fused)") == 1, labels
    if H == 64:
        assert "masked-LM head combine" not in labels, labels
    elif I >= 3 * H + 8:
        assert rows and slotq == (L > 64), labels
    else:
        assert not rows and not slotq, labels


@pytest.mark.parametrize("name", available_configs())
def test_train_step_matches_oracle_at_every_shipped_config(name, gemm_mode):
    if gemm_mode == "f32" and name not in F32_CASES:
        pytest.skip("exact-fp32 mode: one configuration per hidden size (F32_CASES)")
    cfg_o, batch, hp_o = shipped_case(name)
    clipped, labels = two_steps(cfg_o, batch, hp_o, rel=5e-3)
    if name in CLIPPED:
        assert all(clipped)
    if gemm_mode == "bf16x3":
        assert_train_step_paths(cfg_o, labels)


@pytest.mark.parametrize("name", ["steam_64", "ml-1m_128", "ml-1m_256"])
def test_train_step_without_dropout_matches_oracle(name):
    """one configuration per hidden size with both dropout rates 0: the gradient tolerance of eval mode"""
    cfg_o, batch, hp_o = shipped_case(name, dropout=False)
    two_steps(cfg_o, batch, hp_o, rel=2e-3)


def test_train_step_at_the_four_layer_ml20m_shape_matches_oracle(gemm_mode):
    """BASELINE.json configs[3]: ml-20m_256 with four layers"""
    if gemm_mode == "f32":
        pytest.skip("exact-fp32 mode: one configuration per hidden size (F32_CASES)")
    cfg_o, batch, hp_o = shipped_case("ml-20m_256", num_layers=4)
    clipped, labels = two_steps(cfg_o, batch, hp_o, rel=5e-3)
    assert all(clipped)
    assert_train_step_paths(cfg_o, labels)
