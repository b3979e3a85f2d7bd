"""The feature-by-form matrix (tests/feature_matrix.py): factorised embeddings, the runtime activations and the three arithmetic
modes, each cell one Engine.train_step with the benchmark's flags (fused head, head rows only) at the sequence lengths where the
launch forms of real training run, checked against tests/activation_ref.py mask for mask.

Per cell and mode:

* the step's launch labels, parsed into forms, equal the cell's expected forms (a moved plan_step threshold fails here);
* f32 / bf16x3: run_and_check_train_step with the restatement -- the gradient buffer, the gradient AdamW consumed, AdamW to fp32
  rounding on the device's own gradient, loss, gradient norm, counts and accuracy sums (1e-3 on the loss, relative 5e-3 on the
  gradients);
* bf16 (mode 2): loss relative error and per-tensor cosine / relative norm error against the restatement (bounds: DESIGN.md §4.6),
  the gradient norm against the device's own gradient buffer, AdamW to fp32 rounding, the counts;
* mode 2 plans mode 1's launches: the same labels in the same order, the three-term kernels (hidden-64 blocks, slot-query
  attention, the Wide pair, the head, embed_proj) under the same label, the tile products and the cores tagged "bf16".

Plus the evaluation forward at EVAL_CELLS and, in mode 2, reproducibility and graph replay at REPRO_CELL."""
import functools
import re

import pytest
import torch

from bert4rec_amd import _lib, activations
from bert4rec_amd.engine import Engine, make_model_config
from oracle import bert4rec_oracle as orc
from tests import activation_ref as ar
from tests import factorized_ref as fr
from tests.b4r_testlib import maxdiff
from tests.feature_matrix import BATCH, CELLS, EVAL_CELLS, LAYERS, MODES, REPRO_CELL, VOCAB, Forms
from tests.test_gpu_mixed_precision import cosine
from tests.test_gpu_train_step import (assert_adamw_exact, assert_counts_match, hip_adamw_config, launch_labels,
                                       run_and_check_train_step, set_edge_rows)

pytestmark = pytest.mark.gpu

MODE_OF = {"f32": _lib.GEMM_F32, "bf16x3": _lib.GEMM_BF16X3, "bf16": _lib.GEMM_BF16}
SEED = 4321
DROPOUT = 0.1
# mode-2 bounds of the train step against the fp32 restatement: (loss relative, worst per-tensor cosine, worst relative norm
# error) -- test_train_step_matches_oracle_within_bf16_bounds's, and test_width64_train_mode_matches_oracle_within_bf16_bounds's at
# head width 64 (2-3x the measured worst)
BF16_BOUNDS = {32: (2e-5, 0.99996, 1.5e-2), 64: (1e-3, 0.9999, 2e-2)}
# ... wider where measured so: the two cells with the fewest labelled rows behind a Wide layer's weight
# gradients -- 68 slots at L = 96 (the last layer Wide: its dW1 from the one-term weight-gradient product, x1 from the one-term
# attention products) and 30 at L = 64 (layer 0's db1: column sums of the Wide backward's dF, fed by layer 1's one-term products);
# measured cosine 0.999933 / 0.999951, norm error 1.16e-2 / 9.9e-3
BF16_CELL_BOUNDS = {"h128_2P_gt_L": (2e-5, 0.9998, 3e-2), "b128_L64": (2e-5, 0.9998, 3e-2)}
# mode 2: the accuracy sums may differ at slots whose two best restatement logits lie closer than this
BF16_TIE = 1e-2


@pytest.fixture
def matrix_mode(request):
    """the arithmetic mode of one case (f32, bf16x3 or bf16); the previous mode is restored on exit"""
    lib = _lib.load()
    prev = lib.b4r_get_gemm_mode()
    _lib.check(lib.b4r_set_gemm_mode(MODE_OF[request.param]))
    yield request.param
    lib.b4r_set_gemm_mode(prev)


def set_mode(mode):
    _lib.check(_lib.load().b4r_set_gemm_mode(MODE_OF[mode]))


def build_cell(c, od=DROPOUT, ad=DROPOUT, seed=3):
    cfg_o = orc.OracleConfig(vocab_size=VOCAB, hidden_size=c.H, num_layers=LAYERS, num_attention_heads=c.heads, max_sequence_length=c.L,
                             inner_dim=c.inner, output_dropout=od, attention_dropout=ad)
    eng = Engine(make_model_config(VOCAB, c.H, LAYERS, c.heads, c.L, c.inner, od, ad), "cuda", embedding_width=c.E,
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
    return set_edge_rows(orc.synthetic_batch(BATCH, c.L, c.P, VOCAB, seed=seed + c.L, ragged=True))


def cell_ref(c):
    return functools.partial(ar.loss_and_grads, inner=c.acts[0], mlm=c.acts[1])


# ---- the launch labels as forms -------------------------------------------------------------------------------------------------
GEMM_DETAIL = re.compile(r"^b4r_gemm_f32\b.*\[M=(\d+) N=(\d+) K=(\d+) epi=(\d+)")
TN_DETAIL = re.compile(r"^b4r_gemm_tn_f32\b.*\[R=(\d+) Mo=(\d+) No=(\d+)( \+dgrad)?")


def is_wo_grad(label, N, H):
    """the launch after an unfolded attention block backward: dWo (with dWqkv as one pair launch, or as the first of two products).
    A folded one formed them itself, and the previous layer's feed-forward backward follows (its first weight gradient carries the
    input gradient, "+dgrad", or comes after the dF product).  Reductions the full reduce queue no longer takes (deep stacks) run as
    "slab_reduce" launches in between and are skipped."""
    t = TN_DETAIL.match(label)
    return label.startswith("b4r_gemm_tn_f32 pair") or bool(t and not t[4] and (int(t[1]), int(t[2]), int(t[3])) == (N, H, H))


def parse_forward(fwd, c, B):
    """the forward half of a step's forms -- or the forms of a forward alone (tests/test_gpu_inference_matrix.py) -- from its launch
    labels: (attention form per layer, feed-forward form per layer, emb_proj, emb_fused, slotq_rows).  The activation product
    (EPI_BIAS_GELU, [., inner] from [., hidden]) runs on B*L rows as a tile product and on B*P compact rows on the head's rows"""
    N, M = B * c.L, B * c.P
    attn_fwd, ffn_fwd = [], []
    slotq_rows = False
    for j, l in enumerate(fwd):
        g = GEMM_DETAIL.match(l)
        if l.startswith("b4r_attn_block_fwd"):
            attn_fwd.append("Block")
        elif l.startswith("attention core forward, queries = the head's slots"):
            attn_fwd.append("SlotQuery")
        elif l.startswith("b4r_attn_fwd_hd"):
            attn_fwd.append("Core64")
        elif l.startswith("b4r_attn_fwd"):
            attn_fwd.append("Core")
        elif l == "b4r_ffn_block_fwd":
            ffn_fwd.append("Block")
        elif l.startswith("wide feed-forward block forward"):
            ffn_fwd.append("Wide")
        elif g and int(g[4]) == _lib.EPI_BIAS_GELU and (int(g[2]), int(g[3])) == (c.inner, c.H) and int(g[1]) in (N, M):
            ffn_fwd.append("TileProducts" if int(g[1]) == N else "CompactRows")
            if int(g[1]) == M:   # no gather in front of it: the slot-query attention left the compact rows
                slotq_rows = not fwd[j - 1].startswith("last layer on the head's rows: gather")
    emb_proj = "embed_proj_fwd" in fwd
    emb_fused = not emb_proj and "b4r_embed_ln_fwd" not in fwd
    return attn_fwd, ffn_fwd, emb_proj, emb_fused, slotq_rows


def parse_forms(labels, c, B):
    """the forms of one train step (forward, then the backward from its opening "zero fill" launch), from its launch labels.
    Feed-forward products are told apart by their shapes: the activation product of the forward (parse_forward) and the
    activation-gradient product of the backward (EPI_GELU_BWD) run on B*L rows as tile products and on B*P compact rows on the
    head's rows.  slot_only_last is not visible in the labels: the plan asks for it exactly where the last
    layer runs the folded block backward with the feed-forward block (on the head's rows in a train step)."""
    split = next(j for j, l in enumerate(labels) if l.startswith("zero fill"))
    fwd, bwd = labels[:split], labels[split:]
    N, M = B * c.L, B * c.P
    attn_fwd, ffn_fwd, emb_proj, emb_fused, slotq_rows = parse_forward(fwd, c, B)
    attn_bwd, ffn_bwd = [], []
    for j, l in enumerate(bwd):
        g, t = GEMM_DETAIL.match(l), TN_DETAIL.match(l)
        if l.startswith("b4r_attn_block_bwd"):
            nxt = next(m for m in bwd[j + 1:] if not m.startswith("slab_reduce"))
            attn_bwd.append("Block" if is_wo_grad(nxt, N, c.H) else "BlockFolded")
        elif l.startswith("attention core backward, queries = the head's slots"):
            attn_bwd.append("SlotQuery")
        elif l.startswith("b4r_attn_bwd_hd"):
            attn_bwd.append("Core64")
        elif l.startswith("b4r_attn_bwd (32-token tiles"):
            attn_bwd.append("Core32")
        elif l.startswith("b4r_attn_bwd dq"):
            attn_bwd.append("Core16")
        elif l == "b4r_ffn_block_bwd (dx)":
            ffn_bwd.append("Block")
        elif l.startswith("wide feed-forward block backward"):
            ffn_bwd.append("Wide")
        elif g and int(g[4]) == _lib.EPI_GELU_BWD and (int(g[2]), int(g[3])) == (c.inner, c.H) and int(g[1]) in (N, M):
            ffn_bwd.append("TileProducts" if int(g[1]) == N else "CompactRows")
        elif t and t[4] and (int(t[1]), int(t[2]), int(t[3])) == (N, c.inner, c.H):   # dF with dW2 from one pass
            ffn_bwd.append("TileProducts")
    attn_bwd.reverse()
    ffn_bwd.reverse()
    assert emb_proj == ("embed_proj_bwd" in bwd), labels
    assert ffn_fwd == ffn_bwd, (ffn_fwd, ffn_bwd, labels)
    slot_only_last = bool(attn_bwd) and attn_bwd[-1] == "BlockFolded" and ffn_fwd[-1:] == ["Block"]
    return Forms(tuple(attn_fwd), tuple(attn_bwd), tuple(ffn_fwd), emb_proj, emb_fused, slot_only_last, slotq_rows)


def assert_forms(labels, c, mode, B):
    got = parse_forms(labels, c, B)
    want = c.forms(mode)
    print(f"forms [{mode}]: {got}")
    assert got == want, f"forms of the {mode} step: {got}, expected {want}\n{labels}"


# ---- the train step ---------------------------------------------------------------------------------------------------------------
def bf16_gradient_errors(grads, grads_ref, cnt):
    """the worst per-tensor cosine and relative norm error (each with its tensor's name) of a mode-2 gradient buffer over the valid
    count against the restatement's gradients"""
    big = max(float(g.norm()) for g in grads_ref.values())
    worst_cos, worst_norm = (1.0, ""), (0.0, "")
    for n, g in grads_ref.items():
        if float(g.norm()) < 1e-3 * big:   # the key-bias gradient is analytically zero: rounding noise on both sides
            continue
        a = grads[n].double() / cnt
        worst_cos = min(worst_cos, (cosine(a, g), n))
        worst_norm = max(worst_norm, (float((a - g.double()).norm() / g.double().norm()), n))
    return worst_cos, worst_norm


def check_bf16_step(eng, cfg_o, batch, cb, hp_o, c, labels, name, step_fn=None, ref=None):
    """one mode-2 Engine.train_step against the fp32 restatement within the bf16 bounds; AdamW and the counts exactly as in mode 1.
    step_fn(hp, cb): the step under test (default eng.train_step); ref: the restatement (default cell_ref(c))"""
    step_fn = step_fn or eng.train_step
    hp = hip_adamw_config(hp_o)
    eng.ensure_training_buffers()
    names = [n for n in eng.variable_names() if orc.is_trainable(n)]
    params_now = eng.export_named()
    m_now, v_now = eng.export_named(eng.adam_m), eng.export_named(eng.adam_v)
    loss_ref, grads_ref, out_ref = (ref or cell_ref(c))(params_now, batch, cfg_o, training=True, rng=(SEED, 0))
    labels[:] = launch_labels(lambda: step_fn(hp, cb))
    torch.cuda.synchronize()
    st = eng.read_state()
    assert st["step"] == 1
    cnt = st["valid_count"]
    grads = eng.export_named(eng.grads)
    assert_counts_match(st, batch, out_ref["mlm_logits"], tie_width=BF16_TIE)
    # the norm the clip used is the norm of the gradient the step left
    own = float(eng.grads[:eng.n_params].double().pow(2).sum().sqrt()) / cnt
    assert own > 0.0 and abs(st["grad_norm"] - own) <= 2e-6 * own, (st["grad_norm"], own)
    loss_err = abs(st["loss_sum"] / cnt - float(loss_ref)) / abs(float(loss_ref))
    worst_cos, worst_norm = bf16_gradient_errors(grads, grads_ref, cnt)
    print(f"{name} mode 2: loss rel err {loss_err:.2e}, worst cosine {worst_cos[0]:.6f} ({worst_cos[1]}), "
          f"worst rel norm err {worst_norm[0]:.2e} ({worst_norm[1]})")
    b_loss, b_cos, b_norm = BF16_CELL_BOUNDS.get(name, BF16_BOUNDS[c.head_dim])
    assert loss_err <= b_loss
    assert worst_cos[0] >= b_cos, worst_cos
    assert worst_norm[0] <= b_norm, worst_norm
    assert_adamw_exact(st, names, grads, (params_now, m_now, v_now),
                       (eng.export_named(), eng.export_named(eng.adam_m), eng.export_named(eng.adam_v)), 0, hp_o)


CASES = [pytest.param(name, mode, id=f"{name}-{mode}") for name, c in CELLS.items() for mode in c.modes]


@pytest.mark.parametrize("name,matrix_mode", CASES, indirect=["matrix_mode"])
def test_train_step_of_every_cell_follows_the_restatement_in_its_forms(name, matrix_mode):
    c = CELLS[name]
    cfg_o, eng, _ = build_cell(c)
    batch = cell_batch(c)
    hp_o = orc.AdamWConfig(num_warmup_steps=0, num_train_steps=100, gradient_clip_norm=5.0)
    eng.set_seed(SEED)
    cb, _ = eng.prepare_batch(batch)
    labels = []
    if matrix_mode == "bf16":
        check_bf16_step(eng, cfg_o, batch, cb, hp_o, c, labels, name)
    else:
        run_and_check_train_step(eng, cfg_o, batch, cb, hp_o, 0, SEED, rel=5e-3, labels=labels, ref=cell_ref(c))
    assert_forms(labels, c, matrix_mode, BATCH)


# ---- mode 2 plans mode 1's launches ---------------------------------------------------------------------------------------------------
def step_labels(c, mode):
    set_mode(mode)
    cfg_o, eng, _ = build_cell(c)
    eng.set_seed(SEED)
    cb, _ = eng.prepare_batch(cell_batch(c))
    eng.ensure_training_buffers()
    hp = hip_adamw_config(orc.AdamWConfig(num_warmup_steps=0, num_train_steps=100))
    return launch_labels(lambda: eng.train_step(hp, cb))


def one_term_label(label):
    """the mode-2 label of a mode-1 launch whose kernel has a one-term instance: the tile products and the attention cores"""
    label = label.replace("bf16x3", "bf16").replace("(32-token tiles)", "(32-token tiles, bf16)")
    return re.sub(r"^(b4r_attn_(?:fwd|bwd)_hd)\b", r"\1 (bf16)", label)


# labels of kernels with a one-term instance (every other launch keeps its three terms, or fp32, in mode 2)
ONE_TERM = re.compile(r"^(b4r_gemm_f32 \(|gemm_splitk \(|b4r_gemm_tn_f32( pair)? \(|b4r_attn_(fwd|bwd)( dq| dkv|_hd)?( \(|$| \[))")


@pytest.mark.parametrize("name", [n for n, c in CELLS.items() if "bf16" in c.modes])
def test_mode_two_plans_the_launches_of_mode_one_at_every_cell(name):
    c = CELLS[name]
    lib = _lib.load()
    prev = lib.b4r_get_gemm_mode()
    try:
        l1, l2 = step_labels(c, "bf16x3"), step_labels(c, "bf16")
    finally:
        lib.b4r_set_gemm_mode(prev)
    assert len(l1) > 10 and len(l1) == len(l2), (l1, l2)
    want = [one_term_label(l) if ONE_TERM.match(l) else l for l in l1]
    for j, (a, b) in enumerate(zip(want, l2)):
        assert a == b, f"launch {j}: mode 1 {l1[j]!r}, mode 2 {b!r} (expected {a!r})"
    # the three-term kernels of DESIGN.md §4.6 that the cell's forms run, by their (unchanged) labels
    f = c.split
    kept = {"b4r_attn_block_fwd": "Block" in f.attn_fwd, "b4r_ffn_block_fwd": "Block" in f.ffn,
            "attention core forward, queries = the head's slots": "SlotQuery" in f.attn_fwd,
            "wide feed-forward block forward": "Wide" in f.ffn, "masked-LM head forward (fused)": True, "embed_proj_fwd": f.emb_proj}
    for label, expected in kept.items():
        assert (label in l2) == expected, (label, l2)
    # the one-term ones run as such: a tagged core per dense attention layer, tagged tile products wherever products run
    cores = sum(1 for a in f.attn_fwd if a.startswith("Core"))
    assert sum(1 for l in l2 if re.match(r"^b4r_attn_fwd(_hd)? \(bf16\)", l)) == cores, l2
    assert not any("bf16x3" in l for l in l2), l2
    assert any(re.match(r"^b4r_gemm_(f32|tn_f32)( pair)? \(bf16", l) for l in l2) or set(f.ffn) == {"Block"}, l2


# ---- the evaluation forward -------------------------------------------------------------------------------------------------------------
EVAL_CASES = [pytest.param(name, mode, id=f"{name}-{mode}") for name in EVAL_CELLS for mode in MODES]


@pytest.mark.parametrize("name,matrix_mode", EVAL_CASES, indirect=["matrix_mode"])
def test_eval_forward_follows_the_restatement(name, matrix_mode):
    """the full eval forward's logits against the restatement (1e-3; mode 2: test_eval_logits_match_oracle_within_bf16_bounds's
    5e-2); in bf16x3 the encoder-only forward on the ranked rows (at hidden 256 with the Wide pair in its first layer) must give the
    full forward's rows there.  (In mode 2 the two forwards differ in term count: the Wide pair keeps three.)"""
    c = CELLS[name]
    cfg_o, eng, params = build_cell(c, od=0.0, ad=0.0)
    batch = cell_batch(c, seed=21)
    cb, _ = eng.prepare_batch(batch)
    B, L, P = cb.B, cb.L, cb.P
    eng.forward(cb, training=False, pooler=False)
    torch.cuda.synchronize()
    ref = ar.model_forward(params, batch, cfg_o, *c.acts)
    logits = eng.region("mlm_logits", B, L, P)[:, :VOCAB].cpu()
    err = maxdiff(logits, ref["mlm_logits"].reshape(logits.shape))
    print(f"{name} [{matrix_mode}]: eval logits max-abs {err:.2e}")
    assert err <= (5e-2 if matrix_mode == "bf16" else 1e-3)
    if matrix_mode != "bf16x3":
        return
    full = eng.region("sequence_output", B, L, P).clone()
    eng.region("sequence_output", B, L, P).fill_(float("nan"))
    labels = launch_labels(lambda: eng.forward(cb, training=False, pooler=False, head_rows_only=True, encoder_only=True))
    torch.cuda.synchronize()
    got = eng.region("sequence_output", B, L, P)
    valid = batch["masked_lm_ids"] != 0
    rows = (torch.arange(B)[:, None] * L + batch["masked_lm_positions"].clamp(0, L - 1))[valid].to(got.device)
    assert rows.numel() > 0
    d = maxdiff(got[rows], full[rows])
    print(f"{name}: encoder-only rows max-abs {d:.2e}; launches {labels}")
    assert d < 2e-5
    if c.H == 256:   # the one-launch feed-forward pair runs at hidden 256 in encoder-only forwards only
        assert "wide feed-forward block forward" in labels, labels


# ---- reproducibility and graph replay in mode 2 ----------------------------------------------------------------------------------------
def run_steps(c, n, graphed=False):
    cfg_o, eng, _ = build_cell(c)
    eng.set_seed(77)
    cb, _ = eng.prepare_batch(cell_batch(c))
    eng.ensure_training_buffers()
    hp = hip_adamw_config(orc.AdamWConfig(num_warmup_steps=0, num_train_steps=100))
    for _ in range(n):
        (eng.train_step_graphed if graphed else eng.train_step)(hp, cb)
    torch.cuda.synchronize()
    return eng.params.clone(), eng.read_state()["loss_sum"]


@pytest.mark.parametrize("matrix_mode", ["bf16"], indirect=True)
def test_mode_two_steps_of_the_factorised_model_are_reproducible_and_graphs_replay_them(matrix_mode):
    c = CELLS[REPRO_CELL]
    p1, l1 = run_steps(c, 4)
    p2, l2 = run_steps(c, 4)
    assert torch.equal(p1, p2) and l1 == l2
    pg, lg = run_steps(c, 4, graphed=True)
    assert torch.equal(p1, pg) and l1 == lg
