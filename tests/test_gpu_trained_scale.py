"""The model-level launch chains at weight scales a trained model reaches (tests/trained_scale.py: levels `moderate` and `sharp`,
six cells of tests/feature_matrix.py that between them take every launch form of a train step), against the restatement in
float64.  At the initialisers' scale -- where every other model-level test runs -- attention rows and the catalogue softmax are
uniform to a few percent; here the layer-0 scores have a standard deviation of 4.8 to 27 at `sharp`, some queries attend to a single
key, and the head sees a confident slot (top probability 0.39 to 0.95) next to a long-tail one (ground truth below 1e-6), on a batch
with a row of one token, a full row, a row whose later key tiles are wholly masked, a row that repeats one item on every second
token and a row without weighted slots.

Per cell, level and mode (bf16x3 everywhere, exact fp32 where the cell lists it):

a. the eval forward with the materialising head: sequence_output, mlm_hidden and logits on the weighted slots; the argmax of every
   such slot whose two best fp64 logits lie further apart than the logits bound (fewer than 5 % lie closer);
b. loss and every gradient tensor without dropout, in the train step's own flavour (logits-free head where the mode has it, the
   last layer on the head's rows; its launch labels must parse to the cell's record) and with the materialising head on all rows;
   the state's counts and accuracy sums;
c. the same in training mode with both dropouts at 0.2, the train step's flavour, mask for mask (forms asserted again);
d. at `sharp`, three cells: encoder_forward(ranked_rows_only=True) -> mlm_transform_rows -> rank_full, the top 10 and gt_rank of
   every weighted slot by inference_checks.check_top_k / check_gt_ranks with tol = the logits bound of the case.

Bounds: tests/trained_scale.py (forward and loss: 16 e32 exact fp32, min(512 e32, 1e-3 max(1, max |ref64|)) bf16x3; gradients per
tensor: max(16 e32g, 1e-5) exact fp32, min(max(512 e32g, 1e-5), G) bf16x3, G = 2e-3 without dropout, 5e-3 with).  The loss is one
fp32 number formed from the fp32 sum the state holds, so its e32 is never taken below one rounding of that sum, 2^-24 |loss| (the
fp32 restatement's own scalar can land nearer to fp64 than that by luck: 2.7e-8 at h128hd64_L200, training mode).  No tensor has
a rule of its own.  The key-bias gradients, analytically zero, miss the gradient bound in bf16x3: their rounding noise reaches
0.20 of compare_grads's floor at `sharp` (2e-5 of the model's largest gradient; up to 0.018 at `moderate`) against G = 2e-3 of
that floor.  Tests b and c print them and assert every other tensor; test_key_bias_gradients_in_bf16x3 asserts them, case by case
a strict expected failure with the measured figure (KEY_BIAS_MEASURED) and the cause.  The steps of one case are launched once
for the tests that judge them (measured_steps).  Where the two attention tile choices differ (b64_L64 in bf16x3: 16-token tiles by
default, 32-token tiles under b4r_attn32_set_min_len(1)) both run, each with its launch forms asserted.  Every figure is printed
("MEASURED ...") before it is asserted.

Measured on an MI355X at `sharp`, worst over the cells and flavours, error / bound (share of the bound): bf16x3 sequence_output
9.0e-4 / 5.5e-3, mlm_hidden 7.7e-4 / 6.5e-3, logits 2.4e-3 / 1.6e-2 (all h256_I512, 12 to 17 %), loss 3.6e-5 / 6.8e-4, item-table
gradient 5.2e-5 / 1.9e-4 (b64_L209, training mode, 28 %), position-table gradient 4.6e-4 / 2e-3, every other gradient tensor but
the key biases at most 29 % of its bound (embedding_projection/bias, h256_I512, 5.7e-4 / 2e-3); exact fp32 logits 2.2e-5 / 2.2e-4, gradients at most 21 %
of their bounds.  At `moderate` nothing passes 23 % of its bound.  No argmax differs; at most 2 of 109 slots lie within the logits
bound of a tie.  122 cases, 17 of them strict expected failures (key biases), about 6 s."""
import functools

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib
from tests import feature_matrix as fm
from tests import inference_checks as ic
from tests import test_gpu_feature_matrix as tfm
from tests import trained_scale as ts
from tests.test_gpu_feature_matrix import assert_forms, matrix_mode  # noqa: F401 (matrix_mode: a fixture)
from tests.test_gpu_model import run_loss_and_grads
from tests.test_gpu_train_step import assert_counts_match, launch_labels

pytestmark = pytest.mark.gpu

K = ic.TOP_K
TILES = ("tiles_by_length", "tiles32_always")


def tile_choices(name, mode):
    """The attention kernels on 32-token tiles (b4r_attn32.hip) serve hidden 64 with two heads in the split modes and are preferred
    from L = 65 on; b4r_attn32_set_min_len(1) prefers them at every length.  Both choices where they differ: b64_L64 in bf16x3,
    which then takes the launch forms of b64_L65 (FORMS_TILES32)."""
    c = fm.CELLS[name]
    return TILES if mode == "bf16x3" and (c.H, c.heads) == (64, 2) and c.L < 65 else TILES[:1]


def case_id(name, level, mode, tiles):
    return f"{name}-{level}-{mode}" + ("" if tiles == TILES[0] else f"-{tiles}")


FORMS_TILES32 = {"b64_L64": "b64_L65"}
CASES = [pytest.param(name, level, mode, tiles, id=case_id(name, level, mode, tiles))
         for name in ts.CELLS for level in ts.LEVELS for mode in ts.modes_of(name) for tiles in tile_choices(name, mode)]
# The key-bias gradients in bf16x3 (test_key_bias_gradients_in_bf16x3), measured on an MI355X relative to compare_grads's floor, the
# worse of the two layers and of the launch flavours: (cell, level, tile choice) -> (without dropout, bound 2e-3; training mode,
# bound 5e-3).  17 of the 28 cases miss their bound -- every `sharp` one without dropout -- and are strict expected failures.
# The bound these cases are marked against is 2e-3 / 5e-3 of a floor, the figures are rounding noise, and several lie within a few
# percent of it (b64_L64 moderate: 2.03e-3 on 16-token tiles, 1.9e-3 on 32-token tiles): another summation order can move such a case
# across its bound with no kernel being wrong -- update its figure here then.  A marked case has no bound that it meets, so
# test_key_bias_noise_stays_where_measured also holds every case below KEY_BIAS_CAP times its figure.
T16, T32 = TILES
KEY_BIAS_CAP = 4.0
KEY_BIAS_MEASURED = {
    ("h64_L200", "moderate", T16): (5.8e-4, 4.7e-4), ("h64_L200", "sharp", T16): (3.1e-3, 4.5e-3),
    ("b64_L64", "moderate", T16): (2.03e-3, 1.7e-3), ("b64_L64", "sharp", T16): (1.2e-2, 1.7e-2),
    ("b64_L64", "moderate", T32): (1.9e-3, 1.6e-3), ("b64_L64", "sharp", T32): (1.7e-2, 2.4e-2),
    ("b64_L209", "moderate", T16): (3.9e-4, 4.1e-4), ("b64_L209", "sharp", T16): (2.4e-3, 4.7e-3),
    ("h128_L200", "moderate", T16): (5.0e-3, 1.2e-2), ("h128_L200", "sharp", T16): (2.0e-1, 1.9e-1),
    ("h128hd64_L200", "moderate", T16): (5.6e-4, 8.0e-4), ("h128hd64_L200", "sharp", T16): (1.1e-2, 1.4e-2),
    ("h256_I512", "moderate", T16): (1.3e-2, 1.8e-2), ("h256_I512", "sharp", T16): (1.2e-1, 1.7e-1),
}


def key_bias_case(name, level, tiles, training):
    got, bound = KEY_BIAS_MEASURED[name, level, tiles][training], ts.GRAD_CONTRACT[training]
    marks = []
    if got > bound:
        marks = [pytest.mark.xfail(strict=True, reason=f"rounding noise of an analytically zero gradient: measured {got:.2e} of the "
                                                         f"floor, bound {bound:.0e}")]
    return pytest.param(name, level, "bf16x3", tiles, training, marks=marks,
                        id=case_id(name, level, "bf16x3", tiles) + ("-train" if training else "-eval"))


KEY_BIAS_CASES = [key_bias_case(name, level, tiles, training) for name in ts.CELLS for level in ts.LEVELS
                  for tiles in tile_choices(name, "bf16x3") for training in (False, True)]
EVAL_PATH_CASES = [pytest.param(name, mode, id=f"{name}-sharp-{mode}") for name in ts.EVAL_PATH_CELLS for mode in ts.modes_of(name)]


@pytest.fixture
def attention_tile_choice(request):
    lib = _lib.load()
    prev = lib.b4r_attn32_set_min_len(1 if request.param == "tiles32_always" else -1)
    yield request.param
    lib.b4r_attn32_set_min_len(prev)


def check_forms(labels, name, mode, tiles, rows_only, fused_head):
    """The launch forms of one forward / loss / backward.  The train step's own flavour (last layer on the head's rows) must parse to
    the cell's record -- under the forced 32-token tiles to the record of the cell FORMS_TILES32 names.  The matrix keeps no record
    of the all-rows flavour and its parser reads a train step's launches: there the head's launch is what tells the flavour."""
    c = fm.CELLS[name]
    assert ("masked-LM head forward (fused)" in labels) == fused_head, labels
    if not rows_only:
        return
    if tiles == TILES[0]:
        assert_forms(labels, c, mode, ts.BATCH)
        return
    got = tfm.parse_forms(labels, c, ts.BATCH)
    print(f"forms [{mode}, {tiles}]: {got}")
    like = fm.CELLS[FORMS_TILES32[name]]
    assert (like.H, like.heads, like.inner, like.E) == (c.H, c.heads, c.inner, c.E)
    assert got == like.forms(mode), (got, labels)


def build(name, level, training=False):
    """the cell's engine (its own build_cell) holding the level's weights"""
    rate = ts.TRAIN_RATE if training else 0.0
    _, eng, _ = tfm.build_cell(fm.CELLS[name], od=rate, ad=rate)
    eng.load_named(ts.cell_weights(name, level))
    return eng


def forward_bounds(name, level, mode, training=False):
    """bound, e32 and contract of the forward quantities and the loss"""
    batch = ts.cell_batch(name)
    r64 = ts.reference(name, level, torch.float64, training)
    e32, _ = ts.fp32_errors(name, level, training)
    e32 = dict(e32, loss=max(e32["loss"], 2.0 ** -24 * abs(float(r64["loss"]))))
    contract = {q: ts.contract_of(batch, q, r64[q]) for q in e32}
    return {q: ts.forward_bound(mode, e32[q], contract[q]) for q in e32}, e32, contract


def check_forward(tag, name, level, mode, got, training=False):
    """got: quantity -> device tensor ([rows, .], the reference's layout; the loss a 1-element tensor)"""
    batch = ts.cell_batch(name)
    r64 = ts.reference(name, level, torch.float64, training)
    bounds, e32, contract = forward_bounds(name, level, mode, training)
    failed = []
    for q, t in got.items():
        err = ts.forward_error(batch, q, t, r64[q])
        print(f"MEASURED {name} [{level}, {mode}] {tag} {q}: err {err:.3e} e32 {e32[q]:.3e} contract {contract[q]:.3e} "
              f"bound {bounds[q]:.3e}")
        if not err <= bounds[q]:
            failed.append(f"{q}: {err:.3e} > {bounds[q]:.3e}")
    assert not failed, f"{name} [{level}, {mode}] {tag}: " + "; ".join(failed)
    return bounds


def is_key_bias_finding(n, mode):
    """the tensors test_key_bias_gradients_in_bf16x3 judges on their own (same bound)"""
    return mode == "bf16x3" and n.endswith("key/bias")


def check_grads(tag, name, level, mode, errs, training, judged):
    """errs: tensor -> relative error (trained_scale.grad_errors); every tensor is printed, those `judged` picks are asserted"""
    _, e32g = ts.fp32_errors(name, level, training)
    failed = []
    for n, err in errs.items():
        bound = ts.grad_bound(mode, e32g[n], training)
        print(f"MEASURED {name} [{level}, {mode}] {tag} d {n}: rel err {err:.3e} e32g {e32g[n]:.3e} bound {bound:.3e}")
        if judged(n) and not err <= bound:
            failed.append(f"{n}: {err:.3e} > {bound:.3e}")
    assert not failed, f"{name} [{level}, {mode}] {tag}: " + "; ".join(failed)


def check_step(tag, name, level, mode, st, errs, training=False):
    """loss, counts, accuracy sums and every gradient tensor of one forward / loss / backward against fp64"""
    c = fm.CELLS[name]
    batch = ts.cell_batch(name)
    r64 = ts.reference(name, level, torch.float64, training)
    cnt = st["valid_count"]
    bounds = check_forward(tag, name, level, mode, {"loss": torch.tensor([st["loss_sum"] / cnt], dtype=torch.float64)}, training)
    logit_bound = bounds["logits"]
    _, tie = ts.tie_slots(batch, r64["logits"], logit_bound)
    assert float(tie.double().mean()) < ts.TIE_CAP, (int(tie.sum()), tie.numel())
    assert_counts_match(st, batch, r64["logits"].reshape(ts.BATCH, c.P, -1), tie_width=logit_bound)
    check_grads(tag, name, level, mode, errs, training, lambda n: not is_key_bias_finding(n, mode))


@functools.lru_cache(maxsize=None)
def measured_steps(name, level, mode, tiles, training):
    """One case's forward / loss / backward launches, run once for the tests that judge them (under the case's matrix_mode):
    [(tag, state, relative error per gradient tensor)].  First the train step's own flavour -- the logits-free head where the mode has
    it, the last layer on the head's rows; without dropout then the materialising head on all rows; the launch forms of each are
    asserted (check_forms).  What is kept are host numbers, so a later test's global state cannot reach them; the global state at
    the time of the launches is asserted here."""
    lib = _lib.load()
    assert lib.b4r_get_gemm_mode() == tfm.MODE_OF[mode] and lib.b4r_attn32_set_min_len(-1) == (65 if tiles == TILES[0] else 1)
    batch = ts.cell_batch(name)
    r64 = ts.reference(name, level, torch.float64, training)
    eng = build(name, level, training)
    fused = eng.fused_head_supported()
    assert fused == (mode == "bf16x3")
    flavours = [("training mode" if training else "train-step flavour", fused, True)]
    if not training:
        flavours.append(("materialising head, all rows", False, False))
    out = []
    for tag, fused_head, rows_only in flavours:
        got = []
        labels = launch_labels(lambda: got.append(run_loss_and_grads(eng, batch, training, seed=ts.TRAIN_SEED, step=ts.TRAIN_STEP,
                                                                     fused_head=fused_head, head_rows_only=rows_only)))
        st, grads = got[0]
        check_forms(labels, name, mode, tiles, rows_only, fused_head)
        out.append((tag, st, ts.grad_errors(grads, r64["grads"], st["valid_count"])))
    return out


# ---- a. the eval forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,level,matrix_mode,attention_tile_choice", CASES, indirect=["matrix_mode", "attention_tile_choice"])
def test_eval_forward_follows_fp64(name, level, matrix_mode, attention_tile_choice):
    mode = matrix_mode
    batch = ts.cell_batch(name)
    eng = build(name, level)
    cb, keep = eng.prepare_batch(batch)
    B, L, P = cb.B, cb.L, cb.P
    eng.forward(cb, training=False, pooler=False)
    torch.cuda.synchronize()
    got = {"sequence_output": eng.region("sequence_output", B, L, P), "mlm_hidden": eng.region("mlm_hidden", B, L, P),
           "logits": eng.region("mlm_logits", B, L, P)[:, :fm.VOCAB]}
    bounds = check_forward("eval forward", name, level, mode, got)
    best, tie = ts.tie_slots(batch, ts.reference(name, level)["logits"], bounds["logits"])
    pred = ts.on_slots(batch, "logits", got["logits"]).argmax(dim=-1).cpu()
    print(f"MEASURED {name} [{level}, {mode}] eval forward argmax: {int((pred != best).sum())} of {best.numel()} slots differ, "
          f"{int(tie.sum())} within the bound of a tie")
    assert float(tie.double().mean()) < ts.TIE_CAP
    assert bool((pred == best)[~tie].all())


# ---- b. loss and gradients without dropout, both launch flavours ---------------------------------------------------------------------
@pytest.mark.parametrize("name,level,matrix_mode,attention_tile_choice", CASES, indirect=["matrix_mode", "attention_tile_choice"])
def test_loss_and_gradients_follow_fp64_in_both_launch_flavours(name, level, matrix_mode, attention_tile_choice):
    for tag, st, errs in measured_steps(name, level, matrix_mode, attention_tile_choice, False):
        check_step(tag, name, level, matrix_mode, st, errs)


# ---- c. training mode, mask for mask ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,level,matrix_mode,attention_tile_choice", CASES, indirect=["matrix_mode", "attention_tile_choice"])
def test_training_mode_follows_fp64_mask_for_mask(name, level, matrix_mode, attention_tile_choice):
    for tag, st, errs in measured_steps(name, level, matrix_mode, attention_tile_choice, True):
        check_step(tag, name, level, matrix_mode, st, errs, training=True)


# ---- the key-bias gradients in bf16x3: a finding -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,level,matrix_mode,attention_tile_choice,training", KEY_BIAS_CASES,
                         indirect=["matrix_mode", "attention_tile_choice"])
def test_key_bias_gradients_in_bf16x3(name, level, matrix_mode, attention_tile_choice, training):
    """The gradient of a key bias is analytically zero -- a softmax does not see a shift of its scores -- so what a kernel returns
    for it is the rounding of d bk = sum over (query, key) of dS Q~ with dS = P (dP - delta), whose rows cancel to zero only in
    exact arithmetic (then dK = dS^T Q~ and its sum over the tokens).  Every attention backward states it alike.  The worst figures
    (layer 0 of h128_L200, 0.20, and of h256_I512, 0.17; also b64_L209) come from attn32_core_bwd_kernel, b4r_attn32.hip:
    a32_bwd_dense_sweep -> a32_bwd_vector, `ds[j] = pr * (dA[tt] - Dq[tt])` (with dropout `pr * fmaf(dA[tt], kf, -Dq[tt])`); the
    folded and forced-tile blocks of hidden 64 run the same a32_bwd_vector; h128hd64_L200 runs b4r_attn64.hip
    `ds[u][r] = pr * (dA - Dq)`, b64_L64 by default b4r_attn_block.hip `ds[r] = pr * (da_ - Dq)`.  dA and Dq arrive from three-term bf16 products (2^-17 relative); near a one-hot row they are large and nearly equal,
    and |Q~| is several units, so the noise grows with the level.  Same bound as every tensor, min(max(512 e32g, 1e-5), G) of
    compare_grads's floor; the flavours of tests b and c (their launches are reused).  Missed at 17 of 28 cases, by up to 100 x
    (h128_L200 at `sharp`: 0.20 of the floor): the figures are in KEY_BIAS_MEASURED, and each such case is a strict expected failure.
    A finding about the bound, not a kernel defect: 1.0 of the floor is 1e-4 of the model's largest gradient."""
    mode = matrix_mode
    for tag, _, errs in measured_steps(name, level, mode, attention_tile_choice, training):
        check_grads(tag, name, level, mode, errs, training, lambda n: is_key_bias_finding(n, mode))


@pytest.mark.parametrize("name,level,matrix_mode,attention_tile_choice,training",
                         [pytest.param(*p.values, id=p.id) for p in KEY_BIAS_CASES], indirect=["matrix_mode", "attention_tile_choice"])
def test_key_bias_noise_stays_where_measured(name, level, matrix_mode, attention_tile_choice, training):
    """every case of the test above, marked or not, within KEY_BIAS_CAP times the figure recorded for it: a marked case meets no
    bound, and noise that grew would otherwise go unseen there"""
    recorded = KEY_BIAS_MEASURED[name, level, attention_tile_choice][training]
    worst = max(err for _, _, errs in measured_steps(name, level, matrix_mode, attention_tile_choice, training)
                for n, err in errs.items() if is_key_bias_finding(n, matrix_mode))
    print(f"MEASURED {name} [{level}, {matrix_mode}, {attention_tile_choice}] training {training} key biases: worst rel err {worst:.3e}, "
          f"recorded {recorded:.2e}")
    assert worst <= KEY_BIAS_CAP * recorded


# ---- d. the evaluation path -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,matrix_mode", EVAL_PATH_CASES, indirect=["matrix_mode"])
def test_evaluation_path_ranks_as_fp64_does(name, matrix_mode):
    mode, level = matrix_mode, "sharp"
    batch = ts.cell_batch(name)
    rk = ic.ranked_slots(batch)
    r64 = ts.reference(name, level)
    bounds, e32, _ = forward_bounds(name, level, mode)
    eng = build(name, level)
    cb, keep = eng.prepare_batch(batch)
    eng.encoder_forward(cb, ranked_rows_only=True)
    seq = eng.region("sequence_output", cb.B, cb.L, cb.P, encoder_only=True)
    hidden = eng.mlm_transform_rows(seq, rk.rows)
    ids, scores, gt_rank = eng.rank_full(hidden, None, None, ic.FIRST_ITEM, rk.gt, K)
    torch.cuda.synchronize()
    s64 = ts.on_slots(batch, "logits", r64["logits"]).numpy()
    err_h = float((hidden.cpu().double() - ts.on_slots(batch, "mlm_hidden", r64["mlm_hidden"])).abs().max())
    ids_h, sc_h = ids.cpu().numpy(), scores.cpu().numpy().astype(np.float64)
    err_s = float(np.abs(sc_h - np.take_along_axis(s64, ids_h, 1)).max())
    print(f"MEASURED {name} [{level}, {mode}] evaluation path mlm_hidden: err {err_h:.3e} bound {bounds['mlm_hidden']:.3e}; "
          f"scores: err {err_s:.3e} e32 {e32['logits']:.3e} bound {bounds['logits']:.3e}")
    assert err_h <= bounds["mlm_hidden"] and err_s <= bounds["logits"]
    gt = rk.gt.numpy()
    ok = ic.allowed(fm.VOCAB, np.empty((len(gt), 0), np.int64), gt)
    ic.check_top_k(ids_h, s64, ok, K, bounds["logits"], f"{name} [{mode}] rank_full")
    ic.check_gt_ranks(gt_rank.cpu().numpy(), s64, gt, bounds["logits"], ok, f"{name} [{mode}] rank_full")
    lo_hi = [ic.rank_interval(s64[r], int(gt[r]), bounds["logits"], ok[r]) for r in range(len(gt))]
    print(f"MEASURED {name} [{level}, {mode}] evaluation path: {len(gt)} slots, gt ranks {min(l for l, _ in lo_hi)} .. "
          f"{max(h for _, h in lo_hi)}, {sum(1 for l, h in lo_hi if l != h)} rank intervals wider than one rank")
