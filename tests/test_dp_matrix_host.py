"""The cases of the data-parallel step's tests (tests/dp_matrix.py) cover what they claim to, and the joined reference they are held
to is the restatement's step on the joined batch.  Runs without a GPU, so the lists cannot silently shrink."""
import functools

import pytest
import torch

from oracle import bert4rec_oracle as orc
from tests import activation_ref as ar
from tests import dp_matrix as dm
from tests import feature_matrix as fm
from tests import geometry_matrix as gm
from tests.test_gpu_model import compare_grads


def all_cells():
    return [c for cells in dm.MATRICES.values() for c in cells.values()]


def test_joined_cases_reach_every_form_and_both_head_variants():
    for field in ("attn_fwd", "attn_bwd", "ffn"):
        everywhere = {v for c in all_cells() for mode in c.modes for v in getattr(c.forms(mode), field)}
        joined = {v for matrix, name, mode in dm.JOINED_CASES for v in getattr(dm.cell_of(matrix, name).forms(mode), field)}
        assert joined == everywhere, (field, sorted(everywhere - joined))
    for flag in ("emb_proj", "emb_fused"):
        assert {getattr(dm.cell_of(m, n).forms(mode), flag) for m, n, mode in dm.JOINED_CASES} == {False, True}, flag
    assert {dm.head_is_fused(dm.cell_of(m, n), mode) for m, n, mode in dm.JOINED_CASES} == {False, True}
    # every name resolves in its matrix, in a mode the cell runs in; the graph cells likewise
    for matrix, name, mode in dm.JOINED_CASES + dm.DP_GRAPH_CELLS:
        assert name in dm.MATRICES[matrix] and mode in dm.cell_of(matrix, name).modes, (matrix, name, mode)
    assert len(set(dm.JOINED_CASES)) == len(dm.JOINED_CASES) and len(set(dm.DP_GRAPH_CELLS)) == len(dm.DP_GRAPH_CELLS)
    assert set(dm.DP_GRAPH_CELLS) == {c for c in dm.JOINED_CASES if c[2] == "bf16x3"} | {("feature", "h64_L200", "f32")}
    assert {mode for _, _, mode in dm.JOINED_CASES} == set(fm.MODES)


def test_every_cell_of_both_matrices_is_a_step_case_in_every_mode():
    want = [("feature", name, mode) for name, c in fm.CELLS.items() for mode in c.modes] + \
           [("geometry", name, mode) for name, c in gm.CELLS.items() for mode in c.modes]
    assert sorted(dm.STEP_CASES) == sorted(want) and len(set(dm.STEP_CASES)) == len(want)
    assert len(want) == sum(len(c.modes) for c in fm.CELLS.values()) + sum(len(c.modes) for c in gm.CELLS.values())
    assert len({dm.case_id(case) for case in dm.STEP_CASES}) == len(want)
    assert not set(fm.CELLS) & set(gm.CELLS)


def test_joined_reference_is_the_restatement_on_the_concatenated_batch_without_dropout():
    """two ragged shards with unequal valid counts, dropout 0 (so that the rows of a rank need no rank-local dropout indices): the
    count-weighted join of the per-shard losses and gradients is the loss and the gradient of the concatenation.  Measured with
    orc.loss_and_grads at hidden 64, two layers: loss 1.3e-7, worst tensor 7.0e-7 under compare_grads' rule (the two key biases, whose
    gradient is analytically zero, are measured against its floor); bounds 1e-6 and 1e-5."""
    cfg_o = orc.OracleConfig(vocab_size=203, hidden_size=64, num_layers=2, num_attention_heads=2, max_sequence_length=48, inner_dim=256,
                             output_dropout=0.0, attention_dropout=0.0)
    params = orc.init_params(cfg_o, seed=3)
    shards = [orc.synthetic_batch(5, 48, 10, 203, seed=31, ragged=True), orc.synthetic_batch(5, 48, 10, 203, seed=32, ragged=True)]
    shards[1]["masked_lm_ids"][3:] = 0   # the second rank holds fewer labelled slots
    counts = [float((s["masked_lm_ids"] != 0).sum()) for s in shards]
    assert counts[0] > counts[1] > 0
    loss, grads, per_shard, got_counts = dm.joined_reference(orc.loss_and_grads, params, shards, cfg_o, [(7, 0), (8, 0)])
    assert got_counts == counts and len(per_shard) == 2
    whole = {k: torch.cat([shards[0][k], shards[1][k]]) for k in shards[0]}
    loss_w, grads_w, _ = orc.loss_and_grads(params, whole, cfg_o, training=True, rng=(7, 0))
    print(f"MEASURED joined reference: loss {abs(loss - float(loss_w)):.2e}")
    assert abs(loss - float(loss_w)) <= 1e-6
    worst = compare_grads(grads, grads_w, 1.0, rel=1e-5)
    print(f"MEASURED joined reference: worst tensor {worst[1]:.2e} ({worst[0]})")
    assert set(grads) == set(grads_w)


@pytest.mark.parametrize("inner", sorted(dm.KINKS))
def test_a_step_on_the_other_side_of_an_activations_jump_is_found_and_a_wrong_gradient_is_not(inner):
    """reference_at_kink_ties: a unit's bias is set so that one pre-activation of layer 0 lies 2e-7 above 0 (within the rounding error
    of the product, kink_tolerance); the "device" is the restatement with that bias 4e-7 lower, i.e. the same step from the other side
    of the jump.  The restatement as it stands misses it, the search finds exactly that element, and the restatement it returns agrees
    to 1e-5; a gradient that is wrong by 1 % in one tensor is not explained by any tie."""
    c = fm.Cell(64, 2, 256, 40, 8, None, (inner, "relu"), ("f32",), None, None)
    cfg_o = orc.OracleConfig(vocab_size=203, hidden_size=64, num_layers=2, num_attention_heads=2, max_sequence_length=40, inner_dim=256,
                             output_dropout=0.1, attention_dropout=0.1)
    params = orc.init_params(cfg_o, seed=3)
    batch = orc.synthetic_batch(4, 40, 8, 203, seed=5, ragged=True)
    ref = functools.partial(ar.loss_and_grads, inner=c.acts[0], mlm=c.acts[1])
    roles = dm.kink_roles(c, cfg_o)
    assert roles == [("inner", 0), ("inner", 1), ("mlm",)]
    own = dict(ar.ACT)
    bias = "transformer/layer_0/intermediate/bias"
    with dm.kink_sides() as calls:
        ref(params, batch, cfg_o, training=True, rng=(9, 0))
    assert len(calls) == 3 and calls[0].shape == (4, 40, 256)
    row, unit = 7, 31   # a row inside the first sequence (a ragged sequence holds at least 5 tokens)
    params[bias][unit] -= calls[0].reshape(-1, 256)[row, unit] - 2e-7
    with dm.kink_sides() as calls:
        loss, grads, _ = ref(params, batch, cfg_o, training=True, rng=(9, 0))
    pre = float(calls[0].reshape(-1, 256)[row, unit])
    assert 1e-7 < pre < 3e-7 and pre < float(dm.kink_tolerance(roles[0], params, cfg_o)[unit]), pre
    ties = dm.kink_ties(calls, roles, params, cfg_o)
    assert ties and ties[0][:2] == (0, row * 256 + unit), ties
    below = {n: p.clone() for n, p in params.items()}
    below[bias][unit] -= 4e-7
    _, device, _ = ref(below, batch, cfg_o, training=True, rng=(9, 0))

    def check(reference):
        compare_grads(device, reference[1], 1.0, rel=1e-5)

    with pytest.raises(AssertionError):
        check((loss, grads, None))

    def measure_against(got):
        floor = 1e-4 * max(float(g.abs().max()) for g in got.values())
        return lambda r: max(float((got[n] - g).abs().max()) / max(float(g.abs().max()), floor) for n, g in r[1].items())

    found = dm.reference_at_kink_ties(c, ref, params, batch, cfg_o, (9, 0), check, measure_against(device))
    check(found)
    assert ar.ACT == own   # the activations are the restatement's own again
    again = ref(params, batch, cfg_o, training=True, rng=(9, 0))
    assert all(torch.equal(again[1][n], grads[n]) for n in grads)
    wrong = {n: g.clone() for n, g in device.items()}
    wrong["transformer/layer_1/output/kernel"] *= 1.01
    with pytest.raises(AssertionError, match="gradient of"):
        dm.reference_at_kink_ties(c, ref, params, batch, cfg_o, (9, 0), lambda r: compare_grads(wrong, r[1], 1.0, rel=1e-5),
                                  measure_against(wrong))


def test_head_is_fused_against_the_list_of_unfused_cases():
    """the materialising head: every exact-fp32 case, and in the split modes the cells whose item table is 32, 512 or 1024 wide"""
    wide_or_narrow = {"h32", "h32_I104", "h32_I100", "h512hd32", "h1024hd32"}
    assert wide_or_narrow <= set(gm.CELLS)
    unfused = {case for case in dm.STEP_CASES if case[2] == "f32"} | \
              {case for case in dm.STEP_CASES if case[0] == "geometry" and case[1] in wide_or_narrow}
    got = {case for case in dm.STEP_CASES if not dm.head_is_fused(dm.cell_of(case[0], case[1]), case[2])}
    assert got == unfused, (sorted(got - unfused), sorted(unfused - got))
    assert {(dm.cell_of(m, n).E or dm.cell_of(m, n).H) for m, n, _ in dm.STEP_CASES} == {32, 64, 128, 256, 512, 1024}
