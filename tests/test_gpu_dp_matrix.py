"""The data-parallel train step (Engine.dp_train_step, dp_train_step_graphed, dp_idle_step) at the cells of tests/feature_matrix.py and
tests/geometry_matrix.py -- what BERT4RecModel.fit runs under a process group and bench.py --gpus N times.  It is not b4r_train_step:
it is a composition of public calls, each of which plans for itself, with the all-reduce between the backward and the optimizer.
Everything here runs in one process (cases: tests/dp_matrix.py): without a process group allreduce_step returns at once, and where
ranks are needed the collective is played on the current stream.

What the composition launches (b4r_model.hip: forward_impl / head_fwd, b4r_loss, head_bwd; b4r_rowops.hip: b4r_zero2,
b4r_optimizer_fused), stated here and asserted from the launch labels:

* the logits-free head (item-table width 64 / 128 / 256 in a split mode, tests/dp_matrix.py::head_is_fused; the engine must agree,
  Engine.fused_head_supported): forward ends with "masked-LM head forward (fused)" and "masked-LM head combine" -- the public forward
  never defers the merge, at hidden 64 neither --, the backward opens with "zero fill + loss sums" (the last workgroup of the clearing
  launch forms the loss sums and copies them into the tail); no b4r_state_begin_step, no b4r_loss launch;
* the materialising head (exact fp32, or width 32 / 512 / 1024): "b4r_state_begin_step" first, no head launches of the fused kind,
  b4r_loss's "b4r_softmax_ce" and "b4r_softmax_ce finalize" between the forward and the backward, which opens with "zero fill" (its
  first workgroup copies the sums b4r_loss left into the tail);
* both: b4r_optimizer_step_reduced closes the step with one "global norm" launch (its first workgroup moves the tail into the
  state) and one "optimizer step" launch -- never the norm partials of the closing reduce launch, those belong to b4r_train_step.

(a) the step alone at every cell and mode: the train-step checkers of the two matrices with the data-parallel step in place of
    Engine.train_step (same bounds, mask for mask with dropout on), the forms the cell records for the train step, the launches above,
    the tail after the backward and after the step, and a rerun on a fresh engine over a workspace filled with NaN;
(b) dp_train_step_graphed against eager steps, bit for bit, at DP_GRAPH_CELLS;
(c) two working ranks and an idle one at JOINED_CASES: the rank that receives both contributions holds the restatement's step on the
    joined batch (tests/dp_matrix.py::joined_reference) within the bounds a single step has at that cell, the idle rank equals it bit
    for bit, over two rounds.  Each rank's contribution is held to the restatement of its shard first; where relu or selu leaves the
    restatement's side of the derivative's jump open (tests/dp_matrix.py::reference_at_kink_ties: a pre-activation within its own
    rounding error of 0), the comparison is repeated, unchanged, from the other side, and the joined reference is formed from the
    restatements the contributions met.

Measured worst figures per mode: DESIGN.md section 8.

The restatement of a cell's first step (CPU, the same in every mode) is computed once and shared by the modes of (a) and by (c)."""
import pytest
import torch
import torch.distributed as dist

from bert4rec_amd import _lib
from bert4rec_amd import distributed as b4r_dist
from bert4rec_amd.engine import Engine
from oracle import bert4rec_oracle as orc
from tests import dp_matrix as dm
from tests import test_gpu_feature_matrix as fmx
from tests import test_gpu_geometry as geo
from tests.test_gpu_feature_matrix import (BF16_BOUNDS, BF16_CELL_BOUNDS, BF16_TIE, SEED, bf16_gradient_errors, check_bf16_step,  # noqa: F401
                                           matrix_mode, parse_forms)   # (matrix_mode: a fixture)
from tests.test_gpu_model import LOGIT_TOL, compare_grads
from tests.test_gpu_train_step import (TIE, assert_adamw_exact, assert_counts_match, hip_adamw_config, launch_labels,
                                       run_and_check_train_step)

pytestmark = pytest.mark.gpu

HP_O = orc.AdamWConfig(num_warmup_steps=0, num_train_steps=100, gradient_clip_norm=5.0)   # the two matrices' own
REL = 5e-3
HEAD_FWD, COMBINE = "masked-LM head forward (fused)", "masked-LM head combine"
BEGIN, LOSS_LAUNCHES = "b4r_state_begin_step", ["b4r_softmax_ce", "b4r_softmax_ce finalize"]
SUMS = slice(_lib.ST_LOSS_SUM, _lib.ST_SLOTS_ALL + 1)      # the five sums of the state, in the tail's order
SHARED = slice(_lib.ST_STEP_LO, _lib.ST_LR + 1)            # step, the sums, the norm and the learning rate: all but the seed
TAIL = b4r_dist.TAIL


def side(matrix):
    return fmx if matrix == "feature" else geo


def label_cap(matrix, c):
    return 256 if matrix == "feature" else geo.label_cap(c)


def params_of(cases):
    return [pytest.param(case, case[2], id=dm.case_id(case)) for case in cases]


# ---- the restatement of a cell's first step, shared ------------------------------------------------------------------------------
_KEPT = {(matrix, name) for matrix, name, _ in dm.JOINED_CASES}   # the cells part (c) meets again
_REFS = {}


def shared_ref(matrix, name, c):
    """the cell's restatement as the checkers call it, answering from a cache keyed by the cell: the CPU restatement dominates a case and
    is the same in every mode.  A cell of JOINED_CASES stays cached for part (c), any other until the next cell is computed.  An entry
    answers only the question it was computed for (parameters, batch and dropout stream fingerprinted), and holds of the outputs the
    logits alone."""
    base = fmx.cell_ref(c)

    def ref(params, batch, cfg_o, training, rng):
        mark = (tuple(float(p.double().sum()) for p in params.values()), int(batch["input_word_ids"].sum()),
                int(batch["masked_lm_positions"].sum()), tuple(rng), training)
        hit = _REFS.get((matrix, name))
        if hit is None or hit[0] != mark:
            loss, grads, out = base(params, batch, cfg_o, training=training, rng=rng)
            for k in [k for k in _REFS if k not in _KEPT]:
                del _REFS[k]
            hit = _REFS[(matrix, name)] = (mark, (loss, grads, {"mlm_logits": out["mlm_logits"]}))
        return hit[1]
    return ref


# ---- the launches of the composition ------------------------------------------------------------------------------------------------
def assert_head_and_optimizer_launches(labels, fused):
    """the module docstring's list, from the labels of one data-parallel step"""
    opening = [j for j, l in enumerate(labels) if l.startswith("zero fill")]
    assert len(opening) == 1, labels
    z = opening[0]
    assert labels[z] == ("zero fill + loss sums" if fused else "zero fill"), labels[z]
    assert labels[-2:] == ["global norm", "optimizer step"], labels[-4:]
    assert labels.count("global norm") == 1 and labels.count("optimizer step") == 1, labels
    if fused:
        assert labels[z - 2:z] == [HEAD_FWD, COMBINE], labels[:z]
        assert labels.count(HEAD_FWD) == 1 and labels.count(COMBINE) == 1, labels
        assert not any(l in (BEGIN, "b4r_loss finalize", *LOSS_LAUNCHES) for l in labels), labels
    else:
        assert HEAD_FWD not in labels and COMBINE not in labels, labels
        assert labels[0] == BEGIN and labels.count(BEGIN) == 1, labels
        assert labels[z - 2:z] == LOSS_LAUNCHES, labels[:z]
        assert all(labels.count(l) == 1 for l in LOSS_LAUNCHES), labels


class CollectiveSpy:
    """allreduce_step observed, not replaced: it keeps what the gradient tail and the state held when the step reached its collective
    (after the backward, before the optimizer) and hands the call on"""

    def __init__(self, real):
        self.real, self.calls, self.eng, self.tail, self.state = real, 0, None, None, None

    def __call__(self, grad_ext, group=None, single_rank_too=False):
        self.calls += 1
        assert grad_ext is self.eng.grad_ext and grad_ext.numel() == self.eng.n_params + TAIL
        self.tail, self.state = grad_ext[self.eng.n_params:].clone(), self.eng.state.clone()
        return self.real(grad_ext, group, single_rank_too)


def assert_tail_is_the_state_sums(tail, state, when):
    """bit for bit [loss_sum, valid_count, correct_masked, correct_all, slots_all, 0, 0, 0]"""
    tail, state = tail.cpu(), state.cpu()
    assert tail.numel() == TAIL
    assert torch.equal(tail.view(torch.int32)[:5], state[SUMS]), (when, tail.tolist(), state[SUMS].view(torch.float32).tolist())
    assert not bool(tail.view(torch.int32)[5:].any()), (when, tail.tolist())


# ---- (a) the step alone, at every cell and mode ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,matrix_mode", params_of(dm.STEP_CASES), indirect=["matrix_mode"])
def test_dp_step_of_every_cell_follows_the_restatement_in_the_forms_of_the_train_step(case, matrix_mode, monkeypatch):
    matrix, name, mode = case
    c = dm.cell_of(matrix, name)
    B = dm.batch_size(matrix, c)
    assert not (dist.is_available() and dist.is_initialized()), "this test runs the step's local composition: no process group"
    cfg_o, eng, _ = side(matrix).build_cell(c)
    batch = side(matrix).cell_batch(c)
    eng.set_seed(SEED)
    cb, _keep = eng.prepare_batch(batch)
    spy = CollectiveSpy(b4r_dist.allreduce_step)
    spy.eng = eng
    monkeypatch.setattr(b4r_dist, "allreduce_step", spy)
    step_fn = lambda hp, cb: eng.dp_train_step(hp, cb)   # noqa: E731

    # the restatement, mask for mask, within the bounds of the train step at this cell
    labels = []
    ref = shared_ref(matrix, name, c)
    if mode == "bf16":
        check_bf16_step(eng, cfg_o, batch, cb, HP_O, c, labels, name, step_fn=step_fn, ref=ref)
    else:
        run_and_check_train_step(eng, cfg_o, batch, cb, HP_O, 0, SEED, rel=REL, labels=labels, ref=ref, label_cap=label_cap(matrix, c),
                                 step_fn=step_fn)
    torch.cuda.synchronize()

    # the forms the cell records for Engine.train_step: the forward's plan and the backward's are that one plan
    got, want = parse_forms(labels, c, B), c.forms(mode)
    print(f"forms [{mode}]: {got}")
    assert got == want, f"forms of the {mode} data-parallel step: {got}, expected {want}\n{labels}"

    # the head's and the optimizer's launches
    fused = dm.head_is_fused(c, mode)
    assert eng.fused_head_supported() == fused
    assert_head_and_optimizer_launches(labels, fused)

    # the tail, after the backward and after the whole step
    assert spy.calls == 1
    tail = eng.grad_ext[eng.n_params:].clone()
    assert_tail_is_the_state_sums(spy.tail, spy.state, "after the backward")
    assert_tail_is_the_state_sums(tail, eng.state, "after the step")
    assert torch.equal(tail.view(torch.int32), spy.tail.view(torch.int32))
    assert eng.read_state()["slots_all"] == float(B * c.P)

    # no stale reads: a fresh engine over a workspace full of NaN takes the same step, bit for bit
    _, again, _ = side(matrix).build_cell(c)
    again.set_seed(SEED)
    cb2, _keep2 = again.prepare_batch(batch)
    again.ensure_training_buffers()
    again.workspace(B, c.L, c.P).fill_(float("nan"))
    spy.eng = again
    again.dp_train_step(hip_adamw_config(HP_O), cb2)
    torch.cuda.synchronize()
    assert spy.calls == 2
    for what, a, b in (("parameters", again.params, eng.params), ("adam_m", again.adam_m, eng.adam_m), ("adam_v", again.adam_v, eng.adam_v)):
        assert bool(torch.isfinite(a).all()), f"{what} after a step over a NaN-filled workspace"
        assert torch.equal(a, b), f"{what} after a step over a NaN-filled workspace"
    assert torch.equal(again.state[SHARED], eng.state[SHARED]), (again.read_state(), eng.read_state())


# ---- (b) the graph-replayed step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,matrix_mode", params_of(dm.DP_GRAPH_CELLS), indirect=["matrix_mode"])
def test_graphed_dp_steps_equal_eager_dp_steps_bit_for_bit(case, matrix_mode):
    """four steps on one batch: the first eager, the second captured (the two halves around the all-reduce, one graph each), the third
    and fourth replayed -- against four eager steps of a twin engine"""
    matrix, name, mode = case
    c = dm.cell_of(matrix, name)
    batch = side(matrix).cell_batch(c)
    hp = hip_adamw_config(HP_O)
    runs = []
    for graphed in (False, True):
        _, eng, _ = side(matrix).build_cell(c)
        eng.set_seed(SEED)
        cb, _keep = eng.prepare_batch(batch)
        states = []
        for _ in range(4):
            (eng.dp_train_step_graphed if graphed else eng.dp_train_step)(hp, cb)
            torch.cuda.synchronize()
            states.append(eng.state.cpu())
        runs.append((eng, states))
    (eager, want), (replayed, got) = runs
    assert len(replayed.__dict__["_dp_graphs"]) == 1 and "_dp_graphs" not in eager.__dict__
    assert all(len(pair) == 2 for pair in replayed.__dict__["_dp_graphs"].values())
    for j, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), (j, a.view(torch.float32).tolist(), b.view(torch.float32).tolist())
    assert int(got[-1][_lib.ST_STEP:_lib.ST_STEP + 2].view(torch.int64)[0]) == 4
    for what in ("params", "adam_m", "adam_v"):
        assert bool(torch.isfinite(getattr(replayed, what)).all()), what
        assert torch.equal(getattr(replayed, what), getattr(eager, what)), what


# ---- (c) two working ranks and an idle one ----------------------------------------------------------------------------------------------
class PlayedCollective:
    """allreduce_step for three ranks that take their turns in one process, on the current stream: A (a working rank) leaves its
    buffer, B (the other working rank) receives A's and holds the sum, C (the idle rank) receives that sum.  So B and C hold what an
    all-reduce leaves on every rank; A goes on with its own contribution alone and is set back to B's parameters before the next round."""

    def __init__(self, n_params):
        self.n, self.calls, self.turn, self.entered, self.reduced = n_params, 0, None, {}, None

    def __call__(self, grad_ext, group=None, single_rank_too=False):
        self.calls += 1
        assert grad_ext.dtype == torch.float32 and grad_ext.numel() == self.n + TAIL
        self.entered[self.turn] = grad_ext.clone()
        if self.turn == "B":
            grad_ext.add_(self.entered["A"])
            self.reduced = grad_ext.clone()
        elif self.turn == "C":
            grad_ext.add_(self.reduced)

    def step(self, turn, fn):
        """one rank's step: exactly one collective"""
        before, self.turn = self.calls, turn
        fn()
        assert self.calls == before + 1, f"rank {turn} entered the collective {self.calls - before} times"


def twin(eng):
    t = Engine(eng.cfg, "cuda", embedding_width=eng.embedding_width, inner_activation=eng.inner_activation, mlm_activation=eng.mlm_activation)
    t.params.copy_(eng.params)
    t.pooler.copy_(eng.pooler)
    return t


def gradient_errors(got, ref, count):
    """compare_grads' measure without its assertion: the worst tensor's relative error (every tensor against at least 1e-4 of the
    largest gradient magnitude of the model)"""
    floor = 1e-4 * max(float(g.abs().max()) for g in ref.values()) + 1e-7
    return max((float((got[n].double() / count - g.double().reshape(got[n].shape)).abs().max()) / max(float(g.abs().max()), floor), n)
               for n, g in ref.items())


def check_contribution(what, own, own_sums, reference, mode, c, name):
    """one rank's [gradients | sums] as it entered the collective against the restatement of its shard: the loss and the gradient
    buffer within the bounds a single step has at the cell (run_and_check_train_step's, check_bf16_step's)"""
    loss_ref, grads_ref, _ = reference
    cnt = own_sums[1]
    loss_err = abs(own_sums[0] / cnt - float(loss_ref))
    if mode == "bf16":
        worst_cos, worst_norm = bf16_gradient_errors(own, grads_ref, cnt)
        print(f"MEASURED contribution {what}: loss rel err {loss_err / abs(float(loss_ref)):.2e}, worst cosine {worst_cos[0]:.6f} "
              f"({worst_cos[1]}), worst rel norm err {worst_norm[0]:.2e} ({worst_norm[1]})")
        b_loss, b_cos, b_norm = BF16_CELL_BOUNDS.get(name, BF16_BOUNDS[c.head_dim])
        assert loss_err / abs(float(loss_ref)) <= b_loss
        assert worst_cos[0] >= b_cos, worst_cos
        assert worst_norm[0] <= b_norm, worst_norm
    else:
        worst = gradient_errors(own, grads_ref, cnt)
        print(f"MEASURED contribution {what}: loss err {loss_err:.2e}, worst gradient tensor rel err {worst[0]:.2e} ({worst[1]})")
        assert loss_err < LOGIT_TOL
        compare_grads(own, grads_ref, cnt, rel=REL)


@pytest.mark.parametrize("case,matrix_mode", params_of(dm.JOINED_CASES), indirect=["matrix_mode"])
def test_two_ranks_and_an_idle_one_take_the_restatements_step_on_the_joined_batch(case, matrix_mode, monkeypatch):
    matrix, name, mode = case
    c = dm.cell_of(matrix, name)
    B = dm.batch_size(matrix, c)
    cfg_o, rank_a, _ = side(matrix).build_cell(c)
    rank_b, rank_c = twin(rank_a), twin(rank_a)
    ranks = {"A": rank_a, "B": rank_b, "C": rank_c}
    for j, eng in enumerate(ranks.values()):
        eng.set_seed(SEED + j)
        eng.ensure_training_buffers()
    shards = [side(matrix).cell_batch(c, seed=11), side(matrix).cell_batch(c, seed=12)]
    assert not torch.equal(shards[0]["input_word_ids"], shards[1]["input_word_ids"])
    cb_a, _keep_a = rank_a.prepare_batch(shards[0])
    cb_b, _keep_b = rank_b.prepare_batch(shards[1])
    joined_ids = torch.cat([s["masked_lm_ids"] for s in shards])
    played = PlayedCollective(rank_a.n_params)
    monkeypatch.setattr(b4r_dist, "allreduce_step", played)
    hp = hip_adamw_config(HP_O)
    names = [n for n in rank_b.variable_names() if orc.is_trainable(n)]
    first = shared_ref(matrix, name, c)
    tie = BF16_TIE if mode == "bf16" else TIE

    for rnd in range(2):
        if rnd:   # A went on alone: every working rank starts a round from the parameters all ranks share
            for what in ("params", "adam_m", "adam_v"):
                getattr(rank_a, what).copy_(getattr(rank_b, what))
        assert torch.equal(rank_a.params, rank_b.params) and torch.equal(rank_c.params, rank_b.params)
        before = (rank_b.export_named(), rank_b.export_named(rank_b.adam_m), rank_b.export_named(rank_b.adam_v))
        labels = {}
        for r, eng, cb in (("A", rank_a, cb_a), ("B", rank_b, cb_b)):
            played.step(r, lambda: labels.update({r: launch_labels(lambda: eng.dp_train_step(hp, cb), label_cap(matrix, c))}))
        played.step("C", lambda: rank_c.dp_idle_step(hp))
        torch.cuda.synchronize()
        st_a, st_b = rank_a.read_state(), rank_b.read_state()
        assert st_a["step"] == st_b["step"] == rank_c.read_state()["step"] == rnd + 1

        # each rank's contribution (what it entered the collective with) against the restatement of its shard, within the bounds of a
        # single step; rank A's first step is the step of part (a) -- the same batch, seed and parameters -- and shares its reference.
        # Where the inner or the transform's activation has a jump, the restatement's side of it is open at elements it cannot resolve
        # (tests/dp_matrix.py::reference_at_kink_ties); the joined reference is formed from the restatements the contributions met
        def contribution_ref(params, shard, cfg, training, rng):
            r, eng = ("A", rank_a) if shard is shards[0] else ("B", rank_b)
            own = eng.export_named(played.entered[r][:eng.n_params])
            own_sums = played.entered[r][eng.n_params:eng.n_params + 5].tolist()
            baseline = first(params, shard, cfg, training, rng) if (r == "A" and rnd == 0) else None
            return dm.reference_at_kink_ties(
                c, fmx.cell_ref(c), params, shard, cfg, rng, baseline=baseline,
                check=lambda reference: check_contribution(f"{name} [{mode}] round {rnd} rank {r}", own, own_sums, reference, mode, c, name),
                measure=lambda reference: (1.0 - bf16_gradient_errors(own, reference[1], own_sums[1])[0][0] if mode == "bf16"
                                           else gradient_errors(own, reference[1], own_sums[1])[0]))

        loss_ref, grads_ref, per_shard, counts = dm.joined_reference(contribution_ref, before[0], shards, cfg_o, [(SEED, rnd), (SEED + 1, rnd)])
        cnt = sum(counts)

        # each working rank ran the forms the cell records
        for r in "AB":
            got = parse_forms(labels[r], c, B)
            assert got == c.forms(mode), f"round {rnd}, rank {r}: forms {got}, expected {c.forms(mode)}\n{labels[r]}"

        # counts and accuracy sums: per shard (what each rank brought: A's own state, the tail B entered with), and summed
        assert_counts_match(st_a, shards[0], per_shard[0][2]["mlm_logits"], tie_width=tie)
        b_own = dict(zip(("loss_sum", "valid_count", "correct_masked", "correct_all", "slots_all"),
                         played.entered["B"][rank_b.n_params:rank_b.n_params + 5].tolist()))
        assert_counts_match(b_own, shards[1], per_shard[1][2]["mlm_logits"], tie_width=tie)
        assert_counts_match(st_b, {"masked_lm_ids": joined_ids},
                            torch.cat([per_shard[0][2]["mlm_logits"], per_shard[1][2]["mlm_logits"]]), tie_width=tie)
        # the reduced tail in B's state
        assert st_b["valid_count"] == counts[0] + counts[1] == cnt and st_b["slots_all"] == float(2 * B * c.P)
        assert st_b["loss_sum"] == float(played.reduced[rank_b.n_params])
        assert not bool(played.entered["C"].view(torch.int32).any()), "the idle rank entered the collective with a non-zero buffer"

        # B holds the restatement's step on the joined batch
        grads = rank_b.export_named(rank_b.grads)
        after = (rank_b.export_named(), rank_b.export_named(rank_b.adam_m), rank_b.export_named(rank_b.adam_v))
        gnorm_ref = float(sum(g.double().pow(2).sum() for g in grads_ref.values()).sqrt())
        loss_err = abs(st_b["loss_sum"] / cnt - loss_ref)
        norm_err = abs(st_b["grad_norm"] - gnorm_ref) / gnorm_ref
        # what the optimizer consumed: m = b1 m_before + (1 - b1) clip_scale g.  (Mode 2 holds the norm to the buffer's own below, not to
        # the restatement's, so there the restatement's gradient is scaled as the device clipped.)
        clip_scale = min(1.0, HP_O.gradient_clip_norm / (st_b["grad_norm"] if mode == "bf16" else gnorm_ref))
        consumed = {n: (after[1][n].double() - HP_O.beta_1 * before[1][n].double()) / (1.0 - HP_O.beta_1) for n in names}
        consumed_ref = {n: grads_ref[n] * clip_scale for n in names}
        if mode == "bf16":
            worst_cos, worst_norm = bf16_gradient_errors(grads, grads_ref, cnt)
            used_cos, used_norm = bf16_gradient_errors(consumed, consumed_ref, 1.0)
            own = float(rank_b.grads[:rank_b.n_params].double().pow(2).sum().sqrt()) / cnt
            print(f"MEASURED joined {name} [{mode}] round {rnd}: loss rel err {loss_err / abs(loss_ref):.2e}, worst cosine "
                  f"{worst_cos[0]:.6f} ({worst_cos[1]}), worst rel norm err {worst_norm[0]:.2e} ({worst_norm[1]}); consumed: "
                  f"{used_cos[0]:.6f}, {used_norm[0]:.2e}; gradient norm against the buffer's {abs(st_b['grad_norm'] - own) / own:.2e}")
            b_loss, b_cos, b_norm = BF16_CELL_BOUNDS.get(name, BF16_BOUNDS[c.head_dim])
            assert loss_err / abs(loss_ref) <= b_loss
            assert worst_cos[0] >= b_cos and used_cos[0] >= b_cos, (worst_cos, used_cos)
            assert worst_norm[0] <= b_norm and used_norm[0] <= b_norm, (worst_norm, used_norm)
            assert own > 0.0 and abs(st_b["grad_norm"] - own) <= 2e-6 * own, (st_b["grad_norm"], own)
        else:
            worst, used = gradient_errors(grads, grads_ref, cnt), gradient_errors(consumed, consumed_ref, 1.0)
            print(f"MEASURED joined {name} [{mode}] round {rnd}: loss err {loss_err:.2e}, gradient norm rel err {norm_err:.2e}, worst "
                  f"gradient tensor rel err {worst[0]:.2e} ({worst[1]}), consumed {used[0]:.2e} ({used[1]})")
            assert loss_err < LOGIT_TOL
            assert norm_err <= 2e-3, (st_b["grad_norm"], gnorm_ref)
            compare_grads(grads, grads_ref, cnt, rel=REL)
            compare_grads(consumed, consumed_ref, 1.0, rel=REL)
        assert_adamw_exact(st_b, names, grads, before, after, rnd, HP_O)

        # the idle rank took the same step, bit for bit: ranks never drift apart
        for what in ("params", "adam_m", "adam_v"):
            assert torch.equal(getattr(rank_c, what), getattr(rank_b, what)), f"round {rnd}: {what} of the idle rank"
        assert torch.equal(rank_c.state[SHARED], rank_b.state[SHARED]), (rank_c.read_state(), st_b)
    assert played.calls == 6
