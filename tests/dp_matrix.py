"""The cases of the data-parallel step's tests (tests/test_gpu_dp_matrix.py runs them on the GPU; tests/test_dp_matrix_host.py checks
their coverage on the CPU).

Engine.dp_train_step is a composition of public calls (forward, b4r_loss where the head materialises the logits, backward with the
gradient tail, the all-reduce, b4r_optimizer_step_reduced), each of which plans for itself; Engine.train_step is one call with one
plan.  The cells of tests/feature_matrix.py and tests/geometry_matrix.py record the forms of the latter; the data-parallel step must
run the same ones, so the matrices are not extended here -- a case names a cell of one of them:

* STEP_CASES: every cell of both matrices in every one of its modes -- one data-parallel step alone against the restatement;
* JOINED_CASES: two working ranks and an idle one played in one process, where every attention, feed-forward and embedding form
  and both head variants occur;
* DP_GRAPH_CELLS: the graph-replayed step against the eager one.

A case is (matrix, cell name, mode) with matrix "feature" or "geometry"."""
import contextlib
import math
from typing import Callable, Dict, List, Sequence, Tuple

import torch

from tests import activation_ref as ar
from tests import feature_matrix as fm
from tests import geometry_matrix as gm

MATRICES = {"feature": fm.CELLS, "geometry": gm.CELLS}
Case = Tuple[str, str, str]

# part (a): the same cases, in the same order, as the two train-step matrix tests together
STEP_CASES: List[Case] = [(matrix, name, mode) for matrix, cells in MATRICES.items() for name, c in cells.items() for mode in c.modes]

_JOINED = [
    ("feature", "h64_L200", ("bf16x3", "f32")),        # the folded blocks, the embedding stage inside layer 0's; f32: cores, rows gathered
    ("feature", "h128_L200_e64", ("bf16x3", "bf16")),  # slot-query attention, the Wide pair, compact rows, a factorised embedding
    ("feature", "h256_I512", ("bf16x3",)),             # dense tile products in both layers, head width 128
    ("feature", "h128hd64_L200", ("f32",)),            # the width-64 core in exact fp32
    ("feature", "b64_L64", ("bf16x3",)),               # the unfolded block backward
    ("feature", "b128_L225", ("bf16x3",)),             # the two-launch core backward, compact rows gathered
    ("geometry", "h512hd32", ("bf16x3",)),             # the materialising head in a split mode (item-table width 512)
    ("geometry", "tinyV4", ("bf16x3",)),               # one real item
]
JOINED_CASES: List[Case] = [(matrix, name, mode) for matrix, name, modes in _JOINED for mode in modes]
DP_GRAPH_CELLS: List[Case] = [case for case in JOINED_CASES if case[2] == "bf16x3"] + [("feature", "h64_L200", "f32")]

# the item-table widths of the logits-free head (b4r_head32_hidden_ok)
FUSED_HEAD_WIDTHS = (64, 128, 256)


def cell_of(matrix: str, name: str):
    return MATRICES[matrix][name]


def batch_size(matrix: str, c) -> int:
    return fm.BATCH if matrix == "feature" else c.B


def case_id(case: Case) -> str:
    return "-".join(case)


def head_is_fused(c, mode: str) -> bool:
    """fused_head_ok (bert4rec_amd/csrc/b4r_model.hip) restated: the logits-free head answers on the item table's width (the embedding
    width of a factorised model, else the hidden size) and needs a split mode; everywhere else the data-parallel step materialises the
    logits and runs b4r_loss"""
    return (c.E or c.H) in FUSED_HEAD_WIDTHS and mode != "f32"


# ---- the restatement where an activation's derivative jumps -------------------------------------------------------------------------
# relu' and selu' jump at 0.  Where the restatement's own pre-activation x . w + b lies closer to 0 than its fp32 rounding error, its
# side of the jump is an accident of the summation order: a kernel that lands on the other side is as right as the restatement, and
# the gradients of the two differ by that one element's whole contribution (seen on an MI355X: |pre| = 8.0e-7 at one of 614 400
# elements of a relu layer moved a column of dW1 by 2e-2 of the tensor's largest entry, parallel to that row's input to six digits).
# So a comparison that fails against the restatement as it stands is repeated against the restatement with the derivative taken from
# the other side at such elements -- the full comparison, unchanged, every tensor: a wrong kernel is not explained by one sign.
KINKS = {"relu": (0.0, 1.0), "selu": (ar.SELU_SCALE * ar.SELU_ALPHA, ar.SELU_SCALE)}   # the derivative left and right of 0
KINK_TIE_LIMIT = 16   # at most this many elements (those closest to 0) are tried


def kink_roles(c, cfg_o) -> List[Tuple[str, ...]]:
    """the calls of activations with a jump, in the order the restatement makes them: the feed-forward blocks, then the transform"""
    return [("inner", i) for i in range(cfg_o.num_layers) if c.acts[0] in KINKS] + ([("mlm",)] if c.acts[1] in KINKS else [])


def kink_tolerance(role, params, cfg_o) -> torch.Tensor:
    """per unit j, the bound on the fp32 rounding error of the restatement's pre-activation x . w_j + b_j: K u |x|_2 |w_j|_2 + u |b_j|
    (u = 2^-24, K = hidden size terms), where x is a LayerNorm output: |x|_2 <= sqrt(K) max|gamma| + |beta|_2"""
    if role[0] == "inner":
        p = f"transformer/layer_{role[1]}"
        ln, w, b = f"{p}/self_attention_layer_norm", f"{p}/intermediate/kernel", f"{p}/intermediate/bias"
    else:
        ln = f"transformer/layer_{cfg_o.num_layers - 1}/output_layer_norm"
        w, b = "cls/predictions/transform/dense/kernel", "cls/predictions/transform/dense/bias"
    K = cfg_o.hidden_size
    x_norm = math.sqrt(K) * float(params[f"{ln}/gamma"].abs().max()) + float(params[f"{ln}/beta"].double().norm())
    W = params[w].double().reshape(K, -1)
    return 2.0 ** -24 * (K * x_norm * W.norm(dim=0) + params[b].double().reshape(-1).abs())


@contextlib.contextmanager
def kink_sides(flips=()):
    """while active, the restatement's activations with a jump record their inputs (yielded list, in call order) and take the
    derivative from the other side of 0 at `flips`, a collection of (call, flat element index); values are unchanged"""
    calls: List[torch.Tensor] = []
    saved = {n: ar.ACT[n] for n in KINKS}

    def wrap(name):
        left, right = KINKS[name]

        def act(x):
            k = len(calls)
            calls.append(x.detach())
            y = saved[name](x)
            idx = [i for kk, i in flips if kk == k]
            if idx:
                other = torch.zeros(x.numel(), dtype=x.dtype)
                at = x.detach().reshape(-1)[idx]
                other[idx] = torch.where(at < 0, right - left, left - right).to(x.dtype)
                y = y + other.reshape(x.shape) * (x - x.detach())
            return y
        return act

    try:
        for n in KINKS:
            ar.ACT[n] = wrap(n)
        yield calls
    finally:
        ar.ACT.update(saved)


def kink_ties(calls: Sequence[torch.Tensor], roles, params, cfg_o, limit: int = KINK_TIE_LIMIT) -> List[Tuple[int, int, float]]:
    """the elements (call, flat index, |pre|) whose pre-activation lies within the restatement's own rounding error of the jump; the
    `limit` closest to it"""
    assert len(calls) == len(roles), (len(calls), roles)
    found = []
    for k, (pre, role) in enumerate(zip(calls, roles)):
        tol = kink_tolerance(role, params, cfg_o)
        flat = pre.double().reshape(-1, tol.numel())
        for i in (flat.abs() <= tol).reshape(-1).nonzero().reshape(-1).tolist():
            found.append((k, i, float(flat.reshape(-1)[i].abs())))
    return sorted(found, key=lambda t: t[2])[:limit]


def reference_at_kink_ties(c, ref: Callable, params: Dict, shard: Dict, cfg_o, rng, check: Callable, measure: Callable, baseline=None):
    """the restatement of one step, (loss, gradients, outputs), under which check(reference) passes: the restatement as it stands
    (`baseline` where the caller has it already), else -- where the model has an activation with a jump -- with the derivative from the
    other side at some of the (at most KINK_TIE_LIMIT) elements kink_ties finds: they are tried one by one, closest to the jump first,
    and one is kept where it at least halves measure(reference), the device's worst error.  check raises AssertionError where the device
    disagrees; it decides, on the restatement so found, with nothing about it changed."""
    reference = baseline if baseline is not None else ref(params, shard, cfg_o, training=True, rng=rng)
    try:
        check(reference)
        return reference
    except AssertionError:
        roles = kink_roles(c, cfg_o)
        if not roles:
            raise
        with kink_sides() as calls:
            ref(params, shard, cfg_o, training=True, rng=rng)
        taken, best = [], measure(reference)
        for k, i, a in kink_ties(calls, roles, params, cfg_o):
            with kink_sides([(kk, ii) for kk, ii, _ in taken] + [(k, i)]):
                other = ref(params, shard, cfg_o, training=True, rng=rng)
            if measure(other) <= 0.5 * best:
                taken, best, reference = taken + [(k, i, a)], measure(other), other
        if not taken:
            raise
    print(f"MEASURED kink ties: the device took the other side of {c.acts}'s jump at {[(roles[k], i, a) for k, i, a in taken]}")
    check(reference)
    return reference


def joined_reference(ref: Callable, params: Dict, shards: Sequence[Dict], cfg_o, rngs: Sequence[Tuple[int, int]]):
    """The step of len(shards) data-parallel ranks as the restatement sees it: ref(params, shard, cfg_o, training=True, rng=rng_r) per
    shard -- one at a time, not concatenated, because dropout indices are local to a rank's batch -- joined by the law of the
    all-reduce: every rank contributes the gradient of its loss SUM (cnt_r * g_r) and its count, the optimizer divides by the reduced
    count.  Returns (joined mean loss, joined gradients sum cnt_r g_r / sum cnt_r, per-shard (loss, gradients, outputs), counts)."""
    assert len(shards) == len(rngs) > 0
    per_shard = [ref(params, shard, cfg_o, training=True, rng=rng) for shard, rng in zip(shards, rngs)]
    counts = [float((shard["masked_lm_ids"] != 0).sum()) for shard in shards]
    total = sum(counts)
    assert total > 0
    loss = sum(cnt * float(out[0]) for cnt, out in zip(counts, per_shard)) / total
    grads = {n: sum(cnt * out[1][n].double() for cnt, out in zip(counts, per_shard)) / total for n in per_shard[0][1]}
    return loss, grads, per_shard, counts
