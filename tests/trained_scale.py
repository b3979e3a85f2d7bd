"""Weights at the scales a trained model reaches, and the float64 reference the model-level launch chains are held to there
(tests/test_trained_scale_host.py runs the fp32 restatement through the same criteria on the CPU; tests/test_gpu_trained_scale.py
runs the device).

Every other model-level test builds its weights from the initialisers (truncated normal, std 0.02): attention rows and the
catalogue softmax are then uniform to a few percent, and a slip in a running maximum, the -1e9 adder next to a large score, the
exp2 range or dS = P (dP - delta) with P near 0 or 1 cannot show.  sharpen() rescales a cell's initialised parameters -- the same
draw at every level -- to

    level      tables (item, position)  query / key kernels  other kernels (projection too)  biases, betas  gammas
    moderate   0.15                     0.14                 0.08                            0.1            1 +- 0.2
    sharp      0.36                     0.29                 0.12                            0.3            1 +- 0.3

The masked-LM transform's Glorot kernel keeps its scale.  These are the final scales.  The proposal's starting values (query / key
0.12 and 0.25, sharp tables 0.30) missed the level conditions of tests/test_trained_scale_host.py at the weakest cells: at head
width 64 the moderate scores had std 0.495 and a largest probability of 2.98 x uniform; at hidden 64 the sharp median largest
probability was 0.37 - 0.39 and the sharp top catalogue probability 0.22 (h64_L200, h128hd64_L200).  At the scales above the worst
cell has, moderate: score std 0.67, 4.2 x uniform, logit span 7.9; sharp: score std 4.8 (27 at hidden 256), median largest
probability 0.53, logit span 19, top catalogue probability 0.39, smallest ground-truth probability 1.5e-7 or less; every cell is on
the same scales.  Where a cell uses relu, a few biases are then moved by at most 2.1e-3 so that no relu sits on its kink ("ReLU
kinks" below).

Cells (tests/feature_matrix.py, so build_cell and the launch-label parser are reused): between their split and exact-fp32 records
they take every form a train step can take (the host test asserts it from the records).

Bounds.  e32 is the largest absolute difference between the fp32 and the fp64 restatement of a quantity at that cell and level:

* forward quantities and the loss: contract = 1e-3 max(1, max |ref64|) (the BASELINE contract, scaled as tests/test_gpu_blocks.py
  scales its tolerances); exact fp32 16 e32; bf16x3 min(512 e32, contract) -- three-term products carry 2^-17 relative against
  fp32's 2^-24 (128), margin 4 (tests/inference_checks.py);
* gradients, per tensor: relative error with compare_grads's floor (1e-4 of the model's largest gradient), e32g the fp32
  restatement's; exact fp32 max(16 e32g, 1e-5); bf16x3 min(max(512 e32g, 1e-5), G), G the suite's gradient contract (2e-3 without
  dropout, 5e-3 in training mode).  No tensor has another rule."""
import functools
from typing import Dict, Tuple

import numpy as np
import torch

from oracle import bert4rec_oracle as orc
from tests import activation_ref as ar
from tests import feature_matrix as fm
from tests import inference_checks as ic
from tests import inference_matrix as im
from tests.b4r_testlib import set_row_slots

CELLS = ("h64_L200", "b64_L64", "b64_L209", "h128_L200", "h128hd64_L200", "h256_I512")
EVAL_PATH_CELLS = ("h64_L200", "h128_L200", "h128hd64_L200")
MODES = ("bf16x3", "f32")      # mode 2 is out of scope: its bounds were measured at init scale
BATCH = 6
INIT_STD, INIT_GAMMA = 0.02, 0.05      # what every build_cell / cell_params draws

# level -> (tables, query / key kernels, other kernels, biases and betas, gammas' spread)
LEVELS: Dict[str, Tuple[float, float, float, float, float]] = {
    "moderate": (0.15, 0.14, 0.08, 0.1, 0.2),
    "sharp": (0.36, 0.29, 0.12, 0.3, 0.3),
}
# what a level has to be on the fp64 reference: (layer-0 score std >=, median largest attention probability >= (x uniform at
# moderate, absolute at sharp), logit span over the weighted slots >=)
CONDITIONS = {"moderate": (0.5, 3.0, 6.0), "sharp": (3.0, 0.4, 12.0)}

CONTRACT = 1e-3
GRAD_CONTRACT = {False: 2e-3, True: 5e-3}      # by training mode (tests/test_gpu_model.py)
GRAD_MIN = 1e-5
TIE_CAP = 0.05                                  # slots whose fp64 top-two gap is below the logits bound: fewer than this share
TRAIN_RATE, TRAIN_SEED, TRAIN_STEP = 0.2, 4242, 17   # 1 / 0.8 is exact: fp64 and the device scale kept elements alike
BATCH_SEED = 51
TRANSFORM_KERNEL = "cls/predictions/transform/dense/kernel"


def modes_of(name: str) -> Tuple[str, ...]:
    return tuple(m for m in MODES if m in fm.CELLS[name].modes)


# ---- the weights ------------------------------------------------------------------------------------------------------------------
def sharpen(params: Dict[str, torch.Tensor], level: str, seed: int = 0) -> Dict[str, torch.Tensor]:
    """the initialised parameters (Keras names; the oracle's or the factorised ones) at `level`: every tensor times target / 0.02
    (gammas: their distance from 1 times target / 0.05), so a cell's weights are one draw at every level.  A bias, beta or gamma
    the initialisers left trivial (all 0 / all 1) is drawn from `seed` instead."""
    table, qk, kernel, bias, gamma = LEVELS[level]
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n, p in params.items():
        p = p.detach().to(torch.float32)
        if n == TRANSFORM_KERNEL:
            t = p.clone()
        elif n.endswith("gamma"):
            d = p - 1.0
            t = 1.0 + (d * (gamma / INIT_GAMMA) if bool(d.any()) else torch.randn(p.shape, generator=g) * gamma)
        elif n.endswith(("bias", "beta")):
            t = p * (bias / INIT_STD) if bool(p.any()) else torch.randn(p.shape, generator=g) * bias
        elif n.endswith("embeddings"):
            t = p * (table / INIT_STD)
        elif n.endswith(("query/kernel", "key/kernel")):
            t = p * (qk / INIT_STD)
        else:
            assert n.endswith("kernel"), n
            t = p * (kernel / INIT_STD)
        out[n] = t.to(torch.float32).contiguous()
    return out


def cell_config(name: str, training: bool = False) -> orc.OracleConfig:
    c = im.CELLS[name]
    rate = TRAIN_RATE if training else 0.0
    return orc.OracleConfig(vocab_size=c.V, hidden_size=c.H, num_layers=c.layers, num_attention_heads=c.heads,
                            max_sequence_length=c.L, inner_dim=c.inner, output_dropout=rate, attention_dropout=rate)


# ---- the batch -------------------------------------------------------------------------------------------------------------------
ROW_SINGLE, ROW_FULL, ROW_SHORT, ROW_REPEAT, ROW_UNWEIGHTED = 0, 1, 2, 3, 4


def sharp_batch(c, seed: int = BATCH_SEED) -> Dict[str, torch.Tensor]:
    """orc.synthetic_batch at B = 6 (ragged) with, by hand: row 0 of length 1; row 1 of full length; row 2 (where L >= 65) of 20
    tokens, so that every key tile of its sweeps after the first is wholly masked; row 3 with one item id on every second token --
    half of its slots on that item -- so that one table row and the [MASK] row take many contributions of the scatter; row 4 with
    every slot padding (weight 0); row 5 as drawn"""
    L, P, V = c.L, c.P, fm.VOCAB
    batch = orc.synthetic_batch(BATCH, L, P, V, seed=seed + L, ragged=True)
    rng = np.random.default_rng(seed)

    def resize(row, n):
        batch["labels"][row] = 0
        batch["labels"][row, :n] = torch.from_numpy(rng.integers(ic.FIRST_ITEM, V, size=n).astype(np.int64))
        batch["input_mask"][row] = 0
        batch["input_mask"][row, :n] = 1

    def slots(n, k, among=None):
        pool = np.arange(n) if among is None else np.asarray(among)
        return np.sort(rng.choice(pool, size=min(k, len(pool)), replace=False)).tolist()

    resize(ROW_SINGLE, 1)
    set_row_slots(batch, ROW_SINGLE, [0], orc.MASK_TOKEN_ID)
    resize(ROW_FULL, L)
    set_row_slots(batch, ROW_FULL, slots(L, P), orc.MASK_TOKEN_ID)
    if L >= 65:
        resize(ROW_SHORT, 20)
        set_row_slots(batch, ROW_SHORT, slots(20, min(P, 4)), orc.MASK_TOKEN_ID)
    n = max(8, (3 * L) // 4)
    resize(ROW_REPEAT, n)
    batch["labels"][ROW_REPEAT, 0:n:2] = int(rng.integers(ic.FIRST_ITEM, V))
    k = max(2, min(P, n // 5))
    pos = slots(n, k // 2, np.arange(0, n, 2)) + slots(n, k - k // 2, np.arange(1, n, 2))
    set_row_slots(batch, ROW_REPEAT, sorted(pos), orc.MASK_TOKEN_ID)
    set_row_slots(batch, ROW_UNWEIGHTED, [], orc.MASK_TOKEN_ID)
    return batch


@functools.lru_cache(maxsize=None)
def cell_batch(name: str) -> Dict[str, torch.Tensor]:
    return sharp_batch(fm.CELLS[name])


# ---- ReLU kinks ---------------------------------------------------------------------------------------------------------------------
# The gradient of a ReLU model jumps where a pre-activation crosses zero.  Three cells use relu (the feed-forward blocks of h128_L200
# and b64_L64, the masked-LM transform of h64_L200); with 10^4 - 10^5 pre-activations behind their gradients, some lie within 1e-5
# of zero (2.4e-6 at h128_L200 / moderate), where the device's bf16x3 product and the fp64 reference take different branches.  One
# such flip in the last layer moves its intermediate kernel's gradient by 2e-2 of its largest element -- in fp64 itself, under a
# relative perturbation of 1e-5 of the weights -- so a gradient comparison there measures the input, not the kernels.  The cells'
# weights are therefore put in general position: the bias of a unit is shifted (by multiples of the clearance, at most a few 1e-3)
# until no pre-activation that carries a gradient, in the eval or the training-mode forward, lies within RELU_CLEARANCE of zero.
# This conditions the input and cannot hide a kernel's error: the kernels still see every row, and a device pre-activation that is
# off by more than the clearance flips its branch and fails the gradient comparison as before.  So the clearance errs to the
# failing side: it only has to exceed the error of a correct pre-activation (the hidden rows of these cells measure within 1.7e-4 of
# fp64 in bf16x3), and one chosen too small shows as a failed case, never as a passed one.  The host test asserts the clearance.
RELU_CLEARANCE = 3e-4


class Probe(torch.overrides.TorchFunctionMode):
    """records (arguments, result) of every call of `func` inside the `with` block: a look into the restatement's forward that leaves
    tests/activation_ref.py and torch as they are"""

    def __init__(self, func):
        super().__init__()
        self.func, self.calls = func, []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if func is self.func:
            self.calls.append((args, out))
        return out


def relu_preactivations(params: Dict[str, torch.Tensor], name: str) -> Dict[str, torch.Tensor]:
    """fp64: bias name -> the pre-activations of every relu whose output carries a gradient, [rows, units], the rows of the eval
    forward and of the training-mode forward (keep masks of (TRAIN_SEED, TRAIN_STEP)) stacked: a feed-forward block's on the valid
    tokens (the last layer's: on the weighted slots' rows), the masked-LM transform's on the weighted slots"""
    c = im.CELLS[name]
    batch = cell_batch(name)
    rk = ic.ranked_slots(batch)
    valid = torch.nonzero(batch["input_mask"].reshape(-1), as_tuple=True)[0]
    sites = [(f"transformer/layer_{i}/intermediate/bias", rk.rows if i == c.layers - 1 else valid)
             for i in range(c.layers)] if c.acts[0] == "relu" else []
    if c.acts[1] == "relu":
        sites.append(("cls/predictions/transform/dense/bias", rk.slots))
    out: Dict[str, list] = {n: [] for n, _ in sites}
    if not sites:
        return {}
    p64 = {n: p.double() for n, p in params.items()}
    assert ar.ACT["relu"] is torch.relu
    for training in (False, True):
        with Probe(torch.relu) as relus:
            ar.model_forward(p64, batch, cell_config(name, training), c.acts[0], c.acts[1], training=training,
                             rng=(TRAIN_SEED, TRAIN_STEP))
        assert len(relus.calls) == len(sites), (len(relus.calls), len(sites))
        for (n, rows), ((z,), _) in zip(sites, relus.calls):
            out[n].append(z.detach().reshape(-1, z.shape[-1])[rows])
    return {n: torch.cat(zs) for n, zs in out.items()}


def clear_relu_kinks(params: Dict[str, torch.Tensor], name: str, clearance: float = RELU_CLEARANCE) -> Dict[str, torch.Tensor]:
    """params with the biases in front of every relu shifted so that relu_preactivations() has no entry within `clearance` of zero"""
    params = {n: p.clone() for n, p in params.items()}
    for _ in range(16):
        moved = False
        for n, z in relu_preactivations(params, name).items():
            for j in torch.nonzero((z.abs() < clearance).any(dim=0), as_tuple=True)[0].tolist():
                col = z[:, j]
                shift = next(s for k in range(1, 200) for s in (k * clearance, -k * clearance)
                             if float((col + s).abs().min()) >= 1.5 * clearance)
                params[n][j] += shift
                moved = True
        if not moved:
            return params
    raise AssertionError(f"{name}: relu pre-activations still within {clearance} of zero")


@functools.lru_cache(maxsize=None)
def cell_weights(name: str, level: str) -> Dict[str, torch.Tensor]:
    """the parameters build_cell loads (inference_checks.cell_params) at `level`, clear of the relu kinks (read-only: shared by every
    case of the cell)"""
    _, params = ic.cell_params(im.CELLS[name])
    return clear_relu_kinks(sharpen(params, level), name)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name: str, level: str, dtype: torch.dtype = torch.float64, training: bool = False) -> Dict[str, object]:
    """activation_ref.loss_and_grads with the cell's activations (and the factorised embedding stage where the cell has a width E) on
    cell_batch(name), parameters cast to `dtype`: loss, grads (per tensor), sequence_output [B*L, H], mlm_hidden [B*P, E], logits
    [B*P, V].  fp64 is the reference; fp32 measures e32.  training: both dropouts at TRAIN_RATE with the keep masks of
    (TRAIN_SEED, TRAIN_STEP), which the device draws too.  Cached: treat as read-only."""
    c = im.CELLS[name]
    cfg, batch = cell_config(name, training), cell_batch(name)
    params = {n: p.to(dtype) for n, p in cell_weights(name, level).items()}
    loss, grads, out = ar.loss_and_grads(params, batch, cfg, c.acts[0], c.acts[1], training=training, rng=(TRAIN_SEED, TRAIN_STEP))
    assert out["mlm_logits"].dtype == dtype
    return {"loss": loss.reshape(1), "grads": grads, "sequence_output": out["sequence_output"].reshape(-1, c.H),
            "mlm_hidden": out["mlm_hidden"].reshape(-1, c.width), "logits": out["mlm_logits"].reshape(-1, c.V)}


FORWARD = ("sequence_output", "mlm_hidden", "logits")


def on_slots(batch, quantity: str, t: torch.Tensor) -> torch.Tensor:
    """the rows of a forward quantity that belong to the weighted slots (sequence_output: the rows they read)"""
    rk = ic.ranked_slots(batch)
    return t[rk.rows if quantity == "sequence_output" else rk.slots]


def forward_error(batch, quantity: str, got: torch.Tensor, ref64: torch.Tensor) -> float:
    if quantity != "loss":
        got, ref64 = on_slots(batch, quantity, got), on_slots(batch, quantity, ref64)
    return float((got.detach().cpu().double().reshape(ref64.shape) - ref64).abs().max())


def contract_of(batch, quantity: str, ref64: torch.Tensor) -> float:
    ref = ref64 if quantity == "loss" else on_slots(batch, quantity, ref64)
    return CONTRACT * max(1.0, float(ref.abs().max()))


def forward_bound(mode: str, e32: float, contract: float) -> float:
    if mode == "f32":
        return 16.0 * e32
    assert mode == "bf16x3"
    return min(512.0 * e32, contract)


def grad_errors(got: Dict[str, torch.Tensor], ref64: Dict[str, torch.Tensor], count: float = 1.0) -> Dict[str, float]:
    """per tensor: max |got / count - ref| over max(max |ref|, floor), compare_grads's floor (1e-4 of the largest gradient of the
    model: the key-bias gradient is analytically zero)"""
    floor = 1e-4 * max(float(g.abs().max()) for g in ref64.values()) + 1e-7
    out = {}
    for n, g in ref64.items():
        a = got[n].detach().cpu().double() / count
        b = g.double().reshape(a.shape)
        out[n] = float((a - b).abs().max()) / max(float(b.abs().max()), floor)
    return out


def grad_bound(mode: str, e32g: float, training: bool) -> float:
    if mode == "f32":
        return max(16.0 * e32g, GRAD_MIN)
    assert mode == "bf16x3"
    return min(max(512.0 * e32g, GRAD_MIN), GRAD_CONTRACT[training])


@functools.lru_cache(maxsize=None)
def fp32_errors(name: str, level: str, training: bool = False):
    """(e32 per forward quantity and the loss, e32g per gradient tensor) of the fp32 restatement against fp64"""
    r64, r32 = reference(name, level, torch.float64, training), reference(name, level, torch.float32, training)
    batch = cell_batch(name)
    e32 = {q: forward_error(batch, q, r32[q], r64[q]) for q in FORWARD + ("loss",)}
    return e32, grad_errors(r32["grads"], r64["grads"])


def tie_slots(batch, logits64: torch.Tensor, width: float):
    """over the weighted slots: (argmax of the fp64 logits, whether the two best lie closer than `width`)"""
    top = on_slots(batch, "logits", logits64).topk(2, dim=-1)
    return top.indices[:, 0], (top.values[:, 0] - top.values[:, 1]) < width


# ---- what a level is ----------------------------------------------------------------------------------------------------------------
def layer0_attention(name: str, level: str):
    """fp64, layer 0, over valid (query, key) pairs: the scores (1-D) and each valid query's largest probability with its row's
    uniform value ([queries * heads] each)"""
    c = im.CELLS[name]
    cfg = cell_config(name)
    params = {n: p.double() for n, p in cell_weights(name, level).items()}
    batch = cell_batch(name)
    with Probe(torch.softmax) as softmaxes:      # the restatement's own: one per layer, on the scores plus the mask's adder
        ar.encoder_forward(params, batch["input_word_ids"], batch["input_mask"], cfg, c.acts[0])
    assert len(softmaxes.calls) == c.layers
    (s, *_), prob = softmaxes.calls[0]
    m = batch["input_mask"].bool()
    pair = (m[:, None, :, None] & m[:, None, None, :]).expand_as(s)      # the adder is zero on these
    valid_q = m[:, None, :].expand(-1, c.heads, -1)
    uniform = (1.0 / m.sum(dim=1).double())[:, None, None].expand(-1, c.heads, m.shape[1])
    return s[pair], prob.max(dim=-1).values[valid_q], uniform[valid_q]


def level_statistics(name: str, level: str) -> Dict[str, float]:
    scores, pmax, uniform = layer0_attention(name, level)
    batch = cell_batch(name)
    r64 = reference(name, level)
    logits = on_slots(batch, "logits", r64["logits"])
    prob = torch.softmax(logits, dim=-1)
    gt = ic.ranked_slots(batch).gt
    return {"score_std": float(scores.std()), "score_range": float(scores.max() - scores.min()),
            "pmax_median": float(pmax.median()), "pmax_over_uniform_median": float((pmax / uniform).median()),
            "pmax_max": float(pmax.max()), "logit_span": float(logits.max() - logits.min()),
            "top_prob_max": float(prob.max()), "gt_prob_min": float(prob.gather(1, gt[:, None]).min())}
