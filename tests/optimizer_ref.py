"""AdamWeightDecay.apply_gradients (adam_w_optimizer.py:100-137) over FLAT buffers in numpy float64: the reference of the
optimizer kernels (adamw_kernel / adamw_fused_kernel, bert4rec_amd/csrc/b4r_rowops.hip).

One input is float32 by definition: the learning rate.  The reference's schedule (WarmUp over PolynomialDecay) is evaluated in
float32 by TF, so its value -- orc.learning_rate, rounding for rounding -- is what every implementation has to use.  Everything else
(hyper-parameters as the float32 values the C struct carries, division by the count, norm, clip, decay, moments, update) is float64.

    g      = grad_sum / valid_count                      (the kernels receive the gradient of the loss SUM)
    norm   = sqrt(sum g^2)
    g     *= clip / max(norm, clip)                      (tf.clip_by_global_norm; clip <= 0: off)
    p     -= lr * p * wd          on the decayed set     (_decay_weights_op, BEFORE Adam; wd == 0: off)
    m     += (g - m) (1 - b1);  v += (g g - v) (1 - b2)  (Keras Adam, local_step = step + 1)
    p     -= m * [lr sqrt(1 - b2^t) / (1 - b1^t)] / (sqrt(v) + eps)
"""
from dataclasses import replace

import numpy as np
import torch

from oracle import bert4rec_oracle as orc

F32 = np.float32


def f32(x) -> float:
    """the float32 value a C float field holds, as a python float"""
    return float(F32(x))


def decay_selection(n: int, n_decay: int = 0, decay_mask=None) -> np.ndarray:
    """bool [n]: the elements that decay -- the first n_decay, or the non-zero bytes of a mask (the mask wins, as in the kernels)"""
    if decay_mask is not None:
        sel = np.asarray(decay_mask).reshape(-1) != 0
        assert sel.shape == (n,)
        return sel
    return np.arange(n) < int(n_decay)


def adamw_apply64(p, g_sum, m, v, step: int, hp: orc.AdamWConfig, valid_count: float = 1.0, n_decay: int = 0, decay_mask=None):
    """One step.  p, g_sum, m, v: flat arrays (any float dtype; read as float64, not modified).
    Returns (p, m, v, info) in float64; info: lr (np.float32), grad_norm, clip_scale."""
    p, g, m, v = (np.array(a, dtype=np.float64).reshape(-1) for a in (p, g_sum, m, v))
    n = p.size
    cnt = float(valid_count)
    g = g / (cnt if cnt > 0.0 else 1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        norm = float(np.sqrt(np.sum(g * g)))
        clip = f32(hp.gradient_clip_norm)
        scale = clip / max(norm, clip) if clip > 0.0 else 1.0
        if norm != norm:
            scale = float("nan")     # tf.clip_by_global_norm: a NaN norm poisons every gradient (python's max() would hide it)
        g = g * scale
        lr32 = orc.learning_rate(int(step), hp)
        lr = float(lr32)
        b1, b2, eps, wd = f32(hp.beta_1), f32(hp.beta_2), f32(hp.epsilon), f32(hp.weight_decay_rate)
        t = float(int(step) + 1)
        alpha = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        if wd != 0.0:
            sel = decay_selection(n, n_decay, decay_mask)
            p = np.where(sel, p - lr * p * wd, p)
        m = m + (g - m) * (1.0 - b1)
        v = v + (g * g - v) * (1.0 - b2)
        p = p - (m * alpha) / (np.sqrt(v) + eps)
    return p, m, v, dict(lr=lr32, grad_norm=norm, clip_scale=scale)


def adamw_apply32(p, g_sum, m, v, step: int, hp: orc.AdamWConfig, valid_count: float = 1.0, n_decay: int = 0, decay_mask=None):
    """The same step by the fp32 oracle (orc.adamw_apply) on the same flat float32 buffers: the decayed and the undecayed elements go in
    as two named tensors, of which the oracle's name rule decays the first.  Returns float32 arrays (p, m, v, grad_norm)."""
    n = int(np.asarray(p).size)
    sel = torch.from_numpy(decay_selection(n, n_decay, decay_mask))
    cnt = float(valid_count) if float(valid_count) > 0.0 else 1.0

    def split(a, scale=None):
        t = torch.from_numpy(np.array(a, dtype=np.float32).reshape(-1))
        if scale is not None:
            t = t / torch.tensor(scale, dtype=torch.float32)
        return {"w/kernel": t[sel].clone(), "b/bias": t[~sel].clone()}

    def join(d):
        out = torch.empty(n, dtype=torch.float32)
        out[sel] = d["w/kernel"]
        out[~sel] = d["b/bias"]
        return out.numpy()

    P_, G_, M_, V_ = split(p), split(g_sum, cnt), split(m), split(v)
    gnorm = orc.adamw_apply(P_, G_, M_, V_, int(step), hp)
    return join(P_), join(M_), join(V_), gnorm


class Trajectory64:
    """Multi-step driver: carries p, m, v (float64) and the step, as the optimizer's slots and `iterations` do."""

    def __init__(self, p, m, v, hp: orc.AdamWConfig, step: int = 0, n_decay: int = 0, decay_mask=None):
        self.p, self.m, self.v = (np.array(a, dtype=np.float64).reshape(-1) for a in (p, m, v))
        self.hp, self.step, self.n_decay, self.decay_mask = hp, int(step), int(n_decay), decay_mask
        self.info = None

    def apply(self, g_sum, valid_count: float = 1.0):
        self.p, self.m, self.v, self.info = adamw_apply64(self.p, g_sum, self.m, self.v, self.step, self.hp, valid_count,
                                                          self.n_decay, self.decay_mask)
        self.step += 1
        return self.info


class Trajectory32:
    """The same driver on the fp32 oracle: its distance from Trajectory64 after k steps is the fp32 noise of k steps."""

    def __init__(self, p, m, v, hp: orc.AdamWConfig, step: int = 0, n_decay: int = 0, decay_mask=None):
        self.p, self.m, self.v = (np.array(a, dtype=np.float32).reshape(-1) for a in (p, m, v))
        self.hp, self.step, self.n_decay, self.decay_mask = hp, int(step), int(n_decay), decay_mask

    def apply(self, g_sum, valid_count: float = 1.0):
        self.p, self.m, self.v, gnorm = adamw_apply32(self.p, g_sum, self.m, self.v, self.step, self.hp, valid_count, self.n_decay,
                                                      self.decay_mask)
        self.step += 1
        return gnorm


def ulp32(x) -> np.ndarray:
    """one float32 unit in the last place at |x| (float64 array in, float64 out; the smallest normal's spacing below it)"""
    a = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), float(np.finfo(np.float32).tiny)).astype(np.float32)
    return np.spacing(a).astype(np.float64)


def with_hp(hp: orc.AdamWConfig, **kw) -> orc.AdamWConfig:
    return replace(hp, **kw)


# ----------------------------------------------------------------------------------------------------------------------------------
# The case matrix of the optimizer tests (tests/test_optimizer_ref_host.py on the CPU, tests/test_gpu_step_kernels.py on the device)
# ----------------------------------------------------------------------------------------------------------------------------------
N_STD = 4096 + 8                        # the size of the older op-level test: one workgroup row and a bit
N_TWO_TURNS = 4 * (2048 * 256) + 4 * 300   # more float4 than the largest grid has threads: 300 threads take a second turn
SCHEDULES = {"w0": (0, 10, 0.0), "w3": (3, 10, 1e-5), "default": (100, 400000, 0.0)}   # (warmup, train_steps, end_lr)
MIN_GROUP = 64   # a group of fewer elements is a poor sample of the fp32 noise: it is judged with the whole buffer's distance


class Case:
    """One single-step cell.  norm_ratio: |mean gradient| / 5.0 (the default clip norm; None: randn * gscale as it comes);
    values: 'randn' or 'edges' (blocks of v = g = m = 0, of m != 0 with v = 0, and of magnitudes 1e-6 .. 1e3)."""

    def __init__(self, name, schedule="w3", step=4, n=N_STD, n_decay=3001, mask=False, count=7.0, norm_ratio=0.5, clip_norm=5.0,
                 wd=0.01, values="randn", fused=False, seed=0):
        self.name, self.schedule, self.step, self.n, self.n_decay, self.mask = name, schedule, step, n, n_decay, mask
        self.count, self.norm_ratio, self.clip_norm, self.wd, self.values, self.fused, self.seed = \
            count, norm_ratio, clip_norm, wd, values, fused, seed

    def hp(self) -> orc.AdamWConfig:
        w, T, end = SCHEDULES[self.schedule]
        return orc.AdamWConfig(num_warmup_steps=w, num_train_steps=T, end_lr=end, gradient_clip_norm=self.clip_norm,
                               weight_decay_rate=self.wd)

    def __repr__(self):
        return self.name


EDGE_BLOCKS = ["zero", "m_only_g", "m_only"] + [f"1e{k}" for k in range(-6, 4)]


def make_buffers(case: Case, n: int = None, n_decay: int = None):
    """float32 p, g_sum, m, v (v >= 0), the uint8 decay mask (or None), n_decay and the named index groups of the case.  n / n_decay
    override the case's (the model-level step fixes both by its configuration)."""
    n = case.n if n is None else int(n)
    n_decay = min(case.n_decay, n) if n_decay is None else int(n_decay)
    rng = np.random.default_rng(1000 + case.seed)
    p = rng.standard_normal(n)
    g = rng.standard_normal(n)
    m = rng.standard_normal(n) * 0.01
    v = np.abs(rng.standard_normal(n)) * 0.01
    mask = (rng.random(n) < 0.4).astype(np.uint8) if case.mask else None
    blocks = {}
    if case.values == "edges":
        edges = np.linspace(0, n, len(EDGE_BLOCKS) + 1).astype(np.int64)
        for k, name in enumerate(EDGE_BLOCKS):
            sl = slice(int(edges[k]), int(edges[k + 1]))
            blocks[name] = sl
            if name == "zero":
                g[sl] = 0.0; m[sl] = 0.0; v[sl] = 0.0
            elif name == "m_only_g":
                v[sl] = 0.0
            elif name == "m_only":
                g[sl] = 0.0; v[sl] = 0.0
            else:
                s = float(name)
                p[sl] *= s; g[sl] *= s; m[sl] *= s; v[sl] *= s * s
    if case.norm_ratio is not None:
        nrm = float(np.sqrt(np.sum(g * g)))
        g = g * (case.norm_ratio * 5.0 * case.count / nrm) if nrm > 0 and case.norm_ratio > 0 else g * 0.0
    if mask is None and not blocks and 0 < n_decay < n:
        p[n_decay - 1], p[n_decay] = 1.5, -1.5      # the two elements at the decay boundary are of full size
    p, g, m, v = (a.astype(np.float32) for a in (p, g, m, v))
    sel = decay_selection(n, n_decay, mask)
    groups = {}
    for gname, gsel in (("decayed", sel), ("undecayed", ~sel)):
        if blocks:
            for bname, sl in blocks.items():
                idx = np.zeros(n, dtype=bool)
                idx[sl] = True
                groups[f"{gname}/{bname}"] = idx & gsel
        else:
            groups[gname] = gsel
    groups = {k: s for k, s in groups.items() if s.any()}
    return dict(p=p, g=g, m=m, v=v, mask=mask, n=n, n_decay=n_decay, groups=groups)


def _schedule_cases():
    out = []
    for name, (w, T, end) in SCHEDULES.items():
        steps = sorted({0, max(w - 1, 0), w, T - 1, T, T + 1000})
        for s in steps:
            out.append(Case(f"schedule-{name}-step{s}", schedule=name, step=s, fused=True, seed=len(out)))
    return out


CASES = _schedule_cases() + [
    # clip: the mean gradient's norm at 0.5 x, 1 x and 2 x gradient_clip_norm; clipping off under a norm of 1e4; no gradient at all
    Case("clip-half", norm_ratio=0.5, fused=True, seed=30),
    Case("clip-at-norm", norm_ratio=1.0, fused=True, seed=31),
    Case("clip-double", norm_ratio=2.0, fused=True, seed=32),
    Case("clip-off-norm1e4", norm_ratio=2000.0, clip_norm=0.0, fused=True, seed=33),
    Case("zero-gradient", norm_ratio=0.0, fused=True, seed=34),
    # decay: off, nothing / everything decayed, a boundary at each position inside a float4, a byte mask.  The reference's rate 0.01
    # moves a parameter by lr * 0.01 = 6e-7 of itself, a few ulp: these cells use rate 1 (6e-5 of the parameter), so that ONE element
    # decayed or spared in error is far outside the tolerance
    Case("decay-rate0", wd=0.0, fused=True, seed=40),
    Case("decay-none", n_decay=0, wd=1.0, seed=41),
    Case("decay-all", n_decay=N_STD, wd=1.0, seed=42),
    Case("decay-3001", n_decay=3001, wd=1.0, seed=43),
    Case("decay-3002", n_decay=3002, wd=1.0, seed=44),
    Case("decay-3003", n_decay=3003, wd=1.0, seed=45),
    Case("decay-mask", mask=True, wd=1.0, fused=True, seed=46),
    # counts
    Case("count-1", count=1.0, norm_ratio=2.0, fused=True, seed=50),
    Case("count-7", count=7.0, norm_ratio=2.0, fused=True, seed=51),
    Case("count-10240", count=10240.0, norm_ratio=2.0, fused=True, seed=52),
    # sizes: one float4; a second turn through the loop for 300 threads, the decay boundary inside those turns
    Case("size-4", n=4, n_decay=2, seed=60),
    Case("size-two-turns", n=N_TWO_TURNS, n_decay=N_TWO_TURNS - 601, norm_ratio=2.0, seed=61),
    # values
    Case("values-edges", values="edges", norm_ratio=2.0, n_decay=2051, fused=True, seed=70),
    Case("values-edges-unclipped", values="edges", norm_ratio=None, clip_norm=0.0, mask=True, fused=True, seed=71),
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
TRAJECTORY_STEPS = 20
# |mean gradient| / clip norm of the trajectory's steps: clipping active in the steps above 1
TRAJECTORY_RATIOS = [0.3, 2.0, 0.9, 4.0, 0.1, 1.5, 0.5, 3.0, 0.7, 1.1, 0.2, 2.5, 0.6, 0.05, 1.0, 6.0, 0.4, 0.8, 1.3, 0.3]
TRAJECTORY_CASE = Case("trajectory", schedule="w3", step=0, n_decay=3001, count=7.0, seed=90)


def trajectory_gradient(k: int, n: int, count: float) -> np.ndarray:
    """the (summed) gradient of trajectory step k: fresh values, norm of the mean gradient = TRAJECTORY_RATIOS[k] * 5"""
    g = np.random.default_rng(2000 + k).standard_normal(n)
    return (g * (TRAJECTORY_RATIOS[k] * 5.0 * count / float(np.sqrt(np.sum(g * g))))).astype(np.float32)


def case_distances(case: Case, n: int = None, n_decay: int = None):
    """Buffers of a case, its fp64 result, the fp32 oracle's result and, per index group and array, the oracle's largest distance from
    fp64 (d_case).  A group of fewer than MIN_GROUP elements gets the whole buffer's distance."""
    b = make_buffers(case, n, n_decay)
    hp = case.hp()
    p64, m64, v64, info = adamw_apply64(b["p"], b["g"], b["m"], b["v"], case.step, hp, case.count, b["n_decay"], b["mask"])
    p32, m32, v32, gnorm32 = adamw_apply32(b["p"], b["g"], b["m"], b["v"], case.step, hp, case.count, b["n_decay"], b["mask"])
    ref = dict(p=p64, m=m64, v=v64)
    o32 = dict(p=p32, m=m32, v=v32)
    d = distances(ref, o32, b["groups"])
    return b, ref, o32, info, gnorm32, d


def distances(ref, got, groups):
    """{(group, array): max |got - ref|} with the MIN_GROUP rule"""
    whole = {a: float(np.max(np.abs(got[a].astype(np.float64) - ref[a]))) for a in ("p", "m", "v")}
    d = {}
    for gname, sel in groups.items():
        for a in ("p", "m", "v"):
            d[(gname, a)] = whole[a] if int(sel.sum()) < MIN_GROUP else float(np.max(np.abs(got[a][sel].astype(np.float64) - ref[a][sel])))
    return d


def check_against(ref, got, groups, d, factor=4.0):
    """the kernel tolerance: per element |got - fp64| <= factor * d_case + 1 fp32 ulp of the element.  Returns the list of violations
    [(group, array, worst excess index, |diff|, bound)] and {(group, array): worst |diff|}."""
    bad, worst = [], {}
    for gname, sel in groups.items():
        for a in ("p", "m", "v"):
            diff = np.abs(np.asarray(got[a], dtype=np.float64)[sel] - ref[a][sel])
            bound = factor * d[(gname, a)] + ulp32(ref[a][sel])
            worst[(gname, a)] = float(diff.max())
            over = ~(diff <= bound)     # (a NaN difference is a violation)
            if over.any():
                i = int(np.argmax(np.where(over, diff - bound, -np.inf))) if np.isfinite(diff[over]).all() else int(np.argmax(over))
                bad.append((gname, a, i, float(diff[i]), float(bound[i])))
    return bad, worst
