"""GPU parity tests of the kernels that close a train step (bert4rec_amd/csrc/b4r_rowops.hip) at their edges, against float64:
  a. global norm + clip + decay + Adam: adamw_kernel (b4r_global_sqnorm + b4r_adamw_step) and adamw_fused_kernel (b4r_optimizer_step
     through Engine), on the matrix of tests/optimizer_ref.py
  b. b4r_softmax_ce: shapes around every loop bound, confident and shifted rows, exact ties, the state's accumulation
  c. the logits-free head's argmax merge at exact ties (b4r_head32.hip, b4r_head_merge.h)
  d. b4r_gather_rows / b4r_scatter_add_rows

Optimizer tolerance: per element |kernel - fp64| <= 4 d_case + 1 fp32 ulp of the element, d_case = the fp32 oracle's own distance from
fp64 on the same inputs (computed here on the CPU, per index group and array; optimizer_ref.case_distances).  The factor 4 covers a
different but equally valid fp32 evaluation order (powf, sqrtf, the norm's summation tree)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib
from bert4rec_amd.engine import Engine, make_adamw_config, make_model_config
from oracle import bert4rec_oracle as orc
from tests import b4r_testlib as T
from tests import optimizer_ref as R
from tests.b4r_testlib import P, stream

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gemm_mode")]

DEV = "cuda"
U = 2.0 ** -24
ST_TICKET = 12   # b4r_train_state.reserved[0]


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.float32)


def bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def state_step(st) -> int:
    return int(st.cpu()[_lib.ST_STEP:_lib.ST_STEP + 2].view(torch.int64)[0])


# ======================================================================================================================================
# a. AdamW
# ======================================================================================================================================
def c_hp(hp: orc.AdamWConfig, mask_dev=None):
    return make_adamw_config(hp.init_lr, hp.num_train_steps, hp.num_warmup_steps, hp.end_lr, hp.weight_decay_rate, hp.beta_1, hp.beta_2,
                             hp.epsilon, hp.gradient_clip_norm, decay_mask=mask_dev)


@functools.lru_cache(maxsize=None)
def tiny_engine():
    """the `tiny` configuration of tests/test_gpu_model.py: its flat parameter buffer is what b4r_optimizer_step steps"""
    cfg = make_model_config(37, 64, 2, 2, 20, 64, 0.1, 0.1)
    eng = Engine(cfg, DEV)
    eng.ensure_training_buffers()
    cb, keep = eng.prepare_batch(orc.synthetic_batch(4, 16, 5, 37, seed=1))
    return eng, cb, keep


@functools.lru_cache(maxsize=None)
def distances_of(name: str, n=None, n_decay=None):
    """the CPU side of a case, computed once and shared (both arithmetic modes of the fixture, both kernels where the sizes agree)"""
    return R.case_distances(R.CASE_BY_NAME[name], n, n_decay)


def run_direct(b, hp, step, count):
    """b4r_global_sqnorm + b4r_adamw_step on device copies of the buffers; returns the arrays, the state words and the state floats"""
    lib = _lib.load()
    n = b["n"]
    d = {k: torch.from_numpy(b[k]).to(DEV) for k in ("p", "g", "m", "v")}
    mask = torch.from_numpy(b["mask"]).to(DEV) if b["mask"] is not None else None
    st = T.new_state(step=step)
    st.view(torch.float32)[_lib.ST_VALID] = count
    scratch = torch.empty(4096, device=DEV)
    chp = c_hp(hp, mask)
    _lib.check(lib.b4r_global_sqnorm(P(d["g"]), n, P(scratch), P(st), stream()))
    _lib.check(lib.b4r_adamw_step(C.byref(chp), P(d["p"]), P(d["g"]), P(d["m"]), P(d["v"]), n, b["n_decay"], P(st), stream()))
    torch.cuda.synchronize()
    return {k: d[k].cpu().numpy() for k in ("p", "m", "v")}, st.cpu(), T.state_floats(st)


def load_engine(eng, b, step, count):
    eng.params.copy_(torch.from_numpy(b["p"]))
    eng.grads.copy_(torch.from_numpy(b["g"]))
    eng.adam_m.copy_(torch.from_numpy(b["m"]))
    eng.adam_v.copy_(torch.from_numpy(b["v"]))
    eng.state.zero_()
    eng.set_step(step)
    eng.state.view(torch.float32)[_lib.ST_VALID] = count


def run_fused(eng, cb, b, hp, step, count):
    """b4r_optimizer_step through Engine: one norm launch and adamw_fused_kernel"""
    load_engine(eng, b, step, count)
    mask = torch.from_numpy(b["mask"]).to(DEV) if b["mask"] is not None else None
    eng.optimizer_step(c_hp(hp, mask), cb)
    torch.cuda.synchronize()
    return {"p": eng.params.cpu().numpy(), "m": eng.adam_m.cpu().numpy(), "v": eng.adam_v.cpu().numpy()}, eng.state.cpu(), \
        T.state_floats(eng.state)


def check_step_state(words, f, b, info, hp, step, count):
    """norm (against float64), learning rate (bit for bit TF's), step counter, ticket"""
    g64 = b["g"].astype(np.float64)
    sq = float(np.sum(g64 * g64))
    # every term is non-negative, so the relative error of the fp32 sum is at most (roundings a term passes through) u: product 1, the
    # float4's sum 2, the thread's turns <= 5, wave 6, workgroup 2, the partials' strided turns <= 4 and tree 8 = 28; the norm: half of
    # that, the root, 1 / count and the product with it
    assert abs(float(f[_lib.ST_SQNORM]) - sq) <= 28 * U * sq, (float(f[_lib.ST_SQNORM]), sq)
    assert abs(float(f[_lib.ST_GRAD_NORM]) - info["grad_norm"]) <= 17 * U * info["grad_norm"], (float(f[_lib.ST_GRAD_NORM]), info["grad_norm"])
    want_lr = orc.learning_rate(step, hp)
    assert bits(f[_lib.ST_LR]) == bits(want_lr), (step, float(f[_lib.ST_LR]), float(want_lr))
    if step >= hp.num_train_steps:
        assert bits(f[_lib.ST_LR]) == bits(np.float32(hp.end_lr))
    assert int(words[_lib.ST_STEP:_lib.ST_STEP + 2].view(torch.int64)[0]) == step + 1
    assert int(words[_lib.ST_STEP_LO]) == step + 1
    assert int(words[ST_TICKET]) == 0
    assert float(f[_lib.ST_VALID]) == count


def assert_within(ref, got, groups, d, what):
    bad, worst = R.check_against(ref, got, groups, d)
    print(f"[step-kernels] {what}: worst |kernel - fp64| / d_case per group and array:",
          {f"{g_}/{a}": (f"{w:.3e}", f"{d[(g_, a)]:.3e}") for (g_, a), w in worst.items()})
    assert not bad, (what, bad)
    for a in ("p", "m", "v"):
        assert np.isfinite(got[a]).all(), (what, a)


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_adamw_step_matches_float64(name):
    """adamw_kernel: every cell of the matrix"""
    case = R.CASE_BY_NAME[name]
    b, ref, o32, info, _, d = distances_of(name)
    got, words, f = run_direct(b, case.hp(), case.step, case.count)
    check_step_state(words, f, b, info, case.hp(), case.step, case.count)
    assert_within(ref, got, b["groups"], d, f"adamw_step {name}")


@pytest.mark.parametrize("name", [c.name for c in R.CASES if c.fused])
def test_optimizer_step_matches_float64(name):
    """adamw_fused_kernel: the cells that do not fix n or n_decay (the model's configuration does), on the tiny model's buffers"""
    case = R.CASE_BY_NAME[name]
    eng, cb, _ = tiny_engine()
    b, ref, o32, info, _, d = distances_of(name, eng.n_params, eng.n_decay)
    assert 0 < eng.n_decay < eng.n_params and eng.n_params % 4 == 0
    got, words, f = run_fused(eng, cb, b, case.hp(), case.step, case.count)
    check_step_state(words, f, b, info, case.hp(), case.step, case.count)
    assert_within(ref, got, b["groups"], d, f"optimizer_step {name}")


def test_optimizer_step_second_turn_through_the_loop():
    """adamw_fused_kernel where n / 4 exceeds the 2048 x 256 threads of its largest grid: the prefetched first turn, then the loop's own
    loads (a vocabulary of 33 000 x 64 floats does it; only the optimizer runs on this model)"""
    cfg = make_model_config(33000, 64, 1, 2, 20, 64, 0.1, 0.1)
    eng = Engine(cfg, DEV)
    eng.ensure_training_buffers()
    assert eng.n_params // 4 > 2048 * 256
    cb, keep = eng.prepare_batch(orc.synthetic_batch(2, 16, 4, 37, seed=1))
    case = R.CASE_BY_NAME["size-two-turns"]
    b, ref, o32, info, _, d = distances_of(case.name, eng.n_params, eng.n_decay)
    got, words, f = run_fused(eng, cb, b, case.hp(), case.step, case.count)
    check_step_state(words, f, b, info, case.hp(), case.step, case.count)
    assert_within(ref, got, b["groups"], d, "optimizer_step two turns")


@functools.lru_cache(maxsize=None)
def norm_input(n):
    g = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    return g, float(np.sum(g.astype(np.float64) ** 2))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 4095, R.N_STD, 4 * 1024 * 1024 + 4100 + 3])
def test_global_sqnorm_any_size(n):
    """sqnorm_partial_kernel / sqnorm_final_kernel: no float4 at all, an n % 4 tail (the last workgroup's), the cap of 1024 partial sums
    with more than 1024 float4 per workgroup.  The buffer ends at the end of its allocation: nothing behind n may be read into the sum
    (the floats behind it hold a large value)."""
    lib = _lib.load()
    g, sq = norm_input(n)
    pad = (-n) % 4 + 4
    buf = torch.full((n + pad,), 1.0e6, device=DEV)
    buf[:n] = torch.from_numpy(g)
    st = T.new_state()
    scratch = torch.full((4096,), float("nan"), device=DEV)
    _lib.check(lib.b4r_global_sqnorm(P(buf), n, P(scratch), P(st), stream()))
    got = float(T.state_floats(st)[_lib.ST_SQNORM])
    print(f"[step-kernels] sqnorm n={n}: relative error {abs(got - sq) / sq:.3e}")
    assert abs(got - sq) <= 28 * U * sq, (n, got, sq)     # (the count of roundings: check_step_state)


def run_trajectory(apply_step, read, n, n_decay):
    """20 consecutive steps on one state against the float64 driver, after every step; the bound uses the fp32 oracle's distance after the
    same number of steps"""
    case = R.TRAJECTORY_CASE
    hp = case.hp()
    b = R.make_buffers(case, n, n_decay)
    t64 = R.Trajectory64(b["p"], b["m"], b["v"], hp, 0, b["n_decay"])
    t32 = R.Trajectory32(b["p"], b["m"], b["v"], hp, 0, b["n_decay"])
    ratio = {}
    for k in range(R.TRAJECTORY_STEPS):
        g = R.trajectory_gradient(k, b["n"], case.count)
        info = t64.apply(g, case.count)
        t32.apply(g, case.count)
        apply_step(k, g)
        got, words, f = read()
        bk = dict(b, g=g)
        check_step_state(words, f, bk, info, hp, k, case.count)
        ref = dict(p=t64.p, m=t64.m, v=t64.v)
        d = R.distances(ref, dict(p=t32.p, m=t32.m, v=t32.v), b["groups"])
        bad, worst = R.check_against(ref, got, b["groups"], d)
        for key, w in worst.items():
            ratio[key] = max(ratio.get(key, 0.0), w / d[key] if d[key] > 0 else 0.0)
        if k == R.TRAJECTORY_STEPS - 1:
            print("[step-kernels] trajectory after 20 steps: |kernel - fp64| and d:", {f"{g_}/{a}": (f"{w:.3e}", f"{d[(g_, a)]:.3e}")
                                                                                       for (g_, a), w in worst.items()})
        assert not bad, (k, bad)
    print("[step-kernels] trajectory: largest |kernel - fp64| / d_case over the steps:", {f"{g_}/{a}": f"{r:.2f}" for (g_, a), r in ratio.items()})
    assert state_step_words(read()[1]) == R.TRAJECTORY_STEPS
    return b


def state_step_words(words) -> int:
    return int(words[_lib.ST_STEP:_lib.ST_STEP + 2].view(torch.int64)[0])


def test_adamw_step_trajectory():
    lib = _lib.load()
    case = R.TRAJECTORY_CASE
    b0 = R.make_buffers(case)
    n = b0["n"]
    d = {k: torch.from_numpy(b0[k]).to(DEV) for k in ("p", "m", "v")}
    gd = torch.empty(n, device=DEV)
    st = T.new_state(step=0)
    scratch = torch.empty(4096, device=DEV)
    chp = c_hp(case.hp())

    def apply_step(k, g):
        gd.copy_(torch.from_numpy(g))
        # what a step leaves in the state before the optimizer runs: the count (the loss reduction's)
        st.view(torch.float32)[_lib.ST_VALID] = case.count
        _lib.check(lib.b4r_global_sqnorm(P(gd), n, P(scratch), P(st), stream()))
        _lib.check(lib.b4r_adamw_step(C.byref(chp), P(d["p"]), P(gd), P(d["m"]), P(d["v"]), n, b0["n_decay"], P(st), stream()))

    def read():
        torch.cuda.synchronize()
        return {k: d[k].cpu().numpy() for k in ("p", "m", "v")}, st.cpu(), T.state_floats(st)

    run_trajectory(apply_step, read, None, None)


def test_optimizer_step_trajectory():
    eng, cb, _ = tiny_engine()
    case = R.TRAJECTORY_CASE
    b0 = R.make_buffers(case, eng.n_params, eng.n_decay)
    load_engine(eng, b0, 0, case.count)
    chp = c_hp(case.hp())

    def apply_step(k, g):
        eng.grads.copy_(torch.from_numpy(g))
        eng.optimizer_step(chp, cb)

    def read():
        torch.cuda.synchronize()
        return {"p": eng.params.cpu().numpy(), "m": eng.adam_m.cpu().numpy(), "v": eng.adam_v.cpu().numpy()}, eng.state.cpu(), \
            T.state_floats(eng.state)

    run_trajectory(apply_step, read, eng.n_params, eng.n_decay)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("fused", [False, True], ids=["adamw_step", "optimizer_step"])
def test_non_finite_gradient_is_never_dropped(bad, fused):
    """One non-finite element in the gradient (include/b4r.h, b4r_optimizer_step): the reported norm is non-finite and that element's
    parameter and moments are NaN afterwards.  The rest of the buffer:
      Inf -> the clip scale is clip / Inf = 0: every finite gradient counts as 0 (the moments decay, the parameters take the step of an
             all-zero gradient)
      NaN -> fmaxf(NaN, clip) = clip, the scale is 1: the finite elements take the UNCLIPPED step of their own gradients
    (tf.clip_by_global_norm turns every gradient into NaN in the second case; the kernels keep the damage to the element and to the
    reported norm, which is what a caller has to watch).  Nothing here faults: the kernels only compute on the values."""
    case = R.Case("non-finite", norm_ratio=2.0, seed=80)       # the finite part alone would be clipped
    hp = case.hp()
    if fused:
        eng, cb, _ = tiny_engine()
        b = R.make_buffers(case, eng.n_params, eng.n_decay)
    else:
        b = R.make_buffers(case)
    k = 1234
    twin = dict(b, g=b["g"].copy())
    if bad == float("inf"):
        twin["g"][:] = 0.0
        twin_hp = hp
    else:
        twin["g"][k] = 0.0
        twin_hp = R.with_hp(hp, gradient_clip_norm=0.0)
    b = dict(b, g=b["g"].copy())
    b["g"][k] = bad
    ref = dict(zip("pmv", R.adamw_apply64(twin["p"], twin["g"], twin["m"], twin["v"], case.step, twin_hp, case.count, b["n_decay"])[:3]))
    o32 = dict(zip("pmv", R.adamw_apply32(twin["p"], twin["g"], twin["m"], twin["v"], case.step, twin_hp, case.count, b["n_decay"])[:3]))
    rest = np.ones(b["n"], dtype=bool)
    rest[k] = False
    groups = {name: sel & rest for name, sel in b["groups"].items()}
    d = R.distances(ref, o32, groups)
    got, words, f = run_fused(eng, cb, b, hp, case.step, case.count) if fused else run_direct(b, hp, case.step, case.count)
    assert not np.isfinite(float(f[_lib.ST_GRAD_NORM])) and not np.isfinite(float(f[_lib.ST_SQNORM]))
    assert np.isnan(got["p"][k]) and np.isnan(got["m"][k]) and np.isnan(got["v"][k])
    bad_, worst = R.check_against(ref, got, groups, d)
    assert not bad_, bad_
    assert all(np.isfinite(got[a][rest]).all() for a in "pmv")
    assert state_step_words(words) == case.step + 1 and int(words[ST_TICKET]) == 0
    assert bits(f[_lib.ST_LR]) == bits(orc.learning_rate(case.step, hp))


# ======================================================================================================================================
# b. b4r_softmax_ce
# ======================================================================================================================================
def run_ce(logits, V, ld, y, want_grad=1, st=None, begin=True, fill=7.0):
    """logits [M, V] (CPU) in a [M, ld] device buffer whose padding columns hold `fill`; returns the buffer after the call (CPU), the
    per-row scalars [M, 4], the state floats and the state"""
    lib = _lib.load()
    M = logits.shape[0]
    buf = torch.full((M, ld), fill)
    buf[:, :V] = logits
    bd = buf.to(DEV)
    st = T.new_state() if st is None else st
    rows = torch.full((4 * M,), float("nan"), device=DEV)
    yd = y.to(DEV)
    if begin:
        _lib.check(lib.b4r_state_begin_step(P(st), stream()))
    _lib.check(lib.b4r_softmax_ce(P(bd), M, V, ld, P(yd), P(rows), P(st), want_grad, stream()))
    torch.cuda.synchronize()
    return bd.cpu(), rows.cpu().view(M, 4), T.state_floats(st), st


def ce_reference(logits, y):
    """float64 logsumexp / autograd: per-row loss (0 for ignored slots), gradient of the loss sum, first-index argmax"""
    M = logits.shape[0]
    lr = logits.double().requires_grad_(True)
    valid = y != 0
    per = (torch.logsumexp(lr, -1) - lr[torch.arange(M), y]) * valid
    per.sum().backward()
    pred = torch.from_numpy(np.argmax(logits.numpy(), axis=-1))     # numpy: the FIRST index of the maximum, as tf.argmax
    return per.detach(), lr.grad, pred, valid


def loss_bound(logits):
    """per row: 4 ulp_fp32 of the largest magnitude among the logits and their log-sum-exp (the cancellation in lse - y_logit) + 1e-6 (the
    fast log near 1)"""
    big = torch.maximum(logits.double().abs().max(-1).values, torch.logsumexp(logits.double(), -1).abs())
    return 4.0 * torch.from_numpy(R.ulp32(big.numpy())) + 1e-6


@pytest.mark.parametrize("M,V,ld", [(1, 4, 4), (5, 33, 36), (3, 1023, 1024), (3, 1024, 1024), (3, 1025, 1028), (4095, 8, 8), (4096, 8, 8),
                                    (4097, 8, 8), (8193, 8, 8), (64, 3709, 3712)])
def test_softmax_ce_shapes(M, V, ld):
    """one float4 for 256 threads, a last float4 that is half padding, one column past a full turn of the workgroup, and row counts around
    the 16 x 256 rows one pass of loss_rows_reduce covers.  Bounds of test_gpu_ops.py::test_softmax_cross_entropy_and_metrics."""
    logits = rnd(M, V, seed=31 + V, scale=2.0)
    y = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(5 + M))
    y[::4] = 0
    y[M - 1] = int(logits[M - 1].argmax())        # the LAST row counts: a reduction that stops early loses it
    if y[M - 1] == 0:
        logits[M - 1, 1] = logits[M - 1].max() + 1.0
        y[M - 1] = 1
    if M > 2:
        y[1] = int(logits[1].argmax())
    per, grad, pred, valid = ce_reference(logits, y)
    out, rows, f, _ = run_ce(logits, V, ld, y)
    loss_sum = float(per.sum())
    assert abs(float(f[_lib.ST_LOSS_SUM]) - loss_sum) < 1e-3 * max(1.0, loss_sum) * 1e-2 + 1e-3
    assert float(f[_lib.ST_VALID]) == float(valid.sum())
    assert float(f[_lib.ST_CORRECT_MASKED]) == float(((pred == y) & valid).sum())
    assert float(f[_lib.ST_CORRECT_ALL]) == float((pred == y).sum())
    assert float(f[_lib.ST_SLOTS_ALL]) == M
    assert torch.equal(rows[:, 1], valid.float())
    assert torch.equal(rows[:, 2], ((pred == y) & valid).float()) and torch.equal(rows[:, 3], (pred == y).float())
    assert bool(((rows[:, 0].double() - per).abs() <= loss_bound(logits)).all())
    assert T.maxdiff(out[:, :V], grad) < 2e-6
    if ld > V:
        assert float(out[:, V:].abs().max()) == 0.0


def test_softmax_ce_confident_and_shifted_rows():
    """Logits of scale 30; the same row shifted by +1e4 and by -1e4 (exactly: the row is a multiple of 2^-8, ulp(1e4) is 2^-10); a row
    whose label holds all the mass and one whose label holds nearly all.  Per-row loss within 4 ulp_fp32(max |logit|) + 1e-6 of float64
    (the cancellation in lse - y_logit; the fast log near 1), gradient within 2e-6."""
    M, V, ld = 8, 3709, 3712
    logits = rnd(M, V, seed=77, scale=30.0)
    logits[0] = torch.round(logits[0] * 256.0) / 256.0
    logits[1] = logits[0] + 1.0e4
    logits[2] = logits[0] - 1.0e4
    assert torch.equal((logits[1] - 1.0e4), logits[0]) and torch.equal((logits[2] + 1.0e4), logits[0])
    y = torch.randint(1, V, (M,), generator=torch.Generator().manual_seed(78))
    y[1] = y[2] = y[0]
    logits[3] = rnd(V, seed=79)
    logits[3, y[3]] = 50.0
    logits[4] = rnd(V, seed=80)
    logits[4, y[4]] = 12.0
    y[5] = int(logits[5].argmax())
    per, grad, pred, valid = ce_reference(logits, y)
    out, rows, f, _ = run_ce(logits, V, ld, y)
    bound = loss_bound(logits)
    err = (rows[:, 0].double() - per).abs()
    print("[step-kernels] softmax_ce confident rows: loss error / bound per row:", [(f"{float(e):.2e}", f"{float(b_):.2e}") for e, b_ in zip(err, bound)])
    gerr = T.maxdiff(out[:, :V], grad)
    print(f"[step-kernels] softmax_ce confident rows: gradient error {gerr:.3e}")
    assert bool((err <= bound).all()), (err, bound)
    assert gerr < 2e-6
    # shift invariance between the kernel's own rows
    for r in (1, 2):
        assert abs(float(rows[r, 0]) - float(rows[0, 0])) <= float(bound[r])
        assert T.maxdiff(out[r, :V], out[0, :V]) < 2e-6
    assert float(per[3]) < 1e-12 and float(rows[3, 0]) <= 1e-6
    assert torch.equal(rows[:, 2], (pred == y).float()) and torch.equal(rows[:, 3], (pred == y).float())
    assert float(out[:, V:].abs().max()) == 0.0


# the maximum planted at two columns: (lower, higher).  Thread t of the 256 owns columns 4t .. 4t + 3 and, a turn later, those + 1024.
TIE_PAIRS = [(5, 6),          # one float4
             (5, 1029),       # one thread's successive turns (c and c + 1024)
             (5, 41),         # two lanes of one wave
             (5, 261),        # two waves
             (8, 1029),       # the lower column in the HIGHER lane (lane 2's first turn, lane 1's second)
             (300, 1029),     # the lower column in the higher wave
             (2047, 2050)]    # the last full float4 and the last, half padded one


def test_softmax_ce_exact_ties_take_the_first_index():
    """tf.argmax / SparseCategoricalAccuracy: the FIRST index of the maximum.  Each pair runs with y = the lower column (correct) and with
    y = the higher one (not correct); an all-equal row predicts column 0."""
    V, ld = 2051, 2052
    rows_y = []
    for lo, hi in TIE_PAIRS:
        rows_y += [(lo, hi, lo), (lo, hi, hi)]
    M = len(rows_y) + 3
    logits = rnd(M, V, seed=90, scale=2.0)
    y = torch.zeros(M, dtype=torch.int64)
    for r, (lo, hi, yy) in enumerate(rows_y):
        logits[r, lo] = 9.0
        logits[r, hi] = 9.0
        y[r] = yy
    eq = len(rows_y)
    logits[eq:eq + 3] = 1.25
    y[eq], y[eq + 1], y[eq + 2] = 0, 3, V - 1     # predicted 0 == the ignore label: counts in correct_all only; other labels: wrong
    per, grad, pred, valid = ce_reference(logits, y)
    assert pred[:eq].tolist() == [lo for lo, _, _ in rows_y] and pred[eq:].tolist() == [0, 0, 0]
    out, rows, f, _ = run_ce(logits, V, ld, y)
    want_all = (pred == y).float()
    want_masked = ((pred == y) & valid).float()
    assert want_all[:eq].tolist() == [1.0, 0.0] * len(TIE_PAIRS) and want_all[eq:].tolist() == [1.0, 0.0, 0.0]
    assert want_masked[eq:].tolist() == [0.0, 0.0, 0.0]
    assert torch.equal(rows[:, 3], want_all), rows[:, 3]
    assert torch.equal(rows[:, 2], want_masked), rows[:, 2]
    assert torch.equal(rows[:, 1], valid.float())
    assert float(f[_lib.ST_CORRECT_ALL]) == float(want_all.sum()) and float(f[_lib.ST_CORRECT_MASKED]) == float(want_masked.sum())
    assert float(f[_lib.ST_VALID]) == float(valid.sum())
    assert bool(((rows[:, 0].double() - per).abs() <= loss_bound(logits)).all()) and T.maxdiff(out[:, :V], grad) < 2e-6


def test_softmax_ce_state_adds_until_told_to_overwrite():
    lib = _lib.load()
    M, V, ld = 4099, 8, 8          # more rows than one pass of the reduction
    logits = rnd(M, V, seed=95, scale=2.0)
    y = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(96))
    _, rows1, f1, st = run_ce(logits, V, ld, y, want_grad=0)
    one = [float(f1[i]) for i in (_lib.ST_LOSS_SUM, _lib.ST_VALID, _lib.ST_CORRECT_MASKED, _lib.ST_CORRECT_ALL, _lib.ST_SLOTS_ALL)]
    assert one[4] == M and one[1] == float((y != 0).sum())
    # a second call without b4r_state_begin_step adds (the same rows in the same order: exactly twice the sums)
    _, _, f2, st = run_ce(logits, V, ld, y, want_grad=0, st=st, begin=False)
    two = [float(f2[i]) for i in (_lib.ST_LOSS_SUM, _lib.ST_VALID, _lib.ST_CORRECT_MASKED, _lib.ST_CORRECT_ALL, _lib.ST_SLOTS_ALL)]
    assert two == [2.0 * x for x in one]
    # want_grad | B4R_LOSS_OVERWRITE on a state full of garbage: the sums are SET, the gradient norms zeroed, seed and step kept
    st = T.new_state(seed=77, step=9)
    fl = st.view(torch.float32)
    for i in range(_lib.ST_LOSS_SUM, _lib.ST_LR):
        fl[i] = float("nan") if i % 2 else 1.0e30
    fl[_lib.ST_LR] = 0.125
    out, rows3, f3, st = run_ce(logits, V, ld, y, want_grad=1 | 4, st=st, begin=False)
    three = [float(f3[i]) for i in (_lib.ST_LOSS_SUM, _lib.ST_VALID, _lib.ST_CORRECT_MASKED, _lib.ST_CORRECT_ALL, _lib.ST_SLOTS_ALL)]
    assert three == one
    assert float(f3[_lib.ST_SQNORM]) == 0.0 and float(f3[_lib.ST_GRAD_NORM]) == 0.0 and float(f3[_lib.ST_LR]) == 0.125
    assert int(st.cpu()[_lib.ST_SEED]) == 77 and state_step(st) == 9
    assert torch.equal(rows3, rows1)
    per, grad, pred, valid = ce_reference(logits, y)
    assert T.maxdiff(out, grad) < 2e-6            # the overwrite bit does not switch the gradient off


# ======================================================================================================================================
# c. the logits-free head: argmax ties across tiles and vocabulary slices
# ======================================================================================================================================
def head_fwd_slices(M, V, H):
    """h32_slices of b4r_head32.hip for the forward sweep (own rows = M, swept = V, at most 16 slices, about one workgroup per CU of
    256): (slices, 32-row tiles per slice)"""
    rows_wg = 128 if H == 256 else 256
    blocks, tiles = -(-M // rows_wg), -(-V // 32)
    s = max(1, min(16, 256 // blocks, tiles))
    slices = -(-tiles // (-(-tiles // s)))
    return slices, -(-tiles // slices)


def head_tie_setup():
    H, M = 64, 40
    # the smallest vocabulary whose forward has a slice of two tiles AND a second slice: 16 slices of one tile up to 512 ids, then
    # 17 tiles in slices of two
    V = next(v for v in range(33, 4096) if head_fwd_slices(M, v, H)[1] >= 2 and head_fwd_slices(M, v, H)[0] >= 2)
    slices, per = head_fwd_slices(M, V, H)
    return H, M, V, 32 * per


def _head_pairs():
    H, M, V, w = head_tie_setup()
    return [(1, 9), (2, 5), (5, 9), (31, 32), (w - 1, w)]


@pytest.mark.parametrize("pair_index", range(5), ids=["tile-one-lane", "tile-two-lanes", "tile-lower-id-in-upper-lane", "tiles-31-32",
                                                      "slice-boundary"])
@pytest.mark.parametrize("label", ["lower", "higher"])
def test_fused_head_exact_ties_take_the_first_index(pair_index, label):
    """b4r_mlm_head_fused_fwd's best-logit merge (per lane inside a tile, across a lane's tiles, between the two lanes of a row, across the
    vocabulary slices in head_merge_row): two ids with the SAME table row and bias are the maximum of every row; the lower id must win,
    so y = lower counts as correct and y = higher does not.  The setup of test_gpu_ops.py::test_fused_mlm_head_matches_materialised_math
    at H = 64, M = 40, V = 513 (17 tiles: slices of two tiles, so that a tile boundary inside a slice (31 | 32) and a slice boundary
    (63 | 64) both exist).  A logit is the same sum of the same products wherever its column sits in a tile, so the pair is bit-equal on
    the device; the float64 logits of the two ids are equal by construction."""
    lib = _lib.load()
    H, M, V, width = head_tie_setup()
    assert (V, width) == (513, 64)
    cfg = make_model_config(V, H, 2, 2, 50, 256, 0.1, 0.1)
    if not lib.b4r_fused_head_supported(C.byref(cfg)):
        pytest.skip("the logits-free head does not run in this arithmetic mode")
    lo, hi = _head_pairs()[pair_index]
    T_, E_, b_ = rnd(M, H, seed=41, scale=1.5), rnd(V, H, seed=42, scale=0.1), rnd(V, seed=43, scale=0.5)
    E_[hi] = E_[lo]
    b_[lo] = b_[hi] = 12.0
    y = torch.full((M,), lo if label == "lower" else hi, dtype=torch.int64)
    y[::5] = 0                                            # ignored slots
    y[3] = 7 if 7 not in (lo, hi) else 11                 # a label that is not the prediction
    logits = T_.double() @ E_.double().T + b_.double()
    assert torch.equal(logits[:, lo], logits[:, hi])
    others = logits.clone()
    others[:, [lo, hi]] = -1e30
    assert float((logits[:, lo] - others.max(-1).values).min()) > 1.0     # the pair is every row's maximum, by a margin no rounding closes
    Td, Ed, bd, yd = T_.to(DEV), E_.to(DEV), b_.to(DEV), y.to(DEV)
    scratch = torch.empty(lib.b4r_mlm_head_fused_scratch_floats(M, V, H), device=DEV)
    dT = torch.full((M, H), float("nan"), device=DEV)
    rows = torch.full((4 * M,), float("nan"), device=DEV)
    lse = torch.empty(M, device=DEV)
    lab = torch.empty(M, dtype=torch.int32, device=DEV)
    _lib.check(lib.b4r_mlm_head_fused_fwd(P(Td), P(Ed), P(bd), P(yd), M, V, H, P(scratch), P(dT), P(rows), P(lse), P(lab), 0, stream()))
    torch.cuda.synchronize()
    valid = y != 0
    per = torch.logsumexp(logits, -1) - logits[torch.arange(M), y]
    r = rows.cpu().view(M, 4)
    pred = torch.full((M,), lo, dtype=torch.int64)        # first index of the maximum
    assert torch.equal(r[:, 1], valid.float())
    assert torch.equal(r[:, 3], (pred == y).float()), (lo, hi, r[:, 3])
    assert torch.equal(r[:, 2], ((pred == y) & valid).float()), (lo, hi, r[:, 2])
    assert float(r[:, 3].sum()) == (float(valid.sum()) - 1.0 if label == "lower" else 0.0)
    assert T.maxdiff(r[:, 0], (per * valid)) < 2e-4
    assert T.maxdiff(lse.cpu()[valid], torch.logsumexp(logits, -1)[valid]) < 2e-4 and bool(torch.isinf(lse.cpu()[~valid]).all())
    assert torch.equal(lab.cpu().long(), torch.where(valid, y, torch.full_like(y, -1)))


# ======================================================================================================================================
# d. b4r_gather_rows / b4r_scatter_add_rows
# ======================================================================================================================================
GROUP_L, GROUP_P = 10, 7     # idx_add_per = L (rows per group of the source), per = P (index entries per group)


def row_indices(n, grouped, seed):
    """idx [n] and the rows they name: plain row numbers (idx_add_per = 0), or positions inside groups of GROUP_L rows, GROUP_P entries per
    group, with positions below 0 and at or above L that clamp into the group; every fourth entry repeats its neighbour (duplicates)"""
    g = torch.Generator().manual_seed(seed)
    if grouped:
        groups = -(-n // GROUP_P)
        idx = torch.randint(-3, GROUP_L + 3, (n,), generator=g)
        idx[1::4] = idx[0::4][: idx[1::4].numel()]
        rows = idx.clamp(0, GROUP_L - 1) + (torch.arange(n) // GROUP_P) * GROUP_L
        return idx, rows, groups * GROUP_L
    n_rows = max(3, n // 3)
    idx = torch.randint(0, n_rows, (n,), generator=g)
    idx[1::4] = idx[0::4][: idx[1::4].numel()]
    return idx, idx.clone(), n_rows


@pytest.mark.parametrize("grouped", [False, True], ids=["rows", "groups"])
@pytest.mark.parametrize("n", [1, 257, 5000])
@pytest.mark.parametrize("H", [4, 64, 1024])
def test_gather_rows(H, n, grouped):
    lib = _lib.load()
    idx, rows, n_rows = row_indices(n, grouped, seed=H + n)
    assert int(rows.min()) >= 0 and int(rows.max()) < n_rows
    src_ld = H + 8
    src = torch.randn(n_rows, src_ld, device=DEV)
    dst = torch.full((n + 1, H), float("nan"), device=DEV)     # one guard row behind the n the call may write
    idx_d = idx.to(DEV)
    _lib.check(lib.b4r_gather_rows(P(src), src_ld, P(idx_d), GROUP_L if grouped else 0, GROUP_P if grouped else 1, n, H, P(dst), stream()))
    want = src[rows.to(DEV), :H]
    assert torch.equal(dst[:n], want)
    assert bool(torch.isnan(dst[n]).all())
    if grouped:
        assert int((idx < 0).sum()) > 0 or n == 1
        assert int((idx >= GROUP_L).sum()) > 0 or n == 1


@pytest.mark.parametrize("grouped", [False, True], ids=["rows", "groups"])
@pytest.mark.parametrize("n", [1, 257, 5000])
@pytest.mark.parametrize("H", [4, 64, 1024])
def test_scatter_add_rows(H, n, grouped):
    """dst[row(i), :H] += src[i, :] for the entries whose skip word is not 0, in fp32 atomics: against the float64 sum, within
    n_dup ulp (each of a destination element's n_dup additions rounds at most half an ulp of a partial sum, none of which exceeds
    |dst| + sum |src|); rows that receive nothing and the gap columns of dst (dst_ld > H) keep their bits."""
    lib = _lib.load()
    idx, rows, n_rows = row_indices(n, grouped, seed=2 * H + n)
    assert int(rows.min()) >= 0 and int(rows.max()) < n_rows
    dst_ld = H + 4
    g = torch.Generator().manual_seed(n + H)
    skip = (torch.rand(n, generator=g) < 0.8).to(torch.int64)
    if n == 1:
        skip[0] = 1
    src = torch.randn(n, H, device=DEV)
    dst0 = torch.randn(n_rows + 1, dst_ld, device=DEV)          # one guard row
    dst = dst0.clone()
    idx_d, skip_d, rows_d = idx.to(DEV), skip.to(DEV), rows.to(DEV)
    _lib.check(lib.b4r_scatter_add_rows(P(src), P(idx_d), GROUP_L if grouped else 0, GROUP_P if grouped else 1, n, H, P(dst), dst_ld,
                                        P(skip_d), stream()))
    live = skip_d != 0
    want = dst0[:, :H].double().index_add(0, rows_d[live], src[live].double())
    mag = dst0[:, :H].double().abs().index_add(0, rows_d[live], src[live].double().abs())
    n_dup = torch.zeros(n_rows + 1, dtype=torch.float64, device=DEV).index_add(0, rows_d[live], torch.ones(int(live.sum()), dtype=torch.float64, device=DEV))
    assert n == 1 or float(n_dup.max()) >= 2
    ulp = torch.from_numpy(R.ulp32(mag.cpu().numpy()))
    err = (dst[:, :H].double() - want).abs().cpu()
    assert bool((err <= n_dup.cpu()[:, None] * ulp).all()), float((err / ulp).max())
    untouched = (n_dup == 0)
    assert torch.equal(dst[untouched], dst0[untouched])          # rows that receive nothing, the guard row and skipped entries' rows
    assert torch.equal(dst[:, H:], dst0[:, H:])                  # the gap columns
    # without the skip list every entry lands
    dst2 = dst0.clone()
    _lib.check(lib.b4r_scatter_add_rows(P(src), P(idx_d), GROUP_L if grouped else 0, GROUP_P if grouped else 1, n, H, P(dst2), dst_ld,
                                        None, stream()))
    want2 = dst0[:, :H].double().index_add(0, rows_d, src.double())
    mag2 = dst0[:, :H].double().abs().index_add(0, rows_d, src.double().abs())
    dup2 = torch.zeros(n_rows + 1, dtype=torch.float64, device=DEV).index_add(0, rows_d, torch.ones(n, dtype=torch.float64, device=DEV))
    err2 = (dst2[:, :H].double() - want2).abs().cpu()
    assert bool((err2 <= dup2.cpu()[:, None] * torch.from_numpy(R.ulp32(mag2.cpu().numpy()))).all())
    assert torch.equal(dst2[:, H:], dst0[:, H:])
