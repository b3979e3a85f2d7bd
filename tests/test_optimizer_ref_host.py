"""The optimizer reference itself (CPU): the float64 restatement of AdamWeightDecay.apply_gradients (tests/optimizer_ref.py) against the
hand-computed updates of tests/test_oracle.py, and the fp32 oracle (orc.adamw_apply) against it on every cell of the matrix that the
GPU tests run -- the fp32-vs-fp64 distance d_case their tolerance is built from (tests/test_gpu_step_kernels.py)."""
import math

import numpy as np
import pytest

from oracle import bert4rec_oracle as orc
from tests import optimizer_ref as R

U = 2.0 ** -24   # float32 unit roundoff


def test_float64_restatement_reproduces_the_hand_computed_updates():
    """the three facts of test_oracle.py::test_adamw_update_formula_and_decay_selection, on flat buffers"""
    hp = orc.AdamWConfig(num_warmup_steps=0)
    # a/kernel (2, decays), a/bias, LayerNorm/gamma, layer_norm/beta (3, do not), word_embeddings/embeddings (1, decays): as a byte mask
    p0 = np.array([1.0, -2.0, 0.5, 1.0, 0.1, 0.3])
    mask = np.array([1, 1, 0, 0, 0, 1], dtype=np.uint8)
    g = np.full(6, 0.1)
    z = np.zeros(6)
    p, m, v, info = R.adamw_apply64(p0, g, z, z, 0, hp, decay_mask=mask)
    assert info["grad_norm"] == pytest.approx(0.1 * math.sqrt(6), rel=1e-12) and info["clip_scale"] == 1.0   # below the clip norm 5
    lr = float(orc.learning_rate(0, hp))
    alpha = lr * math.sqrt(1 - R.f32(0.999)) / (1 - R.f32(0.9))
    mm, vv = 0.1 * (1 - R.f32(0.9)), 0.01 * (1 - R.f32(0.999))
    for i in range(6):
        dec = lr * R.f32(0.01) * p0[i] if mask[i] else 0.0
        assert p[i] == pytest.approx(p0[i] - dec - mm * alpha / (math.sqrt(vv) + R.f32(1e-6)), rel=1e-13), i
    # the same numbers as test_oracle.py writes them (float32 hyper-parameters read as decimals: 1e-5 relative)
    for i in range(6):
        dec = lr * 0.01 * p0[i] if mask[i] else 0.0
        assert p[i] == pytest.approx(p0[i] - dec - 0.01 * (lr * math.sqrt(0.001) / 0.1) / (math.sqrt(1e-5) + 1e-6), rel=1e-5), i
    # the same selection by n_decay when the decayed elements come first
    order = np.array([0, 1, 5, 2, 3, 4])
    p2, _, _, _ = R.adamw_apply64(p0[order], g, z, z, 0, hp, n_decay=3)
    assert np.array_equal(p2, p[order])
    # clip_by_global_norm: scale = clip / max(norm, clip)
    _, m3, _, info3 = R.adamw_apply64(p0, np.full(6, 100.0), z, z, 0, hp, decay_mask=mask)
    assert info3["grad_norm"] == pytest.approx(100.0 * math.sqrt(6), rel=1e-12)
    assert m3[2] == pytest.approx((1 - R.f32(0.9)) * 100.0 * 5.0 / info3["grad_norm"], rel=1e-13)
    # division by the count comes before the norm
    _, m4, _, info4 = R.adamw_apply64(p0, np.full(6, 700.0), z, z, 0, hp, valid_count=7.0, decay_mask=mask)
    assert info4["grad_norm"] == pytest.approx(info3["grad_norm"], rel=1e-12) and m4[2] == pytest.approx(m3[2], rel=1e-12)


def test_non_finite_norms_in_the_restatement():
    """what tf.clip_by_global_norm does with them: an Inf norm scales every finite gradient to 0 (and the Inf one to NaN), a NaN norm
    leaves nothing finite"""
    hp = orc.AdamWConfig(num_warmup_steps=0)
    p0, z = np.ones(4), np.zeros(4)
    p, m, v, info = R.adamw_apply64(p0, np.array([1.0, np.inf, 2.0, 3.0]), z, z, 0, hp)
    assert info["grad_norm"] == np.inf and info["clip_scale"] == 0.0
    assert np.isnan(p[1]) and np.isfinite(p[[0, 2, 3]]).all() and (m[[0, 2, 3]] == 0).all()
    p, m, v, info = R.adamw_apply64(p0, np.array([1.0, np.nan, 2.0, 3.0]), z, z, 0, hp)
    assert np.isnan(info["grad_norm"]) and np.isnan(p).all()


def _stated_bounds(b, ref, info, case):
    """How far the fp32 oracle may be from fp64, element by element (u = 2^-24, ulp = 2 u |x|):
      g_c, the clipped mean gradient, carries the division, the norm's sum and square root, the scale's division and product: 8 u |g_c|
      m' = m + (g_c - m)(1 - b1):  3 roundings of terms bounded by |m| + |g_c|, the last at ulp(m')/2
      v' likewise with g_c^2 (relative error 17 u)
      p' = p - decay - upd: upd = m' alpha / (sqrt(v') + eps) inherits the relative errors of m', of v' (halved by the root; v' and eps
      are both non-negative), of alpha and 6 u of its own operations; p and p' are rounded at ulp / 2 each.
      alpha = lr sqrt(1 - b2^t) / (1 - b1^t): the powers are good to 2 u, but 1 - b^t CANCELS for small t (1 - 0.999^5 = 0.005), which
      magnifies that by b^t / (1 - b^t) -- 400 u at t = 5, halved by the root.  Every fp32 evaluation has this term."""
    hp = case.hp()
    g = b["g"].astype(np.float64) / case.count * info["clip_scale"]
    b1, b2 = R.f32(hp.beta_1), R.f32(hp.beta_2)
    m0, v0, p0 = (b[k].astype(np.float64) for k in ("m", "v", "p"))
    dm = 4 * U * (np.abs(m0) + np.abs(g)) + 8 * U * np.abs(g) * (1 - b1) + R.ulp32(ref["m"])
    dv = 4 * U * (v0 + g * g) + 17 * U * g * g * (1 - b2) + R.ulp32(ref["v"])
    lr = float(info["lr"])
    upd = np.abs(ref["p"] - np.where(R.decay_selection(b["n"], b["n_decay"], b["mask"]), p0 - lr * p0 * R.f32(hp.weight_decay_rate), p0))
    t = float(case.step + 1)
    rel_alpha = U * (b2 ** t / (1 - b2 ** t) + 2 * b1 ** t / (1 - b1 ** t) + 4)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ref["m"] != 0, dm / np.abs(ref["m"]), 0.0) + np.where(ref["v"] != 0, 0.5 * dv / ref["v"], 0.0) + rel_alpha + 6 * U
    dp = upd * rel + 4 * U * lr * np.abs(p0) * R.f32(hp.weight_decay_rate) + R.ulp32(p0) + R.ulp32(ref["p"])
    return dict(p=dp, m=dm, v=dv)


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_fp32_oracle_stays_near_the_float64_restatement(case):
    b, ref, o32, info, gnorm32, d = R.case_distances(case)
    assert float(info["lr"]) == float(orc.learning_rate(case.step, case.hp()))
    assert gnorm32 == pytest.approx(info["grad_norm"], rel=64 * U, abs=1e-30)     # torch's fp32 sum of n squares, then one root
    bounds = _stated_bounds(b, ref, info, case)
    for a in ("p", "m", "v"):
        diff = np.abs(o32[a].astype(np.float64) - ref[a])
        worst = int(np.argmax(diff - bounds[a]))
        assert (diff <= bounds[a]).all(), (a, worst, diff[worst], bounds[a][worst])
        assert np.isfinite(ref[a]).all()
    # d_case is a distance of rounding size: never more than a few ulp of the largest element of the array
    for (gname, a), dist in d.items():
        assert dist <= 64 * U * max(float(np.abs(ref[a]).max()), float(np.abs(b[a]).max())) + 1e-30, (gname, a, dist)


def test_trajectory_drivers_carry_state_and_step():
    case = R.TRAJECTORY_CASE
    b = R.make_buffers(case)
    hp = case.hp()
    t64 = R.Trajectory64(b["p"], b["m"], b["v"], hp, 0, b["n_decay"])
    t32 = R.Trajectory32(b["p"], b["m"], b["v"], hp, 0, b["n_decay"])
    clipped = 0
    for k in range(R.TRAJECTORY_STEPS):
        g = R.trajectory_gradient(k, b["n"], case.count)
        info = t64.apply(g, case.count)
        t32.apply(g, case.count)
        assert info["grad_norm"] == pytest.approx(R.TRAJECTORY_RATIOS[k] * 5.0, rel=1e-6)
        assert float(info["lr"]) == float(orc.learning_rate(k, hp))
        clipped += info["clip_scale"] < 1.0
        # step k of the driver is one single step from the state before it
    assert t64.step == t32.step == R.TRAJECTORY_STEPS and 5 <= clipped <= 15
    p1, m1, v1, _ = R.adamw_apply64(b["p"], R.trajectory_gradient(0, b["n"], case.count), b["m"], b["v"], 0, hp, case.count, b["n_decay"])
    t = R.Trajectory64(b["p"], b["m"], b["v"], hp, 0, b["n_decay"])
    t.apply(R.trajectory_gradient(0, b["n"], case.count), case.count)
    assert np.array_equal(t.p, p1) and np.array_equal(t.m, m1) and np.array_equal(t.v, v1)
    # 20 steps of fp32 noise stay of rounding size (the learning rate is 1e-4: the parameters move by ~1e-3 in all)
    assert float(np.abs(t32.p - t64.p).max()) < 1e-5 and float(np.abs(t32.m - t64.m).max()) < 1e-6


def test_mutations_of_the_update_are_far_outside_the_tolerance():
    """t = step instead of step + 1, and a decay boundary off by one, move the result by far more than 4 d_case + 1 ulp: the GPU tests
    that use this bound see them"""
    case = R.CASE_BY_NAME["decay-3001"]
    b, ref, o32, info, _, d = R.case_distances(case)
    hp = case.hp()
    # t = step: alpha changes by tens of percent at step 4
    lr = float(info["lr"])
    b1, b2 = R.f32(hp.beta_1), R.f32(hp.beta_2)
    a_good = lr * math.sqrt(1 - b2 ** 5) / (1 - b1 ** 5)
    a_bad = lr * math.sqrt(1 - b2 ** 4) / (1 - b1 ** 4)
    upd = (ref["m"] * a_good) / (np.sqrt(ref["v"]) + R.f32(hp.epsilon))
    p_bad = ref["p"] + upd - upd * (a_bad / a_good)
    bad, _ = R.check_against(dict(ref, p=ref["p"]), dict(p=p_bad, m=ref["m"], v=ref["v"]), b["groups"], d)
    assert any(a == "p" for _, a, _, _, _ in bad)
    # `<=` instead of `<` in the decay test: element n_decay decays too
    p_le, _, _, _ = R.adamw_apply64(b["p"], b["g"], b["m"], b["v"], case.step, hp, case.count, b["n_decay"] + 1)
    bad, _ = R.check_against(ref, dict(p=p_le, m=ref["m"], v=ref["v"]), b["groups"], d)
    assert [(g_, a) for g_, a, _, _, _ in bad] == [("undecayed", "p")]
    # and the fp32 oracle itself passes its own bound
    bad, _ = R.check_against(ref, o32, b["groups"], d)
    assert not bad
