"""Train step under the "mixed_bfloat16" policy (B4R_GEMM_BF16, one bf16 term per product) against the default "float32" policy
(B4R_GEMM_BF16X3, three split terms), in one process.

Legs: the bench.py shapes ML-1M-64, Steam-64, ML-1M-128 and ML-20M-256 (2 and 4 layers), B 256 and P as in bench.py.  Each leg runs
in both modes on one engine (the mode is a process-wide switch, set before each region).  Every (leg, mode) pair is warmed up, then
the pairs are timed alternating, region by region (device events around --steps train steps), and the median of the regions is
reported, with the evaluation forward (encoder forward on the batch, users/s) timed the same way.

    python tools/bench_precision.py [--steps 10] [--regions 9] [--legs ml1m,steam,...]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4rec_amd.engine import Engine, make_adamw_config, make_model_config  # noqa: E402
from bert4rec_amd import _lib  # noqa: E402

# name: (vocab, hidden, layers, heads, inner, L, P, out_drop, att_drop) -- bench.py CONFIGS
LEGS = {
    "ml1m": (3709, 64, 2, 2, 256, 200, 40, 0.2, 0.2),
    "steam": (13047, 64, 2, 2, 256, 50, 20, 0.1, 0.1),
    "ml1m_128": (3709, 128, 2, 4, 512, 200, 40, 0.5, 0.2),
    "ml20m": (26732, 256, 2, 8, 1024, 200, 40, 0.1, 0.1),
    "ml20m_4l": (26732, 256, 4, 8, 1024, 200, 40, 0.1, 0.1),
}
MODES = {"float32": _lib.GEMM_BF16X3, "mixed_bfloat16": _lib.GEMM_BF16}
B = 256


def batch(V, L, P, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, V, (B, L), generator=g)
    pos = torch.stack([torch.randperm(L, generator=g)[:P].sort().values for _ in range(B)])
    lab = torch.gather(ids, 1, pos)
    ids.scatter_(1, pos, 1)   # [MASK]
    return {"input_word_ids": ids, "input_mask": torch.ones(B, L, dtype=torch.int64), "masked_lm_positions": pos, "masked_lm_ids": lab}


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--modes", default=",".join(MODES), help="policies to run (one of them: a per-kernel profile of that mode)")
    a = ap.parse_args()
    assert a.regions >= 7, "at least 7 timed regions per leg"
    modes = {m: MODES[m] for m in a.modes.split(",")}
    lib = _lib.load()
    prev = lib.b4r_get_gemm_mode()
    hp = make_adamw_config(num_warmup_steps=100, num_train_steps=400000)
    legs = {}
    for name in a.legs.split(","):
        V, H, layers, heads, inner, L, P, od, ad = LEGS[name]
        eng = Engine(make_model_config(V, H, layers, heads, L, inner, od, ad), "cuda")
        eng.init_parameters(seed=1)
        eng.set_seed(7)
        cb, keep = eng.prepare_batch(batch(V, L, P, 3))
        for mode in modes.values():
            _lib.check(lib.b4r_set_gemm_mode(mode))
            for _ in range(a.warmup):
                eng.train_step(hp, cb)
                eng.encoder_forward(cb)
        legs[name] = (eng, cb, keep, {m: ([], []) for m in modes})
    torch.cuda.synchronize()
    try:
        for _ in range(a.regions):
            for name, (eng, cb, keep, times) in legs.items():
                for m, mode in modes.items():
                    _lib.check(lib.b4r_set_gemm_mode(mode))
                    times[m][0].append(timed(lambda: eng.train_step(hp, cb), a.steps))
                    times[m][1].append(timed(lambda: eng.encoder_forward(cb), a.steps))
    finally:
        lib.b4r_set_gemm_mode(prev)
    for name, (eng, cb, keep, times) in legs.items():
        out = {"leg": name, "H": LEGS[name][1], "layers": LEGS[name][2], "L": LEGS[name][5], "B": B, "regions": a.regions,
               "steps_per_region": a.steps}
        for m in modes:
            tr, ev = times[m]
            out[m] = {"ms_per_step": round(statistics.median(tr), 4), "min": round(min(tr), 4), "max": round(max(tr), 4),
                      "eval_users_per_s": round(B / (statistics.median(ev) * 1e-3))}
        if len(modes) == 2:
            out["speedup"] = round(out["float32"]["ms_per_step"] / out["mixed_bfloat16"]["ms_per_step"], 4)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
