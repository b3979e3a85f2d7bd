"""Train step per feed-forward activation (Bert4RecEncoder inner_activation; the masked-LM transform's follows it), in one process.

Shapes: ml-1m_64 (V 3709, H 64, 2 layers, 2 heads, inner 256), ml-1m_128 (H 128, 4 heads, inner 512) and ml-20m_256 (V 26 732, H 256,
8 heads, inner 1024); B 256, L 200, P 40.  Every (shape, activation) leg is warmed up, then the legs of a shape are timed alternating,
region by region (device events around --steps train steps); the median of the regions is reported with masked positions per second.
A `rocprofv3 --kernel-trace --stats` run of this script (one shape, --regions 7) gives the feed-forward kernels' time per activation.

    python tools/bench_activation.py [--steps 10] [--regions 9] [--shapes ml1m_64,ml1m_128,ml20m_256] [--acts gelu,relu,...]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4rec_amd import activations  # noqa: E402
from bert4rec_amd.engine import Engine, make_adamw_config, make_model_config  # noqa: E402

SHAPES = {"ml1m_64": dict(V=3709, H=64, heads=2, inner=256, od=0.2, ad=0.2),
          "ml1m_128": dict(V=3709, H=128, heads=4, inner=512, od=0.5, ad=0.2),
          "ml20m_256": dict(V=26732, H=256, heads=8, inner=1024, od=0.1, ad=0.1)}
B, L, P = 256, 200, 40


def batch(V, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, V, (B, L), generator=g)
    pos = torch.stack([torch.randperm(L, generator=g)[:P].sort().values for _ in range(B)])
    lab = torch.gather(ids, 1, pos)
    ids.scatter_(1, pos, 1)   # [MASK]
    return {"input_word_ids": ids, "input_mask": torch.ones(B, L, dtype=torch.int64), "masked_lm_positions": pos, "masked_lm_ids": lab}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--acts", default="gelu,relu,swish,tanh,sigmoid,elu,selu,softplus,linear")
    a = ap.parse_args()
    assert a.regions >= 7, "at least 7 timed regions per leg"
    hp = make_adamw_config(num_warmup_steps=100, num_train_steps=400000)
    for shape in a.shapes.split(","):
        s = SHAPES[shape]
        legs = {}
        for act in a.acts.split(","):
            aid = activations.IDS[act]
            eng = Engine(make_model_config(s["V"], s["H"], 2, s["heads"], L, s["inner"], s["od"], s["ad"]), "cuda",
                         inner_activation=aid, mlm_activation=aid)
            eng.init_parameters(seed=1)
            eng.set_seed(7)
            cb, keep = eng.prepare_batch(batch(s["V"], 3))
            for _ in range(a.warmup):
                eng.train_step(hp, cb)
            legs[act] = (eng, cb, keep, [])
        torch.cuda.synchronize()
        for _ in range(a.regions):
            for act, (eng, cb, keep, times) in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    eng.train_step(hp, cb)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) / a.steps)
        for act, (eng, cb, keep, times) in legs.items():
            ms = statistics.median(times)
            print(json.dumps({"shape": shape, "activation": act, "ms_per_step": round(ms, 4), "min": round(min(times), 4),
                              "max": round(max(times), 4), "masked_positions_per_s": round(B * P / (ms * 1e-3)),
                              "regions": len(times), "steps_per_region": a.steps}), flush=True)
        legs.clear()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
