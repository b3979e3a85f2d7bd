"""Train step with factorised item embeddings (embedding_width E < hidden_size) against its unfactorised twin, in one process.

Legs: the ML-20M shape (V 26 732, H 256, 2 layers, 8 heads, inner 1024) at E = 256 (unfactorised), 128 and 64, and the Reddit shape
(V 335 423, H 128, 2 layers, 4 heads, inner 512) at E = 128 (unfactorised) and 64; B 256, L 200, P 40 everywhere.  Every leg is warmed
up, then the legs are timed alternating, region by region (device events around --steps train steps), and the median of the regions
is reported.  Also printed: the algorithmic HBM bytes of the two new launches (embed_proj_fwd / embed_proj_bwd) per step, so that the
kernel times of a `rocprofv3 --kernel-trace --stats` run of this script give their share of the HBM roof.

    python tools/bench_factorized.py [--steps 10] [--regions 9] [--legs ml20m_e64,reddit_e64,...]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4rec_amd.engine import Engine, make_adamw_config, make_model_config  # noqa: E402
from bert4rec_amd import _lib  # noqa: E402

SHAPES = {"ml20m": dict(V=26732, H=256, layers=2, heads=8, inner=1024), "reddit": dict(V=335423, H=128, layers=2, heads=4, inner=512)}
LEGS = {"ml20m_e256": ("ml20m", 256), "ml20m_e128": ("ml20m", 128), "ml20m_e64": ("ml20m", 64),
        "reddit_e128": ("reddit", 128), "reddit_e64": ("reddit", 64)}
B, L, P = 256, 200, 40


def batch(V, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, V, (B, L), generator=g)
    pos = torch.stack([torch.randperm(L, generator=g)[:P].sort().values for _ in range(B)])
    lab = torch.gather(ids, 1, pos)
    ids.scatter_(1, pos, 1)   # [MASK]
    return {"input_word_ids": ids, "input_mask": torch.ones(B, L, dtype=torch.int64), "masked_lm_positions": pos, "masked_lm_ids": lab}


def kernel_bytes(E, H, V):
    """algorithmic HBM bytes of one embed_proj_fwd and one embed_proj_bwd launch at N = B * L (tables read once per token row)"""
    N = B * L
    fwd = N * 8 + N * E * 4 + L * E * 4 + E * H * 4 + N * H * 4 + N * 8
    _lib.load()
    slabs = int(_lib.load().b4r_embed_proj_bwd_scratch_floats(N, E, H)) * 4
    # dx0 read by the row part and the weight part, the embedding rows recomputed by both, the rows written, the slabs written
    bwd = 2 * N * H * 4 + 2 * (N * 8 + N * E * 4 + N * 8) + N * E * 4 + slabs
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--legs", default=",".join(LEGS))
    a = ap.parse_args()
    assert a.regions >= 7, "at least 7 timed regions per leg"
    hp = make_adamw_config(num_warmup_steps=100, num_train_steps=400000)
    legs = {}
    for name in a.legs.split(","):
        shape, E = LEGS[name]
        s = SHAPES[shape]
        eng = Engine(make_model_config(s["V"], s["H"], s["layers"], s["heads"], L, s["inner"], 0.1, 0.1), "cuda", embedding_width=E)
        eng.init_parameters(seed=1)
        eng.set_seed(7)
        cb, keep = eng.prepare_batch(batch(s["V"], 3))
        for _ in range(a.warmup):
            eng.train_step(hp, cb)
        legs[name] = (eng, cb, keep, [])
    torch.cuda.synchronize()
    for _ in range(a.regions):
        for name, (eng, cb, keep, times) in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                eng.train_step(hp, cb)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / a.steps)
    for name, (eng, cb, keep, times) in legs.items():
        shape, E = LEGS[name]
        s = SHAPES[shape]
        out = {"leg": name, "V": s["V"], "H": s["H"], "E": E, "ms_per_step": round(statistics.median(times), 4),
               "min": round(min(times), 4), "max": round(max(times), 4), "regions": len(times), "steps_per_region": a.steps}
        if E < s["H"]:
            fb, bb = kernel_bytes(E, s["H"], s["V"])
            out["embed_proj_fwd_bytes"], out["embed_proj_bwd_bytes"] = fb, bb
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
