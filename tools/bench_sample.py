"""Sampled recommendations for R users (b4r_sample_full: k items drawn without replacement from the catalogue softmax) beside the cost
of the same sweep without the noise and a torch version, over the same hidden states and exclusions, in the same run:
  b4r_rank_full(k)        the top-k sweep over the same allowed set
  b4r_score_dist          the softmax sweep (normaliser, entropy, log probability of k queried items)
  torch on the device     logits = hidden @ table.T + bias as an [R, V] buffer, masked_fill of the disallowed ids, + Gumbel noise
                          (-log(-log(rand))), topk
  b4r_sample_pool         the truncated draw of k from the best M, for (M, k) = (100, 10) and (1024, 100) (the pool given)
python tools/bench_sample.py [R [H]].  What is timed: the enqueue-to-completion time of one call between two device events, the
median of 20 calls, then the median of 5 such rounds taken alternately over the paths; the smallest and largest round of
b4r_sample_full are printed as its spread.  Prints one line per (V, k), then a JSON line."""
import json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4rec_amd.engine import Engine, SPECIAL_IDS, make_model_config

R = int(sys.argv[1]) if len(sys.argv) > 1 else 256
H = int(sys.argv[2]) if len(sys.argv) > 2 else 128
SEEN = 200   # history length excluded per user
SEED = 0x0123456789ABCDEF


def time_ms(f, reps=20):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); f(); b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[reps // 2]


results = []
for V in (3709, 26732, 335423):
    eng = Engine(make_model_config(V, H, 2, H // 32, 200, 4 * H), device="cuda")
    eng.init_parameters(seed=1)
    g = torch.Generator(device="cuda").manual_seed(0)
    hidden = torch.randn(R, H, device="cuda", generator=g)
    seen = torch.randint(SPECIAL_IDS, V, (R, SEEN), device="cuda", generator=g)
    table, bias = eng.view("word_embeddings/embeddings"), eng.view("cls/predictions/output_bias/bias")
    banned = torch.zeros(R, V, dtype=torch.bool, device="cuda")
    banned[:, :SPECIAL_IDS] = True
    banned.scatter_(1, seen, True)
    for k in (10, 100):
        M = 100 if k == 10 else 1024
        pool_ids, pool_scores, _ = eng.rank_full(hidden, None, seen, SPECIAL_IDS, None, M)
        drawn = eng.sample_full(hidden, None, seen, SPECIAL_IDS, None, k, SEED)[0]
        paths = {
            "sample_full": lambda: eng.sample_full(hidden, None, seen, SPECIAL_IDS, None, k, SEED),
            "rank_full": lambda: eng.rank_full(hidden, None, seen, SPECIAL_IDS, None, k),
            "score_dist": lambda: eng.score_distribution(hidden, None, seen, SPECIAL_IDS, None, None, None, 1.0, drawn),
            "sample_pool": lambda: eng.sample_pool(pool_ids, pool_scores, k, SEED),
        }

        def eager():
            logits = (hidden @ table.T + bias).masked_fill(banned, float("-inf"))
            noise = -torch.log(-torch.log(torch.rand(R, V, device="cuda").clamp_(1e-20, 1.0 - 1e-7)))
            return torch.topk(logits + noise, k, dim=1)

        paths["torch"] = eager
        assert not banned.gather(1, drawn).any() and not banned.gather(1, eager()[1]).any()
        for _ in range(3):
            for f in paths.values():
                f()
        t = {name: [] for name in paths}
        for _ in range(5):   # alternated repeats
            for name, f in paths.items():
                t[name].append(time_ms(f))
        med = {name: sorted(v)[2] for name, v in t.items()}
        results.append({"R": R, "H": H, "V": V, "k": k, "pool": M, **{f"{name}_ms": round(v, 4) for name, v in med.items()},
                        "sample_full_spread_ms": [round(min(t["sample_full"]), 4), round(max(t["sample_full"]), 4)],
                        "rank_full_spread_ms": [round(min(t["rank_full"]), 4), round(max(t["rank_full"]), 4)],
                        "score_dist_spread_ms": [round(min(t["score_dist"]), 4), round(max(t["score_dist"]), 4)]})
        print("R %d H %d V %6d k %3d: b4r_sample_full %8.3f ms [%.3f, %.3f]   b4r_rank_full %8.3f ms   b4r_score_dist %8.3f ms   "
              "torch [R, V] Gumbel top-k %8.3f ms   b4r_sample_pool(M = %d) %7.3f ms"
              % (R, H, V, k, med["sample_full"], min(t["sample_full"]), max(t["sample_full"]), med["rank_full"], med["score_dist"],
                 med["torch"], M, med["sample_pool"]), flush=True)
    del eng
    torch.cuda.empty_cache()
print(json.dumps({"bench_sample": results}))
