"""Catalogue softmax for R users (b4r_score_dist: row count, maximum, log normaliser, entropy, and the log probability of 10 queried
items per user) beside two comparisons over the same hidden states, exclusions and filter, in the same run:
  b4r_rank_full(k = 10)   the top-10 sweep over the same allowed set (b4r_rank_full_ex when a filter is given)
  torch on the device     logits = hidden @ table.T + bias as an [R, V] buffer, masked_fill of the disallowed ids, logsumexp
python tools/bench_score_dist.py [R [H]].  What is timed: the enqueue-to-completion time of one call between two device events, the
median of 20 calls, then the median of 5 such rounds taken alternately over the three paths.  The filter allows a random 10 % of the
catalogue.  Prints one line per (V, filter), then a JSON line."""
import json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4rec_amd.engine import Engine, SPECIAL_IDS, make_model_config

R = int(sys.argv[1]) if len(sys.argv) > 1 else 256
H = int(sys.argv[2]) if len(sys.argv) > 2 else 128
SEEN = 200   # history length excluded per user


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
    for share in (None, 0.10):
        allow = None if share is None else torch.rand(V, device="cuda", generator=g) < share
        top = eng.rank_full(hidden, None, seen, SPECIAL_IDS, None, 10, allow)[0]
        dist = lambda: eng.score_distribution(hidden, None, seen, SPECIAL_IDS, None, allow, None, 1.0, top)
        sweep = lambda: eng.rank_full(hidden, None, seen, SPECIAL_IDS, None, 10, allow)
        banned = torch.zeros(R, V, dtype=torch.bool, device="cuda")
        banned[:, :SPECIAL_IDS] = True
        banned.scatter_(1, seen, True)
        if allow is not None:
            banned |= ~allow[None, :]

        def eager():
            logits = hidden @ table.T + bias
            return torch.logsumexp(logits.masked_fill(banned, float("-inf")), dim=1)

        lse = dist()[2]
        gap = float((lse - eager().to(torch.float64)).abs().max())
        assert gap < 1e-3, f"the two normalisers disagree by {gap}"
        for _ in range(3):
            dist(); sweep(); eager()
        t = {"dist": [], "sweep": [], "eager": []}
        for _ in range(5):   # alternated repeats
            t["dist"].append(time_ms(dist)); t["sweep"].append(time_ms(sweep)); t["eager"].append(time_ms(eager))
        td, ts, te = (sorted(t[k])[2] for k in ("dist", "sweep", "eager"))
        results.append({"R": R, "H": H, "V": V, "filter": share or 0.0, "score_dist_ms": round(td, 4), "rank_full_k10_ms": round(ts, 4),
                        "torch_logsumexp_ms": round(te, 4), "score_dist_spread_ms": [round(min(t["dist"]), 4), round(max(t["dist"]), 4)]})
        print("R %d H %d V %6d filter %4s: b4r_score_dist %8.3f ms   b4r_rank_full(k=10) %8.3f ms   torch [R, V] logsumexp %8.3f ms"
              % (R, H, V, "none" if share is None else "10 %", td, ts, te), flush=True)
    del eng
    torch.cuda.empty_cache()
print(json.dumps({"bench_score_dist": results}))
