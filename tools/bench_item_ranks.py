"""Item ranks for R users (b4r_item_ranks: the exact rank of Q queried items per user among the items the user could be served, "strict")
beside the two ways to get the same ranks without it, over the same hidden states and exclusions, in the same run:
  (a) Q x b4r_rank_full_ex   one sweep per query column (gt = the column, K = 0): how these ranks were obtained before
  (b) torch on the device    logits = hidden @ table.T + bias as an [R, V] buffer, masked_fill of the disallowed ids, then per query
                             1 + #{score greater} + #{score equal and id lower}
python tools/bench_item_ranks.py [R [H]].  What is timed: the enqueue-to-completion time of one call between two device events, the
median of `reps` calls (fewer for the slow legs), then the median of 5 such rounds taken alternately over the three paths, with the
smallest and the largest round.  Prints one line per (V, Q), then a JSON line."""
import json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4rec_amd.engine import Engine, SPECIAL_IDS, make_model_config

R = int(sys.argv[1]) if len(sys.argv) > 1 else 256
H = int(sys.argv[2]) if len(sys.argv) > 2 else 128
SEEN = 200   # history length excluded per user


def time_ms(f, reps):
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
    ids = torch.arange(V, device="cuda")[None, :]
    one_sweep = time_ms(lambda: eng.rank_full(hidden, None, seen, SPECIAL_IDS, None, 0), 10)
    for Q in (1, 16, 256):
        query = torch.randint(SPECIAL_IDS, V, (R, Q), device="cuda", generator=g)
        cols = [query[:, i].contiguous() for i in range(Q)]
        ranks = lambda: eng.item_ranks(hidden, None, seen, SPECIAL_IDS, query, "self")[0]

        def sweeps():
            return torch.stack([eng.rank_full(hidden, None, seen, SPECIAL_IDS, c, 0)[2] for c in cols], dim=1)

        def eager():
            raw = hidden @ table.T + bias
            logits = raw.masked_fill(banned, float("-inf"))
            out = []
            for c in cols:
                s = raw.gather(1, c[:, None])
                out.append(1 + ((logits > s) | ((logits == s) & (ids < c[:, None]))).sum(dim=1))
            return torch.stack(out, dim=1)

        got = ranks()
        assert torch.equal(got, sweeps()), "b4r_item_ranks and the column-by-column sweeps disagree"
        slow = max(1, 10 // Q) if Q > 1 else 10
        for _ in range(2):
            ranks()
        t = {"ranks": [], "sweeps": [], "eager": []}
        for _ in range(5):   # alternated repeats
            t["ranks"].append(time_ms(ranks, 10)); t["sweeps"].append(time_ms(sweeps, slow)); t["eager"].append(time_ms(eager, slow))
        tr, ts, te = (sorted(t[k])[2] for k in ("ranks", "sweeps", "eager"))
        results.append({"R": R, "H": H, "V": V, "Q": Q, "item_ranks_ms": round(tr, 4),
                        "item_ranks_spread_ms": [round(min(t["ranks"]), 4), round(max(t["ranks"]), 4)],
                        "q_rank_full_sweeps_ms": round(ts, 4), "q_rank_full_spread_ms": [round(min(t["sweeps"]), 4), round(max(t["sweeps"]), 4)],
                        "torch_ms": round(te, 4), "torch_spread_ms": [round(min(t["eager"]), 4), round(max(t["eager"]), 4)],
                        "one_rank_full_sweep_ms": round(one_sweep, 4)})
        print("R %d H %d V %6d Q %3d: b4r_item_ranks %8.3f ms [%.3f, %.3f]   Q x b4r_rank_full_ex %9.3f ms   torch [R, V] + counts %9.3f ms"
              "   (one b4r_rank_full sweep %.3f ms)" % (R, H, V, Q, tr, min(t["ranks"]), max(t["ranks"]), ts, te, one_sweep), flush=True)
    del eng
    torch.cuda.empty_cache()
print(json.dumps({"bench_item_ranks": results}))
