"""Full-catalogue top k for R users (b4r_rank_full) against the whole-vocabulary ranking (b4r_rank_candidates with cand = NULL, the
path of rank_items_tensor(batch, None)) followed by the seen-item filter, both over the same hidden states:
python tools/bench_full_rank.py [R [H]].  Prints one line per (V, k) with the median of alternated repeats, then a JSON line."""
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
    for k in (10, 100):
        new = lambda: eng.rank_full(hidden, None, seen, SPECIAL_IDS, None, k)

        def old():
            ranking, _, _ = eng.rank_candidates(hidden, None, None, None, n_candidates=V, n_rows=R)
            allowed = torch.ones(R, V, dtype=torch.bool, device="cuda")
            allowed[:, :SPECIAL_IDS] = False
            allowed.scatter_(1, seen, False)
            keep = allowed.gather(1, ranking)
            sel = keep & (keep.cumsum(1) <= k)
            return ranking[sel].view(R, k)

        ids_new = new()[0]
        ids_old = old()
        assert torch.equal(ids_new, ids_old), "the two paths disagree"
        for _ in range(3):
            new(); old()
        t_new, t_old = [], []
        for _ in range(5):   # alternated repeats
            t_new.append(time_ms(new)); t_old.append(time_ms(old))
        tn, to = sorted(t_new)[2], sorted(t_old)[2]
        results.append({"R": R, "H": H, "V": V, "k": k, "rank_full_ms": round(tn, 4), "rank_all_then_filter_ms": round(to, 4),
                        "speedup": round(to / tn, 2)})
        print("R %d H %d V %6d k %3d: b4r_rank_full %8.3f ms   whole-vocabulary ranking + filter %8.3f ms   x%.1f"
              % (R, H, V, k, tn, to, to / tn), flush=True)
    del eng
    torch.cuda.empty_cache()
print(json.dumps({"bench_full_rank": results}))
