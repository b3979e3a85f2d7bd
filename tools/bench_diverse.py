"""Cost of the diversity-aware re-ranking (b4r_rerank_diverse) for R users: python tools/bench_diverse.py [R [H]].
Per (V, M, K) it times, alternated in one process, medians of repeats of event-timed calls:
  sweep        Engine.rank_full for the pool (k = M), the step in front of the re-ranking
  rerank       Engine.rerank_diverse with a given rnorm (one launch)
  rerank+norm  the same with rnorm = None (1 / |row| of all V table rows first: what recommend_tensor(diversity=) runs)
  torch        greedy MMR over the same pool in torch on the device: gather the pool's table rows [R, M, E], normalise, then per
               step one bmm, a max, and an arg-max (fp32; not the kernel's rounding, so the two may differ at near ties)
Checks that the kernel and the torch loop pick the same items in at least 95 % of the slots (a near tie that rounds the other way
changes the rest of its row), prints one line per case, then a JSON line."""
import json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4rec_amd.engine import Engine, SPECIAL_IDS, make_model_config

R = int(sys.argv[1]) if len(sys.argv) > 1 else 256
H = int(sys.argv[2]) if len(sys.argv) > 2 else 128
SEEN = 200
DIVERSITY = 0.5
CASES = ((100, 10), (1024, 100))


def time_ms(f, reps=20):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); f(); b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[reps // 2]


def torch_mmr(table, rnorm, pool_ids, pool_scores, lam, K):
    Rn, M = pool_ids.shape
    live = (pool_ids >= 0) & (pool_ids < table.shape[0]) & torch.isfinite(pool_scores)   # the kernel's rule
    idx = torch.where(live, pool_ids, torch.zeros_like(pool_ids))
    e = table[idx] * rnorm[idx][..., None]                                    # [R, M, E], unit rows
    smax = pool_scores.masked_fill(~live, float("-inf")).amax(1, keepdim=True)
    smin = pool_scores.masked_fill(~live, float("inf")).amin(1, keepdim=True)
    rel = torch.where(smax == smin, torch.ones_like(pool_scores), (pool_scores - smin) / (smax - smin))
    pen = torch.zeros_like(pool_scores)
    is_open = live.clone()
    rows = torch.arange(Rn, device=table.device)
    out = torch.empty((Rn, K), dtype=torch.int64, device=table.device)
    for t in range(K):
        mmr = (lam * rel - (1.0 - lam) * pen).masked_fill(~is_open, float("-inf"))
        w = mmr.argmax(dim=1)
        out[:, t] = pool_ids[rows, w]
        is_open[rows, w] = False
        sim = torch.bmm(e, e[rows, w].unsqueeze(2)).squeeze(2)                # [R, M]
        pen = sim if t == 0 else torch.maximum(pen, sim)
    return out


results = []
for V in (26732, 335423):
    eng = Engine(make_model_config(V, H, 2, H // 32, 200, 4 * H), device="cuda")
    eng.init_parameters(seed=1)
    g = torch.Generator(device="cuda").manual_seed(0)
    hidden = torch.randn(R, H, device="cuda", generator=g)
    seen = torch.randint(SPECIAL_IDS, V, (R, SEEN), device="cuda", generator=g)
    table = eng.view("word_embeddings/embeddings")
    rnorm = 1.0 / table.double().pow(2).sum(1).clamp(min=1e-24).sqrt()
    rnorm = rnorm.float().contiguous()
    lam = 1.0 - DIVERSITY
    for M, K in CASES:
        pool_ids, pool_scores, _ = eng.rank_full(hidden, None, seen, SPECIAL_IDS, None, M)
        legs = {
            "sweep_ms": lambda: eng.rank_full(hidden, None, seen, SPECIAL_IDS, None, M),
            "rerank_ms": lambda: eng.rerank_diverse(pool_ids, pool_scores, K, DIVERSITY, rnorm),
            "rerank_norm_ms": lambda: eng.rerank_diverse(pool_ids, pool_scores, K, DIVERSITY),
            "torch_ms": lambda: torch_mmr(table, rnorm, pool_ids, pool_scores, lam, K),
        }
        same = float((legs["rerank_ms"]()[0] == legs["torch_ms"]()).float().mean())
        assert same >= 0.95, f"the kernel and the torch loop agree in only {same:.4f} of the slots"
        assert torch.equal(legs["rerank_ms"]()[0][:, 0], pool_ids[:, 0])
        times = {name: [] for name in legs}
        for f in legs.values():
            for _ in range(3):
                f()
        reps = 20 if K <= 10 else 10
        for _ in range(5):   # alternated repeats
            for name, f in legs.items():
                times[name].append(time_ms(f, reps))
        row = {"R": R, "H": H, "V": V, "M": M, "K": K, "same_picks": round(same, 5),
               **{name: round(sorted(t)[2], 4) for name, t in times.items()}}
        results.append(row)
        print("R %d H %d V %6d M %4d K %3d: sweep %7.3f  rerank %7.3f  rerank + rnorm %7.3f  torch loop %8.3f ms  (same picks %.4f)"
              % (R, H, V, M, K, row["sweep_ms"], row["rerank_ms"], row["rerank_norm_ms"], row["torch_ms"], same), flush=True)
    del eng
    torch.cuda.empty_cache()
print(json.dumps({"bench_diverse": results}))
