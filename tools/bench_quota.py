"""Cost of the re-ranking under category quotas (b4r_rerank_quota) for R users: python tools/bench_quota.py [R [H]].
Per (V, M, K) it times, alternated in one process, medians of repeats of event-timed calls, all on the same pool with a given rnorm:
  diverse      Engine.rerank_diverse (b4r_rerank_diverse)
  quota0       Engine.rerank_quota without a quota (the same picks, by the new kernel)
  quota1       ... with one quota: about 20 groups, cap 2
  quota4       ... with four: that one, about 5 000 groups with cap 1, and, to reach the largest n_quotas, two more of the same two
               kinds: about 20 groups with cap 3 and about 5 000 groups with cap 2
  torch        a greedy capped loop in torch on the device under the quota of quota1, at lambda = 1 (relevance order under the caps:
               per step a masked arg-max, a gather of the pick's group and a compare; no similarities)
Asserts that the kernel (quota1 at lambda = 1) and the torch loop pick the same items, and that quota0 equals diverse bit for bit.
Reports quota0 / diverse with the run-to-run spread of both legs (the largest over the smallest of the alternated repeats), prints one
line per case, then a JSON line, and writes profiles/quota_measurements.json when given --write."""
import json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bert4rec_amd.engine import Engine, SPECIAL_IDS, make_model_config, pack_item_groups

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
R = int(argv[0]) if len(argv) > 0 else 256
H = int(argv[1]) if len(argv) > 1 else 128
SEEN = 200
DIVERSITY = 0.5
CASES = ((100, 10), (1024, 100))


def time_ms(f, reps=20):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); f(); b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[reps // 2]


def torch_capped(pool_ids, pool_scores, V, item_group, cap, K):
    """lambda = 1 under one quota with a uniform cap: the best open entry per step; an entry closes when its group has given cap picks"""
    Rn, M = pool_ids.shape
    live = (pool_ids >= 0) & (pool_ids < V) & torch.isfinite(pool_scores)   # the kernel's rule
    grp = item_group[torch.where(live, pool_ids, torch.zeros_like(pool_ids))].to(torch.int64)
    grp = torch.where(live, grp, torch.full_like(grp, -1))
    left = torch.full_like(grp, cap)
    is_open = live & (left > 0)
    rows = torch.arange(Rn, device=pool_ids.device)
    out = torch.full((Rn, K), -1, dtype=torch.int64, device=pool_ids.device)
    order = torch.arange(M, 0, -1, device=pool_ids.device, dtype=torch.float32)   # descending scores: the lowest open position wins
    for t in range(K):
        w = (order * is_open).argmax(dim=1)
        has = is_open[rows, w]
        out[:, t] = torch.where(has, pool_ids[rows, w], out[:, t])
        is_open[rows, w] = False
        wg = torch.where(has, grp[rows, w], torch.full_like(w, -2))
        same = is_open & (grp == wg[:, None]) & (grp >= 0)
        left = left - same.to(left.dtype)
        is_open &= ~(same & (left <= 0))
    return out


results = []
for V in (26732, 335423):
    eng = Engine(make_model_config(V, H, 2, H // 32, 200, 4 * H), device="cuda")
    eng.init_parameters(seed=1)
    g = torch.Generator(device="cuda").manual_seed(0)
    hidden = torch.randn(R, H, device="cuda", generator=g)
    seen = torch.randint(SPECIAL_IDS, V, (R, SEEN), device="cuda", generator=g)
    table = eng.view("word_embeddings/embeddings")
    rnorm = (1.0 / table.double().pow(2).sum(1).clamp(min=1e-24).sqrt()).float().contiguous()
    cpu = torch.Generator().manual_seed(1)
    few = torch.randint(0, 20, (V,), generator=cpu)
    many = torch.randint(0, 5000, (V,), generator=cpu)
    q_few, q_many = pack_item_groups(few, 2), pack_item_groups(many, 1)
    q_few3, q_many2 = pack_item_groups(torch.randint(0, 20, (V,), generator=cpu), 3), pack_item_groups(torch.randint(0, 5000, (V,), generator=cpu), 2)
    few_d = few.to(torch.int32).cuda()
    for M, K in CASES:
        pool_ids, pool_scores, _ = eng.rank_full(hidden, None, seen, SPECIAL_IDS, None, M)
        legs = {
            "diverse_ms": lambda: eng.rerank_diverse(pool_ids, pool_scores, K, DIVERSITY, rnorm),
            "quota0_ms": lambda: eng.rerank_quota(pool_ids, pool_scores, K, DIVERSITY, [], rnorm),
            "quota1_ms": lambda: eng.rerank_quota(pool_ids, pool_scores, K, DIVERSITY, [q_few], rnorm),
            "quota4_ms": lambda: eng.rerank_quota(pool_ids, pool_scores, K, DIVERSITY, [q_few, q_many, q_few3, q_many2], rnorm),
            "torch_ms": lambda: torch_capped(pool_ids, pool_scores, V, few_d, 2, K),
        }
        d, q0 = legs["diverse_ms"](), legs["quota0_ms"]()
        assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                   for a, b in zip(d, q0[:3])), "b4r_rerank_quota without quotas differs from b4r_rerank_diverse"
        kernel = eng.rerank_quota(pool_ids, pool_scores, K, 0.0, [q_few], rnorm)[0]
        loop = legs["torch_ms"]()
        assert torch.equal(kernel, loop), "the kernel and the torch loop pick different items"
        picks1 = float((legs["quota1_ms"]()[0] >= 0).float().sum(1).mean())
        picks4 = float((legs["quota4_ms"]()[0] >= 0).float().sum(1).mean())
        times = {name: [] for name in legs}
        for f in legs.values():
            for _ in range(3):
                f()
        reps = 20 if K <= 10 else 10
        for _ in range(5):   # alternated repeats
            for name, f in legs.items():
                times[name].append(time_ms(f, reps))
        med = {name: sorted(t)[2] for name, t in times.items()}
        spread = {name: max(t) / min(t) for name, t in times.items()}
        ratio = med["quota0_ms"] / med["diverse_ms"]
        noise = max(spread["quota0_ms"], spread["diverse_ms"])
        row = {"R": R, "H": H, "V": V, "M": M, "K": K, **{name: round(v, 4) for name, v in med.items()},
               "quota0_over_diverse": round(ratio, 4), "run_to_run_spread": round(noise, 4),
               "quota0_beyond_spread": bool(ratio > noise or ratio < 1.0 / noise),
               "mean_picks_quota1": round(picks1, 2), "mean_picks_quota4": round(picks4, 2), "same_picks_as_torch": True}
        results.append(row)
        print("R %d H %d V %6d M %4d K %3d: diverse %7.3f  quota x0 %7.3f  x1 %7.3f  x4 %7.3f  torch loop %8.3f ms  (x0 / diverse %.3f, "
              "spread %.3f; picks x1 %.1f x4 %.1f)" % (R, H, V, M, K, med["diverse_ms"], med["quota0_ms"], med["quota1_ms"], med["quota4_ms"],
                                                      med["torch_ms"], ratio, noise, picks1, picks4), flush=True)
    del eng
    torch.cuda.empty_cache()
print(json.dumps({"bench_quota": results}))
if "--write" in sys.argv:
    with open(os.path.join(ROOT, "profiles", "quota_measurements.json"), "w") as f:
        json.dump({"tool": "tools/bench_quota.py", "bench_quota": results}, f, indent=1)
        f.write("\n")
