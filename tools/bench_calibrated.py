"""Cost of the calibrated re-ranking (b4r_rerank_calibrated) for R users: python tools/bench_calibrated.py [R [H]].
Per (M, K) and G it times, alternated in one process, medians of repeats of event-timed calls, all on the same pool:
  sparse       Engine.rerank_calibrated at lambda = 0.5 with a target as a history gives it: the label counts of 50 items per user (with
               G = 1000 most groups have no mass, hence no gain to form)
  dense        ... with a target as the affinity gives it: every group has mass, so all G gains are formed at every step
  quota0       Engine.rerank_quota without quotas at lambda = 1 on the same pool: the same pick loop without the gains (and with the
               MMR kernel's walk over the item table, which lambda = 1 does not switch off)
  torch        a greedy loop in torch on the device for the dense target: per step the [R, G] gains with torch.log in fp64, a gather to
               the pool entries, the fp32 value, a masked arg-max and a scatter-add of the pick's label
Reports how many rows of the torch loop hold exactly the kernel's picks (torch.log is not b4r_xln: a gain may round the other way and
a near tie then falls the other way) and fails below 99 %.  Prints one line per case, then a JSON line, and writes
profiles/calibrated_measurements.json when given --write."""
import json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bert4rec_amd.engine import Engine, SPECIAL_IDS, make_model_config

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
R = int(argv[0]) if len(argv) > 0 else 256
H = int(argv[1]) if len(argv) > 1 else 128
V = 26732
SEEN = 200
LAMBDA, ALPHA = 0.5, 0.01
CASES = ((100, 10), (1024, 100))
GROUPS = (20, 1000)


def time_ms(f, reps=20):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); f(); b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[reps // 2]


def torch_calibrated(pool_ids, pool_scores, V, item_group, G, target, lam, alpha, K):
    """the greedy loop a caller writes by hand: the contract's formulas with torch.log; returns the picked ids [R, K]"""
    Rn, M = pool_ids.shape
    dev = pool_ids.device
    live = (pool_ids >= 0) & (pool_ids < V) & torch.isfinite(pool_scores)
    lab = item_group[torch.where(live, pool_ids, torch.zeros_like(pool_ids))].to(torch.int64)
    lab = torch.where(live & (lab >= 0) & (lab < G), lab, torch.full_like(lab, -1))
    lab0 = lab.clamp(min=0)
    smax = torch.where(live, pool_scores, torch.full_like(pool_scores, -float("inf"))).max(dim=1, keepdim=True).values
    smin = torch.where(live, pool_scores, torch.full_like(pool_scores, float("inf"))).min(dim=1, keepdim=True).values
    rel = torch.where(smax == smin, torch.ones_like(pool_scores), (pool_scores - smin) / (smax - smin))
    mass = target.clamp(min=0)
    T = mass.sum(dim=1, keepdim=True)
    p = torch.where(T > 0, mass.double() / T.double().clamp(min=1.0), torch.zeros_like(mass, dtype=torch.float64))
    has_p = p > 0
    ap, A = alpha * p, 1.0 - alpha
    la = torch.tensor(lam, dtype=torch.float32, device=dev)
    a = (1.0 - la) * rel
    n_g = torch.zeros((Rn, G), dtype=torch.int64, device=dev)
    is_open = live.clone()
    rows = torch.arange(Rn, device=dev)
    order = torch.arange(M, 0, -1, device=dev, dtype=torch.int64)
    out = torch.full((Rn, K), -1, dtype=torch.int64, device=dev)
    for t in range(K):
        c = n_g.double()
        d = torch.log((A * (c + 1.0)) / (t + 1.0) + ap) - torch.log((A * c) / (t + 1.0) + ap)
        gain = torch.where(has_p, p * d, torch.zeros_like(d)).float()
        val = a + la * torch.where(lab >= 0, gain.gather(1, lab0), torch.zeros_like(rel))
        val = torch.where(is_open, val, torch.full_like(val, -float("inf")))
        best = val.max(dim=1, keepdim=True).values
        w = ((is_open & (val == best)).to(torch.int64) * order).argmax(dim=1)   # the lowest position among the best
        has = is_open[rows, w]
        out[:, t] = torch.where(has, pool_ids[rows, w], out[:, t])
        is_open[rows, w] = False
        wl = lab[rows, w]
        n_g.scatter_add_(1, wl.clamp(min=0)[:, None], (has & (wl >= 0)).to(torch.int64)[:, None])
    return out


eng = Engine(make_model_config(V, H, 2, H // 32, 200, 4 * H), device="cuda")
eng.init_parameters(seed=1)
g = torch.Generator(device="cuda").manual_seed(0)
hidden = torch.randn(R, H, device="cuda", generator=g)
seen = torch.randint(SPECIAL_IDS, V, (R, SEEN), device="cuda", generator=g)
table = eng.view("word_embeddings/embeddings")
rnorm = (1.0 / table.double().pow(2).sum(1).clamp(min=1e-24).sqrt()).float().contiguous()
cpu = torch.Generator().manual_seed(1)
results = []
for M, K in CASES:
    pool_ids, pool_scores, _ = eng.rank_full(hidden, None, seen, SPECIAL_IDS, None, M)
    for G in GROUPS:
        labels = torch.randint(0, G, (V,), generator=cpu).to(torch.int32).cuda()
        history = labels.to(torch.int64)[torch.randint(SPECIAL_IDS, V, (R, 50), generator=cpu).cuda()]
        sparse = torch.zeros((R, G), dtype=torch.int64, device="cuda").scatter_add_(1, history, torch.ones_like(history))
        dense = torch.randint(1, 1 << 30, (R, G), generator=cpu).cuda()
        legs = {
            "sparse_ms": lambda: eng.rerank_calibrated(pool_ids, pool_scores, K, LAMBDA, labels, G, sparse, ALPHA),
            "dense_ms": lambda: eng.rerank_calibrated(pool_ids, pool_scores, K, LAMBDA, labels, G, dense, ALPHA),
            "quota0_ms": lambda: eng.rerank_quota(pool_ids, pool_scores, K, 0.0, [], rnorm),
            "torch_ms": lambda: torch_calibrated(pool_ids, pool_scores, V, labels, G, dense, LAMBDA, ALPHA, K),
        }
        kernel, loop = legs["dense_ms"](), legs["torch_ms"]()
        same_rows = int((kernel[0] == loop).all(dim=1).sum())
        assert same_rows >= 0.99 * R, f"the torch loop holds the kernel's picks in {same_rows} of {R} rows only"
        moved = float((kernel[3] != torch.arange(K, device="cuda", dtype=torch.int32)[None, :]).any(dim=1).float().mean())
        kl = {name: float(torch.nanmean(legs[name]()[4])) for name in ("sparse_ms", "dense_ms")}
        kl_plain = float(torch.nanmean(eng.rerank_calibrated(pool_ids, pool_scores, K, 0.0, labels, G, dense, ALPHA)[4]))
        times = {name: [] for name in legs}
        for f in legs.values():
            for _ in range(3):
                f()
        reps = 20 if K <= 10 else 10
        for _ in range(5):   # alternated repeats
            for name, f in legs.items():
                times[name].append(time_ms(f, reps))
        med = {name: sorted(t)[2] for name, t in times.items()}
        row = {"R": R, "H": H, "V": V, "M": M, "K": K, "G": G, **{name: round(v, 4) for name, v in med.items()},
               **{name.replace("_ms", "_range_ms"): [round(min(t), 4), round(max(t), 4)] for name, t in times.items()},
               "dense_over_quota0": round(med["dense_ms"] / med["quota0_ms"], 3), "torch_over_dense": round(med["torch_ms"] / med["dense_ms"], 2),
               "rows_with_the_torch_loops_picks": same_rows, "rows_reordered": round(moved, 3),
               "mean_kl_dense": round(kl["dense_ms"], 5), "mean_kl_dense_plain_top_k": round(kl_plain, 5)}
        results.append(row)
        print("R %d M %4d K %3d G %4d: calibrated sparse %7.3f [%.3f, %.3f]  dense %7.3f [%.3f, %.3f]  quota x0 %7.3f [%.3f, %.3f]  "
              "torch loop %8.3f [%.3f, %.3f] ms  (same picks in %d / %d rows; kl %.4f against %.4f for the plain top k)"
              % (R, M, K, G, med["sparse_ms"], min(times["sparse_ms"]), max(times["sparse_ms"]), med["dense_ms"], min(times["dense_ms"]),
                 max(times["dense_ms"]), med["quota0_ms"], min(times["quota0_ms"]), max(times["quota0_ms"]), med["torch_ms"],
                 min(times["torch_ms"]), max(times["torch_ms"]), same_rows, R, kl["dense_ms"], kl_plain), flush=True)
print(json.dumps({"bench_calibrated": results}))
if "--write" in sys.argv:
    with open(os.path.join(ROOT, "profiles", "calibrated_measurements.json"), "w") as f:
        json.dump({"tool": "tools/bench_calibrated.py", "bench_calibrated": results}, f, indent=1)
        f.write("\n")
