"""Cost of the beyond-accuracy list metrics (b4r_list_metrics) for R lists: python tools/bench_list_metrics.py [R [H]].
Per (V, K) it times, alternated in one process, medians of 7 repeats of event-timed regions of several calls each:
  kernel       Engine.list_metrics with a given rnorm, into exposure / sums / counts accumulators (two launches)
  kernel+norm  the same with rnorm = None (1 / |row| of all V table rows first: what the evaluator and Recommender.list_quality run)
  torch        the obvious torch expression on the same device over the same lists: gather the K rows [R, K, E], normalise, bmm to
               [R, K, K], the mean of the upper triangle per list, summed; bincount for the exposure (fp32 with the BLAS library's
               rounding: not the kernel's integers)
The lists are b4r_rank_full's top K for random hidden rows.  Checks that the two mean intra-list distances agree to 1e-4 and that the
exposure counts are equal, prints one line per case, then a JSON line.  The kernel's claim is exact integers, no [R, K, K] tensor and
no host synchronisation, not a speed-up: both times are reported as measured."""
import json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4rec_amd.engine import Engine, SPECIAL_IDS, make_model_config

R = int(sys.argv[1]) if len(sys.argv) > 1 else 256
H = int(sys.argv[2]) if len(sys.argv) > 2 else 128
SEEN = 200
REPEATS = 7


def time_ms(f, reps):
    """The median time of one call over `reps` event-timed calls enqueued back to back."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); f(); b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[reps // 2]


def torch_lists(table, ids, V):
    K = ids.shape[1]
    e = table[ids]
    e = e / e.norm(dim=2, keepdim=True).clamp_min(1e-12)
    cos = torch.bmm(e, e.transpose(1, 2))                                     # [R, K, K]
    iu = torch.triu_indices(K, K, 1, device=ids.device)
    ild = (1.0 - cos[:, iu[0], iu[1]]).mean(dim=1).double().sum()
    return ild, torch.bincount(ids.reshape(-1), minlength=V)


results = []
for V in (26732, 335423):
    eng = Engine(make_model_config(V, H, 2, H // 32, 200, 4 * H), device="cuda")
    eng.init_parameters(seed=1)
    g = torch.Generator(device="cuda").manual_seed(0)
    hidden = torch.randn(R, H, device="cuda", generator=g)
    seen = torch.randint(SPECIAL_IDS, V, (R, SEEN), device="cuda", generator=g)
    table = eng.view("word_embeddings/embeddings")
    rnorm = (1.0 / table.double().pow(2).sum(1).clamp(min=1e-24).sqrt()).float().contiguous()
    exposure = torch.zeros(V, dtype=torch.int64, device="cuda")
    sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    for K in (10, 100):
        ids, _, _ = eng.rank_full(hidden, None, seen, SPECIAL_IDS, None, K)
        assert bool((ids >= 0).all())
        legs = {
            "kernel_ms": lambda: eng.list_metrics(ids, None, None, rnorm, exposure, sums, counts),
            "kernel_norm_ms": lambda: eng.list_metrics(ids, None, None, None, exposure, sums, counts),
            "torch_ms": lambda: torch_lists(table, ids, V),
        }
        for t in (exposure, sums, counts):
            t.zero_()
        legs["kernel_ms"]()
        ild_t, exp_t = legs["torch_ms"]()
        ild_k = float(sums[0]) / float(counts[0]) if int(counts[0]) else 0.0
        assert torch.equal(exposure, exp_t), "exposure counts differ"
        assert abs(ild_k - float(ild_t) / R) <= 1e-4 * max(abs(ild_k), 1e-6), (ild_k, float(ild_t) / R)
        times = {name: [] for name in legs}
        for f in legs.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        for _ in range(REPEATS):   # alternated repeats
            for name, f in legs.items():
                times[name].append(time_ms(f, 20))
        row = {"R": R, "H": H, "V": V, "K": K, "ild": round(ild_k, 6),
               **{name: round(sorted(t)[REPEATS // 2], 4) for name, t in times.items()},
               **{name.replace("_ms", "_spread_ms"): [round(min(t), 4), round(max(t), 4)] for name, t in times.items()}}
        results.append(row)
        print("R %d H %d V %6d K %3d: kernel %7.4f  kernel + rnorm %7.4f  torch %7.4f ms  (ILD %.4f)"
              % (R, H, V, K, row["kernel_ms"], row["kernel_norm_ms"], row["torch_ms"], ild_k), flush=True)
    del eng
    torch.cuda.empty_cache()
print(json.dumps({"bench_list_metrics": results}))
