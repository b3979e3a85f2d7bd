"""Cost of the catalogue filter and of item-to-item neighbours on the full-catalogue sweep, for R users / query items:
python tools/bench_item_neighbours.py [R [H]].  Per (V, k) it times, alternated in one process, medians of repeats:
  unfiltered   Engine.rank_full (b4r_rank_full)
  all-ones     the same call under a filter that allows every item (b4r_rank_full_ex)
  10 %         under a random filter of density 0.1
  cosine       Engine.item_neighbours for R query items (rnorm + query rows + sweep)
  rank + mask  what the filtered call replaces: the whole-vocabulary ranking (b4r_rank_candidates with cand = NULL, the path of
               rank_items_tensor(batch, None)) followed by the seen-item and catalogue masks, on the device
Prints one line per (V, k), then a JSON line."""
import json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4rec_amd.engine import Engine, SPECIAL_IDS, make_model_config, pack_item_filter

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
    query = torch.randint(SPECIAL_IDS, V, (R,), device="cuda", generator=g)
    mask = torch.rand(V, device="cuda", generator=g) < 0.1
    ones, tenth = pack_item_filter(torch.ones(V, dtype=torch.bool, device="cuda")), pack_item_filter(mask)
    for k in (10, 100):
        def rank_then_mask():
            ranking, _, _ = eng.rank_candidates(hidden, None, None, None, n_candidates=V, n_rows=R)
            allowed = mask.repeat(R, 1)
            allowed[:, :SPECIAL_IDS] = False
            allowed.scatter_(1, seen, False)
            keep = allowed.gather(1, ranking)
            sel = keep & (keep.cumsum(1) <= k)
            return ranking[sel].view(R, k)

        legs = {
            "unfiltered_ms": lambda: eng.rank_full(hidden, None, seen, SPECIAL_IDS, None, k),
            "all_ones_ms": lambda: eng.rank_full(hidden, None, seen, SPECIAL_IDS, None, k, allow=ones),
            "tenth_ms": lambda: eng.rank_full(hidden, None, seen, SPECIAL_IDS, None, k, allow=tenth),
            "cosine_neighbours_ms": lambda: eng.item_neighbours(query, k, "cosine"),
            "rank_then_mask_ms": rank_then_mask,
        }
        assert torch.equal(legs["unfiltered_ms"]()[0], legs["all_ones_ms"]()[0]), "an all-ones filter changed the answer"
        assert torch.equal(legs["tenth_ms"]()[0], rank_then_mask()), "the two filtered paths disagree"
        times = {name: [] for name in legs}
        for f in legs.values():
            for _ in range(3):
                f()
        for _ in range(5):   # alternated repeats
            for name, f in legs.items():
                times[name].append(time_ms(f))
        row = {"R": R, "H": H, "V": V, "k": k, **{name: round(sorted(t)[2], 4) for name, t in times.items()}}
        results.append(row)
        print("R %d H %d V %6d k %3d: unfiltered %7.3f  all-ones %7.3f  10 %% %7.3f  cosine neighbours %7.3f  rank + mask %8.3f ms"
              % (R, H, V, k, row["unfiltered_ms"], row["all_ones_ms"], row["tenth_ms"], row["cosine_neighbours_ms"],
                 row["rank_then_mask_ms"]), flush=True)
    del eng
    torch.cuda.empty_cache()
print(json.dumps({"bench_item_neighbours": results}))
