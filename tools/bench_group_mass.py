"""Category affinity for R users (b4r_group_mass: the probability mass and the item count of every item group, given the rows'
normalisers) beside two yardsticks over the same hidden states and exclusions, in the same run:
  b4r_score_dist        the same products without the grouping (count, maximum, normaliser, entropy; no queries)
  torch on the device   logits = hidden @ table.T + bias as an [R, V] buffer, masked_fill of the disallowed ids, softmax, index_add_ by label
python tools/bench_group_mass.py [R [H]].  Labels per V:
  20 by rank     label = rank * 20 // V: few large groups, every wave of the sweep sees one label (two at a boundary)
  20 scattered   a random label in [0, 20) per item: every wave sees all 20 labels, about 3 lanes each
  5000           a random label in [0, 5000): a brand list, 20 windows of 256 groups, each found in every chunk
  per item       label = id up to the limit of 65536 groups (the ids beyond are the rest): one window per chunk does the work
What is timed: the enqueue-to-completion time of one call between two device events, the median of 20 calls, then the median of 5 such
rounds taken alternately over the paths, with the smallest and the largest round.  Prints one line per (V, labels), then a JSON line."""
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
    banned = torch.zeros(R, V, dtype=torch.bool, device="cuda")
    banned[:, :SPECIAL_IDS] = True
    banned.scatter_(1, seen, True)
    rank = torch.arange(V, device="cuda")
    legs = (("20 by rank", (rank * 20 // V).to(torch.int32), 20),
            ("20 scattered", torch.randint(0, 20, (V,), device="cuda", generator=g, dtype=torch.int32), 20),
            ("5000", torch.randint(0, 5000, (V,), device="cuda", generator=g, dtype=torch.int32), 5000),
            ("per item", rank.to(torch.int32), min(V, 65536)))
    dist = lambda: eng.score_distribution(hidden, None, seen, SPECIAL_IDS, None)
    lse = dist()[2]
    for name, labels, G in legs:
        mass = lambda: eng.group_mass(hidden, None, seen, SPECIAL_IDS, lse, labels, G)
        index = labels.to(torch.int64).clamp(max=G)       # the labels beyond G: one more column, dropped

        def eager():
            logits = hidden @ table.T + bias
            p = torch.softmax(logits.masked_fill(banned, float("-inf")), dim=1)
            return torch.zeros(R, G + 1, device="cuda").index_add_(1, index, p)[:, :G]

        got = mass()[0].to(torch.float64) / float(1 << 40)
        gap = float((got - eager().to(torch.float64)).abs().max())
        assert gap < 1e-4, f"the two group sums disagree by {gap}"
        for _ in range(3):
            mass(); dist(); eager()
        t = {"mass": [], "dist": [], "eager": []}
        for _ in range(5):   # alternated repeats
            t["mass"].append(time_ms(mass)); t["dist"].append(time_ms(dist)); t["eager"].append(time_ms(eager))
        tm, td, te = (sorted(t[k])[2] for k in ("mass", "dist", "eager"))
        results.append({"R": R, "H": H, "V": V, "labels": name, "G": G, "group_mass_ms": round(tm, 4), "score_dist_ms": round(td, 4),
                        "torch_softmax_index_add_ms": round(te, 4), "group_mass_spread_ms": [round(min(t["mass"]), 4), round(max(t["mass"]), 4)],
                        "score_dist_spread_ms": [round(min(t["dist"]), 4), round(max(t["dist"]), 4)],
                        "torch_spread_ms": [round(min(t["eager"]), 4), round(max(t["eager"]), 4)]})
        print("R %d H %d V %6d labels %-12s G %5d: b4r_group_mass %8.3f ms [%.3f, %.3f]   b4r_score_dist %8.3f ms   torch softmax + index_add_ %8.3f ms"
              % (R, H, V, name, G, tm, min(t["mass"]), max(t["mass"]), td, te), flush=True)
    del eng
    torch.cuda.empty_cache()
print(json.dumps({"bench_group_mass": results}))
