"""Joint recommendations for 256 parties of 2 / 4 / 16 members, k = 10 (Engine.rank_joint: one b4r_rank_joint sweep that reduces over a
party's members before it selects, no [R, V] scores) beside what a user would write without it and beside the sweep it is built
from, on the same hidden states of width 128 over catalogues of 3 709, 26 732 and 335 423 items (random hidden rows, the model's
initial item table, 50 seen items per member):
  joint        b4r_rank_joint alone, the members' normalisers given (additive, calibrated)
  dist+joint   what recommend_joint_tensor runs after its forward: b4r_score_dist for the normalisers, then b4r_rank_joint
  rank_full    b4r_rank_full(k = 10) on the same R = members x parties rows: the same products, one list per ROW -- the yardstick
  torch        [R, V] logits (one matmul), the seen and special ids masked, log_softmax, the sum over the members, torch.topk
  agreement    the share of (party, place) cells where joint and torch name the same item (torch's scores come from another
               summation order, so near-ties may swap)
python tools/bench_joint.py.  Every shape is warmed first; every wall time is the median of 5 alternated rounds with the smallest and
the largest round as its spread, synchronised inside the timed window.  Prints one line per leg, then a JSON line."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4rec_amd import config, engine as engine_mod, models  # noqa: E402
from bert4rec_amd.models.components import networks  # noqa: E402

PARTIES = 256
MEMBERS = (2, 4, 16)
K = 10
SEEN = 50
ROUNDS = 5
FIRST = engine_mod.SPECIAL_IDS


def wall_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


results = []
for V in (3709, 26732, 335423):
    cfg = config.get_encoder_config("ml-1m_128")
    model = models.BERT4RecModel(networks.Bert4RecEncoder(V, seed=1, **{**cfg, "attention_dropout": 0.0, "output_dropout": 0.0}))
    eng = model.engine
    width = eng.embedding_width
    table, bias = eng.view("word_embeddings/embeddings"), eng.view("cls/predictions/output_bias/bias")
    for M in MEMBERS:
        R = PARTIES * M
        gen = torch.Generator(device="cuda").manual_seed(V + M)
        hidden = torch.randn((R, width), generator=gen, device="cuda", dtype=torch.float32)
        seen = torch.randint(FIRST, V, (R, SEEN), generator=gen, device="cuda", dtype=torch.int64)
        parties = torch.arange(R, dtype=torch.int64).reshape(PARTIES, M)
        lse = eng.score_distribution(hidden, None, seen, FIRST, None)[2]

        def joint():
            return eng.rank_joint(hidden, None, seen, FIRST, parties, K, "additive", row_lse=lse)

        def dist_joint():
            own = eng.score_distribution(hidden, None, seen, FIRST, None)[2]
            return eng.rank_joint(hidden, None, seen, FIRST, parties, K, "additive", row_lse=own)

        def rank_full():
            return eng.rank_full(hidden, None, seen, FIRST, None, K)

        def torch_path():
            logits = torch.addmm(bias.reshape(1, V), hidden, table.t())
            logits[:, :FIRST] = float("-inf")
            logits.scatter_(1, seen, float("-inf"))
            logp = torch.log_softmax(logits, dim=1)
            return torch.topk(logp.reshape(PARTIES, M, V).sum(dim=1), K, dim=1)

        legs = {"joint": joint, "dist_joint": dist_joint, "rank_full": rank_full, "torch": torch_path}
        outs = {k: f() for k, f in legs.items()}       # warm-up: scratch buffers of every shape, torch's allocator
        same = float((outs["joint"][0] == outs["torch"].indices).double().mean())
        t = {k: [] for k in legs}
        for _ in range(ROUNDS):
            for k, f in legs.items():
                t[k].append(wall_ms(f)[0])
        med = {k: sorted(v)[ROUNDS // 2] for k, v in t.items()}
        row = {"V": V, "width": width, "parties": PARTIES, "members": M, "rows": R, "k": K, "same_items": round(same, 6),
               "logits_bytes": R * V * 4}
        for k in legs:
            row[k + "_ms"] = round(med[k], 3)
            row[k + "_spread_ms"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
        results.append(row)
        print("V %d, %d parties of %d (R = %d): " % (V, PARTIES, M, R) +
              "   ".join("%s %.3f ms [%.3f, %.3f]" % (k, med[k], min(t[k]), max(t[k])) for k in legs) +
              "   same items %.4f" % same, flush=True)
        del outs
    del model, eng, table, bias
    torch.cuda.empty_cache()
print(json.dumps({"bench_joint": results}))
