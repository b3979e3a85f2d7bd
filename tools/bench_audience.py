"""Audience selection over 16 384 synthetic users in batches of 1 024 (BERT4RecModel.audience_tensor: the K most likely users of each
of Q items, merged on the device while the batches go by, O(Q * K) state) beside the loop a user would write without it: the same
forward and b4r_score_dist sweep per batch, every batch's log probabilities stored into a [users, Q] device tensor, then one
torch.topk(dim=0) over it.  On the ML-1M-64 and ML-20M-256 encoder configurations with vocabularies of 3 709 and 26 732 (a synthetic
log; the vocabulary is padded to the catalogue size), for (Q, K) = (16, 100) and (256, 1000).
  audience      wall time of the audience_tensor loop over all batches (batches uploaded beforehand, the state left on the device)
  merge share   one such loop under the library's launch timer (b4r_timing_begin / _end): the b4r_audience_merge launches over all
                launches; a torch copy between two launches counts to the launch after it
  matrix+topk   wall time of the baseline loop on the same hidden states and of its torch.topk; its [users, Q] matrix grows with the
                user base, and its order under ties is whatever torch.topk gives
  agreement     the share of (item, rank) cells where both name the same user (ties may be ordered differently by torch.topk)
python tools/bench_audience.py [users].  Every shape is warmed first; every wall time is the median of 5 alternated rounds with the
smallest and the largest round as its spread, synchronised inside the timed window.  Prints one line per leg, then a JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4rec_amd import _lib, config, dataloaders, datasets, engine as engine_mod, models  # noqa: E402
from bert4rec_amd.models.components import networks  # noqa: E402

USERS = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
BATCH = 1024
ROUNDS = 5
SHAPES = ((16, 100), (256, 1000))
KEYS = ("input_word_ids", "input_mask", "masked_lm_positions", "masked_lm_weights")


def wall_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def merge_share(loop):
    """(microseconds of the b4r_audience_merge launches, of all launches, launch marks) of one loop"""
    lib = _lib.load()
    cap, stride = 32768, 128
    torch.cuda.synchronize()
    _lib.check(lib.b4r_timing_begin(torch.cuda.current_stream().cuda_stream, cap), "b4r_timing_begin")
    loop()
    n, us, names = C.c_int32(0), (C.c_float * cap)(), C.create_string_buffer(cap * stride)
    _lib.check(lib.b4r_timing_end(C.byref(n), us, names, stride, cap), "b4r_timing_end")
    merge = total = 0.0
    for j in range(n.value):
        label = names.raw[j * stride:(j + 1) * stride].split(b"\0", 1)[0].decode()
        total += us[j]
        if label.startswith("b4r_audience_merge"):
            merge += us[j]
    return merge, total, n.value


results = []
for name, V in (("ml-1m_64", 3709), ("ml-20m_256", 26732)):
    cfg = config.get_encoder_config(name)
    L = cfg["max_sequence_length"]
    ds = datasets.synthetic_dataset(n_users=256, n_items=V - 3, min_len=20, max_len=L, seed=0)
    dl = dataloaders.get_dataloader_factory("bert4rec").create_ml_1m_dataloader(data_source=ds, max_seq_len=L)
    dl.generate_vocab()
    tok = dl.get_tokenizer()
    pad = 0
    while tok.get_vocab_size() < V:                    # items nobody interacted with yet: the catalogue is larger than the log
        tok.tokenize("unseen-item-%d" % pad)
        pad += 1
    model = models.BERT4RecModel(networks.Bert4RecEncoder(V, seed=1, **{**cfg, "attention_dropout": 0.0, "output_dropout": 0.0}))
    items = dl.create_item_list()
    rng = np.random.default_rng(0)
    batches = []
    for b0 in range(0, USERS, BATCH):
        parts = []
        for u in range(b0, min(USERS, b0 + BATCH)):
            n = int(rng.integers(20, L + 40))
            s = int(rng.integers(0, len(items) - n))
            parts.append(dl.prepare_inference(list(items[s:s + n])))
        host = {k: torch.from_numpy(np.concatenate([np.asarray(p[k]) for p in parts], axis=0)) for k in KEYS}
        # the weights stay on the host: audience_tensor checks "one ranked slot per row" where they live, without a device sync
        batches.append({k: (v if k == "masked_lm_weights" else v.cuda()) for k, v in host.items()})
    P = int(batches[0]["masked_lm_positions"].shape[1])

    for Q, K in SHAPES:
        item_ids = torch.as_tensor(rng.choice(np.arange(3, V), size=Q, replace=False), dtype=torch.int64)
        queries = item_ids.cuda()

        def audience():
            state = None
            for batch in batches:
                state = model.audience_tensor(batch, item_ids, state=state, k=K)
            return state

        def matrix_topk():
            """the same forward and sweep per batch, the log probabilities kept: [users, Q], then the K best rows of every column"""
            big = torch.empty((USERS, Q), dtype=torch.float32, device="cuda")
            b0 = 0
            for batch in batches:
                B = int(batch["input_word_ids"].shape[0])
                slot = (batch["masked_lm_weights"].reshape(B, P) != 0).to(torch.int64).argmax(dim=1)
                slots = torch.arange(B, dtype=torch.int64, device="cuda") * P + slot.cuda()
                hidden, slots, _ = model._ranked_slot_hidden(batch, slots=slots)
                ex_rows = model._excluded_rows(batch, slots, True, None)
                big[b0:b0 + B] = model.engine.score_distribution(hidden, None, ex_rows, engine_mod.SPECIAL_IDS, None, None, None, 1.0,
                                                                 queries[None, :].expand(B, Q))[4]
                b0 += B
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            top = torch.topk(big, min(K, USERS), dim=0)
            torch.cuda.synchronize()
            matrix_topk.topk_ms = (time.perf_counter() - t0) * 1e3
            return top

        legs = {"audience": audience, "matrix_topk": matrix_topk}
        outs = {k: f() for k, f in legs.items()}       # warm-up: workspaces, scratch buffers, launch plans of every shape
        kk = min(K, USERS)
        same = float((outs["audience"]["users"][:, :kk].t() == outs["matrix_topk"].indices).double().mean())
        same_logp = bool(torch.equal(outs["audience"]["logp"][:, :kk].t(), outs["matrix_topk"].values))
        t = {k: [] for k in legs}
        topk_ms = []
        for _ in range(ROUNDS):
            for k, f in legs.items():
                t[k].append(wall_ms(f)[0])
            topk_ms.append(matrix_topk.topk_ms)
        med = {k: sorted(v)[ROUNDS // 2] for k, v in t.items()}
        merge_us, total_us, marks = merge_share(audience)
        row = {"config": name, "V": V, "users": USERS, "batch": BATCH, "Q": Q, "K": K, "same_users": round(same, 6), "same_logp": same_logp,
               "merge_us": round(merge_us, 1), "launches_us": round(total_us, 1), "merge_share": round(merge_us / total_us, 4) if total_us else None,
               "launch_marks": marks, "topk_ms": round(sorted(topk_ms)[ROUNDS // 2], 3), "state_bytes": Q * K * 12 + Q * 16,
               "matrix_bytes": USERS * Q * 4}
        for k in legs:
            row[k + "_ms"] = round(med[k], 3)
            row[k + "_spread_ms"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
        results.append(row)
        print("%s V %d users %d Q %d K %d: audience %8.2f ms [%.2f, %.2f]   matrix + topk %8.2f ms [%.2f, %.2f] (topk alone %.2f ms)   merge "
              "%.1f us of %.1f us of launches (%.2f %%), %.1f us per batch   same users %.4f, same logp %s" %
              (name, V, USERS, Q, K, med["audience"], min(t["audience"]), max(t["audience"]), med["matrix_topk"], min(t["matrix_topk"]),
               max(t["matrix_topk"]), row["topk_ms"], merge_us, total_us, 100.0 * (row["merge_share"] or 0.0), merge_us / len(batches), same,
               same_logp), flush=True)
    del model
    torch.cuda.empty_cache()
print(json.dumps({"bench_audience": results}))
