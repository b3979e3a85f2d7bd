"""The session store (Recommender.open_sessions: histories on the device, b4r_history_append / b4r_history_batch) beside
Recommender.recommend_batch on the same 256 users, in the same run, on the ML-1M-64 and ML-20M-256 encoder configurations with
vocabularies of 3 709 and 26 732 (a synthetic log; the vocabulary is padded to the catalogue size), histories of U{5..200} items, k = 10.
  recommend_batch      wall time of recommend_batch(sequences): tokenise and prepare every history on the host, upload, forward, sweep,
                       read-back, detokenise
  store                wall time of sessions.append(one new event per user) followed by sessions.recommend(keys)
  _requests / requests the request preparation alone, on the host and from the store (ending in a device synchronise)
  identical lists      the fraction of the users whose list is the same on both paths (it must be 1)
  device times         b4r_history_append at N = 256, 4 096 and 65 536 (spread over the users, and all on one user) and
                       b4r_history_batch at R = 256 and 1 024 with L = 200, C = 256 and 1 024, by device events around a captured graph of
                       10 back-to-back calls, next to the bytes the call has to move
python tools/bench_session_store.py [users] [out.json].  Every time is the median of 5 alternated rounds after a warm-up, with the
smallest and the largest round as its spread.  Prints one line per leg, then a JSON line; with out.json the same JSON goes there."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4rec_amd import config, dataloaders, datasets, models  # noqa: E402
from bert4rec_amd.apps import Recommender  # noqa: E402
from bert4rec_amd.models.components import networks  # noqa: E402

USERS = int(sys.argv[1]) if len(sys.argv) > 1 else 256
OUT = sys.argv[2] if len(sys.argv) > 2 else None
ROUNDS, K = 5, 10


def wall_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def device_timer(f, calls=10):
    """`calls` back-to-back calls of f captured in one graph, so that the host's enqueue rate (about 20 us per call from Python) is
    not what the device events see.  Returns a function that replays the graph and gives the microseconds per call."""
    f()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for _ in range(calls):
                f()
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()

    def once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / calls
    return once


def stats(v):
    return round(sorted(v)[len(v) // 2], 3), [round(min(v), 3), round(max(v), 3)]


wall, engine = [], None
for name, V in (("ml-1m_64", 3709), ("ml-20m_256", 26732)):
    cfg = config.get_encoder_config(name)
    L = cfg["max_sequence_length"]
    ds = datasets.synthetic_dataset(n_users=max(USERS, 64), n_items=V - 3, min_len=20, max_len=L, seed=0)
    dl = dataloaders.get_dataloader_factory("bert4rec").create_ml_1m_dataloader(data_source=ds, max_seq_len=L)
    dl.generate_vocab()
    tok = dl.get_tokenizer()
    pad = 0
    while tok.get_vocab_size() < V:                    # items nobody interacted with yet: the catalogue is larger than the log
        tok.tokenize("unseen-item-%d" % pad)
        pad += 1
    model = models.BERT4RecModel(networks.Bert4RecEncoder(V, seed=1, **{**cfg, "attention_dropout": 0.0, "output_dropout": 0.0}))
    rec = Recommender(model, dl)
    items = dl.create_item_list()
    rng = np.random.default_rng(0)
    histories = []
    for u in range(USERS):
        n = int(rng.integers(5, 201))
        s = int(rng.integers(0, len(items) - n - 2 * ROUNDS - 2))
        histories.append(list(items[s:s + n]))
    keys = ["user-%d" % u for u in range(USERS)]
    sessions = rec.open_sessions(USERS)
    log = [(keys[u], h[t]) for t in range(200) for u, h in enumerate(histories) if t < len(h)]
    assert sessions.append([k for k, _ in log], [i for _, i in log]) == len(log)
    t = {k: [] for k in ("recommend_batch", "store", "_requests", "requests")}
    same = []
    for r in range(ROUNDS + 1):                       # round 0 is the warm-up: workspaces, scratch buffers
        new = [items[int(rng.integers(0, len(items)))] for _ in range(USERS)]      # one new event per user, for both paths
        for h, item in zip(histories, new):
            h.append(item)
        ms_b, want = wall_ms(lambda: rec.recommend_batch(histories, k=K))
        ms_s, got = wall_ms(lambda: (sessions.append(keys, new), sessions.recommend(keys, k=K))[1])
        ms_hr, _ = wall_ms(lambda: rec._requests(histories))
        ms_sr, _ = wall_ms(lambda: sessions.requests(keys))
        if r:
            t["recommend_batch"].append(ms_b), t["store"].append(ms_s), t["_requests"].append(ms_hr), t["requests"].append(ms_sr)
            same.append(sum(a == b for a, b in zip(got, want)) / USERS)
    row = {"config": name, "V": V, "users": USERS, "L": L, "k": K, "history_capacity": sessions.history_capacity,
           "identical_lists": min(same)}
    for k, v in t.items():
        row[k + "_ms"], row[k + "_spread_ms"] = stats(v)
    row["store_faster"] = row["store_ms"] < row["recommend_batch_ms"]
    wall.append(row)
    print("%s V %d users %d: recommend_batch %8.3f ms %s   store append + recommend %8.3f ms %s%s   _requests %8.3f ms   requests %8.3f ms   "
          "identical lists %.4f" % (name, V, USERS, row["recommend_batch_ms"], row["recommend_batch_spread_ms"], row["store_ms"],
                                    row["store_spread_ms"], "" if row["store_faster"] else "  THE STORE IS NOT FASTER", row["_requests_ms"],
                                    row["requests_ms"], row["identical_lists"]), flush=True)
    engine = model.engine if engine is None else engine   # (the ML-1M engine serves the device times: its V bounds the items)
    del rec, sessions
    torch.cuda.empty_cache()

# ---- device times ---------------------------------------------------------------------------------------------------------------------
V = engine.cfg.vocab_size
dev = engine.device
rng = np.random.default_rng(1)
device = []
U, C = 100_000, 256
for N, pattern in ((256, "spread"), (4096, "spread"), (65536, "spread"), (65536, "one user")):
    state = engine.history_state(U, C)
    users = torch.from_numpy(rng.integers(0, U, size=N).astype(np.int32) if pattern == "spread" else np.zeros(N, np.int32)).to(dev)
    its = torch.from_numpy(rng.integers(3, V, size=N).astype(np.int64)).to(dev)
    acc = torch.empty(N, dtype=torch.int32, device=dev)
    timer = device_timer(lambda: engine.history_append(state, users, its, acc))
    us = [timer() for _ in range(ROUNDS)]
    # the events read once (12 N), the flags (4 N), the plan written and read (2 x 16 N), one count read per event (8 N), the stores
    # (at most 8 N into hist and 8 N into count); the N / 256 further passes over the 12 N bytes of events stay in the caches
    moved = 12 * N + 4 * N + 32 * N + 8 * N + 16 * N
    med, spread = stats(us)
    device.append({"call": "b4r_history_append", "N": N, "pattern": pattern, "U": U, "C": C, "us": med, "spread_us": spread, "bytes": moved,
                   "event_list_passes": -(-N // 256)})
    print("b4r_history_append N %6d %-8s: %10.2f us %s   %d bytes" % (N, pattern, med, spread, moved), flush=True)
for R in (256, 1024):
    for C in (256, 1024):
        U, L, P = 4096, 200, 40
        state = engine.history_state(U, C)
        state["count"].copy_(torch.from_numpy(rng.integers(5, 3 * C, size=U)).to(dev))
        state["hist"].copy_(torch.from_numpy(rng.integers(3, V, size=(U, C))).to(dev))
        req = torch.from_numpy(rng.integers(0, U, size=R).astype(np.int32)).to(dev)
        timer = device_timer(lambda: engine.history_batch(state, req, L, P, C))
        us = [timer() for _ in range(ROUNDS)]
        held = np.minimum(state["count"].cpu().numpy()[req.cpu().numpy()], C)
        # written: tokens and mask (16 L), positions and weights (16 P), exclusions (8 C), len and live (8); read: the request and the
        # count (12), the window and the exclusions out of the ring (8 per item)
        moved = int(R * (16 * L + 16 * P + 8 * C + 8 + 12) + 8 * (np.minimum(held, L - 1).sum() + held.sum()))
        med, spread = stats(us)
        device.append({"call": "b4r_history_batch", "R": R, "L": L, "P": P, "C": C, "E": C, "us": med, "spread_us": spread, "bytes": moved})
        print("b4r_history_batch R %5d L %d C %5d: %10.2f us %s   %d bytes" % (R, L, C, med, spread, moved), flush=True)
result = {"bench_session_store": {"wall": wall, "device": device}}
print(json.dumps(result))
if OUT:
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
