"""Multi-step roll-outs for 256 users (Recommender.recommend_sequences: the items are appended on the device between the forwards,
one read-back) beside the same greedy paths from a Python loop over Recommender.recommend_batch(k=1) per step (detokenise, append,
re-tokenise, re-upload and read back every step), in the same run, on the ML-1M-64 and ML-20M-256 encoder configurations with
vocabularies of 3 709 and 26 732 (a synthetic log; the vocabulary is padded to the catalogue size), steps 5 and 10.
  device greedy / device beams=4   wall time of one recommend_sequences call (host work, upload, device loop, one read-back)
  host loop                        wall time of `steps` recommend_batch(k=1) calls (greedy only)
  breakdown                        one recommend_sequence_tensor call under the library's launch timer (b4r_timing_begin / _end), its
                                   launches summed per step into forward (encoder + transform), sweep (b4r_rank_full and
                                   b4r_score_dist), select (b4r_beam_select) and advance (b4r_rollout_advance); a torch copy between
                                   two launches counts to the launch after it
python tools/bench_rollout.py [users].  Every wall time is the median of 5 alternated rounds with the smallest and the largest round as
its spread.  Prints one line per leg, then a JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4rec_amd import _lib, config, dataloaders, datasets, models  # noqa: E402
from bert4rec_amd.apps import Recommender  # noqa: E402
from bert4rec_amd.models.components import networks  # noqa: E402

USERS = int(sys.argv[1]) if len(sys.argv) > 1 else 256
ROUNDS = 5


def wall_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def breakdown(model, batch, steps, beams):
    """per-step microseconds of the device loop by launch label"""
    lib = _lib.load()
    cap, stride = 8192, 128
    torch.cuda.synchronize()
    _lib.check(lib.b4r_timing_begin(torch.cuda.current_stream().cuda_stream, cap), "b4r_timing_begin")
    model.recommend_sequence_tensor(batch, steps, beams=beams)
    n, us, names = C.c_int32(0), (C.c_float * cap)(), C.create_string_buffer(cap * stride)
    _lib.check(lib.b4r_timing_end(C.byref(n), us, names, stride, cap), "b4r_timing_end")
    parts = {"forward": 0.0, "sweep": 0.0, "select": 0.0, "advance": 0.0}
    for j in range(n.value):
        label = names.raw[j * stride:(j + 1) * stride].split(b"\0", 1)[0].decode()
        kind = "sweep" if label.startswith(("b4r_rank_full", "b4r_score_dist", "b4r_sample_full")) else \
            "select" if label.startswith("b4r_beam_select") else "advance" if label.startswith("b4r_rollout_advance") else "forward"
        parts[kind] += us[j]
    return {k: round(v / steps, 2) for k, v in parts.items()}, n.value


results = []
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
        n = int(rng.integers(20, L + 40))
        s = int(rng.integers(0, len(items) - n))
        histories.append(items[s:s + n])
    batch = {k: torch.from_numpy(np.concatenate([np.asarray(dl.prepare_inference(list(h))[k]) for h in histories], axis=0))
             for k in ("input_word_ids", "input_mask", "masked_lm_positions", "masked_lm_weights")}

    def host_loop(steps):
        seqs = [list(h) for h in histories]
        for _ in range(steps):
            for s, nxt in zip(seqs, rec.recommend_batch(seqs, k=1)):
                if nxt is not None:
                    s.append(nxt)
        return [s[len(h):] for s, h in zip(seqs, histories)]

    for steps in (5, 10):
        legs = {"device_greedy": lambda: rec.recommend_sequences(histories, steps),
                "host_loop": lambda: host_loop(steps),
                "device_beams4": lambda: rec.recommend_sequences(histories, steps, beams=4)}
        outs = {k: f() for k, f in legs.items()}       # warm-up: workspaces, scratch buffers
        same = outs["device_greedy"] == outs["host_loop"]
        t = {k: [] for k in legs}
        for _ in range(ROUNDS):
            for k, f in legs.items():
                t[k].append(wall_ms(f)[0])
        med = {k: sorted(v)[ROUNDS // 2] for k, v in t.items()}
        row = {"config": name, "V": V, "users": USERS, "L": L, "steps": steps, "same_paths_as_host_loop": same}
        for k in legs:
            row[k + "_ms"] = round(med[k], 3)
            row[k + "_spread_ms"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
        for beams in (1, 4):
            parts, launches = breakdown(model, batch, steps, beams)
            total = sum(parts.values())
            row["breakdown_beams%d_us_per_step" % beams] = parts
            row["launch_marks_beams%d" % beams] = launches
            row["select_advance_share_beams%d" % beams] = round((parts["select"] + parts["advance"]) / total, 4) if total else None
        results.append(row)
        print("%s V %d users %d steps %2d: device greedy %8.2f ms [%.2f, %.2f]   host loop %8.2f ms [%.2f, %.2f]   device beams=4 %8.2f ms "
              "[%.2f, %.2f]   same paths %s" % (name, V, USERS, steps, med["device_greedy"], min(t["device_greedy"]), max(t["device_greedy"]),
                                               med["host_loop"], min(t["host_loop"]), max(t["host_loop"]), med["device_beams4"],
                                               min(t["device_beams4"]), max(t["device_beams4"]), same), flush=True)
        for beams in (1, 4):
            p = row["breakdown_beams%d_us_per_step" % beams]
            print("    device loop, beams=%d, per step: forward %.1f us   sweep %.1f us   select %.1f us   advance %.1f us   (select + advance "
                  "%.1f %% of the step)" % (beams, p["forward"], p["sweep"], p["select"], p["advance"],
                                            100.0 * row["select_advance_share_beams%d" % beams]), flush=True)
    del model, rec
    torch.cuda.empty_cache()
print(json.dumps({"bench_rollout": results}))
