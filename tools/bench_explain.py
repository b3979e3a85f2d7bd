"""Occlusion explanations for 256 users (Recommender.explain_batch / BERT4RecModel.explain_tensor: the occluded rows are built on
the device, one host synchronisation at entry, one read-back) beside the loop a user would write without them: one
score_distribution_tensor call per recency index, on the prepare_inference batch of every history without that item (re-tokenise,
upload, read back every time), in the same run, on the ML-1M-64 and ML-20M-256 encoder configurations with vocabularies of 3 709 and
26 732 (a synthetic log; the vocabulary is padded to the catalogue size).  The top 10 of every user are explained at window 10 and
over all history (L - 1 = 199 items).
  explain_batch    wall time of one Recommender.explain_batch call (host work, upload, device loop, one read-back, detokenise)
  explain_tensor   wall time of one BERT4RecModel.explain_tensor call on the uploaded batch, its result left on the device
  host loop        wall time of the window + 1 score_distribution_tensor calls and the selection in numpy
  breakdown        one explain_tensor call under the library's launch timer (b4r_timing_begin / _end), its launches summed into
                   forward (encoder + transform), sweep (b4r_rank_full, b4r_score_dist), occlude (b4r_occlude_rows) and select
                   (b4r_attribution_select); a torch copy between two launches counts to the launch after it
  agreement        explain_tensor's top units and deltas against the host loop's: bit for bit where a chunk's forward has the host
                   loop's row count (rows_per_forward = users); a forward over more rows may take other launch forms, whose hidden
                   states differ in the last bits, so the default chunking is reported by the units it names and the largest
                   difference of a delta
python tools/bench_explain.py [users].  Every shape is warmed first; every wall time is the median of 5 alternated rounds with the
smallest and the largest round as its spread, synchronised inside the timed window.  Prints one line per leg, then a JSON line."""
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
K, TOP = 10, 3
KEYS = ("input_word_ids", "input_mask", "masked_lm_positions", "masked_lm_weights")


def wall_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def breakdown(model, batch, target, window):
    """microseconds of one explain_tensor call by launch label"""
    lib = _lib.load()
    cap, stride = 32768, 128
    torch.cuda.synchronize()
    _lib.check(lib.b4r_timing_begin(torch.cuda.current_stream().cuda_stream, cap), "b4r_timing_begin")
    model.explain_tensor(batch, target, top=TOP, window=window)
    n, us, names = C.c_int32(0), (C.c_float * cap)(), C.create_string_buffer(cap * stride)
    _lib.check(lib.b4r_timing_end(C.byref(n), us, names, stride, cap), "b4r_timing_end")
    parts = {"forward": 0.0, "sweep": 0.0, "occlude": 0.0, "select": 0.0}
    for j in range(n.value):
        label = names.raw[j * stride:(j + 1) * stride].split(b"\0", 1)[0].decode()
        kind = "sweep" if label.startswith(("b4r_rank_full", "b4r_score_dist")) else "occlude" if label.startswith("b4r_occlude_rows") else \
            "select" if label.startswith("b4r_attribution_select") else "forward"
        parts[kind] += us[j]
    return {k: round(v, 2) for k, v in parts.items()}, n.value


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

    def prepared(hs):
        parts = [dl.prepare_inference(list(h)) for h in hs]
        return {k: torch.from_numpy(np.concatenate([np.asarray(p[k]) for p in parts], axis=0)) for k in KEYS}

    batch = prepared(histories)
    batch_d = {k: v.cuda() for k, v in batch.items()}
    target = model.recommend_tensor(batch, k=K)[0]
    windows = [list(h[-(L - 1):]) for h in histories]

    def host_loop(window):
        """what a user would write with the existing calls: returns (top_w, top_delta) [users, K, TOP]"""
        kw = dict(query_ids=target, exclude_seen=False, exclude=batch["input_word_ids"])
        base = model.score_distribution_tensor(batch, **kw)["logp"].cpu().numpy()
        occ = np.full((USERS, window, K), -np.inf, np.float32)
        for w in range(window):
            rows = [win[:len(win) - 1 - w] + win[len(win) - w:] if w < len(win) else win for win in windows]
            lp = model.score_distribution_tensor(prepared(rows), **kw)["logp"].cpu().numpy()
            has = np.asarray([w < len(win) for win in windows])
            occ[:, w] = np.where(has[:, None], lp, -np.inf)
        delta = np.where(np.isfinite(occ) & np.isfinite(base[:, None, :]), base[:, None, :] - occ, -np.inf).transpose(0, 2, 1)
        order = np.argsort(-delta, axis=2, kind="stable")[:, :, :TOP]
        return order.astype(np.int32), np.take_along_axis(delta, order, axis=2)

    for window in (10, L - 1):
        legs = {"explain_batch": lambda: rec.explain_batch(histories, k=K, top=TOP, window=window),
                "explain_tensor": lambda: model.explain_tensor(batch_d, target, top=TOP, window=window),
                "host_loop": lambda: host_loop(window)}
        outs = {k: f() for k, f in legs.items()}       # warm-up: workspaces, scratch buffers, launch plans of every shape
        want_w, want_d = outs["host_loop"]

        def against_host_loop(got):
            """(the deltas are equal in every bit, the share of (user, item) lists that name the same units, the largest |difference|)"""
            got_w, got_d = got["top_w"].cpu().numpy(), got["top_delta"].cpu().numpy()
            both = np.isfinite(got_d) & np.isfinite(want_d)
            with np.errstate(invalid="ignore"):
                gap = np.where(both, np.abs(got_d - want_d), 0.0).max()
            return bool(np.array_equal(got_d, want_d)), float((got_w == want_w).all(axis=2).mean()), float(gap)

        # chunks of one recency index have the host loop's row count; the default chunks hold four of them in one forward
        same_rows, same = against_host_loop(model.explain_tensor(batch_d, target, top=TOP, window=window, rows_per_forward=USERS)), \
            against_host_loop(outs["explain_tensor"])
        t = {k: [] for k in legs}
        for _ in range(ROUNDS):
            for k, f in legs.items():
                t[k].append(wall_ms(f)[0])
        med = {k: sorted(v)[ROUNDS // 2] for k, v in t.items()}
        row = {"config": name, "V": V, "users": USERS, "L": L, "k": K, "top": TOP, "window": window,
               "host_loop_agreement": dict(zip(("same_bits", "same_units", "max_abs_diff"), same)),
               "host_loop_agreement_one_index_per_forward": dict(zip(("same_bits", "same_units", "max_abs_diff"), same_rows))}
        for k in legs:
            row[k + "_ms"] = round(med[k], 3)
            row[k + "_spread_ms"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
        parts, launches = breakdown(model, batch_d, target, window)
        total = sum(parts.values())
        row["breakdown_us"] = parts
        row["launch_marks"] = launches
        row["occlude_select_share"] = round((parts["occlude"] + parts["select"]) / total, 4) if total else None
        results.append(row)
        print("%s V %d users %d window %3d: explain_batch %8.2f ms [%.2f, %.2f]   explain_tensor %8.2f ms [%.2f, %.2f]   host loop %9.2f ms "
              "[%.2f, %.2f]   against the host loop: same units %.4f, max |delta diff| %.2e (one index per forward: %.4f, %.2e)" % (name, V, USERS, window, med["explain_batch"], min(t["explain_batch"]), max(t["explain_batch"]),
                                                  med["explain_tensor"], min(t["explain_tensor"]), max(t["explain_tensor"]), med["host_loop"],
                                                  min(t["host_loop"]), max(t["host_loop"]), same[1], same[2], same_rows[1], same_rows[2]), flush=True)
        print("    one explain_tensor call: forward %.1f us   sweep %.1f us   occlude %.1f us   select %.1f us   (occlude + select %.2f %% of "
              "the call's launches)" % (parts["forward"], parts["sweep"], parts["occlude"], parts["select"],
                                        100.0 * row["occlude_select_share"]), flush=True)
    del model, rec
    torch.cuda.empty_cache()
print(json.dumps({"bench_explain": results}))
