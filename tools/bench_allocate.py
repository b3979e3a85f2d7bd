"""The stock-aware allocation (Engine.allocate, b4r_allocate) beside the host route on the same pools, in the same run: R = 256 / 1 024 /
4 096 users, pools of M = 100 with k = 10, catalogues of V = 3 709 and 26 732, and three kinds of stock -- one unit of every item, ten
units of every item, and a "coupon" catalogue in which 1 % of the items are limited (R / 20 units each) and the rest are not.  The
pools are synthetic: every user's M best of popularity (Zipf, exponent 1) plus personal Gumbel noise, the noisy log popularity being
the utility, so that the head of the catalogue is contended as it is in practice.
  settle_ms    wall time of Engine.allocate(max_rounds=None): rounds enqueued 32 at a time, 4 bytes read back per chunk
  rounds       the rounds until a round rejects nothing (counted once, with rounds = 1 and resume)
  device_ms    device events around one call that enqueues exactly `rounds` rounds and reads nothing back
  host_ms      the route without the call: read the pools back, walk the edges greedily in numpy order on the host, upload the lists
  identical    the host walk and the device agree on every list (it must be true)
python tools/bench_allocate.py [out.json].  Every time is the median of 5 alternated rounds after a warm-up, with [smallest, largest].
Prints one line per cell, then a JSON line; with out.json the same JSON goes there."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4rec_amd import _lib  # noqa: E402
from bert4rec_amd.engine import ALLOCATE_UNLIMITED, Engine, _ptr, _stream, make_model_config  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
ROUNDS, M, K = 5, 100, 10
DEV = torch.device("cuda")


def stats(v):
    return round(sorted(v)[len(v) // 2], 4), [round(min(v), 4), round(max(v), 4)]


def wall_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def device_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def make_pools(R, V, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    logpop = -torch.log(torch.arange(1, V + 1, device=DEV, dtype=torch.float32))
    logpop[:3] = float("-inf")                                        # the special ids are never in a pool
    ids, util = [], []
    for r0 in range(0, R, 512):
        n = min(512, R - r0)
        u = torch.rand((n, V), generator=g, device=DEV).clamp_(1e-9, 1 - 1e-7)
        s = logpop[None, :] - torch.log(-torch.log(u))
        top = torch.topk(s, M, dim=1)
        ids.append(top.indices), util.append(top.values)
    return torch.cat(ids).contiguous(), torch.cat(util).contiguous()


def host_greedy(ids, util, cap):
    """the walk on the host: one sort of all edges (utility descending, row, position), one pass"""
    R, Mn = ids.shape
    order = np.lexsort((np.tile(np.arange(Mn), R), np.repeat(np.arange(R), Mn), -(util.reshape(-1) + np.float32(0.0))))
    left = cap.astype(np.int64)
    row_n = np.zeros(R, np.int64)
    out = np.full((R, K), -1, np.int64)
    pos = np.full((R, K), Mn, np.int64)
    flat = ids.reshape(-1)
    for e in order.tolist():
        r, j = e // Mn, flat[e]
        if row_n[r] < K and left[j] > 0:
            pos[r, row_n[r]] = e - r * Mn
            row_n[r] += 1
            left[j] -= 1
    pos.sort(axis=1)                                                  # ascending pool position
    for r in range(R):
        out[r, :row_n[r]] = ids[r, pos[r, :row_n[r]]]
    return out


def count_rounds(eng, ids, util, cap, V):
    R = ids.shape[0]
    lib = eng.lib
    sc = torch.empty(int(lib.b4r_allocate_scratch_bytes(R, M, K, V)), dtype=torch.uint8, device=DEV)
    uns = torch.zeros(1, dtype=torch.int32, device=DEV)
    n = 0
    while True:
        _lib.check(lib.b4r_allocate(_ptr(ids), _ptr(util), R, M, K, V, _ptr(cap), None, 1, 0 if n == 0 else 1, None, None, None, None, None,
                                    _ptr(uns), _ptr(sc), sc.numel(), _stream(DEV)), "b4r_allocate")
        n += 1
        if int(uns.item()) == 0:
            return n


cells = []
for V in (3709, 26732):
    eng = Engine(make_model_config(V, 64, 2, 2, 32, 256, 0.0, 0.0), DEV)
    for R in (256, 1024, 4096):
        ids, util = make_pools(R, V, seed=R + V)
        stocks = {"capacity 1": np.ones(V, np.int32), "capacity 10": np.full(V, 10, np.int32)}
        coupon = np.full(V, ALLOCATE_UNLIMITED, np.int32)
        coupon[3 + np.random.default_rng(V).choice(V // 4, size=V // 100, replace=False)] = max(R // 20, 1)   # limited items from the popular quarter
        stocks["coupons 1 %"] = coupon
        for name, cap_h in stocks.items():
            cap = torch.from_numpy(cap_h).to(DEV)
            rounds = count_rounds(eng, ids, util, cap, V)

            def host_route():
                got = host_greedy(ids.cpu().numpy(), util.cpu().numpy(), cap_h)
                return torch.from_numpy(got).to(DEV)

            t = {"settle": [], "device": [], "host": []}
            for r in range(ROUNDS + 1):                                # round 0 is the warm-up
                ms_s, got = wall_ms(lambda: eng.allocate(ids, util, K, cap))
                ms_d, fixed = device_ms(lambda: eng.allocate(ids, util, K, cap, max_rounds=rounds))
                ms_h, want = wall_ms(host_route)
                if r:
                    t["settle"].append(ms_s), t["device"].append(ms_d), t["host"].append(ms_h)
            same = bool(torch.equal(got[0], want)) and bool(torch.equal(fixed[0], want)) and int(fixed[5].item()) == 0
            row = {"R": R, "M": M, "K": K, "V": V, "stock": name, "rounds": rounds, "identical": same,
                   "assigned": int(got[3].sum()), "rows_short_of_k": int((got[3] < K).sum())}
            for k, v in t.items():
                row[k + "_ms"], row[k + "_range_ms"] = stats(v)
            row["host_over_settle"] = round(row["host_ms"] / row["settle_ms"], 2)
            cells.append(row)
            print("V %5d R %4d %-12s: rounds %3d   settle %9.3f ms %s   device %9.3f ms %s   host route %10.3f ms %s   host / settle %8.2f%s"
                  % (V, R, name, rounds, row["settle_ms"], row["settle_range_ms"], row["device_ms"], row["device_range_ms"], row["host_ms"],
                     row["host_range_ms"], row["host_over_settle"], "" if same else "   THE LISTS DIFFER"), flush=True)
    del eng
    torch.cuda.empty_cache()
result = {"tool": "tools/bench_allocate.py", "bench_allocate": cells}
print(json.dumps(result))
if OUT:
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
