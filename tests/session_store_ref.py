"""The session store's two device calls (include/b4r.h: b4r_history_append, b4r_history_batch) restated in plain Python: one list per
user that only ever grows, no ring.  This is the definition the kernels are held to, bit for bit."""
import numpy as np


class RefStore:
    def __init__(self, U, C):
        self.U, self.C = U, C
        self.lists = [[] for _ in range(U)]            # every accepted item of the user, oldest first

    def append(self, users, items, V, first_item):
        """the events one at a time, in order; returns accepted [N] int32"""
        accepted = np.zeros(len(users), np.int32)
        for n, (u, it) in enumerate(zip(users, items)):
            u, it = int(u), int(it)
            if 0 <= u < self.U and first_item <= it < V:
                self.lists[u].append(it)
                accepted[n] = 1
        return accepted

    def count(self):
        return np.array([len(h) for h in self.lists], np.int64)

    def cells(self):
        """what the ring defines: {(u, position): item} for the last min(n, C) events of every user -- event n lives at n mod C"""
        out = {}
        for u, h in enumerate(self.lists):
            for n in range(max(0, len(h) - self.C), len(h)):
                out[(u, n % self.C)] = h[n]
        return out

    def batch(self, req, L, P, E, mask_id):
        R = len(req)
        out = dict(tokens=np.zeros((R, L), np.int64), mask=np.zeros((R, L), np.int64), len=np.zeros(R, np.int32),
                   positions=np.zeros((R, P), np.int64), weights=np.zeros((R, P), np.int64), exclude=np.full((R, E), -1, np.int64),
                   live=np.zeros(R, np.int32))
        for r, u in enumerate(req):
            u = int(u)
            live = 0 <= u < self.U
            known = self.lists[u][-self.C:] if live else []       # the store forgets what is older than C events
            window = known[-(L - 1):]
            h = len(window)
            out["tokens"][r, :h] = window
            out["tokens"][r, h] = mask_id
            out["mask"][r, :h + 1] = 1
            out["len"][r] = h + 1
            out["positions"][r, 0] = h
            out["weights"][r, 0] = 1
            ex = known[-E:]
            out["exclude"][r, :len(ex)] = ex
            out["live"][r] = int(live)
        return out


BATCH_OUTS = ("tokens", "mask", "len", "positions", "weights", "exclude", "live")


def log_patterns(U, C, V, N, first_item=3, seed=0):
    """The event logs of the append tests: name -> (users int32 [N], items int64 [N])"""
    rng = np.random.default_rng(seed + 1000 * U + N)
    items = rng.integers(first_item, V, size=N).astype(np.int64)
    j = np.arange(N)
    users_mod = (j % U).astype(np.int32)
    out = {
        "one_user": (np.full(N, U - 1, np.int32), items),                                   # the ring wraps inside one call when N > C
        "every_user_once": (np.arange(U, dtype=np.int32), rng.integers(first_item, V, size=U).astype(np.int64)),   # (U events, not N)
        "users_mod": (users_mod, items),
        "random_users": (rng.integers(0, U, size=N).astype(np.int32), items),
        "users_out_of_range": (np.where(j % 3 == 0, -1, np.where(j % 3 == 1, U, users_mod)).astype(np.int32), items),
        "items_out_of_range": (users_mod, np.where(j % 2 == 0, items, np.array([0, 1, 2, V, -5], np.int64)[j % 5])),
        "same_item": (users_mod, np.full(N, first_item, np.int64)),
    }
    return out
