"""CPU restatement of the beyond-accuracy list metrics (b4r_list_metrics, include/b4r.h), for the list-metric tests only: numpy fp32 on
top of tests/diverse_ref.sim_matrix and tests/catalogue_ref (the fma chain is oracle/rank_oracle.c's).  rnorm is an input, so a
comparison with the kernel fed the same rnorm is bit for bit and does not depend on a device reciprocal square root.  The per-row sums
are Python integers; the double sums over the rows are taken with math.fsum, and the exposure statistics restate the evaluator's."""
import math

import numpy as np

from tests import diverse_ref as dref

F32 = np.float32
UNIT = 2.0 ** 30


def q30(x):
    """(int64) rint(x * 2^30) of fp32 values: the product is exact (in fp32 as in float64), np.rint rounds ties to even."""
    return np.rint(np.asarray(x, F32).astype(np.float64) * UNIT).astype(np.int64)


def list_metrics(table, rnorm, list_ids, gt=None, item_weight=None, first_item=3, sim=None):
    """b4r_list_metrics restated.  sim: dref.sim_matrix(table, rnorm) when the caller has it already.  Returns a dict: n, dist, nov,
    hit_pos (int64 [R] each), exposure (int64 [V]), sums (two floats, by fsum) and counts (two ints)."""
    ids = np.asarray(list_ids, np.int64)
    R, K = ids.shape
    V = np.asarray(table).shape[0]
    assert 1 <= K <= 1024
    if sim is None:
        sim = dref.sim_matrix(table, rnorm)
    w = None if item_weight is None else np.asarray(item_weight, F32)
    n, dist, nov, hit = (np.zeros(R, np.int64) for _ in range(4))
    exposure = np.zeros(V, np.int64)
    for r in range(R):
        live = ids[r][(ids[r] >= 0) & (ids[r] < V)]                # in list order
        n[r] = len(live)
        np.add.at(exposure, live, 1)
        if len(live) >= 2:
            s = sim[np.ix_(live, live)]                             # s[p, p'] = sim(c = item at p', q = item at p)
            d = (F32(1.0) - s).astype(F32)                          # rounded on its own
            dist[r] = int(np.triu(q30(d), k=1).sum())
        if w is not None and len(live):
            nov[r] = int(q30(w[live]).sum())
        if gt is not None and first_item <= gt[r] < V:
            at = np.nonzero(ids[r] == gt[r])[0]                     # (gt is in [0, V): an entry equal to it is live)
            hit[r] = 0 if len(at) == 0 else int(at[0]) + 1
    sums, counts = fold(n, dist, nov)
    return dict(n=n, dist=dist, nov=nov, hit_pos=hit, exposure=exposure, sums=sums, counts=counts)


def row_terms(n, dist, nov):
    """The per-row terms of the two sums: (dist / 2^30) / (n (n - 1) / 2) for n >= 2, (nov / 2^30) / n for n >= 1, as floats."""
    ild = [(int(d) / UNIT) / (int(k) * (int(k) - 1) // 2) for k, d in zip(n, dist) if k >= 2]
    novelty = [(int(v) / UNIT) / int(k) for k, v in zip(n, nov) if k >= 1]
    return ild, novelty


def fold(n, dist, nov):
    ild, novelty = row_terms(n, dist, nov)
    return [math.fsum(ild), math.fsum(novelty)], [len(ild), len(novelty)]


def coverage(exposure, first_item=3):
    """#{exposure > 0 in [first_item, V)} / (V - first_item)"""
    c = np.asarray(exposure)[first_item:]
    return int((c > 0).sum()) / len(c)


def gini(exposure, first_item=3):
    """sum_i (2 i - n - 1) c_i / (n sum c) over the ascending counts of the n = V - first_item items, in exact integers until the one
    division; 0 when nothing was recommended."""
    c = sorted(int(x) for x in np.asarray(exposure)[first_item:])
    n, total = len(c), sum(c)
    if total == 0:
        return 0.0
    return sum((2 * i - n - 1) * x for i, x in enumerate(c, start=1)) / (n * total)
