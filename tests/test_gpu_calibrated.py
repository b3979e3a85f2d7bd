"""Calibrated re-ranking on the GPU (b4r_rerank_calibrated): the kernel against the CPU restatement (tests/calibrated_ref.py) bit for bit
in out_ids, out_scores, out_value, out_pos and out_kl, and the model / app / evaluator layers built on it.

Shapes: a workgroup has 256 threads (4 waves); a thread owns 1, 2 or 4 pool entries (M <= 256, <= 512, <= 1024) and up to 4 groups (g =
tid, tid + 256, ...), so M = 1, 2, 63, 64, 65, 256, 1023, 1024 cross the wave, workgroup and loop boundaries, 257, 512, 513 the
boundaries between the three instances, and G = 1, 2, 255, 256, 257, 1024 the group loop's.  The catalogue has four regions of 1100
items, one per label pattern (labels partly negative or >= G; j % G; contiguous blocks; one group for all), and pool row r draws from
region r % 4; its target is of kind r % 8 (target_rows).  The restatement runs the six (lambda, alpha) pairs of a shape as rows of one
call.  K = M runs on the first rows only from M = 66 on (4 rows, 2 from M = 258 on: the pick loop of the restatement is a numpy loop of
M steps); K = min(M, 10) runs on all 17.  Every case with lambda > 0 and M >= 13 is checked on the CPU to re-order some row."""
import functools
import math

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, evaluation
from bert4rec_amd import engine as engine_mod
from oracle import bert4rec_oracle as orc
from tests import calibrated_ref as cref
from tests.b4r_testlib import P, stream
from tests.test_gpu_diverse import bits_equal, build_small_app

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
VR = 1100                       # items per region
V = 4 * VR
MS = (1, 2, 63, 64, 65, 256, 257, 512, 513, 1023, 1024)
GS = (1, 2, 255, 256, 257, 1024)
LAMBDAS = (0.0, 0.3, 1.0)
ALPHAS = (0.01, 0.5)
PAIRS = tuple((lam, alpha) for lam in LAMBDAS for alpha in ALPHAS)
R_MAX = 17


@functools.lru_cache(maxsize=None)
def item_labels(G):
    """int32 [V]: region 0 mixes j % G with labels that are negative or >= G (two items of three), region 1 is j % G, region 2
    contiguous blocks, region 3 one group for every item."""
    j = np.arange(VR, dtype=np.int64)
    wild = np.where(j % 3 == 0, -(j + 1), np.where(j % 3 == 1, G + j, j % G))
    return np.concatenate([wild, j % G, j * G // VR, np.full(VR, min(1, G - 1))]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def make_pool(M, R=R_MAX, seed=0):
    """R pool rows of M distinct ids, row r from region r % 4; scores descending with an exact repeat."""
    rng = np.random.default_rng(seed + 31 * M)
    ids = np.stack([(r % 4) * VR + rng.permutation(VR)[:M] for r in range(R)]).astype(np.int64)
    sc = -np.sort(-rng.standard_normal((R, M)).astype(F32), axis=1)
    if M > 3:
        sc[:, 2] = sc[:, 1]
    return ids, sc


@functools.lru_cache(maxsize=None)
def target_rows(G, R=R_MAX, seed=0):
    """int64 [R, G], row r of kind r % 8: uniform; small counts, as a history gives; all mass on one group; an all-zero row; negative
    entries among small counts; 2^40-scale masses; T = 2^63 - 1; masses on every third group only."""
    rng = np.random.default_rng(seed + 7 * G)
    t = np.zeros((R, G), np.int64)
    for r in range(R):
        kind = r % 8
        if kind == 0:
            t[r] = 1000
        elif kind == 1:
            t[r] = rng.integers(0, 4, size=G)
            t[r, rng.integers(0, G)] += 2
        elif kind == 2:
            t[r, (G // 2 + r) % G] = 5
        elif kind == 4:
            t[r] = rng.integers(-3, 4, size=G)
            t[r, 0] = 2
        elif kind == 5:
            t[r] = rng.integers(0, 1 << 40, size=G)
        elif kind == 6:
            t[r, 1:] = rng.integers(0, 1 << 30, size=G - 1)
            t[r, 0] = (1 << 63) - 1 - int(t[r, 1:].sum())
        elif kind == 7:
            t[r, ::3] = rng.integers(1, 50, size=len(t[r, ::3]))
    return t


class Case:
    """A pool, labels and targets on the device, uploaded once."""

    def __init__(self, ids, sc, labels, G, target, n_items=V):
        self.ids, self.sc, self.labels, self.G, self.target, self.V = ids, sc, np.asarray(labels, np.int32), G, np.asarray(target, np.int64), n_items
        up = lambda a: torch.as_tensor(a).to(DEV).contiguous()
        self.ids_d, self.sc_d, self.lab_d, self.t_d = up(ids), up(sc), up(self.labels), up(self.target)

    def ref(self, lam, alpha, K, R=None):
        R = self.ids.shape[0] if R is None else R
        return cref.rerank(self.ids[:R], self.sc[:R], self.V, K, self.labels, self.G, self.target[:R], lam, alpha)

    def ref_pairs(self, K, R):
        """the restatement of the six (lambda, alpha) pairs as 6 R rows of one call -> {pair: its five outputs}"""
        n = len(PAIRS)
        lam = np.repeat([p[0] for p in PAIRS], R)
        alpha = np.repeat([p[1] for p in PAIRS], R)
        out = cref.rerank(np.tile(self.ids[:R], (n, 1)), np.tile(self.sc[:R], (n, 1)), self.V, K, self.labels, self.G,
                          np.tile(self.target[:R], (n, 1)), lam, alpha)
        return {pair: tuple(o[i * R:(i + 1) * R] for o in out) for i, pair in enumerate(PAIRS)}


OUT_DTYPES = (torch.int64, torch.float32, torch.float32, torch.int32, torch.float64)


def run(c, lam, alpha, K, R=None, outputs=(True,) * 5):
    """b4r_rerank_calibrated on the first R rows; returns (rc, ids, scores, value, pos, kl, call, read) with the outputs as numpy ([R, K]
    and [R]; None where not asked for).  Every output buffer is one element longer than needed; that element must stay as it is."""
    lib = _lib.load()
    R = c.ids.shape[0] if R is None else R
    M = c.ids.shape[1]
    sizes = [R * K] * 4 + [R]
    outs = [torch.full((n + 1,), 7, dtype=dt, device=DEV) if on else None for dt, n, on in zip(OUT_DTYPES, sizes, outputs)]

    def call():
        return lib.b4r_rerank_calibrated(P(c.ids_d), P(c.sc_d), R, M, K, c.V, P(c.lab_d), c.G, P(c.t_d), float(lam), float(alpha),
                                         *(P(o) for o in outs), stream())

    def read():
        torch.cuda.synchronize()
        got = []
        for i, (o, n) in enumerate(zip(outs, sizes)):
            if o is None:
                got.append(None)
                continue
            assert o[n] == 7, "written beyond the output"
            got.append(o[:n].reshape(R, K).cpu().numpy() if i < 4 else o[:n].cpu().numpy())
        return tuple(got)
    rc = call()
    return (rc,) + read() + (call, read)


def kl_equal(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: ids"
    assert bits_equal(got[1], want[1]), f"{what}: scores not bit-identical"
    assert bits_equal(got[2], want[2]), f"{what}: value not bit-identical"
    assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3]), f"{what}: pos"
    assert got[4].dtype == np.float64 and kl_equal(got[4], want[4]), f"{what}: kl not bit-identical: {got[4]} != {want[4]}"


def reordered(want):
    """some row's picks are not its pool's first positions in order"""
    pos = want[3]
    return bool((pos != np.arange(pos.shape[1])[None, :]).any())


@pytest.mark.parametrize("M", MS)
def test_grid_bit_exact(M):
    ids, sc = make_pool(M)
    r_full = R_MAX if M <= 65 else 4 if M <= 257 else 2
    runs = [(M, r_full)] + ([(10, R_MAX)] if M > 10 else [])
    for G in GS:
        c = Case(ids, sc, item_labels(G), G, target_rows(G))
        for K, R in runs:
            want = c.ref_pairs(K, R)
            for lam, alpha in PAIRS:
                what = f"M={M} G={G} K={K} R={R} lambda={lam} alpha={alpha}"
                w = want[(lam, alpha)]
                if lam == 0.0:                                          # the pool order, and the miscalibration of the plain top K
                    assert not reordered(w), what
                elif M >= 13:                                           # a case that re-orders nothing would test nothing
                    assert reordered(w), f"{what}: the calibration re-orders no row"
                rc, *got = run(c, lam, alpha, K, R)[:6]
                assert rc == 0, _lib.last_error()
                assert_same(got, w, what)


def test_lambda_zero_is_the_pool_and_its_miscalibration():
    M, G = 300, 20
    ids, sc = make_pool(M, seed=3)
    c = Case(ids, sc, item_labels(G), G, target_rows(G))
    rc, g_ids, g_sc, g_val, g_pos, g_kl = run(c, 0.0, 0.01, 10)[:6]
    assert rc == 0, _lib.last_error()
    assert np.array_equal(g_ids, ids[:, :10]) and bits_equal(g_sc, sc[:, :10]) and np.array_equal(g_pos, np.tile(np.arange(10), (R_MAX, 1)))
    rel = ((sc - sc[:, -1:]).astype(F32) / (sc[:, :1] - sc[:, -1:]).astype(F32)).astype(F32)
    assert bits_equal(g_val, rel[:, :10])                               # fl32(1 * rel) + fl32(0 * gain)
    # kl against the definition in plain fp64 (b4r_xln is within 1e-15 relative of log; G terms of size <= ln(1 / (alpha p)))
    p, T = cref.target_shares(c.target)
    for r in range(R_MAX):
        if T[r] == 0:
            assert math.isnan(g_kl[r])
            continue
        lab = c.labels[ids[r, :10]]
        want = 0.0
        for g in range(G):
            if p[r, g] > 0:
                q = 0.99 * float((lab == g).sum()) / 10 + 0.01 * p[r, g]
                want += p[r, g] * (math.log(p[r, g]) - math.log(q))
        assert g_kl[r] == pytest.approx(want, rel=1e-12, abs=1e-12)


def test_targets():
    """Every kind of target at one shape (2 entries per thread, one group per thread), with K = M and K = 10: target_rows' eight kinds,
    and a row whose mass lies on a group that no pool item has (group 7: the pool is drawn from the items of the other groups)."""
    M, G, R = 300, 20, 10
    labels = item_labels(G)
    rng = np.random.default_rng(5)
    ids, sc = (a.copy() for a in make_pool(M, R=R, seed=1))
    not7 = np.flatnonzero(labels[VR:2 * VR] != 7) + VR
    ids[8] = rng.permutation(not7)[:M]
    ids[9] = rng.permutation(not7)[:M]
    target = target_rows(G, R=R).copy()
    target[8] = 0; target[8, 7] = 11                                    # all of the mass where the pool has nothing
    target[9] = 3; target[9, 7] = 40                                    # most of it
    c = Case(ids, sc, labels, G, target)
    assert not (c.labels[ids[8:]] == 7).any()
    for lam, alpha in ((0.3, 0.01), (1.0, 0.5)):
        for K in (10, M):
            want = c.ref(lam, alpha, K)
            rc, *got = run(c, lam, alpha, K)[:6]
            assert rc == 0, _lib.last_error()
            assert_same(got, want, f"lambda={lam} alpha={alpha} K={K}")
        assert np.isnan(got[4][3]) and np.isfinite(np.delete(got[4], 3)).all()          # the all-zero row has no target
        assert np.array_equal(got[3][3], np.arange(M)) and np.array_equal(got[3][8], np.arange(M))     # no gain anywhere: the pool order
        assert got[4][8] == pytest.approx(math.log(1.0 / alpha), rel=1e-12)              # q~_7 = alpha p_7 = alpha
        assert reordered(tuple(g[9:] for g in got)) and reordered(tuple(g[:3] for g in got))


@pytest.mark.parametrize("M", [65, 300, 1024])
def test_dead_entries(M):
    G = 20
    ids, sc = (a.copy() for a in make_pool(M, R=10, seed=5))
    ids[0, :] = -1; sc[0, :] = -np.inf                                # the -1 / -inf tail from 0 live entries,
    ids[1, 1:] = -1; sc[1, 1:] = -np.inf                              # from 1 (a pool with one live entry),
    ids[2, M - 1:] = -1; sc[2, M - 1:] = -np.inf                      # from M - 1
    ids[3, [0, 5, M // 2, M - 2]] = -1                                # -1 in the middle, scores left finite
    ids[4, 3] = V; ids[4, 7] = 2 ** 40; ids[4, 9] = -2 ** 40          # ids past V and outside 32 bits
    sc[5, 2] = np.inf; sc[5, 4] = np.nan; sc[5, 6] = -np.inf          # scores that are not finite on good ids
    sc[6, :] = F32(0.75)                                              # all live scores equal: rel = 1
    sc[7, :] = F32(-0.0); sc[7, ::2] = F32(0.0)                       # ... equal as +-0.0
    ids[8, : M - 1] = -1                                              # only the last entry is live
    sc[9, 1::2] = -np.inf                                             # every other entry dead
    target = np.tile(target_rows(G)[:2], (5, 1))                      # uniform and small counts
    c = Case(ids, sc, item_labels(G), G, target)
    live = (ids >= 0) & (ids < V) & np.isfinite(sc)
    for lam, alpha in ((0.3, 0.01), (1.0, 0.5)):
        for K in (1, min(M, 10), M):
            want = c.ref(lam, alpha, K)
            rc, *got = run(c, lam, alpha, K)[:6]
            assert rc == 0, _lib.last_error()
            assert_same(got, want, f"lambda={lam} alpha={alpha} K={K}")
        g_ids, g_sc, g_val, g_pos, g_kl = got
        assert (g_ids[0] == -1).all() and (g_sc[0] == -np.inf).all() and (g_val[0] == -np.inf).all() and (g_pos[0] == -1).all()
        assert np.isnan(g_kl[0]) and np.isfinite(g_kl[1:]).all()       # nothing was picked
        for r in range(10):                                           # a dead entry is never picked, every live one is
            assert sorted(g_pos[r][g_pos[r] >= 0].tolist()) == np.flatnonzero(live[r]).tolist()
            assert (g_pos[r, int(live[r].sum()):] == -1).all()


@pytest.mark.parametrize("where,M,p1,p2", [("one thread's two loop turns", 300, 5, 261), ("two lanes", 300, 5, 6), ("two waves", 300, 5, 70),
                                           ("turns 0 and 3 of one thread", 1000, 9, 777), ("two waves, one turn apart", 1000, 200, 300)])
def test_ties(where, M, p1, p2):
    """Two entries with equal scores.  Rows 0, 1: in ONE group, so their val is equal at every step.  Rows 2, 3: in two groups that
    hold no other pool entry and have equal target masses, so their p and their counts, hence their gains and val, are equal until
    one is picked.  The lower position goes first; the kernel's bits are the restatement's."""
    G = 257
    a, b, x, y = V, V + 1, V + 2, V + 3                                 # four items behind the regions: no pool row holds them yet
    labels = np.concatenate([item_labels(G), [100, 100, 255, 256]])
    labels[:V][(labels[:V] == 255) | (labels[:V] == 256)] = 254         # groups 255 and 256 hold x and y alone
    ids, sc = (arr.copy() for arr in make_pool(M, R=4, seed=M + p1))
    ids[3], sc[3] = ids[2], sc[2]                                       # rows 2 and 3: one pool, the pair swapped
    ids[0, p1], ids[0, p2] = a, b
    ids[1, p1], ids[1, p2] = b, a                                       # the higher id first as well: the position decides, not the id
    ids[2, p1], ids[2, p2] = x, y
    ids[3, p1], ids[3, p2] = y, x
    sc[:, p2] = sc[:, p1]
    target = np.full((4, G), 10, np.int64)
    c = Case(ids, sc, labels, G, target, n_items=V + 4)
    assert ((c.labels[ids[2:]] == 255).sum(axis=1) == 1).all() and ((c.labels[ids[2:]] == 256).sum(axis=1) == 1).all()
    for lam, alpha in ((0.3, 0.01), (1.0, 0.5)):
        want = c.ref(lam, alpha, M)
        rc, *got = run(c, lam, alpha, M)[:6]
        assert rc == 0, _lib.last_error()
        assert_same(got, want, f"{where}, lambda={lam}")
        for r in range(4):
            row = got[3][r].tolist()
            assert row.index(p1) < row.index(p2), f"{where}: row {r}"
        # rows 2 and 3 are each other's pool with the pair swapped: the same position wins the pair's first pick with the same value,
        # whichever of the two groups stands there -- the two entries did tie
        t2, t3 = got[3][2].tolist().index(p1), got[3][3].tolist().index(p1)
        assert t2 == t3 and got[2][2, t2] == got[2][3, t3]


def test_errors_and_null_outputs():
    lib = _lib.load()
    M, G = 100, 20
    ids, sc = make_pool(M, R=3)
    c = Case(ids, sc, item_labels(G), G, target_rows(G, R=3))
    out = torch.full((40,), 7, dtype=torch.int32, device=DEV)
    kl = torch.full((4,), 7.0, dtype=torch.float64, device=DEV)

    def call(R=3, M=M, K=10, G=G, lam=0.5, alpha=0.01, ids_p=P(c.ids_d), t_p=P(c.t_d)):
        return lib.b4r_rerank_calibrated(ids_p, P(c.sc_d), R, M, K, V, P(c.lab_d), G, t_p, lam, alpha, None, None, None, P(out), P(kl), stream())
    for kw, code in ((dict(M=0), -2), (dict(M=1025), -2), (dict(K=101), -2), (dict(K=-1), -2), (dict(R=-1), -2), (dict(G=0), -2),
                     (dict(G=1025), -2), (dict(lam=-0.1), -1), (dict(lam=1.5), -1), (dict(lam=float("nan")), -1), (dict(alpha=0.0), -1),
                     (dict(alpha=1.0), -1), (dict(alpha=float("nan")), -1), (dict(ids_p=None), -1), (dict(t_p=None), -1),
                     (dict(K=0, alpha=1.0), -1), (dict(R=0, G=0), -2)):
        assert call(**kw) == code, kw
        assert "b4r_rerank_calibrated" in _lib.last_error()
    torch.cuda.synchronize()
    assert (out == 7).all() and (kl == 7.0).all()                     # no refused call wrote anything
    assert call(R=0) == 0
    torch.cuda.synchronize()
    assert (out == 7).all() and (kl == 7.0).all()
    assert call(K=0) == 0                                             # nothing is picked: kl alone is written, NaN
    torch.cuda.synchronize()
    assert (out == 7).all() and torch.isnan(kl[:3]).all() and kl[3] == 7.0
    assert call() == 0
    torch.cuda.synchronize()
    assert (out[30:] == 7).all() and (out[:30] >= 0).all() and torch.isfinite(kl[:3]).all() and kl[3] == 7.0
    # any output may be NULL: each alone gives what all five give (run() checks that nothing beyond the output is written)
    full = run(c, 0.3, 0.01, 10)
    assert full[0] == 0
    for i in range(5):
        only = run(c, 0.3, 0.01, 10, outputs=tuple(j == i for j in range(5)))
        assert only[0] == 0 and all(only[1 + j] is None for j in range(5) if j != i)
        assert only[1 + i].tobytes() == full[1 + i].tobytes() and only[1 + i].dtype == full[1 + i].dtype
    assert run(c, 0.3, 0.01, 10, outputs=(False,) * 5)[0] == 0


def test_reproducible_and_in_a_captured_graph():
    M, K, G = 513, 100, 257
    ids, sc = make_pool(M, R=6, seed=11)
    c = Case(ids, sc, item_labels(G), G, target_rows(G, R=6))
    want = c.ref(0.3, 0.01, K)
    rc, *a, call, read = run(c, 0.3, 0.01, K)
    assert rc == 0, _lib.last_error()
    assert_same(a, want, "first call")
    assert call() == 0
    b = read()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert call() == 0
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        graph.replay()
    g = read()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, g))


# ---- the model, the apps and the evaluator --------------------------------------------------------------------------------------------
def model_labels(n_items, groups=5):
    """token j is in group (j // 3) % groups; the specials are in none, and every 11th item neither"""
    j = np.arange(n_items)
    return np.where((j < engine_mod.SPECIAL_IDS) | (j % 11 == 0), -1, (j // 3) % groups).astype(np.int64)


def small_batch(rec, items):
    batches = [rec.dataloader.prepare_inference(list(items[s:s + n])) for s, n in ((0, 9), (30, 20), (60, 5), (95, 14), (140, 9))]
    return {key: torch.from_numpy(np.concatenate([np.asarray(b[key]) for b in batches], axis=0)) for key in batches[0]}


@pytest.mark.parametrize("factorised", [False, True])
def test_recommend_tensor_calibrate(factorised):
    rec, items = build_small_app(factorised)
    model, n_items = rec.model, rec.model.vocab_size
    batch = small_batch(rec, items)
    k, pool, G = 8, 60, 5
    labels = model_labels(n_items, G)
    plain = model.recommend_tensor(batch, k=k)
    same = model.recommend_tensor(batch, k=k, calibrate=None)
    assert len(same) == 3 and all(torch.equal(a, b) for a, b in zip(plain, same))       # unchanged without the argument
    R = int(plain[0].shape[0])
    cand = model.recommend_tensor(batch, k=pool)
    P_ = int(batch["masked_lm_positions"].shape[1])
    tokens = batch["input_word_ids"][torch.div(cand[2].cpu(), P_, rounding_mode="floor")]
    history = engine_mod.group_history_counts(tokens, torch.as_tensor(labels), G)
    assert int(history.sum()) > 0
    affinity = model.group_affinity_tensor(batch, labels, G)["group_mass"]
    given = torch.arange(R * G, dtype=torch.int64).reshape(R, G) % 7
    for target, mass in (("history", history), ("affinity", affinity), (given, given)):
        got = model.recommend_tensor(batch, k=k, calibrate=(labels, G, target), calibration=0.6, calibration_alpha=0.05, pool=pool,
                                     return_calibration=True)
        # the host composition: rank_full (above), then the target, then Engine.rerank_calibrated
        want = model.engine.rerank_calibrated(cand[0], cand[1], k, 0.6, labels, G, mass.to(DEV), 0.05)
        assert len(got) == 4 and torch.equal(got[2], plain[2]) and torch.equal(got[3]["target_mass"].cpu(), mass.cpu())
        assert torch.equal(got[0], want[0]) and bits_equal(got[1].cpu().numpy(), want[1].cpu().numpy())
        assert got[3]["kl"].cpu().numpy().tobytes() == want[4].cpu().numpy().tobytes()
        # ... which is the restatement on that pool
        ref = cref.rerank(cand[0].cpu().numpy(), cand[1].cpu().numpy(), n_items, k, labels, G, mass.cpu().numpy(), F32(0.6), 0.05)
        assert np.array_equal(got[0].cpu().numpy(), ref[0]) and kl_equal(got[3]["kl"].cpu().numpy(), ref[4])
        assert not torch.equal(got[0], plain[0])                         # the calibration binds
        zero = model.recommend_tensor(batch, k=k, calibrate=(labels, G, target), calibration=0.0, pool=pool, return_calibration=True)
        assert torch.equal(zero[0], plain[0]) and bits_equal(zero[1].cpu().numpy(), plain[1].cpu().numpy())
    # calibration = 1 against 0 with the history target: verified on the restatement first, then on the device
    ids_h, sc_h, hist_h = cand[0].cpu().numpy(), cand[1].cpu().numpy(), history.numpy()
    ref0 = cref.rerank(ids_h, sc_h, n_items, k, labels, G, hist_h, 0.0, 0.01)[4]
    ref1 = cref.rerank(ids_h, sc_h, n_items, k, labels, G, hist_h, 1.0, 0.01)[4]
    assert np.isfinite(ref0).all() and (ref1 <= ref0).all() and (ref1 < ref0).any()
    kl0 = model.recommend_tensor(batch, k=k, calibrate=(labels, G, "history"), calibration=0.0, pool=pool, return_calibration=True)[3]["kl"]
    kl1 = model.recommend_tensor(batch, k=k, calibrate=(labels, G, "history"), calibration=1.0, pool=pool, return_calibration=True)[3]["kl"]
    assert kl_equal(kl0.cpu().numpy(), ref0) and kl_equal(kl1.cpu().numpy(), ref1) and bool((kl1 <= kl0).all())
    # the default pool, the default lambda, the distribution beside it, and the list form
    d80 = model.recommend_tensor(batch, k=k, calibrate=(labels, G, "history"))
    c80 = model.recommend_tensor(batch, k=80)
    assert len(d80) == 3 and torch.equal(d80[0], model.engine.rerank_calibrated(c80[0], c80[1], k, 0.5, labels, G, history.to(DEV))[0])
    both = model.recommend_tensor(batch, k=k, calibrate=(labels, G, "history"), calibration=0.6, calibration_alpha=0.05, pool=pool,
                                  return_distribution=True, return_calibration=True)
    hist = model.recommend_tensor(batch, k=k, calibrate=(labels, G, "history"), calibration=0.6, calibration_alpha=0.05, pool=pool)
    assert len(both) == 5 and torch.equal(both[0], hist[0]) and both[3]["logp"].shape == (R, k) and "kl" in both[4]
    dist = model.score_distribution_tensor(batch, query_ids=hist[0])
    assert bits_equal(both[3]["logp"].cpu().numpy(), dist["logp"].cpu().numpy())
    lists, info = model.recommend(batch, k=k, calibrate=(labels, G, "history"), calibration=0.6, calibration_alpha=0.05, pool=pool,
                                  return_calibration=True)
    assert [ids for per_row in lists for ids, _ in per_row] == hist[0].cpu().tolist() and info["kl"].shape == (R,)
    with pytest.raises(ValueError):
        model.recommend_tensor(batch, k=k, calibrate=(labels, G, given[:-1]))


def test_recommend_batch_calibrate_by():
    rec, items = build_small_app()
    model = rec.model
    catalogue = sorted(set(items))
    names = {item: "cat-%d" % (i % 4) for i, item in enumerate(catalogue) if i % 9}       # every 9th item has no category
    histories = [items[s:s + n] for s, n in ((0, 15), (40, 3), (90, 24), (120, 1), (7, 22))]
    plain = rec.recommend_batch(histories, 6)
    assert rec.recommend_batch(histories, 6, calibrate_by=None) == plain
    assert rec.recommend_batch(histories, 6, calibrate_by=names, calibration=0.0) == plain
    labels, G, group_names = rec._affinity_labels(names)
    batch, exclude = rec._requests(histories)
    for to in ("history", "affinity"):
        got = rec.recommend_batch(histories, 6, calibrate_by=names, calibrate_to=to, calibration=0.8, candidate_pool=70)
        want = model.recommend_tensor(batch, k=6, exclude_seen=False, exclude=exclude, calibrate=(labels, G, to), calibration=0.8, pool=70)
        tok = rec.dataloader.get_tokenizer()
        assert got == [tok.detokenize([i for i in row if i >= 0]) for row in want[0].cpu().tolist()]
        assert got != plain and all(len(lst) == 6 and not set(lst) & set(h) for lst, h in zip(got, histories))
    assert rec.recommend_batch(histories, 6, calibrate_by=names.get, calibration=0.8, candidate_pool=70) == \
        rec.recommend_batch(histories, 6, calibrate_by=labels.numpy(), calibration=0.8, candidate_pool=70)


def test_evaluator_miscalibration():
    rec, _ = build_small_app()
    model, n_items = rec.model, rec.model.vocab_size
    K, pool, n_users, G = 10, 60, 16, 5
    labels = model_labels(n_items, G)
    batch = orc.synthetic_batch(n_users, 24, 4, n_items, seed=81, ragged=True, finetune=True)
    b_idx, p_idx = torch.nonzero(batch["masked_lm_weights"] != 0, as_tuple=True)
    assert b_idx.tolist() == list(range(n_users))
    gt = batch["masked_lm_ids"][b_idx, p_idx]
    exclude = batch["labels"].clone()
    exclude[exclude == gt[:, None]] = -1
    metrics = lambda: [evaluation.Counter(name="Valid Ranks")] + [f(k) for f in (evaluation.HR, evaluation.NDCG) for k in (1, 5, 10)]
    for to in ("history", "affinity"):
        ev = evaluation.get(full_ranking=True, list_k=K, calibrate_by=labels, calibrate_to=to, calibration=0.7, candidate_pool=pool,
                            metrics=metrics())
        ev.evaluate(model, [batch, batch])
        res = ev.get_metrics_results()
        lists, _, _, info = model.recommend_tensor(batch, k=K, exclude_seen=False, exclude=exclude, calibrate=(labels, G, to),
                                                   calibration=0.7, pool=pool, return_calibration=True)
        kl = info["kl"].cpu().numpy()
        assert np.isfinite(kl).all() and (kl > 0).all()
        # the device sums 16 values per batch and the host adds two batches: within a few ulp of the mean
        assert res[f"Miscalibration@{K}"] == pytest.approx(float(kl.mean()), rel=1e-13)
        lists = lists.cpu().numpy()
        plain = model.recommend_tensor(batch, k=K, exclude_seen=False, exclude=exclude)[0].cpu().numpy()
        assert not np.array_equal(lists, plain)
        ranks = np.array([row.tolist().index(g) + 1 if g in row else K + 1 for row, g in zip(lists, gt.numpy())])
        assert res["Valid Ranks"] == 2 * n_users
        for k in (1, 5, 10):                                          # HR / NDCG from the position in the calibrated list
            assert res[f"HR@{k}"] == pytest.approx(float((ranks <= k).mean()), abs=1e-12)
            ndcg = [1.0 / math.log2(r + 1) if r <= k else 0.0 for r in ranks.tolist()]
            assert res[f"NDCG@{k}"] == pytest.approx(math.fsum(ndcg) / n_users, abs=1e-12)
        ev.reset_metrics()
        assert ev.get_metrics_results()[f"Miscalibration@{K}"] == 0.0
    # calibration = 0: the plain lists' miscalibration; a row without a target does not count
    ev0 = evaluation.get(full_ranking=True, list_k=K, calibrate_by=(labels, G), calibration=0.0, candidate_pool=pool, metrics=metrics())
    ev0.evaluate(model, [batch])
    kl0 = model.recommend_tensor(batch, k=K, exclude_seen=False, exclude=exclude, calibrate=(labels, G, "history"), calibration=0.0,
                                 pool=pool, return_calibration=True)[3]["kl"].cpu().numpy()
    assert ev0.get_metrics_results()[f"Miscalibration@{K}"] == pytest.approx(float(kl0.mean()), rel=1e-13)
    wrong = evaluation.get(full_ranking=True, list_k=K, calibrate_by=np.zeros(n_items + 1, np.int64), metrics=metrics())
    with pytest.raises(ValueError):
        wrong.evaluate(model, [batch])
