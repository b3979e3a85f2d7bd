"""Re-ranking under category quotas on the GPU (b4r_rerank_quota): the kernel against the CPU restatement (tests/quota_ref.py) bit for
bit in out_ids, out_scores, out_mmr and out_pos, and the model / app / evaluator layers built on it.

The kernel is given an explicit fp32 rnorm wherever it is compared with the restatement (tests/test_gpu_diverse.py's tables and pools,
whose similarities are computed once and shared); the item_rnorm = NULL form is compared with b4r_rerank_diverse's.

Shapes: a workgroup has 256 threads (4 waves) and a thread owns 1, 2 or 4 pool entries (M <= 256, <= 512, <= 1024), so M = 1, 2, 63, 64,
65, 256, 1023, 1024 cross the wave, workgroup and loop boundaries and 257, 512, 513 the boundaries between the three instances.  The four
quotas of the grid (four_quotas) are taken 1, 2 and 4 at a time, always with the first, whose caps admit at most 12 picks, so K = M reaches
the "no open entry is left" exit whenever M >= 13; from M = 256 on the second and third are also run without the first, for pick loops of
a few hundred steps.  Every case with M >= 13 is checked on the CPU to have caps that bind."""
import functools
import math

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, evaluation
from bert4rec_amd import engine as engine_mod
from bert4rec_amd.apps import pack_item_groups
from oracle import bert4rec_oracle as orc
from tests import diverse_ref as dref
from tests import quota_ref as qref
from tests.b4r_testlib import P, stream
from tests.quota_ref import Quota
from tests.test_gpu_diverse import bits_equal, build_small_app, case, device_rnorm, make_pool
from tests.test_gpu_diverse import run as run_diverse

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
TABLES = ((40, 4), (300, 64), (1100, 132))
MS = (1, 2, 63, 64, 65, 256, 257, 512, 513, 1023, 1024)
LAMBDAS = (0.0, 0.3, 1.0)
R_MAX = 17


@functools.lru_cache(maxsize=None)
def four_quotas(V):
    """j % 7 with per-group caps that include a 0 (at most 12 picks); j % 97 with cap 3; j // 5 with cap 2 where every 11th item is in
    no group; and a map whose ids are partly at or beyond n_groups = 9 and partly negative, handed to the kernel as they are."""
    j = np.arange(V)
    wild = (j * 7) % 13
    wild = np.where(j % 4 == 3, -(j + 1), wild)
    return (Quota(j % 7, 7, 0, np.array([1, 2, 3, 1, 2, 3, 0])), Quota(j % 97, 97, 3),
            Quota(np.where(j % 11 == 0, -1, j // 5), V // 5 + 1, 2), Quota(wild, 9, 2))


def quota_sets(V, M):
    q = four_quotas(V)
    sets = [q[:1], q[:2], q[:4]]
    if M >= 256:
        sets += [q[1:2], q[1:3]]
    return sets


_ON_DEVICE = {}


def quotas_on_device(quotas):
    """(the b4r_item_quota array, the tensors it points to) of a tuple of Quota, uploaded once per tuple (kept by identity)"""
    key = tuple(id(q) for q in quotas)
    if key in _ON_DEVICE:
        return _ON_DEVICE[key][:2]
    arr = (_lib.ItemQuota * max(len(quotas), 1))()
    keep = []
    for slot, q in zip(arr, quotas):
        ig = torch.as_tensor(np.asarray(q.item_group, np.int32)).to(DEV)
        gc = None if q.group_cap is None else torch.as_tensor(np.asarray(q.group_cap, np.int32)).to(DEV)
        keep.append((ig, gc))
        slot.item_group, slot.group_cap, slot.n_groups, slot.cap = P(ig), P(gc), q.n_groups, q.cap
    _ON_DEVICE[key] = (arr, keep, quotas)
    return arr, keep


class Pool:
    """A pool on the device, uploaded once."""

    def __init__(self, ids, sc):
        self.ids, self.sc = ids, sc
        self.ids_d, self.sc_d = torch.as_tensor(ids).to(DEV).contiguous(), torch.as_tensor(sc).to(DEV).contiguous()


def run(c, width, V, pool, lam, K, quotas, rnorm="given", outputs=(True, True, True, True), R=None):
    """b4r_rerank_quota on the first R rows of the pool; returns (rc, ids, scores, mmr, pos, call, read, scratch) with the outputs as
    numpy ([R, K]; None where not asked for)."""
    lib = _lib.load()
    R = pool.ids.shape[0] if R is None else R
    M = pool.ids.shape[1]
    dtypes = (torch.int64, torch.float32, torch.float32, torch.int32)
    outs = [torch.full((R, max(K, 1) + 1), 7, dtype=dt, device=DEV) if on else None for dt, on in zip(dtypes, outputs)]
    need = int(lib.b4r_rerank_quota_scratch_bytes(R, M, V))
    scratch = torch.zeros(max(need, 16), dtype=torch.uint8, device=DEV) if rnorm is None else None
    rn = c["rnorm_d"] if isinstance(rnorm, str) else rnorm
    arr, _ = quotas_on_device(tuple(quotas))

    def call():
        # (the outputs are [R, K + 1] buffers used as [R * K]: what lies beyond R * K must stay as it is)
        return lib.b4r_rerank_quota(P(c["table_d"]), width, width, V, P(rn), P(pool.ids_d), P(pool.sc_d), R, M, float(lam), K, arr,
                                    len(quotas), P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), P(scratch),
                                    need if scratch is not None else 0, stream())

    def read():
        torch.cuda.synchronize()
        got = []
        for o in outs:
            if o is None:
                got.append(None)
                continue
            flat = o.reshape(-1)
            assert (flat[R * K:] == 7).all(), "written beyond [R, K]"
            got.append(flat[:R * K].reshape(R, K).cpu().numpy())
        return tuple(got)
    rc = call()
    return (rc,) + read() + (call, read, scratch)


def assert_same(got, want, K, what):
    assert np.array_equal(got[0], want[0][:, :K]), f"{what}: ids"
    assert bits_equal(got[1], want[1][:, :K]), f"{what}: scores not bit-identical"
    assert bits_equal(got[2], want[2][:, :K]), f"{what}: mmr not bit-identical"
    assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3][:, :K]), f"{what}: pos"


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("V,width", TABLES)
def test_grid_bit_exact(V, width, M):
    c = case(V, width)
    ids, sc = make_pool(V, M)
    pool = Pool(ids, sc)
    for lam in LAMBDAS:
        plain = dref.rerank(c["table"], c["rnorm"], ids, sc, lam, M, c["sim"]) if M >= 13 else None
        for quotas in quota_sets(V, M):
            want = qref.rerank(c["table"], c["rnorm"], ids, sc, lam, M, quotas, c["sim"])    # K = M once: a smaller K is its prefix
            assert not qref.violations(want[0], V, quotas)
            if M >= 13:                                                 # a case whose caps never bind would test nothing
                assert not np.array_equal(want[0], plain[0]), f"lambda={lam} n_quotas={len(quotas)}: the caps do not bind"
                if quotas[0] is four_quotas(V)[0]:
                    assert (want[0][:, 12:] == -1).all() and (want[3][:, 12:] == -1).all()
            for R in (1, R_MAX):
                for K in sorted({0, 1, min(M, 10), M}):
                    rc, *got = run(c, width, V, pool, lam, K, quotas, R=R)[:5]
                    assert rc == 0, _lib.last_error()
                    assert_same(got, tuple(w[:R] for w in want), K, f"lambda={lam} n_quotas={len(quotas)} R={R} K={K}")
                    assert not qref.violations(got[0], V, quotas)


@pytest.mark.parametrize("M", [100, 513, 1024])
def test_without_quotas_it_is_rerank_diverse(M):
    V, width = 1100, 132
    c = case(V, width)
    ids, sc = make_pool(V, M, seed=2)
    ids[0, M // 2:] = -1; sc[0, M // 2:] = -np.inf
    pool = Pool(ids, sc)
    for lam in LAMBDAS:
        for K in (min(M, 10), M):
            rc, d_ids, d_sc, d_mmr = run_diverse(c, width, V, ids, sc, lam, K)[:4]
            assert rc == 0, _lib.last_error()
            rc, q_ids, q_sc, q_mmr, q_pos = run(c, width, V, pool, lam, K, ())[:5]
            assert rc == 0, _lib.last_error()
            assert np.array_equal(q_ids, d_ids) and bits_equal(q_sc, d_sc) and bits_equal(q_mmr, d_mmr)
            picked = q_pos >= 0
            assert np.array_equal(picked, q_ids >= 0)
            assert np.array_equal(np.take_along_axis(ids, np.maximum(q_pos, 0).astype(np.int64), axis=1)[picked], q_ids[picked])


@pytest.mark.parametrize("M", [65, 300, 1024])
def test_dead_entries(M):
    """test_gpu_diverse.py's rows of dead entries, now under quotas."""
    V, width = 300, 64
    c = case(V, width)
    ids, sc = make_pool(V, M, R=10, seed=5)
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
    pool = Pool(ids, sc)
    q = four_quotas(V)
    for lam in LAMBDAS:
        plain = dref.rerank(c["table"], c["rnorm"], ids, sc, lam, M, c["sim"])
        for quotas in (q[:1], q[2:4], q):
            want = qref.rerank(c["table"], c["rnorm"], ids, sc, lam, M, quotas, c["sim"])
            assert not np.array_equal(want[0], plain[0])
            for K in (1, min(M, 10), M):
                rc, *got = run(c, width, V, pool, lam, K, quotas)[:5]
                assert rc == 0, _lib.last_error()
                assert_same(got, want, K, f"n_quotas={len(quotas)} lambda={lam} K={K}")
            g_ids, g_sc, g_mmr, g_pos = got
            assert (g_ids[0] == -1).all() and (g_sc[0] == -np.inf).all() and (g_mmr[0] == -np.inf).all() and (g_pos[0] == -1).all()
            assert not qref.violations(g_ids, V, quotas)
            live = (ids >= 0) & (ids < V) & np.isfinite(sc)
            for r in range(10):                                       # a dead entry is never picked
                assert live[r, g_pos[r][g_pos[r] >= 0]].all()
            if lam == 1.0:
                scan = qref.sequential_scan(ids, sc, V, M, quotas)
                for r, picked in enumerate(scan):
                    assert g_pos[r, :len(picked)].tolist() == picked and (g_pos[r, len(picked):] == -1).all()
                assert (g_mmr[6][g_pos[6] >= 0] == 1.0).all()


@pytest.mark.parametrize("where,M,p1,p2", [("one thread's two loop turns", 300, 5, 261), ("two lanes", 300, 5, 6), ("two waves", 300, 5, 70),
                                           ("turns 0 and 3 of one thread", 1000, 9, 777), ("two waves, one turn apart", 1000, 200, 300)])
def test_ties(where, M, p1, p2):
    """ids 4 / 7 and 11 / V - 1 hold identical table rows: given equal scores and equal groups, two such entries have the same mmr at
    every step.  Quota X puts each pair alone in one group of cap 2 (every other item: j % 31 + 1, cap 2): both are picked, the lower
    position first (rows 0, 1).  In rows 2 and 3 quota Y (cap 1) puts the entry at p1 in one group with the row's best entry, item 20
    at position 0: after step 0 the entry at p1 is closed, and the entry at p2 is picked although its twin at the lower position has
    the same mmr."""
    V, width = 1100, 132
    c = case(V, width)
    rng = np.random.default_rng(M + p1)
    rest = np.setdiff1d(np.arange(V), [4, 7, 11, V - 1, 20])
    ids = np.stack([rng.permutation(rest)[:M] for _ in range(4)]).astype(np.int64)
    sc = -np.sort(-rng.standard_normal((4, M)).astype(F32), axis=1)
    ids[0::2, p1], ids[0::2, p2] = 4, 7                                # the higher id first as well: the position decides, not the id
    ids[1::2, p1], ids[1::2, p2] = V - 1, 11
    sc[:, p2] = sc[:, p1]
    ids[2:, 0] = 20
    assert sc[2, 0] > sc[2, 1] and sc[3, 0] > sc[3, 1]
    gx = np.arange(V) % 31 + 1
    gx[[4, 7, 11, V - 1]] = 0
    gy = np.full(V, -1)
    gy[[20, 4, V - 1]] = 0
    quotas = (Quota(gx, 32, 2), Quota(gy, 1, 1))
    pool = Pool(ids, sc)
    for lam in (0.3, 1.0):
        want = qref.rerank(c["table"], c["rnorm"], ids, sc, lam, M, quotas, c["sim"])
        rc, *got = run(c, width, V, pool, lam, M, quotas)[:5]
        assert rc == 0, _lib.last_error()
        assert_same(got, want, M, f"{where}, lambda={lam}")
        g_ids, _, g_mmr, g_pos = got
        assert not qref.violations(g_ids, V, quotas) and (g_pos[:, -1] == -1).all()      # the caps bind: the rows run out
        for r in (0, 1):
            row = g_pos[r].tolist()
            assert row.index(p1) < row.index(p2), f"{where}: row {r}"
            if lam == 1.0:
                assert row.index(p2) == row.index(p1) + 1 and g_mmr[r, row.index(p1)] == g_mmr[r, row.index(p2)]
        for r in (2, 3):
            row = g_pos[r].tolist()
            assert row[0] == 0 and p1 not in row and p2 in row, f"{where}: row {r}"


def test_lambda_one_on_a_real_sweep_is_a_sequential_scan():
    """The pool comes from a real b4r_rank_full call; rows 0 and 1 exclude most of the catalogue, so their pools end in -1 / -inf."""
    lib = _lib.load()
    V, width, R, M, K = 300, 64, R_MAX, 100, 10
    c = case(V, width)
    g = torch.Generator().manual_seed(9)
    hidden = torch.randn(R, width, generator=g).to(DEV)
    bias = (torch.randn(V, generator=g) * 0.01).to(DEV)
    ex = torch.full((R, V), -1, dtype=torch.int64)
    ex[0, :] = torch.arange(V); ex[0, :5] = -1                         # ids 0 .. 4 are left, and 0 .. 2 lie below first_item: 2 items
    ex[1, : V - 50] = torch.arange(V - 50)
    ex = ex.to(DEV)
    pool_ids = torch.empty((R, M), dtype=torch.int64, device=DEV)
    pool_sc = torch.empty((R, M), device=DEV)
    need = int(lib.b4r_rank_full_scratch_bytes(R, V, M))
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert lib.b4r_rank_full(P(hidden), width, None, P(c["table_d"]), P(bias), width, V, 3, R, P(ex), V, None, M, P(pool_ids), P(pool_sc),
                             None, P(scratch), need, stream()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    pool = Pool(pool_ids.cpu().numpy(), pool_sc.cpu().numpy())
    assert int((pool.ids[0] >= 0).sum()) == 2 and int((pool.ids[1] >= 0).sum()) == 50
    q = four_quotas(V)
    for quotas in (q[:1], q[1:], q):
        for K in (10, M):
            rc, g_ids, g_sc, _, g_pos = run(c, width, V, pool, 1.0, K, quotas)[:5]
            assert rc == 0, _lib.last_error()
            scan = qref.sequential_scan(pool.ids, pool.sc, V, K, quotas)
            for r, picked in enumerate(scan):
                assert g_pos[r, :len(picked)].tolist() == picked and (g_pos[r, len(picked):] == -1).all()
                assert g_ids[r, :len(picked)].tolist() == pool.ids[r, picked].tolist() and (g_ids[r, len(picked):] == -1).all()
                assert bits_equal(g_sc[r, :len(picked)], pool.sc[r, picked])
        assert any(picked != list(range(len(picked))) for picked in scan)      # the caps bind


def test_device_rnorm():
    """item_rnorm = NULL leaves the rnorm in the scratch that b4r_rerank_diverse leaves there, and gives the restatement's result with it."""
    V, width = 300, 64
    c = case(V, width)
    ids, sc = make_pool(V, 100, R=5, seed=3)
    pool = Pool(ids, sc)
    quotas = four_quotas(V)[1:3]
    d_scratch = run_diverse(c, width, V, ids, sc, 0.3, 100, rnorm=None)[6]
    rc, *got, _, _, scratch = run(c, width, V, pool, 0.3, 100, quotas, rnorm=None)
    assert rc == 0, _lib.last_error()
    rnorm_dev = []
    for s in (d_scratch, scratch):
        off = (16 - s.data_ptr() % 16) % 16
        rnorm_dev.append(s[off:off + 4 * V].view(torch.float32).cpu().numpy())
    assert bits_equal(rnorm_dev[0], rnorm_dev[1])
    want = qref.rerank(c["table"], rnorm_dev[1], ids, sc, 0.3, 100, quotas)
    assert_same(got, want, 100, "device rnorm")
    rc, *given = run(c, width, V, pool, 0.3, 100, quotas, rnorm=torch.as_tensor(rnorm_dev[1]).to(DEV))[:5]
    assert rc == 0, _lib.last_error()
    assert_same(given, want, 100, "that rnorm given")


def test_errors_and_null_outputs():
    V, width = 300, 64
    c = case(V, width)
    lib = _lib.load()
    ids, sc = make_pool(V, 100, R=3)
    pool = Pool(ids, sc)
    quotas = four_quotas(V)[:2]
    arr, keep = quotas_on_device(tuple(quotas))
    out = torch.full((300,), 7, dtype=torch.int32, device=DEV)

    def call(M=100, K=10, lam=0.5, ld=width, w=width, rnorm=c["rnorm_d"], scratch=None, nbytes=0, q=arr, n=2):
        return lib.b4r_rerank_quota(P(c["table_d"]), ld, w, V, P(rnorm), P(pool.ids_d), P(pool.sc_d), 3, M, lam, K, q, n, None, None, None,
                                    P(out), P(scratch), nbytes, stream())
    bad_group = (_lib.ItemQuota * 1)()
    bad_group[0].item_group, bad_group[0].n_groups = P(keep[0][0]), -1
    no_group = (_lib.ItemQuota * 1)()
    no_group[0].n_groups = 3
    for kw, code in ((dict(M=0), -2), (dict(M=1025), -2), (dict(K=101), -2), (dict(lam=-0.1), -1), (dict(lam=1.5), -1),
                     (dict(lam=float("nan")), -1), (dict(ld=width + 4), -2), (dict(w=6, ld=6), -2), (dict(n=-1), -2), (dict(n=5), -2),
                     (dict(q=None), -1), (dict(q=bad_group, n=1), -1), (dict(q=no_group, n=1), -1)):
        assert call(**kw) == code, kw
        assert "b4r_rerank_quota" in _lib.last_error()
    need = int(lib.b4r_rerank_quota_scratch_bytes(3, 100, V))
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert call(rnorm=None, scratch=scratch, nbytes=4 * V - 1) == -5 and "scratch" in _lib.last_error()    # B4R_E_NOMEM
    assert call(rnorm=None, scratch=None, nbytes=0) == -5
    torch.cuda.synchronize()
    assert (out == 7).all()                                           # no refused call wrote anything
    assert call(rnorm=None, scratch=scratch, nbytes=need) == 0
    assert call(K=0) == 0 and lib.b4r_rerank_quota(None, width, width, V, None, None, None, 0, 100, 0.5, 10, None, 0, None, None, None,
                                                   None, None, 0, stream()) == 0
    torch.cuda.synchronize()
    assert (out[30:] == 7).all() and (out[:30] >= 0).all()            # only [R, K] = [3, 10] was written (10 picks fit the caps)
    # any output may be NULL: each alone gives what all four give (run() checks that nothing beyond [R, K] is written)
    full = run(c, width, V, pool, 0.3, 10, quotas)
    assert full[0] == 0
    for i in range(4):
        only = run(c, width, V, pool, 0.3, 10, quotas, outputs=tuple(j == i for j in range(4)))
        assert only[0] == 0 and all(only[1 + j] is None for j in range(4) if j != i)
        assert only[1 + i].tobytes() == full[1 + i].tobytes() and only[1 + i].dtype == full[1 + i].dtype
    none = run(c, width, V, pool, 0.3, 10, quotas, outputs=(False,) * 4)
    assert none[0] == 0


def test_reproducible_and_in_a_captured_graph():
    V, width, M, K = 1100, 132, 513, 100
    c = case(V, width)
    ids, sc = make_pool(V, M, seed=11)
    pool = Pool(ids, sc)
    quotas = four_quotas(V)[1:3]
    want = qref.rerank(c["table"], c["rnorm"], ids, sc, 0.3, K, quotas, c["sim"])
    for rnorm in ("given", None):
        rc, *a, call, read, _ = run(c, width, V, pool, 0.3, K, quotas, rnorm=rnorm)
        assert rc == 0, _lib.last_error()
        if rnorm == "given":
            assert_same(a, want, K, "first call")
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
def model_quota(V, cap=2, groups=4):
    """(the spec, its restatement): token j is in group j % groups; the specials are in none."""
    g = np.where(np.arange(V) < engine_mod.SPECIAL_IDS, -1, np.arange(V) % groups)
    return pack_item_groups(g, cap), Quota(g, groups, cap)


@pytest.mark.parametrize("factorised", [False, True])
def test_recommend_tensor_max_per_group(factorised, gemm_mode):
    rec, items = build_small_app(factorised)
    model, V = rec.model, rec.model.vocab_size
    batches = [rec.dataloader.prepare_inference(list(items[s:s + 9])) for s in (0, 30, 60, 95, 140)]
    batch = {key: torch.from_numpy(np.concatenate([np.asarray(b[key]) for b in batches], axis=0)) for key in batches[0]}
    k, pool = 8, 60
    spec, quota = model_quota(V)
    by_five, quota5 = model_quota(V, cap=1, groups=5)
    plain = model.recommend_tensor(batch, k=k)
    same = model.recommend_tensor(batch, k=k, max_per_group=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, same))       # unchanged without the argument
    table = model.engine.view("word_embeddings/embeddings").cpu().numpy()
    rnorm = device_rnorm(model)
    cand = model.recommend_tensor(batch, k=pool)
    cand_h = (cand[0].cpu().numpy(), cand[1].cpu().numpy())
    got = model.recommend_tensor(batch, k=k, max_per_group=spec, pool=pool)
    want = qref.rerank(table, rnorm, cand_h[0], cand_h[1], 1.0, k, [quota])
    assert got[0].shape == (plain[0].shape[0], k) and torch.equal(got[2], plain[2])
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and bits_equal(got[1].cpu().numpy(), want[1])
    assert not qref.violations(got[0].cpu().numpy(), V, [quota]) and not torch.equal(got[0], plain[0])
    assert (got[0] >= 0).all()
    scan = qref.sequential_scan(cand_h[0], cand_h[1], V, k, [quota])
    assert [cand_h[0][r, p].tolist() for r, p in enumerate(scan)] == got[0].cpu().tolist()      # relevance order under the caps
    # two specs, and with diversity
    two = model.recommend_tensor(batch, k=k, max_per_group=[spec, by_five], pool=pool)
    want2 = qref.rerank(table, rnorm, cand_h[0], cand_h[1], 1.0, k, [quota, quota5])
    assert np.array_equal(two[0].cpu().numpy(), want2[0]) and not qref.violations(two[0].cpu().numpy(), V, [quota, quota5])
    assert (two[0][:, 5:] == -1).all() and (two[1][:, 5:] == -np.inf).all()                  # five groups, one each: at most 5 picks
    lam = engine_mod.check_rerank_args(k, pool, 0.7)[2]
    div = model.recommend_tensor(batch, k=k, max_per_group=spec, pool=pool, diversity=0.7)
    want_d = qref.rerank(table, rnorm, cand_h[0], cand_h[1], lam, k, [quota])
    assert np.array_equal(div[0].cpu().numpy(), want_d[0]) and bits_equal(div[1].cpu().numpy(), want_d[1])
    assert not qref.violations(div[0].cpu().numpy(), V, [quota]) and not torch.equal(div[0], got[0])
    only_div = model.recommend_tensor(batch, k=k, pool=pool, diversity=0.7)      # diversity alone still is b4r_rerank_diverse's result
    assert np.array_equal(only_div[0].cpu().numpy(), dref.rerank(table, rnorm, cand_h[0], cand_h[1], lam, k)[0])
    # the default pool: min(1024, max(10 k, 50)) = 80 candidates
    d80 = model.recommend_tensor(batch, k=k, max_per_group=spec)
    c80 = model.recommend_tensor(batch, k=80)
    assert np.array_equal(d80[0].cpu().numpy(), qref.rerank(table, rnorm, c80[0].cpu().numpy(), c80[1].cpu().numpy(), 1.0, k, [quota])[0])
    # exclusions and allow-lists stay in force
    allow = torch.zeros(V, dtype=torch.bool)
    allow[::3] = True
    P_ = int(batch["masked_lm_positions"].shape[1])
    ex = torch.full((batch["input_word_ids"].shape[0], 4), -1, dtype=torch.int64)
    for row, slot in zip(got[0].cpu(), got[2].cpu().tolist()):         # bar the first capped picks of every batch row
        ex[slot // P_] = row[:4]
    kept = model.recommend_tensor(batch, k=k, exclude=ex, allow=allow, max_per_group=spec, pool=pool)
    for row, slot in zip(kept[0].cpu().tolist(), kept[2].cpu().tolist()):
        b = slot // P_
        live = [i for i in row if i >= 0]
        assert live and all(i % 3 == 0 and i >= 3 for i in live)
        assert not set(live) & set(ex[b].tolist()) and not set(live) & set(batch["input_word_ids"][b].tolist())
    assert not qref.violations(kept[0].cpu().numpy(), V, [quota])
    lists = model.recommend(batch, k=k, max_per_group=spec, pool=pool)
    assert [ids for per_row in lists for ids, _ in per_row] == got[0].cpu().tolist()
    short = pack_item_groups(np.zeros(V - 1, np.int64), 1)
    for bad in (dict(max_per_group=short), dict(max_per_group=[spec] * 5), dict(max_per_group=(np.zeros(V), 1)),
                dict(max_per_group=spec, pool=k - 1), dict(max_per_group=spec, pool=1025), dict(max_per_group=spec, diversity=1.5),
                dict(pool=50)):
        with pytest.raises(ValueError):
            model.recommend_tensor(batch, k=k, **bad)


def test_recommend_batch_with_distinct_labels():
    rec, items = build_small_app()
    catalogue = sorted(set(items))
    labels = {item: "cat-%d" % (i % 7) for i, item in enumerate(catalogue)}
    histories = [items[s:s + n] for s, n in ((0, 15), (40, 3), (90, 30), (120, 1), (7, 22))]
    plain = rec.recommend_batch(histories, 5)
    assert rec.recommend_batch(histories, 5, max_per_group=None) == plain
    got = rec.recommend_batch(histories, 5, max_per_group=(labels, 1))
    assert all(len(lst) == 5 and len({labels[i] for i in lst}) == 5 for lst in got)
    assert all(not set(lst) & set(h) for lst, h in zip(got, histories))          # and nothing the user has seen
    assert any(len({labels[i] for i in lst}) < 5 for lst in plain)               # the plain lists repeat a label: the cap binds
    assert got[0][0] == plain[0][0]                                              # the best item stays the best
    # a callable, a cap per label (absent label: not capped), two pairs, with allowed_items and with diversity
    per = rec.recommend_batch(histories, 5, max_per_group=(labels.get, {"cat-0": 0, "cat-1": 1}))
    assert all(len(lst) == 5 and not any(labels[i] == "cat-0" for i in lst) and sum(labels[i] == "cat-1" for i in lst) <= 1 for lst in per)
    halves = {item: i % 2 for i, item in enumerate(catalogue)}
    two = rec.recommend_batch(histories, 4, max_per_group=[(labels, 1), (halves, 2)], candidate_pool=100)
    assert all(len(lst) == 4 and len({labels[i] for i in lst}) == 4 and sorted(halves[i] for i in lst) == [0, 0, 1, 1] for lst in two)
    allowed = catalogue[::2]
    both = rec.recommend_batch(histories, 5, allowed_items=allowed, diversity=0.5, max_per_group=(labels, 1))
    assert all(len(lst) == 5 and set(lst) <= set(allowed) and len({labels[i] for i in lst}) == 5 for lst in both)
    assert rec(histories[0], 5, max_per_group=(labels, 1)) == got[0]
    for bad in ((labels, 1.5), (labels,), [(labels, 1)] * 5, (3, 1), (labels, {"cat-0": "many"})):
        with pytest.raises(ValueError):
            rec.recommend_batch(histories, 5, max_per_group=bad)


def test_evaluator_with_max_per_group():
    rec, _ = build_small_app()
    model, V = rec.model, rec.model.vocab_size
    K, pool, n_users = 10, 60, 16
    batch = orc.synthetic_batch(n_users, 24, 4, V, seed=81, ragged=True, finetune=True)
    b_idx, p_idx = torch.nonzero(batch["masked_lm_weights"] != 0, as_tuple=True)
    assert b_idx.tolist() == list(range(n_users))
    gt = batch["masked_lm_ids"][b_idx, p_idx]
    exclude = batch["labels"].clone()
    exclude[exclude == gt[:, None]] = -1
    spec, quota = model_quota(V, cap=2, groups=6)                       # at most 12 items: room for K = 10
    metrics = lambda: [evaluation.Counter(name="Valid Ranks")] + [f(k) for f in (evaluation.HR, evaluation.NDCG) for k in (1, 5, 10)]
    ev = evaluation.get(full_ranking=True, list_k=K, max_per_group=spec, candidate_pool=pool, metrics=metrics())
    ev.evaluate(model, [batch])
    res = ev.get_metrics_results()
    lists = model.recommend_tensor(batch, k=K, exclude_seen=False, exclude=exclude, max_per_group=spec, pool=pool)[0].cpu().numpy()
    assert not qref.violations(lists, V, [quota])
    plain = model.recommend_tensor(batch, k=K, exclude_seen=False, exclude=exclude)[0].cpu().numpy()
    assert not np.array_equal(lists, plain)
    gt_h = gt.numpy()
    ranks = np.array([row.tolist().index(g) + 1 if g in row else K + 1 for row, g in zip(lists, gt_h)])
    assert res["Valid Ranks"] == n_users
    for k in (1, 5, 10):                                              # HR / NDCG from the position in the capped list
        assert res[f"HR@{k}"] == pytest.approx(float((ranks <= k).mean()), abs=1e-12)
        ndcg = [1.0 / math.log2(r + 1) if r <= k else 0.0 for r in ranks.tolist()]
        assert res[f"NDCG@{k}"] == pytest.approx(math.fsum(ndcg) / n_users, abs=1e-12)
    exposure = np.bincount(lists[lists >= 0], minlength=V)[engine_mod.SPECIAL_IDS:]
    assert res[f"Coverage@{K}"] == pytest.approx(float((exposure > 0).mean()), rel=1e-12)
    both = evaluation.get(full_ranking=True, list_k=K, max_per_group=[spec], diversity=0.5, candidate_pool=pool, metrics=metrics())
    both.evaluate(model, [batch])
    lists_d = model.recommend_tensor(batch, k=K, exclude_seen=False, exclude=exclude, max_per_group=spec, pool=pool, diversity=0.5)[0]
    ranks_d = np.array([row.index(g) + 1 if g in row else K + 1 for row, g in zip(lists_d.cpu().tolist(), gt_h.tolist())])
    assert both.get_metrics_results()["HR@10"] == pytest.approx(float((ranks_d <= 10).mean()), abs=1e-12)
    for bad in (dict(max_per_group=spec), dict(full_ranking=True, max_per_group=spec),
                dict(full_ranking=True, list_k=K, max_per_group=spec, metrics=[evaluation.HR(20)]),
                dict(full_ranking=True, list_k=K, max_per_group=spec, metrics=[evaluation.MAP()]),
                dict(full_ranking=True, list_k=K, max_per_group=[spec] * 5, metrics=metrics()),
                dict(full_ranking=True, list_k=K, max_per_group=(np.zeros(V), 1), metrics=metrics()),
                dict(full_ranking=True, list_k=K, max_per_group=spec, candidate_pool=K - 1, metrics=metrics())):
        with pytest.raises(ValueError):
            evaluation.get(**bad)
    wrong = evaluation.get(full_ranking=True, list_k=K, max_per_group=pack_item_groups(np.zeros(V + 1, np.int64), 1), metrics=metrics())
    with pytest.raises(ValueError):
        wrong.evaluate(model, [batch])
