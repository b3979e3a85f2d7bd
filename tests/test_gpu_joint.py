"""Joint recommendations on the GPU (b4r_rank_joint): every output -- topk_ids, topk_scores, party_n, member_util -- bit for bit
against the CPU restatement (tests/joint_ref.py) in all three modes, and the model / app layers built on the call.

The shapes cross the sweep's boundaries: 1024 ids per chunk (V = 4, 33, 1027, 2051), the 16-float k-block and H % 4 (H = 32, 100,
256), every instance of the member template full and padded (M = 1, 2, 3, 5, 8, 9, 16), partly filled and several tiles (NP = 1, 3,
9, 17), K = 1, 10, 1024 and a K beyond the party's allowed set.  make_case's twin table rows with equal bias give exact ties in the
aggregate, inside a chunk and across the chunk boundary.  Planted: a member who can be served nothing (an empty party), a party of
absent slots only, a row shared by two parties, entries of party_rows outside [0, R)."""
import functools

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib
from bert4rec_amd.apps import Recommender
from tests import catalogue_ref as ref
from tests import joint_ref as jr
from tests import score_dist_ref as sref
from tests.b4r_testlib import P, stream
from tests.test_gpu_audience import prepared, setting
from tests.test_gpu_full_rank import make_case

pytestmark = pytest.mark.gpu

DEV = "cuda"
FIRST = 3
F32 = np.float32
NINF = -np.inf
MODES = (jr.ADDITIVE, jr.LEAST_MISERY, jr.MOST_PLEASURE)
# (R, H, V, NP, M, K)
SHAPES = [(3, 32, 4, 1, 1, 1), (5, 100, 33, 3, 2, 10), (9, 32, 1027, 9, 3, 10), (20, 256, 2051, 17, 5, 10), (12, 32, 2051, 9, 8, 1024),
          (24, 100, 1027, 3, 9, 1024), (40, 32, 2051, 17, 16, 10), (6, 32, 33, 17, 1, 1024), (7, 256, 1027, 1, 16, 1),
          (10, 32, 1027, 17, 2, 10), (10, 100, 2051, 9, 4, 10), (18, 32, 33, 3, 8, 10)]
# (calibrated: row_lse given, inv_temperature, bias, item_scale, filters, weights, veto): every value of each at least once
CALLS = [(True, 1.0, True, False, True, True, True), (False, 0.5, False, True, False, False, False),
         (True, 2.0, True, True, True, False, False), (False, 1.0, True, False, True, True, True)]


@functools.lru_cache(maxsize=None)
def planted(R, H, V, NP, M):
    """make_case's inputs, three filters (0: a random 80 %, 1: zeros, row_filter 3: none) and the parties."""
    hidden, table, bias, ex, _ = make_case(R, H, V, seed=R * 31 + H + V % 97 + NP + M, E=12)
    rng = np.random.default_rng(R + V + NP * 17 + M)
    masks = np.zeros((2, V), bool)
    masks[0] = rng.random(V) < 0.8
    masks[0, V - 1] = True
    row_filter = np.full(R, 3, np.int32)
    row_filter[1::5] = 0
    dead = R - 1 if R > 2 else -1
    if dead >= 0:
        row_filter[dead] = 1                                                  # may be served nothing: as good as having seen everything
    parties = rng.integers(0, max(R - 1, 1), size=(NP, M)).astype(np.int32)   # (the dead row only where planted)
    parties[rng.random((NP, M)) < 0.2] = -1
    if NP > 1:
        parties[1] = -1                                                       # absent slots only
        parties[1, ::2] = R + 3                                               # an index past the rows is an absent slot too
        parties[1, M - 1] = -2147483648 if M > 1 else R
    if NP > 2 and dead >= 0:
        parties[2, 0] = 0
        parties[2, M - 1] = dead                                              # a member with nothing to be served: an empty party
    if NP > 4:
        parties[3, 0] = parties[4, M - 1] = 2                                 # one row shared by two parties
        parties[0] = np.arange(M) % max(R - 1, 1)                             # every slot present
    scale = (0.5 + np.random.default_rng(V + 1).random(V)).astype(F32)
    weights = rng.uniform(0.25, 2.0, size=(NP, M)).astype(F32)
    weights[rng.random((NP, M)) < 0.2] = 1.0
    return dict(hidden=hidden.numpy().copy(), table=table.numpy().copy(), bias=bias.numpy().copy(), ex=ex, masks=masks,
                words=ref.pack_bits(masks), row_filter=row_filter, parties=parties, scale=scale, weights=weights, dead=dead)


@functools.lru_cache(maxsize=None)
def rows_of(key, calibrated, inv_t, use_bias, use_scale, filters):
    """(t [R, V], allowed(r) [R, V], row_lse [R] or None) of the case: computed once, shared, never written"""
    c = planted(*key)
    t, ok = jr.row_quantities(c["hidden"], c["table"], c["bias"] if use_bias else None, c["scale"] if use_scale else None, inv_t, FIRST,
                              c["ex"], c["words"] if filters else None, c["row_filter"] if filters else None)
    lse = sref.blocked(t, ok)[2] if calibrated else None
    for a in (t, ok, lse):
        if a is not None:
            a.setflags(write=False)
    return t, ok, lse


def veto_of(key, call, binds):
    """A threshold that vetoes about 30 % / M of a member's items: it binds and leaves something"""
    if not binds:
        return F32(NINF)
    t, ok, lse = rows_of(key, *call[:5])
    u = jr.utilities(t, lse)
    live = ok & np.isfinite(u)
    return F32(np.quantile(u[live], 0.3 / key[4])) if live.any() else F32(NINF)


def dev(x, dtype=None):
    if x is None:
        return None
    t = torch.as_tensor(np.array(x) if isinstance(x, np.ndarray) else x)     # (a copy: the shared references are read-only)
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def run_joint(c, mode, K, lse=None, inv_t=1.0, use_bias=True, use_scale=False, filters=True, weights=None, min_util=NINF, parties=None,
              scratch_bytes=None, hidden=None, hidden_row=None, hidden_ld=None, sync=True, outs=None, keep=None, M=None, want=(1, 1, 1, 1)):
    """b4r_rank_joint on the case; returns (rc, dict of numpy outputs).  The outputs start from sentinels."""
    lib = _lib.load()
    R, H = c["hidden"].shape
    V = c["table"].shape[0]
    parties = c["parties"] if parties is None else parties
    NP, Mp = parties.shape
    M = Mp if M is None else M
    if keep is None:
        d = dict(hidden=dev(c["hidden"] if hidden is None else hidden), table=dev(c["table"]), bias=dev(c["bias"]) if use_bias else None,
                 ex=dev(c["ex"]), words=dev(c["words"].view(np.int32)) if filters else None, rf=dev(c["row_filter"]) if filters else None,
                 scale=dev(c["scale"]) if use_scale else None, hr=dev(hidden_row, torch.int64), lse=dev(lse), pr=dev(parties, torch.int32),
                 w=dev(weights))
        need = int(lib.b4r_rank_joint_scratch_bytes(NP, min(max(M, 1), 16), V, min(max(K, 0), 1024)))
        nbytes = need if scratch_bytes is None else scratch_bytes
        keep = (d, torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV), nbytes)
    d, scratch, nbytes = keep
    if outs is None:
        outs = dict(ids=torch.full((NP, max(K, 1)), -7, dtype=torch.int64, device=DEV), scores=torch.full((NP, max(K, 1)), 7.0, device=DEV),
                    n=torch.full((NP,), -7, dtype=torch.int32, device=DEV), util=torch.full((NP, max(K, 1), Mp), 7.0, device=DEV))
    o = [P(outs[k]) if w else None for k, w in zip(("ids", "scores", "n", "util"), want)]
    rc = lib.b4r_rank_joint(P(d["hidden"]), hidden_ld or H, P(d["hr"]), P(d["table"]), P(d["bias"]), H, V, FIRST, R, P(d["ex"]),
                            c["ex"].shape[1], P(d["words"]), 2 if filters else 0, P(d["rf"]), P(d["scale"]), inv_t, P(d["lse"]), P(d["pr"]),
                            NP, M, P(d["w"]), mode, float(min_util), K, *o, P(scratch), nbytes, stream())
    if not sync:
        return rc, outs, keep
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in outs.items()}


def untouched(got):
    return (got["ids"] == -7).all() and (got["n"] == -7).all() and (got["scores"] == 7.0).all() and (got["util"] == 7.0).all()


def same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def assert_equals_ref(got, want, what):
    ids, scores, n, util = want
    assert np.array_equal(got["n"], n), f"{what}: party_n"
    assert np.array_equal(got["ids"], ids), f"{what}: topk_ids"
    assert np.array_equal(got["scores"].view(np.uint32), scores.view(np.uint32)), f"{what}: topk_scores"
    assert np.array_equal(got["util"].view(np.uint32), util.view(np.uint32)), f"{what}: member_util"
    assert not np.isnan(got["scores"]).any() and not np.isnan(got["util"]).any()


@pytest.mark.parametrize("R,H,V,NP,M,K", SHAPES, ids=["R%d_H%d_V%d_NP%d_M%d_K%d" % s for s in SHAPES])
def test_rank_joint_against_the_restatement(R, H, V, NP, M, K):
    key = (R, H, V, NP, M)
    c = planted(*key)
    bound = short = 0
    for call in CALLS:
        calibrated, inv_t, use_bias, use_scale, filters, weighted, veto = call
        t, ok, lse = rows_of(key, *call[:5])
        min_util = veto_of(key, call, veto)
        for mode in MODES:
            w = c["weights"] if weighted else None
            rc, got = run_joint(c, mode, K, lse, inv_t, use_bias, use_scale, filters, w, min_util)
            assert rc == 0, _lib.last_error()
            want = jr.rank_joint(t, ok, c["parties"], mode, K, lse, w, min_util)
            assert_equals_ref(got, want, f"{call} mode {mode}")
            if veto:
                free = jr.rank_joint(t, ok, c["parties"], mode, K, lse, w)[2]
                bound += int(((want[2] < free) & (want[2] > 0)).sum())
            short += int(((want[2] < K) & (want[2] > 0)).sum())
            if NP > 1:
                assert want[2][1] == 0 and (got["ids"][1] == -1).all() and np.isneginf(got["scores"][1]).all() and np.isneginf(got["util"][1]).all()
            if NP > 2 and c["dead"] >= 0 and filters:
                assert want[2][2] == 0 and (got["ids"][2] == -1).all()
    if V >= 1027 and NP >= 3:
        assert bound > 0, "the veto never bound"
    if K == 1024 and V < 1024:
        assert short > 0, "K never went beyond a party's allowed set"
    # exact ties in the aggregate: the twins come in id order, next to each other
    t, ok, lse = rows_of(key, *CALLS[0][:5])
    ids, scores, _, _ = jr.rank_joint(t, ok, c["parties"], jr.ADDITIVE, K, lse)
    if K >= 10 and V >= 1031:
        tied = [(p, i) for p in range(NP) for i in range(K - 1) if ids[p, i + 1] >= 0 and scores[p, i] == scores[p, i + 1]]
        assert tied and all(ids[p, i] < ids[p, i + 1] for p, i in tied)
        assert any(ids[p, i] < 1024 <= ids[p, i + 1] for p, i in tied), "no tie across the chunk boundary"


@pytest.mark.parametrize("K", (100, 1024))
def test_parties_of_equal_aggregates(K):
    """A party of zero hidden rows without bias, scale or row_lse: every aggregate is +0.0 in every mode, so the 32 score bits are
    resolved at once (kmin == kmax) and the id bits alone decide: the sweep's two 8-bit passes over the local id (K = 100: each chunk
    holds more than K) and the merge's four over the id (K = 1024).  M = 3 (slots of four, one absent), five parties (a second, partly filled tile), three chunks, the last partly beyond V."""
    key = (17, 8, 2049 + FIRST, 5, 3)
    c = dict(planted(*key))
    c["hidden"] = c["hidden"].copy()
    c["hidden"][:3] = 0.0
    assert c["parties"][0].tolist() == [0, 1, 2]
    t, ok = jr.row_quantities(c["hidden"], c["table"], None, None, 1.0, FIRST, c["ex"], None, None)
    assert (t[:3].view(np.uint32) == 0).all()
    for mode in MODES:
        rc, got = run_joint(c, mode, K, None, 1.0, False, False, False, c["weights"])
        assert rc == 0, _lib.last_error()
        want = jr.rank_joint(t, ok, c["parties"], mode, K, None, c["weights"])
        assert_equals_ref(got, want, f"mode {mode}")
        n0 = int(want[2][0])
        assert n0 > 1024 and (np.diff(got["ids"][0]) > 0).all() and (got["scores"][0].view(np.uint32) == 0).all()


def test_null_outputs_and_weights_are_ignored_outside_the_additive_mode():
    key = (9, 32, 1027, 9, 3)
    c = planted(*key)
    t, ok, lse = rows_of(key, True, 1.0, True, False, True)
    rc, full = run_joint(c, jr.LEAST_MISERY, 10, lse)
    assert rc == 0, _lib.last_error()
    rc, weighted = run_joint(c, jr.LEAST_MISERY, 10, lse, weights=c["weights"])
    assert rc == 0 and same_bits(full, weighted)
    for want in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0, 1, 0, 1)):   # member_util without topk_ids: ids in the scratch
        rc, part = run_joint(c, jr.LEAST_MISERY, 10, lse, want=want)
        assert rc == 0, _lib.last_error()
        for k, w in zip(("ids", "scores", "n", "util"), want):
            assert part[k].tobytes() == full[k].tobytes() if w else ((part[k] == -7).all() if k in ("ids", "n") else (part[k] == 7.0).all()), (want, k)
    # NP = 0 and K = 0 launch nothing
    rc, got = run_joint(c, jr.ADDITIVE, 0, lse)
    assert rc == 0 and untouched(got)
    rc, got = run_joint(c, jr.ADDITIVE, 10, lse, parties=np.zeros((0, 3), np.int32))
    assert rc == 0


def test_reduced_scratch_hidden_row_and_two_runs():
    """A scratch for one tile at a time gives the bits of the full scratch; a hidden_ld > H with hidden_row: the same bits; two runs
    are bitwise equal."""
    lib = _lib.load()
    for key, K in (((20, 256, 2051, 17, 5), 10), ((10, 32, 1027, 17, 2), 10), ((12, 32, 2051, 9, 8), 1024), ((40, 32, 2051, 17, 16), 10)):
        R, H, V, NP, M = key
        c = planted(*key)
        t, ok, lse = rows_of(key, True, 1.0, True, False, True)
        args = (c, jr.ADDITIVE, K, lse, 1.0, True, False, True, c["weights"], veto_of(key, CALLS[0], True))
        rc, full = run_joint(*args)
        assert rc == 0, _lib.last_error()
        rc, again = run_joint(*args)
        assert rc == 0 and same_bits(full, again), "two runs differ"
        mp = min(m for m in (1, 2, 4, 8, 16) if m >= M)
        tile = int(lib.b4r_rank_joint_scratch_bytes(16 // mp, M, V, K))
        assert tile < int(lib.b4r_rank_joint_scratch_bytes(NP, M, V, K))
        for nbytes in (tile, tile + tile // 2):
            rc, grouped = run_joint(*args, scratch_bytes=nbytes)
            assert rc == 0 and same_bits(full, grouped), (key, nbytes)
        ld = H + 4
        wide = np.zeros((R + 2, ld), F32)
        perm = np.random.default_rng(1).permutation(R + 2)[:R]
        wide[perm, :H] = c["hidden"]
        rc, moved = run_joint(*args, hidden=wide, hidden_row=perm, hidden_ld=ld)
        assert rc == 0 and same_bits(full, moved), key
        # a negative hidden_row: a member with nothing to be served, its parties are empty
        gone = perm.copy()
        gone[0] = -1
        rc, less = run_joint(*args, hidden=wide, hidden_row=gone, hidden_ld=ld)
        assert rc == 0, _lib.last_error()
        assert_equals_ref(less, jr.rank_joint(t, ok, c["parties"], jr.ADDITIVE, K, lse, c["weights"], args[-1], row_dead=np.arange(R) == 0), key)
        assert (c["parties"] == 0).any(axis=1).sum() > 0 and not same_bits(full, less)


def test_result_does_not_depend_on_the_order_of_the_parties():
    key = (20, 256, 2051, 17, 5)
    c = planted(*key)
    t, ok, lse = rows_of(key, True, 1.0, True, False, True)
    rc, full = run_joint(c, jr.MOST_PLEASURE, 10, lse)
    perm = np.random.default_rng(4).permutation(17)
    rc2, moved = run_joint(c, jr.MOST_PLEASURE, 10, lse, parties=np.ascontiguousarray(c["parties"][perm]))
    assert rc == 0 and rc2 == 0 and all(moved[k].tobytes() == np.ascontiguousarray(full[k][perm]).tobytes() for k in full)


def test_argument_errors_leave_the_outputs_untouched():
    lib = _lib.load()
    key = (20, 256, 2051, 17, 5)
    c = planted(*key)
    lse = rows_of(key, True, 1.0, True, False, True)[2]
    for inv_t in (0.0, -1.0, float("nan"), float("inf")):
        rc, got = run_joint(c, jr.ADDITIVE, 10, lse, inv_t)
        assert rc == -1 and "inv_temperature" in _lib.last_error() and untouched(got)
    for mode in (-1, 3):
        rc, got = run_joint(c, mode, 10, lse)
        assert rc == -1 and "mode" in _lib.last_error() and untouched(got)
    rc, got = run_joint(c, jr.ADDITIVE, 10, lse, min_util=float("nan"))
    assert rc == -1 and untouched(got)
    for M in (0, 17):
        rc, got = run_joint(c, jr.ADDITIVE, 10, lse, M=M)
        assert rc == -2 and "members" in _lib.last_error() and untouched(got)
    rc, got = run_joint(c, jr.ADDITIVE, 1025, lse)
    assert rc == -2 and untouched(got)
    tile = int(lib.b4r_rank_joint_scratch_bytes(2, 5, 2051, 10))
    for nbytes in (tile // 2, 0):
        rc, got = run_joint(c, jr.ADDITIVE, 10, lse, scratch_bytes=nbytes)
        assert rc == -5 and "b4r_rank_joint" in _lib.last_error() and untouched(got)


def test_graph_capture_replays_the_eager_bits():
    key = (20, 256, 2051, 17, 5)
    c = planted(*key)
    lse = rows_of(key, True, 2.0, True, True, True)[2]
    args = (c, jr.ADDITIVE, 10, lse, 2.0, True, True, True, c["weights"], F32(-9.0))
    rc, eager = run_joint(*args)
    assert rc == 0, _lib.last_error()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        rc, outs, keep = run_joint(*args, sync=False)                        # allocations and copies outside the capture
        assert rc == 0
        torch.cuda.synchronize()
        for k, v in outs.items():
            v.fill_(-7 if k in ("ids", "n") else 7)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            rc, _, _ = run_joint(*args, sync=False, outs=outs, keep=keep)
            assert rc == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert (outs["n"] == -7).all(), "a capture must not run the kernels"
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(eager, {k: v.cpu().numpy() for k, v in outs.items()})


# ---- the model ------------------------------------------------------------------------------------------------------------------------
N_MEMBERS = 40


def model_parties(rng, NP=11, M=5):
    parties = rng.integers(0, N_MEMBERS, size=(NP, M)).astype(np.int64)
    parties[rng.random((NP, M)) < 0.25] = -1
    parties[1] = -1
    parties[2, 1:] = -1
    parties[2, 0] = 7                                                        # a party of one
    parties[3, 0] = parties[4, 1] = 9                                        # a shared row
    return parties


@pytest.mark.parametrize("hidden", (64, 128))
def test_recommend_joint_tensor_equals_the_host_composition(hidden):
    """score_distribution_tensor with every id as a query per member, then joint_ref's aggregation and ordering on the host"""
    dl, model, V, histories, _, _ = setting(hidden)
    batch = prepared(dl, histories[:N_MEMBERS])
    rng = np.random.default_rng(hidden)
    parties = model_parties(rng)
    weights = rng.uniform(0.5, 2.0, size=parties.shape).astype(F32)
    allow = torch.as_tensor(np.random.default_rng(3).random(V) < 0.7)
    every = torch.arange(V, dtype=torch.int64)[None, :].expand(N_MEMBERS, -1)
    assert V <= 1024
    K = 10
    for kw in (dict(), dict(allow=allow, temperature=0.5)):
        logp = model.score_distribution_tensor(batch, query_ids=every, **kw)["logp"].cpu().numpy()
        ok = np.isfinite(logp)
        for strategy, mode in jr.MODES.items():
            for extra in (dict(), dict(min_member_probability=0.001), dict(weights=weights) if strategy == "additive" else dict(k=V)):
                k = extra.get("k", K)
                got = model.recommend_joint_tensor(batch, parties, **{"k": K, **kw, **extra}, strategy=strategy, return_members=True)
                least = F32(np.log(extra["min_member_probability"])) if "min_member_probability" in extra else F32(NINF)
                want = jr.rank_joint(logp, ok, parties, mode, k, None, extra.get("weights"), least)
                outs = dict(ids=got[0].cpu().numpy(), scores=got[1].cpu().numpy(), n=got[2].cpu().numpy(), util=got[3].cpu().numpy())
                assert_equals_ref(outs, want, f"{hidden} {kw.keys()} {strategy} {extra.keys()}")
                assert want[2][1] == 0 and (want[2][0] > 0 or "min_member_probability" in extra)
                three = model.recommend_joint_tensor(batch, parties, **{"k": K, **kw, **extra}, strategy=strategy)
                assert len(three) == 3 and all(torch.equal(a, b) for a, b in zip(three, got[:3]))
    lists = model.recommend_joint(batch, parties, k=K, return_members=True)
    got = model.recommend_joint_tensor(batch, parties, k=K, return_members=True)
    assert len(lists) == len(parties) and lists[0] == tuple(x[0].cpu().tolist() for x in got)
    none = model.recommend_joint_tensor(batch, parties, k=0)                 # k = 0: the counts alone
    assert none[0].shape == (len(parties), 0) and none[1].shape == (len(parties), 0) and torch.equal(none[2], got[2])


def test_a_party_of_one_equals_recommend_tensor():
    dl, model, V, histories, _, _ = setting(64)
    batch = prepared(dl, histories[:N_MEMBERS])
    parties = torch.arange(N_MEMBERS)[:, None]
    ids0, scores0, slots, dist = model.recommend_tensor(batch, k=10, return_distribution=True)
    assert slots.numel() == N_MEMBERS
    for strategy in jr.MODES:
        ids, scores, n, logp = model.recommend_joint_tensor(batch, parties, k=10, strategy=strategy, return_members=True)
        assert torch.equal(ids, ids0) and torch.equal(scores.view(torch.int32), dist["logp"].view(torch.int32))
        assert torch.equal(logp[:, :, 0].contiguous().view(torch.int32), dist["logp"].view(torch.int32)) and torch.equal(n, dist["n"])
        raw = model.recommend_joint_tensor(batch, parties, k=10, strategy=strategy, calibrated=False)
        assert torch.equal(raw[0], ids0) and torch.equal(raw[1].view(torch.int32), scores0.view(torch.int32))


# ---- the app ----------------------------------------------------------------------------------------------------------------------------
def test_recommend_together_returns_the_model_calls_items_and_recommend_batchs_probabilities():
    dl, model, V, histories, asked, _ = setting(64)
    rec = Recommender(model, dl)
    tok = dl.get_tokenizer()
    groups = [histories[0:3], histories[3:4], histories[4:9], histories[9:11]]
    members = [h for g in groups for h in g]
    rows = torch.full((4, 5), -1, dtype=torch.int64)
    at = 0
    for p, g in enumerate(groups):
        rows[p, :len(g)] = torch.arange(at, at + len(g))
        at += len(g)
    batch = prepared(dl, members)
    exclude = rec._requests(members)[1]
    served = rec.recommend_batch(members, k=min(V, 1024), return_probabilities=True)
    for kw in (dict(), dict(strategy="least_misery", min_member_probability=0.001), dict(weights=[[1, 2, 0.5], [1], [1, 1, 1, 1, 3], [2, 1]])):
        got = rec.recommend_together(groups, k=8, **kw, return_members=True)
        model_kw = {**kw, "weights": None if "weights" not in kw else torch.as_tensor([w + [0] * (5 - len(w)) for w in kw["weights"]])}
        ids, scores, n = model.recommend_joint_tensor(batch, rows, k=8, exclude_seen=False, exclude=exclude, **model_kw)
        assert len(got) == 4
        at = 0
        for p, g in enumerate(groups):
            keep = [i for i in ids[p].cpu().tolist() if i >= 0]
            assert [item for item, _, _ in got[p]] == tok.detokenize(keep) and len(keep) == min(8, int(n[p]))
            assert [s for _, s, _ in got[p]] == scores[p, :len(keep)].to(torch.float64).cpu().tolist()
            for item, _, probs in got[p]:
                assert len(probs) == len(g) and not any(item in h for h in g)
                assert probs == [dict(served[at + m])[item] for m in range(len(g))], (p, item)
            at += len(g)
        pairs = rec.recommend_together(groups, k=8, **kw)
        assert pairs == [[(item, s) for item, s, _ in row] for row in got]
    only = rec.recommend_together(groups, k=8, allowed_items=asked)
    assert all(item in asked for row in only for item, _ in row) and any(only)
