"""The stock-aware allocation on the GPU: b4r_allocate bit for bit against the greedy walk of tests/allocate_ref.py (the device
computes it by deferred acceptance in rounds: another procedure), the round budget and resume, graph capture, and allocate_tensor /
Recommender.allocate / SessionStore.allocate against the host composition of calls that existed before."""
import functools

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib
from bert4rec_amd import engine as engine_mod
from bert4rec_amd.engine import Engine, make_model_config
from tests import allocate_ref as ar
from tests.b4r_testlib import P, stream
from tests.test_gpu_session_store import fill, same_bits, setting

pytestmark = pytest.mark.gpu

DEV = "cuda"
FILL = -7                                    # what every output holds before a call: a cell nobody writes keeps it
NAMES = ("ids", "util", "pos", "row_n", "remaining")
DTYPES = dict(ids=torch.int64, util=torch.float32, pos=torch.int32, row_n=torch.int32, remaining=torch.int32, unsettled=torch.int32)


def dev(a):
    if a is None or torch.is_tensor(a):
        return a
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def engine_of(V):
    return Engine(make_model_config(V, 64, 2, 2, 32, 256, 0.0, 0.0), DEV)


def assert_same(got, want, what):
    for name in NAMES:
        g = got[name].cpu().numpy() if torch.is_tensor(got[name]) else got[name]
        assert g.dtype == want[name].dtype and g.shape == want[name].shape and g.tobytes() == want[name].tobytes(), (what, name)


def engine_allocate(c, ids, util, cap, uid, **kw):
    out = engine_of(c["V"]).allocate(dev(ids), dev(util), c["K"], dev(cap), dev(uid), **kw)
    return dict(zip(NAMES + ("unsettled",), out))


class Raw:
    """b4r_allocate itself on guarded outputs: one guard row (or word) on either side of every output"""

    def __init__(self, ids, util, K, cap, uid, null=()):
        self.R, self.M = ids.shape
        self.K, self.V = K, cap.shape[0]
        self.ids, self.util, self.cap, self.uid = dev(ids), dev(util), dev(cap), dev(uid)
        R, V = self.R, self.V
        shapes = dict(ids=(R + 2, K), util=(R + 2, K), pos=(R + 2, K), row_n=(R + 2,), remaining=(V + 2,), unsettled=(3,))
        self.out = {k: torch.full(s, FILL, dtype=DTYPES[k], device=DEV) for k, s in shapes.items()}
        self.null = set(null)
        nbytes = _lib.load().b4r_allocate_scratch_bytes(R, self.M, K, V)
        self.scratch = torch.empty(nbytes + 16, dtype=torch.uint8, device=DEV)
        self.scratch[nbytes:] = 0x5A
        self.nbytes = nbytes

    def call(self, rounds, resume):
        ptr = {k: None if k in self.null else P(v[1:]) for k, v in self.out.items()}
        rc = _lib.load().b4r_allocate(P(self.ids), P(self.util), self.R, self.M, self.K, self.V, P(self.cap), P(self.uid), rounds, resume,
                                      ptr["ids"], ptr["util"], ptr["pos"], ptr["row_n"], ptr["remaining"], ptr["unsettled"], P(self.scratch),
                                      self.nbytes, stream())
        assert rc == 0, _lib.last_error()

    def read(self):
        """the outputs on the host, the guards checked; a NULL output must still be all FILL"""
        torch.cuda.synchronize()
        assert (self.scratch[self.nbytes:] == 0x5A).all(), "the scratch was overrun"
        got = {}
        for k, v in self.out.items():
            h = v.cpu().numpy()
            if k in self.null:
                assert (h == FILL).all(), k
                continue
            assert (h[0] == FILL).all() and (h[-1] == FILL).all(), k
            got[k] = h[1:-1]
        return got

    def settle(self, chunk=32, first=True):
        rounds = 0
        while True:
            self.call(chunk, 0 if first and rounds == 0 else 1)
            rounds += chunk
            got = self.read()
            if int(got["unsettled"][0]) == 0:
                return got, rounds
            assert int(got["unsettled"][0]) > 0 and rounds <= self.R * self.M + 1 + chunk


# ---- the grid -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,M", ar.shapes())
def test_allocate_equals_the_restatement(R, M):
    for c in ar.cases_of(R, M):
        ids, util, cap, uid = ar.build_case(c)
        want = ar.greedy(ids, util, c["K"], cap, uid)
        got = engine_allocate(c, ids, util, cap, uid)                      # the default: max_rounds=None
        assert_same(got, want, c)
        assert int(got["unsettled"].item()) == 0


@pytest.mark.parametrize("c", ar.TILE_CASES + [ar.cases_of(65, 65)[-1], ar.cases_of(5, 1024)[-1], ar.cases_of(257, 63)[2]],
                         ids=lambda c: f"R{c['R']}-M{c['M']}-K{c['K']}-V{c['V']}")
def test_the_tile_edges_the_memory_around_the_outputs_and_null_outputs(c):
    ids, util, cap, uid = ar.build_case(c)
    want = ar.greedy(ids, util, c["K"], cap, uid)
    got, rounds = Raw(ids, util, c["K"], cap, uid).settle()
    assert_same(got, want, c)
    assert_same(engine_allocate(c, ids, util, cap, uid), want, c)
    assert rounds <= 256
    for null in (("ids", "util", "pos"), ("row_n", "remaining"), ("unsettled",), NAMES + ("unsettled",)):
        raw = Raw(ids, util, c["K"], cap, uid, null=null)
        raw.call(256, 0)                                                # settled above within that budget: the rest return at once
        part = raw.read()
        assert set(part) == set(NAMES + ("unsettled",)) - set(null)
        assert_same({**want, **part}, want, (c, null))
        assert "unsettled" in null or int(part["unsettled"][0]) == 0


def test_empty_calls_write_the_stock_and_nothing_else():
    ids, util = ar.make_pool(5, 7, 33, seed=1)
    cap = ar.make_capacity(33, 5, "negative")
    for R, K in ((0, 3), (5, 0)):
        raw = Raw(ids[:R], util[:R], K, cap, None)
        raw.call(3, 0)
        got = raw.read()
        assert np.array_equal(got["remaining"], cap) and (got["row_n"] == FILL).all() and (got["unsettled"] == FILL).all()
    c = dict(V=33, K=0)
    got = engine_allocate(c, ids, util, cap, None)
    assert got["ids"].shape == (5, 0) and got["row_n"].tolist() == [0] * 5 and got["remaining"].cpu().numpy().tobytes() == cap.tobytes()
    assert int(got["unsettled"].item()) == 0
    in_place = dev(cap)                                                # remaining may be the capacity buffer itself
    raw = Raw(ids, util, 0, cap, None)
    assert _lib.load().b4r_allocate(P(raw.ids), P(raw.util), 5, 7, 0, 33, P(in_place), None, 1, 0, None, None, None, None, P(in_place), None, None,
                                    0, stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(in_place.cpu().numpy(), cap)


def test_a_refused_call_leaves_the_outputs_untouched():
    ids, util = ar.make_pool(5, 7, 33, seed=1)
    raw = Raw(ids, util, 3, ar.make_capacity(33, 5, "ones"), None)
    lib = _lib.load()
    o = {k: P(v[1:]) for k, v in raw.out.items()}
    tail = (o["ids"], o["util"], o["pos"], o["row_n"], o["remaining"], o["unsettled"], P(raw.scratch))
    assert lib.b4r_allocate(P(raw.ids), P(raw.util), 5, 7, 3, 33, P(raw.cap), None, 4, 0, *tail, raw.nbytes - 4, stream()) == -5
    assert lib.b4r_allocate(P(raw.ids), P(raw.util), 5, 7, 8, 33, P(raw.cap), None, 4, 0, *tail, raw.nbytes, stream()) == -2
    assert lib.b4r_allocate(P(raw.ids), P(raw.util), 5, 7, 3, 33, P(raw.cap), None, 0, 0, *tail, raw.nbytes, stream()) == -1
    torch.cuda.synchronize()
    assert all((v == FILL).all() for v in raw.out.values())


def test_a_resumed_call_on_a_scratch_of_another_shape_changes_nothing():
    ids, util = ar.make_pool(5, 7, 33, seed=1)
    cap = ar.make_capacity(33, 5, "ones")
    raw = Raw(ids, util, 3, cap, None)
    raw.scratch[:raw.nbytes] = 0
    raw.call(2, 1)                                                     # resume without a state: all zeros is no state of this shape
    got = raw.read()
    assert int(got["unsettled"][0]) == -1 and all((got[k] == FILL).all() for k in NAMES)
    got, _ = raw.settle()                                              # the same scratch, initialised now
    assert_same(got, ar.greedy(ids, util, 3, cap), "after init")


# ---- properties ---------------------------------------------------------------------------------------------------------------------
def test_the_chain_needs_one_round_per_row_and_every_budget_ends_in_the_same_bits():
    n = 40
    ids, util, cap = ar.chain_fixture(n)
    want = ar.greedy(ids, util, 1, cap)
    assert want["row_n"].tolist() == [1] * n                            # every row ends up holding an item

    one = Raw(ids, util, 1, cap, None)                                  # rounds = 1, resumed
    rounds = 0
    while True:
        one.call(1, 0 if rounds == 0 else 1)
        rounds += 1
        got = one.read()
        assert ar.feasible(got, ids, util, 1, cap), rounds
        if int(got["unsettled"][0]) == 0:
            break
        assert int(got["unsettled"][0]) == 1 and rounds < n + 2          # each round displaces exactly one further row
        assert int(got["row_n"].sum()) == n - 1                          # ... which holds nothing until it proposes again
    assert rounds == n                                                  # n - 1 displacements, and the round that rejects nothing
    final = got
    assert_same(final, want, "rounds of 1")

    seven = Raw(ids, util, 1, cap, None)                                # chunks of 7
    calls = 0
    while True:
        seven.call(7, 0 if calls == 0 else 1)
        calls += 1
        got = seven.read()
        assert ar.feasible(got, ids, util, 1, cap), calls
        if int(got["unsettled"][0]) == 0:
            break
        assert calls < 7
    assert calls == 6                                                   # 5 * 7 = 35 < 40 <= 42
    big = Raw(ids, util, 1, cap, None)                                  # one call with a large budget: the rounds past the end do nothing
    big.call(500, 0)
    for other in (got, big.read()):
        for k in NAMES + ("unsettled",):
            assert other[k].tobytes() == final[k].tobytes(), k
    small = Raw(ids, util, 1, cap, None)                                # a single-digit budget cannot settle it
    small.call(9, 0)
    part = small.read()
    assert int(part["unsettled"][0]) == 1 and ar.feasible(part, ids, util, 1, cap) and part["ids"].tobytes() != final["ids"].tobytes()
    got = engine_allocate(dict(V=cap.shape[0], K=1), ids, util, cap, None, chunk=3)
    assert_same(got, want, "chunks of 3 through the engine")


@pytest.mark.parametrize("c", [ar.cases_of(65, 64)[3], ar.cases_of(64, 65)[4], ar.TILE_CASES[1]], ids=lambda c: f"R{c['R']}-M{c['M']}-K{c['K']}")
def test_the_lists_follow_the_users_not_the_rows(c):
    ids, util, cap, _ = ar.build_case(c)
    R = c["R"]
    uid = ar.make_user_ids(R, "shuffled", seed=5)
    a = engine_allocate(c, ids, util, cap, uid)
    perm = np.random.default_rng(R).permutation(R)
    b = engine_allocate(c, ids[perm], util[perm], cap, uid[perm])
    perm_d = dev(perm)
    for name in ("ids", "util", "pos", "row_n"):
        assert same_bits(a[name][perm_d], b[name]), name
    assert torch.equal(a["remaining"], b["remaining"])
    assert_same(a, ar.greedy(ids, util, c["K"], cap, uid), c)


def test_two_runs_and_a_captured_graph_give_the_same_bits():
    c = dict(R=257, M=65, K=10, V=33, pool="skewed", cap="ones", uid="repeats", seed=11)
    ids, util, cap, uid = ar.build_case(c)
    want = ar.greedy(ids, util, c["K"], cap, uid)
    eng = engine_of(c["V"])
    ids_d, util_d, cap_d, uid_d = dev(ids), dev(util), dev(cap), dev(uid)
    runs = [eng.allocate(ids_d, util_d, c["K"], cap_d, uid_d, max_rounds=48) for _ in range(2)]
    torch.cuda.synchronize()
    for x, y in zip(*runs):
        assert same_bits(x, y)
    settled = int(runs[0][5].item()) == 0
    if settled:
        assert_same(dict(zip(NAMES, runs[0])), want, "48 rounds")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        pool_i, pool_u = torch.zeros_like(ids_d), torch.zeros_like(util_d)      # the capture's own inputs, filled before every replay
        eng.allocate(pool_i, pool_u, c["K"], cap_d, uid_d, max_rounds=48)       # allocates the scratch outside the capture
        torch.cuda.synchronize()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            out = eng.allocate(pool_i, pool_u, c["K"], cap_d, uid_d, max_rounds=48)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(2):
        pool_i.copy_(ids_d), pool_u.copy_(util_d)
        for t in out:
            t.fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(out, runs[0]):
            assert same_bits(x, y)


def test_remaining_fed_back_serves_the_next_batch_from_what_is_left():
    V, K = 33, 3
    cap = ar.make_capacity(V, 64, "mixed", seed=3)
    first, second = ar.make_pool(64, 65, V, seed=21), ar.make_pool(65, 64, V, seed=22)
    want1 = ar.greedy(*first, K, cap)
    want2 = ar.greedy(*second, K, want1["remaining"])
    c = dict(V=V, K=K)
    got1 = engine_allocate(c, *first, cap, None)
    got2 = engine_of(V).allocate(dev(second[0]), dev(second[1]), K, got1["remaining"], None)      # the device tensor, as it is
    assert_same(got1, want1, "first batch")
    assert_same(dict(zip(NAMES, got2)), want2, "second batch")
    # first come, first served: the one unit of item 3 stays with the early user, however much the late one wants it
    early, late = (np.array([[3, -1]], np.int64), np.array([[1.0, -np.inf]], np.float32)), (np.array([[3, 4]], np.int64), np.array([[5.0, 0.5]], np.float32))
    ones = np.ones(V, np.int32)
    a = engine_allocate(dict(V=V, K=1), *early, ones, None)
    b = engine_allocate(dict(V=V, K=1), *late, a["remaining"], None)
    joint = engine_allocate(dict(V=V, K=1), np.concatenate([early[0], late[0]]), np.concatenate([early[1], late[1]]), ones, None)
    assert a["ids"].tolist() == [[3]] and b["ids"].tolist() == [[4]] and joint["ids"].tolist() == [[-1], [3]]


# ---- the model and the apps ---------------------------------------------------------------------------------------------------------
def scarce_capacity(vocab, pool_ids, units=1):
    """the items the users want most are scarce: `units` of every item that heads somebody's pool, plenty of everything else"""
    cap = np.full(vocab, engine_mod.ALLOCATE_UNLIMITED, np.int32)
    cap[np.unique(pool_ids[:, :3][pool_ids[:, :3] >= 0])] = units
    return cap


def with_twins(histories):
    """five of the users come twice: twins hold the same pool, so whatever is scarce at the head of it is contended for certain"""
    return list(histories) + list(histories[:5])


@pytest.mark.parametrize("with_allow", (False, True))
@pytest.mark.parametrize("hidden", (64, 128))
def test_allocate_tensor_equals_the_host_composition(hidden, with_allow):
    rec, vocab, histories, keys = setting(hidden)
    histories = with_twins(histories)
    batch, exclude = rec._requests(histories)
    allow = None
    if with_allow:
        allow = torch.zeros(vocab, dtype=torch.bool)
        allow[3::2] = True
    k, pool = 4, 50
    kw = dict(exclude_seen=False, exclude=exclude, allow=allow)
    p_ids, p_scores, slots, dist = rec.model.recommend_tensor(batch, k=pool, return_distribution=True, **kw)
    p_ids_h, logp_h, scores_h = p_ids.cpu().numpy(), dist["logp"].cpu().numpy(), p_scores.cpu().numpy()
    cap = scarce_capacity(vocab, p_ids_h)
    uid = np.arange(len(histories), dtype=np.int64)[::-1].copy()
    for calibrated, util_h in ((True, logp_h), (False, scores_h)):
        want = ar.greedy(p_ids_h, util_h, k, cap, uid)
        assert (want["pos"][:, :k].max(axis=1) >= k).any(), "the stock binds: somebody is served from deeper in their pool"
        ids, util, slot_index, info = rec.model.allocate_tensor(batch, cap, k=k, pool=pool, calibrated=calibrated, user_ids=uid, **kw)
        assert torch.equal(slot_index, slots) and int(info["unsettled"].item()) == 0
        assert_same(dict(ids=ids, util=util, pos=info["pos"], row_n=info["row_n"], remaining=info["remaining"]), want, (hidden, calibrated))


def test_without_a_binding_capacity_allocate_tensor_is_recommend_tensor():
    rec, vocab, histories, keys = setting(64)
    batch, exclude = rec._requests(histories)
    plenty = np.full(vocab, len(histories), np.int32)
    ids, util, slots, info = rec.model.allocate_tensor(batch, plenty, k=10, exclude_seen=False, exclude=exclude)
    want = rec.model.recommend_tensor(batch, k=10, exclude_seen=False, exclude=exclude)
    assert torch.equal(ids, want[0]) and torch.equal(slots, want[2])
    assert torch.equal(info["pos"], torch.arange(10, dtype=torch.int32, device=DEV).expand(len(histories), 10))


def test_the_recommender_never_hands_out_more_than_the_stock():
    rec, vocab, histories, keys = setting(64)
    histories = with_twins(histories)
    k, pool = 5, 50
    plain =rec.recommend_batch(histories, k=pool, return_probabilities=True)
    prob = [dict(row) for row in plain]                                 # (user, item) -> probability, for every item of the user's pool
    heads = sorted({item for row in plain for item, _ in row[:2]})
    stock = {item: 1 + (i % 2) for i, item in enumerate(heads)}
    stock["an item nobody knows"] = 3
    lists, left = rec.allocate(histories, stock, k=k, candidate_pool=pool)
    assert len(lists) == len(histories) and all(len(row) == k for row in lists) and set(left) == set(heads)
    given = {}
    for u, row in enumerate(lists):
        order = [item for item, _ in plain[u]]
        assert [order.index(item) for item, _ in row] == sorted(order.index(item) for item, _ in row)     # the user's own order
        for item, p in row:
            given[item] = given.get(item, 0) + 1
            assert p == prob[u][item], (u, item)                        # recommend_batch's probability of the same (user, item)
    assert all(given.get(item, 0) + left[item] == units for item, units in stock.items() if item in left)
    assert all(0 <= left[item] for item in left) and any(left[item] == 0 for item in left)
    assert lists != [row[:k] for row in plain]                          # the stock changed somebody's list
    items_only, left2 = rec.allocate(histories, stock, k=k, candidate_pool=pool, return_probabilities=False)
    assert items_only == [[item for item, _ in row] for row in lists] and left2 == left
    assert rec.allocate([], stock) == ([], {item: stock[item] for item in heads})
    nothing_limited, _ = rec.allocate(histories, {}, k=k, candidate_pool=pool)
    assert nothing_limited == [row[:k] for row in plain]


def test_the_session_store_allocates_what_the_recommender_allocates():
    rec, vocab, histories, keys = setting(64)
    store = rec.open_sessions(16)
    fill(store, histories, keys)
    plain = rec.recommend_batch(histories, k=3)
    stock = {item: 1 for row in plain for item in row}
    uid = list(range(100, 100 + len(keys)))[::-1]
    for kw in (dict(), dict(user_ids=uid), dict(allowed_items=sorted(set(rec.dataloader.create_item_list()))[::2], candidate_pool=60)):
        got = store.allocate(keys, stock, k=4, **kw)
        want = rec.allocate(histories, stock, k=4, **kw)
        assert got == want and len(got[0]) == len(keys), kw
    assert store.allocate([], stock) == rec.allocate([], stock)
