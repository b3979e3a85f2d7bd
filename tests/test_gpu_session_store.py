"""The session store on the GPU: b4r_history_append and b4r_history_batch bit for bit against tests/session_store_ref.py, graph capture,
and SessionStore against Recommender.recommend_batch / recommend_tensor on the same users."""
import functools

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, config, models
from bert4rec_amd.apps import Recommender
from bert4rec_amd.models.components import networks
from tests import session_store_ref as ssr
from tests.b4r_testlib import P, stream
from tests.test_gpu_api import make_loader, make_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
FIRST, MASK, V = 3, 1, 50
FILL = -7                                    # what every buffer holds before a call: a cell nobody writes keeps it


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class DeviceStore:
    """hist / count on the device (hist pre-filled with FILL, with one guard row on either side) and the C calls on them"""

    def __init__(self, U, C):
        self.U, self.C = U, C
        self.hist_all = torch.full((U + 2, C), FILL, dtype=torch.int64, device=DEV)
        self.count_all = torch.full((U + 2,), FILL, dtype=torch.int64, device=DEV)
        self.hist, self.count = self.hist_all[1:U + 1], self.count_all[1:U + 1]
        self.count.zero_()
        self.scratch = torch.empty(16 * 65536, dtype=torch.uint8, device=DEV)

    def append(self, users, items, want_accepted=True):
        N = len(users)
        u, it = dev(np.asarray(users, np.int32)), dev(np.asarray(items, np.int64))
        acc = torch.full((N + 2,), FILL, dtype=torch.int32, device=DEV)
        rc = _lib.load().b4r_history_append(P(self.hist), P(self.count), self.U, self.C, V, FIRST, P(u), P(it), N,
                                            P(acc[1:]) if want_accepted else None, P(self.scratch), 16 * N, stream())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        acc = acc.cpu().numpy()
        assert acc[0] == FILL and acc[-1] == FILL
        return acc[1:N + 1]

    def load(self, ref):
        """the state of the restatement, written by the host"""
        hist = np.full((self.U, self.C), FILL, np.int64)
        for (u, c), item in ref.cells().items():
            hist[u, c] = item
        self.hist.copy_(dev(hist))
        self.count.copy_(dev(ref.count()))

    def assert_equals(self, ref):
        hist, count = self.hist_all.cpu().numpy(), self.count_all.cpu().numpy()
        assert np.array_equal(count[1:-1], ref.count()) and count[0] == FILL and count[-1] == FILL
        want = np.full((self.U + 2, self.C), FILL, np.int64)     # the cells the restatement defines, FILL everywhere else
        for (u, c), item in ref.cells().items():
            want[u + 1, c] = item
        assert hist.tobytes() == want.tobytes()


# ---- b4r_history_append -------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (5, 7), (300, 64), (40, 199), (3, 4096))
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000, 4097)


@pytest.mark.parametrize("U,C", SHAPES)
def test_append_equals_the_restatement(U, C):
    """every size and every pattern on ONE state, so that each call starts from the counts and rings the earlier ones left"""
    store, ref = DeviceStore(U, C), ssr.RefStore(U, C)
    for N in SIZES:
        for name, (users, items) in ssr.log_patterns(U, C, V, N, FIRST).items():
            got = store.append(users, items)
            want = ref.append(users, items, V, FIRST)
            assert got.dtype == want.dtype and np.array_equal(got, want), (N, name)
            store.assert_equals(ref)
    assert (ref.count() > 3 * C).any()                              # the ring wrapped, also several times inside one call
    store.append([0, 0], [FIRST, FIRST + 1], want_accepted=False)   # accepted_out is optional
    ref.append([0, 0], [FIRST, FIRST + 1], V, FIRST)
    store.assert_equals(ref)


def mixed_log(U, N, seed):
    rng = np.random.default_rng(seed)
    users = np.where(rng.random(N) < 0.3, 0, rng.integers(-1, U + 1, size=N)).astype(np.int32)      # user 0 is busy; -1 and U are dropped
    return users, rng.integers(0, V + 2, size=N).astype(np.int64)


@pytest.mark.parametrize("U,C", ((5, 7), (40, 199)))
def test_append_does_not_depend_on_how_the_log_is_cut(U, C):
    users, items = mixed_log(U, 1000, seed=U)
    ref = ssr.RefStore(U, C)
    ref.append(users, items, V, FIRST)
    whole = DeviceStore(U, C)
    whole.append(users, items)
    whole.assert_equals(ref)
    for step in (1, 7, 64, 257):
        cut = DeviceStore(U, C)
        lib, u, it = _lib.load(), dev(users), dev(items)
        for c in range(0, 1000, step):
            n = min(step, 1000 - c)
            assert lib.b4r_history_append(P(cut.hist), P(cut.count), U, C, V, FIRST, P(u[c:]), P(it[c:]), n, None, P(cut.scratch), 16 * n, stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(cut.hist_all, whole.hist_all) and torch.equal(cut.count_all, whole.count_all), step


def test_two_append_runs_give_the_same_bits():
    users, items = mixed_log(300, 4097, seed=9)
    a, b = DeviceStore(300, 64), DeviceStore(300, 64)
    acc_a, acc_b = a.append(users, items), b.append(users, items)
    assert acc_a.tobytes() == acc_b.tobytes() and torch.equal(a.hist_all, b.hist_all) and torch.equal(a.count_all, b.count_all)


# ---- b4r_history_batch --------------------------------------------------------------------------------------------------------------
def filled(U, C, counts):
    """a restatement and a device state whose user i holds counts[i] events (the other users none)"""
    ref = ssr.RefStore(U, C)
    rng = np.random.default_rng(C)
    for u, n in enumerate(counts):
        ref.append([u] * n, rng.integers(FIRST, V, size=n), V, FIRST)
    store = DeviceStore(U, C)
    store.load(ref)
    return ref, store


def run_batch(store, req, L, Pn, E, want_live=True, outs=None, req_d=None, sync=True):
    R = len(req)
    shapes = dict(tokens=(R, L), mask=(R, L), len=(R,), positions=(R, Pn), weights=(R, Pn), exclude=(R, E), live=(R,))
    if outs is None:      # one guard row on either side of every output
        outs = {k: torch.full((s[0] + 2,) + s[1:], FILL, dtype=torch.int32 if k in ("len", "live") else torch.int64, device=DEV)
                for k, s in shapes.items()}
    req_d = dev(np.asarray(req, np.int32)) if req_d is None else req_d
    ptr = {k: P(v[1:]) for k, v in outs.items()}
    rc = _lib.load().b4r_history_batch(P(store.hist), P(store.count), store.U, store.C, P(req_d), R, L, Pn, E, MASK, ptr["tokens"], ptr["mask"],
                                       ptr["len"], ptr["positions"], ptr["weights"], ptr["exclude"], ptr["live"] if want_live else None, stream())
    assert rc == 0, _lib.last_error()
    if sync:
        torch.cuda.synchronize()
    return outs


def assert_batch(outs, want, skip=()):
    for k in ssr.BATCH_OUTS:
        got = outs[k].cpu().numpy()
        assert (got[0] == FILL).all() and (got[-1] == FILL).all(), k      # the memory around the output
        if k in skip:
            assert (got == FILL).all(), k
        else:
            assert got.dtype == want[k].dtype and got[1:-1].tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("L", (2, 3, 33, 200, 256))
@pytest.mark.parametrize("C", (1, 7, 199, 4096))
def test_batch_equals_the_restatement(C, L):
    counts = sorted({max(0, n) for n in (0, 1, L - 2, L - 1, L, C - 1, C, C + 1, 3 * C + 2)})
    U = len(counts) + 2                                              # the last two users hold nothing
    ref, store = filled(U, C, counts)
    rng = np.random.default_rng(L)
    requests = {0: [], 1: [len(counts) - 1], 257: np.concatenate([np.arange(-2, U + 2), rng.integers(-2, U + 2, size=257 - U - 4)]).tolist()}
    for Pn in (1, 40):
        for E in (1, C, C + 3):
            for R, req in requests.items():
                assert len(req) == R
                assert_batch(run_batch(store, req, L, Pn, E), ref.batch(req, L, Pn, E, MASK))
    assert_batch(run_batch(store, requests[257], L, 1, C, want_live=False), ref.batch(requests[257], L, 1, C, MASK), skip=("live",))
    store.assert_equals(ref)                                         # the state is read only


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
def test_a_captured_append_and_batch_replay_with_new_events_and_requests():
    U, C, L, Pn, E, N, R = 40, 33, 24, 6, 36, 300, 50
    lib = _lib.load()
    logs = [mixed_log(U, N, seed=s) for s in (1, 2, 3)]
    reqs = [np.random.default_rng(s).integers(-1, U + 1, size=R).astype(np.int32) for s in (1, 2, 3)]
    eager, ref = DeviceStore(U, C), ssr.RefStore(U, C)
    want = []
    for (users, items), req in zip(logs, reqs):                      # eager: append, then batch, three times
        acc = eager.append(users, items)
        assert np.array_equal(acc, ref.append(users, items, V, FIRST))
        want.append(ref.batch(req, L, Pn, E, MASK))
        assert_batch(run_batch(eager, req, L, Pn, E), want[-1])
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        store = DeviceStore(U, C)                                    # allocations and copies outside the capture
        ev_u, ev_i = torch.zeros(N, dtype=torch.int32, device=DEV), torch.zeros(N, dtype=torch.int64, device=DEV)
        req_d = torch.zeros(R, dtype=torch.int32, device=DEV)
        acc = torch.full((N,), FILL, dtype=torch.int32, device=DEV)
        outs = run_batch(store, reqs[0], L, Pn, E, req_d=req_d)      # (user 0 has nothing yet: placeholders) allocates the outputs
        for v in outs.values():
            v.fill_(FILL)
        torch.cuda.synchronize()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):                   # one stream: a straight chain of three kernels
            assert lib.b4r_history_append(P(store.hist), P(store.count), U, C, V, FIRST, P(ev_u), P(ev_i), N, P(acc), P(store.scratch), 16 * N,
                                          stream()) == 0
            run_batch(store, reqs[0], L, Pn, E, outs=outs, req_d=req_d, sync=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert (outs["tokens"] == FILL).all() and (store.count == 0).all() and (acc == FILL).all(), "a capture must not run the kernels"
    for (users, items), req, w in zip(logs, reqs, want):
        ev_u.copy_(dev(users)), ev_i.copy_(dev(items)), req_d.copy_(dev(req))
        graph.replay()
        torch.cuda.synchronize()
        assert_batch(outs, w)
    assert torch.equal(store.hist_all, eager.hist_all) and torch.equal(store.count_all, eager.count_all)
    store.assert_equals(ref)


# ---- the model and the app ----------------------------------------------------------------------------------------------------------
L_MODEL, P_MODEL = 24, 6
HISTORY_LENGTHS = (3, 21, 22, 23, 30, 1, 24, 40, 0, 12)              # up to the window, past it (an item slides out), a cold user


def model_of(vocab, hidden):
    if hidden == 64:
        return make_model(vocab, L=L_MODEL, seed=11)
    cfgd = {**config.get_encoder_config(f"ml-1m_{hidden}"), "max_sequence_length": L_MODEL, "output_dropout": 0.0, "attention_dropout": 0.0}
    return models.BERT4RecModel(networks.Bert4RecEncoder(vocab, seed=11, **cfgd))


@functools.lru_cache(maxsize=None)
def setting(hidden):
    dl = make_loader()
    dl.generate_vocab()
    vocab = dl.get_tokenizer().get_vocab_size()
    rec = Recommender(model_of(vocab, hidden), dl)
    items = dl.create_item_list()
    histories = [items[43 * i:43 * i + n] for i, n in enumerate(HISTORY_LENGTHS)]
    keys = [f"user {i}" for i in range(len(histories))]
    return rec, vocab, histories, keys


def fill(store, histories, keys):
    """the users' events in round-robin order, as a log would bring them; a user without events is never named"""
    log = [(key, h[t]) for t in range(max(len(h) for h in histories)) for key, h in zip(keys, histories) if t < len(h)]
    half = len(log) // 2
    n = store.append([k for k, _ in log[:half]], [i for _, i in log[:half]])
    store.append([k for k, _ in log[half:]], [i for _, i in log[half:]], return_accepted=False)
    assert n == half


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("hidden", (64, 128))
def test_requests_from_the_store_recommend_what_the_full_sequences_recommend(hidden):
    rec, vocab, histories, keys = setting(hidden)
    store = rec.open_sessions(16)
    assert store.history_capacity == 256 and len(store) == 0
    fill(store, histories, keys)
    assert len(store) == len(keys) - 1 and store.history(keys[4]) == list(histories[4]) and store.history(keys[8]) == []
    batch, exclude = store.requests(keys)
    host_batch, host_exclude = rec._requests(histories)
    assert set(batch) == {"input_word_ids", "input_mask", "masked_lm_positions", "masked_lm_weights", "masked_lm_ids"}
    assert set(host_batch) - set(batch) == {"labels"}                 # the unmasked row, which no inference call reads
    for key in batch:
        assert batch[key].is_cuda and same_bits(batch[key].cpu(), host_batch[key]), key
    E = host_exclude.shape[1]
    assert same_bits(exclude[:, :E].cpu(), host_exclude) and (exclude[:, E:] == -1).all()
    got = rec.model.recommend_tensor(batch, k=10, exclude_seen=False, exclude=exclude)
    want = rec.model.recommend_tensor(host_batch, k=10, exclude_seen=False, exclude=host_exclude)
    for g, w in zip(got, want):
        assert same_bits(g, w)
    # a history that slid past the window: the item that left it is still excluded
    tokens = rec._known_tokens(histories[7])
    left = [t for t in tokens[:-(L_MODEL - 1)] if t not in tokens[-(L_MODEL - 1):]]
    assert left and not set(left) & set(batch["input_word_ids"][7].tolist()) and set(left) <= set(exclude[7].tolist())


@pytest.mark.parametrize("hidden", (64, 128))
def test_recommend_equals_recommend_batch(hidden):
    rec, vocab, histories, keys = setting(hidden)
    store = rec.open_sessions(len(keys))
    fill(store, histories, keys)
    catalogue = rec.dataloader.create_item_list()
    for kw in (dict(), dict(allowed_items=sorted(set(catalogue))[::3]), dict(diversity=0.4),
               dict(sample_seed=11, user_streams=list(range(100, 100 + len(keys))))):
        got = store.recommend(keys, k=10, return_probabilities=True, **kw)
        want = rec.recommend_batch(histories, k=10, return_probabilities=True, **kw)
        assert got == want and len(got) == len(keys) and all(len(row) == 10 for row in got), kw
    assert store.recommend(keys[:3], k=1) == rec.recommend_batch(histories[:3], k=1)
    assert store.recommend([], k=3) == []


def test_a_history_longer_than_the_capacity_excludes_its_last_items_only():
    rec, vocab, histories, keys = setting(64)
    C = L_MODEL - 1
    store = rec.open_sessions(4, history_capacity=C)
    long = list(dict.fromkeys(rec.dataloader.create_item_list()))[:60]        # 60 distinct items
    fill(store, [long], ["long"])
    assert store.history("long") == long[-C:]
    batch, exclude = store.requests(["long"])
    host_batch, full = rec._requests([long])
    assert exclude.shape == (1, C) and same_bits(exclude.cpu(), full[:, -C:].contiguous())
    k = vocab - 3
    got = rec.model.recommend_tensor(batch, k=k, exclude_seen=False, exclude=exclude)
    want = rec.model.recommend_tensor(host_batch, k=k, exclude_seen=False, exclude=full[:, -C:].contiguous())
    assert all(same_bits(g, w) for g, w in zip(got, want))
    everything = store.recommend(["long"], k=k)[0]
    batch_everything = rec.recommend_batch([long], k=k)[0]
    assert long[0] in everything and long[0] not in batch_everything          # older than the last C events: allowed again
    assert not set(long[-C:]) & set(everything) and not set(long) & set(batch_everything)


def test_forget_and_state_dict():
    rec, vocab, histories, keys = setting(64)
    store = rec.open_sessions(16)
    fill(store, histories, keys)
    before = store.requests(keys)
    saved = store.state_dict()
    assert all(not v.is_cuda for v in saved.values() if torch.is_tensor(v))
    store.forget(keys[:2])
    assert len(store) == len(keys) - 3 and keys[0] not in store._rows
    batch, exclude = store.requests(keys[:2] + ["never seen"])
    cold = torch.zeros(L_MODEL, dtype=torch.int64)
    cold[0] = MASK
    for r in range(3):
        assert torch.equal(batch["input_word_ids"][r].cpu(), cold) and int(batch["input_mask"][r].sum()) == 1 and (exclude[r] == -1).all()
    store.append([keys[0]], histories[0][:1])                       # the freed row starts again from nothing
    assert store.history(keys[0]) == list(histories[0][:1])
    again = rec.open_sessions(32)
    again.load_state_dict(saved)
    after = again.requests(keys)
    assert len(again) == len(keys) - 1
    for key in before[0]:
        assert same_bits(before[0][key], after[0][key]), key
    assert same_bits(before[1], after[1])
    assert again.history(keys[4]) == list(histories[4])
