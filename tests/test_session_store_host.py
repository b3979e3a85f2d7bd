"""The session store without a GPU: the plain-Python restatement (tests/session_store_ref.py) against the real preprocessor, its
independence of how a log is cut into calls, every Python-level argument error, and the C entry points' argument errors that return
before any launch."""
import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, dataloaders, datasets
from bert4rec_amd import engine as engine_mod
from bert4rec_amd.apps import Recommender, SessionStore
from bert4rec_amd.apps.session_store import check_session_args
from tests import session_store_ref as ssr

L, P, C = 24, 6, 30
FIRST, MASK = 3, 1
OK, BADARG, SHAPE, NOMEM = 0, -1, -2, -5


class StubEngine:
    """holds the state on the host: enough for the checks that come before any device call"""
    device = torch.device("cpu")

    def history_state(self, max_users, capacity):
        U, Cn = engine_mod.check_history_state_args(max_users, capacity)
        return {"hist": torch.zeros((U, Cn), dtype=torch.int64), "count": torch.zeros((U,), dtype=torch.int64)}

    def history_append(self, state, users, items, accepted=None, first_item=FIRST):
        engine_mod.check_history_state(state)


class StubModel:
    def __init__(self, V):
        self.vocab_size = V
        self.engine = StubEngine()


@pytest.fixture(scope="module")
def setting():
    ds = datasets.synthetic_dataset(n_users=120, n_items=300, min_len=4, max_len=40, seed=1)
    dl = dataloaders.get_dataloader_factory("bert4rec").create_ml_1m_dataloader(data_source=ds, max_seq_len=L, max_predictions_per_seq=P)
    dl.generate_vocab()
    V = dl.get_tokenizer().get_vocab_size()
    return dl, V, Recommender(StubModel(V), dl), dl.create_item_list()


# ---- the restatement against the real preprocessor ----------------------------------------------------------------------------------
LENGTHS = (0, 1, L - 2, L - 1, L, C, C + 7)


def test_the_restated_batch_is_prepare_inference_and_requests(setting):
    dl, V, rec, items = setting
    histories = [items[41 * i:41 * i + n] for i, n in enumerate(LENGTHS)]
    batch, exclude = rec._requests(histories)
    ref = ssr.RefStore(len(histories), C)
    tok = dl.get_tokenizer()
    for u, h in enumerate(histories):
        got = ref.append([u] * len(h), tok.tokenize(list(h)), V, FIRST)
        assert got.sum() == len(h)                                   # known items only
    out = ref.batch(list(range(len(histories))), L, P, C, MASK)
    for key, name in (("input_word_ids", "tokens"), ("input_mask", "mask"), ("masked_lm_positions", "positions"), ("masked_lm_weights", "weights")):
        assert np.array_equal(batch[key].numpy(), out[name]), key
    assert np.array_equal(out["len"], batch["input_mask"].numpy().sum(axis=1))
    assert out["live"].tolist() == [1] * len(histories)
    full = exclude.numpy()
    for u, n in enumerate(LENGTHS):
        held = min(n, C)
        assert out["exclude"][u, :held].tolist() == full[u, n - held:n].tolist()      # the stated difference: cut at the last C items
        assert (out["exclude"][u, held:] == -1).all() and (full[u, n:] == -1).all()
    assert LENGTHS[-1] > C and out["exclude"][-1, 0] != full[-1, 0]
    # the other stated difference: a user the store does not hold is a cold user, the row of an empty history
    cold = ref.batch([-1, len(histories), 0], L, P, C, MASK)
    for name in ("tokens", "mask", "len", "positions", "weights", "exclude"):
        assert np.array_equal(cold[name][0], out[name][0]) and np.array_equal(cold[name][1], out[name][0]), name
    assert cold["live"].tolist() == [0, 0, 1]


def test_the_restatement_does_not_depend_on_how_the_log_is_cut():
    U, Cn, V, N = 40, 9, 50, 1000
    rng = np.random.default_rng(5)
    users = rng.integers(-1, U + 1, size=N)
    items = rng.integers(0, V + 2, size=N)
    whole = ssr.RefStore(U, Cn)
    acc = whole.append(users, items, V, FIRST)
    assert 0 < acc.sum() < N
    for step in (1, 7, 64, 257):
        cut = ssr.RefStore(U, Cn)
        got = np.concatenate([cut.append(users[c:c + step], items[c:c + step], V, FIRST) for c in range(0, N, step)])
        assert cut.lists == whole.lists and np.array_equal(got, acc), step
        assert cut.cells() == whole.cells()


# ---- Python-level argument errors ---------------------------------------------------------------------------------------------------
def test_capacity_below_the_window_and_bad_sizes_are_refused(setting):
    _, _, rec, _ = setting
    with pytest.raises(ValueError, match="history_capacity = 22 is below max_seq_len - 1 = 23"):
        rec.open_sessions(10, history_capacity=L - 2)
    assert check_session_args(10, None, L) == (10, 256) and check_session_args(10, None, 400) == (10, 399)
    assert rec.open_sessions(10, history_capacity=L - 1).history_capacity == L - 1
    for bad in (dict(max_users=0), dict(max_users=2.5), dict(max_users=True), dict(history_capacity=4097), dict(max_users=1 << 40)):
        with pytest.raises(ValueError):
            check_session_args(**{"max_users": 10, "history_capacity": None, "max_seq_len": L, **bad})


def test_a_full_store_raises_and_applies_nothing(setting):
    _, _, rec, items = setting
    store = rec.open_sessions(3)
    assert isinstance(store, SessionStore) and len(store) == 0
    store._assign_rows(["a", "b"])
    with pytest.raises(ValueError, match="the session store is full: 2 new users, room for 1 of 3"):
        store.append(["a", "c", "d", "c"], items[:4])
    assert len(store) == 2 and "c" not in store._rows and store._next_row == 2
    store._assign_rows(["c", "a"])
    store.forget(["b", "nobody"])
    assert len(store) == 2 and store._assign_rows(["e"]) == [1]       # the freed row is taken again


def test_mismatched_lengths_are_refused(setting):
    _, _, rec, items = setting
    store = rec.open_sessions(3)
    with pytest.raises(ValueError, match="2 user keys for 3 items"):
        store.append(["a", "b"], items[:3])
    with pytest.raises(ValueError, match="at most 65536 events per call, got 65537"):
        store.append(["a"] * 65537, items[:1] * 65537)
    assert len(store) == 0


def test_wrong_dtypes_and_devices_are_refused():
    i32, i64 = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    state = {"hist": torch.zeros((2, 3), dtype=torch.int64), "count": torch.zeros(2, dtype=torch.int64)}
    with pytest.raises(ValueError, match="'hist' must be a contiguous int64 tensor of rank 2 on the device"):
        engine_mod.check_history_state(state)                          # host tensors
    with pytest.raises(ValueError, match="a history state is a dict"):
        engine_mod.check_history_state(None)
    with pytest.raises(ValueError, match="users must be a contiguous torch.int32 tensor"):
        engine_mod.check_history_events(i64, i64)
    with pytest.raises(ValueError, match="users must be a contiguous torch.int32 tensor \\[N\\] on the device"):
        engine_mod.check_history_events(i32, i64)                      # right dtypes, on the host
    with pytest.raises(ValueError, match="users must be a contiguous torch.int32 tensor \\[R\\] on the device"):
        engine_mod.check_history_batch_args(i32, L, P, None, C)
    with pytest.raises(ValueError, match="users must be a contiguous torch.int32"):
        engine_mod.check_history_batch_args([0, 1], L, P, None, C)


# ---- C-level argument errors that return before any launch --------------------------------------------------------------------------
FAKE = 4096        # a non-NULL, 8-byte aligned value that is never dereferenced: every call below returns before its launch


def append(lib, hist=FAKE, count=FAKE, U=5, Cn=7, V=50, users=FAKE * 2, items=FAKE * 3, N=4, accepted=None, scratch=FAKE * 4, nbytes=None):
    nbytes = 16 * max(N, 0) if nbytes is None else nbytes
    return lib.b4r_history_append(hist, count, U, Cn, V, FIRST, users, items, N, accepted, scratch, nbytes, None)


def batch(lib, U=5, Cn=7, R=3, Ln=L, Pn=P, E=7, null=None):
    ptr = dict(hist=FAKE, count=FAKE, req=FAKE, tokens=FAKE, mask=FAKE, len=FAKE, positions=FAKE, weights=FAKE, exclude=FAKE, live=FAKE)
    if null:
        ptr[null] = None
    return lib.b4r_history_batch(ptr["hist"], ptr["count"], U, Cn, ptr["req"], R, Ln, Pn, E, MASK, ptr["tokens"], ptr["mask"], ptr["len"],
                                 ptr["positions"], ptr["weights"], ptr["exclude"], ptr["live"], None)


def test_append_argument_errors():
    lib = _lib.load()
    assert lib.b4r_history_append_scratch_bytes(0) == 0 and lib.b4r_history_append_scratch_bytes(65536) == 16 * 65536
    assert lib.b4r_history_append_scratch_bytes(-1) == -1 and lib.b4r_history_append_scratch_bytes(65537) == -1
    for bad in (dict(N=-1), dict(N=65537), dict(Cn=0), dict(Cn=4097), dict(U=0), dict(U=-3), dict(U=1 << 40, Cn=1), dict(U=1 << 28, Cn=4096),
                dict(U=1 << 62, Cn=4096)):
        assert append(lib, **bad) == SHAPE, bad
        assert "bad shape" in _lib.last_error()
    assert append(lib, N=0, hist=None, count=None, users=None, items=None, scratch=None) == OK       # launches nothing
    for null in ("hist", "count", "users", "items", "scratch"):
        assert append(lib, **{null: None}) == BADARG and "null" in _lib.last_error(), null
    assert append(lib, scratch=FAKE * 4 + 4) == BADARG and "aligned" in _lib.last_error()
    assert append(lib, nbytes=63) == NOMEM and "64 needed" in _lib.last_error()
    assert append(lib, accepted=FAKE * 2 + 12) == BADARG and "overlaps" in _lib.last_error()          # the last flag on the first users
    assert append(lib, accepted=FAKE * 3 - 4) == BADARG                                                # ... on the first item


def test_batch_argument_errors():
    lib = _lib.load()
    for bad in (dict(Ln=1), dict(Ln=257), dict(Pn=0), dict(E=0), dict(R=-1), dict(Cn=0), dict(Cn=4097), dict(U=0), dict(U=1 << 40, Cn=1)):
        assert batch(lib, **bad) == SHAPE, bad
    assert batch(lib, R=0, null="tokens") == OK                                                        # launches nothing
    for null in ("hist", "count", "req", "tokens", "mask", "len", "positions", "weights", "exclude"):
        assert batch(lib, null=null) == BADARG and "null" in _lib.last_error(), null
