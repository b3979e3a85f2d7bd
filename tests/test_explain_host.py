"""Occlusion explanations without a GPU: the restatements of tests/explain_ref.py against prepare_inference, against a brute-force
removal and against a brute-force selection, the argument checks of the two C entry points (all made before any launch) and of the
Python layers."""
import ctypes as C

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, engine as engine_mod, models
from bert4rec_amd.apps import Recommender
from tests import explain_ref as er
from tests.test_gpu_api import make_loader

F32 = np.float32
NINF = F32(-np.inf)


# ---- occlude (item mode) = prepare_inference(window items without that item) ------------------------------------------------------
def test_item_occlusion_equals_prepare_inference_of_the_shorter_history():
    L, P = 24, 6
    dl = make_loader()
    dl.generate_vocab()
    items = dl.create_item_list()
    tok = dl.get_tokenizer()
    V = tok.get_vocab_size()
    lengths = (0, 1, 2, 22, 23, 24, 40)
    histories = [items[7 * i:7 * i + n] for i, n in enumerate(lengths)]

    def prepared(hs):
        parts = [dl.prepare_inference(list(h)) for h in hs]
        return {k: np.concatenate([np.asarray(p[k]) for p in parts], axis=0) for k in ("input_word_ids", "input_mask", "masked_lm_positions")}

    cur = prepared(histories)
    assert cur["input_word_ids"].shape == (len(lengths), L) and cur["masked_lm_positions"].shape == (len(lengths), P)
    mask_id = int(cur["input_word_ids"][0, 0])                               # the empty history is the placeholder alone
    assert mask_id == engine_mod.MASK_ID
    tokens, length = cur["input_word_ids"], cur["input_mask"].sum(axis=1).astype(np.int32)
    assert length.tolist() == [1, 2, 3, 23, 24, 24, 24]
    windows = [list(h[-(L - 1):]) for h in histories]                        # what the model sees of a history
    # all recency indices at once, and the same in two chunks (the second starts inside and runs past every history)
    whole = er.occlude_rows(tokens, length, None, V, mask_id, P, 0, L + 2)
    for w0, Wc in ((0, 5), (5, L - 3)):
        part = er.occlude_rows(tokens, length, None, V, mask_id, P, w0, Wc)
        for k, v in part.items():
            full = whole[k].reshape((len(lengths), L + 2) + whole[k].shape[1:])[:, w0:w0 + Wc]
            assert np.array_equal(v, full.reshape(v.shape)), k
    n_live = 0
    for u, win in enumerate(windows):
        for w in range(L + 2):
            n = u * (L + 2) + w
            if w < len(win):
                p = len(win) - 1 - w
                want = prepared([win[:p] + win[p + 1:]])
                assert np.array_equal(whole["tokens"][n], want["input_word_ids"][0]), (u, w)
                assert np.array_equal(whole["mask"][n], want["input_mask"][0]) and np.array_equal(whole["positions"][n], want["masked_lm_positions"][0])
                assert whole["live"][n] == 1 and whole["unit_pos"][n] == p and whole["unit_item"][n] == tok.tokenize(win[p])
                assert whole["unit_label"][n] == -1 and whole["removed"][n] == 1 and whole["len"][n] == len(win)
                n_live += 1
            else:                                                            # beyond the history: a dead copy
                assert np.array_equal(whole["tokens"][n], tokens[u]) and np.array_equal(whole["mask"][n], cur["input_mask"][u])
                assert np.array_equal(whole["positions"][n], cur["masked_lm_positions"][u]) and whole["len"][n] == length[u]
                assert (whole["live"][n], whole["unit_pos"][n], whole["unit_item"][n], whole["unit_label"][n], whole["removed"][n]) == (0, -1, -1, -1, 0)
    assert n_live == 0 + 1 + 2 + 22 + 23 + 23 + 23


# ---- occlude (group mode) = brute-force removal ---------------------------------------------------------------------------------------
def brute_group_rows(row, ln, labels, V, mask_id, L):
    """{recency index: (tokens, len_out, label, removed)} of the live units, by a scan from the most recent item back"""
    hist = [int(x) for x in row[:ln - 1]]
    lab = [int(labels[t]) if 0 <= t < V else -1 for t in hist]
    done, out = set(), {}
    for w in range(len(hist)):
        p = len(hist) - 1 - w
        if lab[p] < 0 or lab[p] in done:
            continue
        done.add(lab[p])
        rest = [t for t, g in zip(hist, lab) if g != lab[p]]
        out[w] = (rest + [mask_id] + [0] * (L - 1 - len(rest)), len(rest) + 1, lab[p], len(hist) - len(rest))
    return out


def group_case(L, U, n_labels, seed, V=40):
    rng = np.random.default_rng(seed)
    labels = rng.integers(-1, n_labels, size=V).astype(np.int32)           # label -1: in no group
    labels[3] = 0
    tokens = rng.integers(3, V, size=(U, L)).astype(np.int64)
    tokens[rng.random((U, L)) < 0.15] = (V, V + 7, -1, -(1 << 40), 1 << 40)[seed % 5]   # ids outside [0, V): in no group either
    if L >= 4 and U >= 4:
        tokens[3, 0] = tokens[3, 2] = tokens[3, L - 2] = 3                   # duplicate items in a full row (row 3), in group 0
    lens = np.asarray([1, 2, L - 1, L, 0, L + 3], np.int32)[np.arange(U) % 6]   # (0 and L + 3 are clamped to 1 and L)
    return tokens, lens, labels


@pytest.mark.parametrize("L,n_labels", [(2, 1), (3, 3), (9, 1), (9, 3), (24, 3), (24, 1000)])
def test_group_occlusion_equals_a_brute_force_removal(L, n_labels):
    V, P, U = 40, 3, 13
    for seed in range(3):
        tokens, lens, labels = group_case(L, U, n_labels, seed, V)
        if n_labels == 1:
            labels[:] = 0                                                    # one label for the whole catalogue: len_out = 1
        got = er.occlude_rows(tokens, lens, labels, V, 1, P, 0, L + 1)
        for u in range(U):
            ln = int(np.clip(lens[u], 1, L))
            want = brute_group_rows(tokens[u], ln, labels, V, 1, L)
            for w in range(L + 1):
                n = u * (L + 1) + w
                if w in want:
                    row, ln_o, label, removed = want[w]
                    assert got["tokens"][n].tolist() == row and got["len"][n] == ln_o and got["mask"][n].tolist() == [1] * ln_o + [0] * (L - ln_o)
                    assert got["positions"][n].tolist() == [ln_o - 1] + [0] * (P - 1)
                    assert (got["live"][n], got["unit_pos"][n], got["unit_item"][n]) == (1, ln - 2 - w, tokens[u, ln - 2 - w])
                    assert got["unit_label"][n] == label and got["removed"][n] == removed and ln_o == ln - removed
                else:
                    assert got["tokens"][n].tolist() == tokens[u].tolist() and got["len"][n] == ln and got["live"][n] == 0
                    assert (got["unit_pos"][n], got["unit_item"][n], got["unit_label"][n], got["removed"][n]) == (-1, -1, -1, 0)
            if n_labels == 1 and ln >= 2 and all(0 <= t < V for t in tokens[u, :ln - 1]):
                assert got["len"][u * (L + 1)] == 1 and got["tokens"][u * (L + 1)].tolist() == [1] + [0] * (L - 1)


# ---- attribution_select = m rounds of strict arg-max --------------------------------------------------------------------------------
def brute_attribution(base, occ, live, m):
    """m rounds of arg-max over the remaining live entries: another algorithm than the restatement's sort"""
    U, K = base.shape
    W = occ.shape[0] // U
    out_w, out_d = np.full((U, K, m), -1, np.int32), np.full((U, K, m), NINF, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for u in range(U):
            for i in range(K):
                delta = (base[u, i] - occ[u * W:(u + 1) * W, i]).astype(F32)
                ok = (live[u * W:(u + 1) * W] != 0) & (base[u, i] > NINF) & (occ[u * W:(u + 1) * W, i] > NINF)
                for t in range(m):
                    best = None
                    for w in range(W):
                        if ok[w] and (best is None or delta[w] > delta[best]):   # strict: the first of equals stays; -0.0 == 0.0
                            best = w
                    if best is None:
                        break
                    ok[best] = False
                    out_w[u, i, t], out_d[u, i, t] = best, delta[best]
    return out_w, out_d


def planted_attribution(U, W, K, seed):
    """Log probabilities on a coarse grid (many exact ties, positive and negative deltas); for user 0 a tie between two units, deltas
    of -0.0 against +0.0, a NaN and a -inf among the occluded values; the items of user 0 take turns at a -inf / NaN base; from two
    users on the last user has no live unit, from three on user 1 has some dead units."""
    rng = np.random.default_rng(seed)
    base = (-np.round(rng.random((U, K)) * 16) / 4).astype(F32)
    occ = (-np.round(rng.random((U * W, K)) * 16) / 4).astype(F32)
    live = np.ones(U * W, np.int32)
    if W >= 2:
        occ[0, 0] = occ[1, 0] = base[0, 0] - F32(0.75)                       # a tie between w = 0 and w = 1
    if W >= 4:
        base[0, K - 1] = F32(-0.0)
        occ[2, K - 1], occ[3, K - 1] = F32(0.0), F32(-0.0)                   # deltas -0.0 (w = 2) and +0.0 (w = 3): equal, w = 2 first
    if W >= 5:
        occ[4, 0] = np.nan
    if W >= 6:
        occ[5, 0] = NINF
    if K >= 3:
        base[0, 1] = NINF
    if K >= 4:
        base[0, 2] = np.nan
    if U >= 2:
        live[(U - 1) * W:] = 0
    if U >= 3:
        live[W:2 * W][rng.random(W) < 0.5] = 0
        live[W] = 7                                                          # any nonzero value is live
    return base, occ, live


def test_restated_attribution_select_orders_ties_zeros_and_negative_deltas():
    base = np.asarray([[-1.0, -0.0]], F32)
    occ = np.asarray([[-3.0, 0.0], [-0.5, -0.0], [-3.0, 5.0], [-1.0, np.nan], [-9.0, 0.0]], F32)
    live = np.asarray([1, 1, 1, 1, 0], np.int32)
    w, d = er.attribution_select(base, occ, live, 5)
    # item 0: deltas 2, -0.5, 2, 0, dead.  item 1: -0 - 0 = -0, -0 - -0 = +0, -5, NaN, dead: -0.0 ties with +0.0, the lower w first
    assert w[0, 0].tolist() == [0, 2, 3, 1, -1] and d[0, 0, :4].tolist() == [2.0, 2.0, 0.0, -0.5] and np.isneginf(d[0, 0, 4])
    assert w[0, 1].tolist() == [0, 1, 2, -1, -1] and np.signbit(d[0, 1, 0]) and not np.signbit(d[0, 1, 1]) and d[0, 1, 2] == -5.0


@pytest.mark.parametrize("U,W,K,m", [(1, 1, 1, 1), (3, 5, 4, 2), (2, 7, 3, 7), (3, 23, 17, 3), (2, 64, 5, 64), (3, 9, 1, 1)])
def test_restated_attribution_select_equals_brute_force(U, W, K, m):
    for seed in range(3):
        base, occ, live = planted_attribution(U, W, K, seed)
        got = er.attribution_select(base, occ, live, m)
        want = brute_attribution(base, occ, live, m)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
        if U >= 2:
            assert (got[0][U - 1] == -1).all() and np.isneginf(got[1][U - 1]).all()
        if K >= 4:
            assert (got[0][0, 1:3] == -1).all()                              # a -inf base and a NaN base


# ---- the C entry points check before they launch --------------------------------------------------------------------------------
OCC_ORDER = ("tokens_in", "len_in", "labels", "U", "L", "P", "V", "mask_id", "w0", "Wc", "tokens_out", "input_mask_out", "len_out",
             "positions_out", "live_out", "unit_pos_out", "unit_item_out", "unit_label_out", "removed_out")


def occlude_call(**change):
    x = [C.create_string_buffer(64) for _ in range(12)]                      # never dereferenced: the checks come first
    ptr = [C.addressof(b) for b in x]
    a = dict(tokens_in=ptr[0], len_in=ptr[1], labels=ptr[2], U=1, L=2, P=1, V=10, mask_id=1, w0=0, Wc=1, tokens_out=ptr[3],
             input_mask_out=ptr[4], len_out=ptr[5], positions_out=ptr[6], live_out=ptr[7], unit_pos_out=ptr[8], unit_item_out=ptr[9],
             unit_label_out=ptr[10], removed_out=ptr[11])
    for k, v in change.items():
        a[k] = a[v] if isinstance(v, str) else v
    return _lib.load().b4r_occlude_rows(*[a[k] for k in OCC_ORDER], None), x


def test_occlude_rows_argument_errors_need_no_gpu():
    for change in (dict(L=1), dict(L=0), dict(L=257), dict(P=0), dict(V=0), dict(U=-1), dict(w0=-1), dict(Wc=0), dict(Wc=-3),
                   dict(U=1 << 16, Wc=1 << 15)):
        rc, _ = occlude_call(**change)
        assert rc == -2 and "b4r_occlude_rows" in _lib.last_error(), (change, _lib.last_error())
    for name in ("tokens_in", "len_in", "tokens_out", "input_mask_out", "len_out", "positions_out", "live_out"):
        rc, _ = occlude_call(**{name: None})
        assert rc == -1 and "null" in _lib.last_error(), name
    for out in ("tokens_out", "input_mask_out", "len_out", "positions_out", "live_out", "unit_pos_out", "unit_item_out", "unit_label_out",
                "removed_out"):
        rc, _ = occlude_call(**{out: "tokens_in"})
        assert rc == -1 and "overlaps" in _lib.last_error(), out
    rc, _ = occlude_call(len_out="len_in")
    assert rc == -1 and "overlaps" in _lib.last_error()
    rc, x = occlude_call(L=4)                                                # a partial overlap: the output begins inside the input
    rc, _ = occlude_call(L=4, tokens_in=C.addressof(x[0]), tokens_out=C.addressof(x[0]) + 24)
    assert rc == -1 and "overlaps" in _lib.last_error()
    # nothing to do: U = 0 succeeds whatever the pointers are
    for change in (dict(U=0), dict(U=0, tokens_in=None, len_in=None, tokens_out=None, live_out=None), dict(U=0, L=256, w0=(1 << 31) - 1)):
        rc, _ = occlude_call(**change)
        assert rc == 0, _lib.last_error()
    rc, _ = occlude_call(U=0, L=257)
    assert rc == -2


def test_attribution_select_argument_errors_need_no_gpu():
    f = _lib.load().b4r_attribution_select
    x = C.create_string_buffer(64)
    p = C.addressof(x)
    ok = dict(U=2, W=8, K=4, m=3)
    for change in (dict(W=0), dict(W=257), dict(K=0), dict(K=1025), dict(m=0), dict(m=9), dict(m=-1), dict(U=-1), dict(W=1, m=2)):
        a = {**ok, **change}
        assert f(p, p, p, a["U"], a["W"], a["K"], a["m"], p, p, None) == -2, (change, _lib.last_error())
        assert "b4r_attribution_select" in _lib.last_error()
    for nulls in ((None, p, p), (p, None, p), (p, p, None)):
        assert f(*nulls, 2, 8, 4, 3, p, p, None) == -1
    for a in (dict(W=256, K=1024, m=256), dict(W=1, K=1, m=1), ok):         # legal shapes: nothing to launch for no user
        assert f(None, None, None, 0, a["W"], a["K"], a["m"], None, None, None) == 0, _lib.last_error()


# ---- the Python layers ----------------------------------------------------------------------------------------------------------------
def test_python_layers_refuse_bad_arguments_before_any_work():
    check = engine_mod.check_explain_args
    assert check(3, None, 24) == (3, 23) and check(1, 1, 2) == (1, 1) and check(np.int64(5), 5, 200, K=1024, rows_per_forward=1) == (5, 5)
    assert check(255, None, 256) == (255, 255)
    for top in (0, 257, 1.0, "3", None, True):
        with pytest.raises(ValueError, match="top"):
            check(top, None, 24)
    for window in (0, 24, 2.0, True):
        with pytest.raises(ValueError, match="window"):
            check(3, window, 24)
    with pytest.raises(ValueError, match="top = 4"):
        check(4, 3, 24)
    with pytest.raises(ValueError, match="top = 24"):
        check(24, None, 24)
    for L in (1, 257):
        with pytest.raises(ValueError, match="tokens"):
            check(1, None, L)
    for K in (0, 1025):
        with pytest.raises(ValueError, match="items"):
            check(1, None, 24, K=K)
    for rows in (0, -1, 2.5):
        with pytest.raises(ValueError, match="rows_per_forward"):
            check(1, None, 24, rows_per_forward=rows)

    model = object.__new__(models.BERT4RecModel)            # the checks come before anything of the model's engine is touched
    model.vocab_size = 50
    ex = models.BERT4RecModel.explain_tensor
    batch = {"input_word_ids": torch.zeros((2, 24), dtype=torch.int64)}
    good = torch.zeros((2, 3), dtype=torch.int64)
    for target, kw, match in ((good, dict(top=4, window=3), "top = 4"), (good, dict(top=0), "top"), (good, dict(window=24), "window"),
                              (good, dict(top=24), "top = 24"), (good, dict(rows_per_forward=0), "rows_per_forward"),
                              (torch.zeros((2, 0), dtype=torch.int64), {}, "items"), (torch.zeros((2, 1025), dtype=torch.int64), {}, "items"),
                              (0, {}, "items"), (1025, {}, "items"),
                              (torch.zeros((3, 3), dtype=torch.int64), {}, "target_ids"), (torch.zeros((2, 3)), {}, "target_ids"),
                              (torch.zeros(6, dtype=torch.int64), {}, "target_ids"),
                              (good, dict(labels=torch.zeros(49, dtype=torch.int32)), "labels"),
                              (good, dict(labels=torch.zeros((50, 1), dtype=torch.int32)), "labels"), (good, dict(labels=torch.zeros(50)), "labels"),
                              (good, dict(temperature=0.0), "temperature"), (good, dict(exclude=torch.zeros(4, dtype=torch.int64)), "exclude"),
                              (good, dict(row_filter=torch.zeros(2, dtype=torch.int32)), "row_filter"),
                              (good, dict(allow=torch.ones((2, 50), dtype=torch.bool), row_filter=torch.zeros(3, dtype=torch.int32)), "row_filter"),
                              (good, dict(allow=torch.ones(49, dtype=torch.bool)), "allow")):
        with pytest.raises(ValueError, match=match):
            ex(model, batch, target, **kw)
    for bad in ({}, {"input_word_ids": torch.zeros(24, dtype=torch.int64)}):
        with pytest.raises(ValueError, match="prepare_inference"):
            ex(model, bad, good)
    with pytest.raises(ValueError, match="tokens"):
        ex(model, {"input_word_ids": torch.zeros((2, 300), dtype=torch.int64)}, good)

    rec = Recommender(None, None)
    for kw, match in ((dict(top=0), "top"), (dict(top=4, window=3), "top = 4"), (dict(window=0), "window"), (dict(k=0), "k"),
                      (dict(k=1025), "k"), (dict(temperature=-1.0), "temperature"), (dict(items=[["a"], ["b"]]), "item lists"),
                      (dict(items=[[]]), "items are explained"), (dict(allowed_items=["a"], allowed_items_per_user=[["a"]]), "not both"),
                      (dict(allowed_items_per_user=[["a"], ["b"]]), "allow-lists")):
        with pytest.raises(ValueError, match=match):
            rec.explain_batch([[1, 2]], **kw)
    rec.model = model
    for by_group in ([0] * 49, np.zeros(50), "genre"):
        with pytest.raises(ValueError, match="by_group"):
            rec.explain_batch([[1, 2]], by_group=by_group)


def test_the_check_returns_the_largest_row_length_with_its_flag():
    L, P = 8, 3
    mask = torch.zeros((3, L), dtype=torch.int64)
    pos = torch.zeros((3, P), dtype=torch.int64)
    w = torch.zeros((3, P), dtype=torch.int64)
    for r, n in enumerate((1, 5, 3)):
        mask[r, :n] = 1
        pos[r, 0] = n - 1
        w[r, 0] = 1
    length, slot, longest = engine_mod.check_rollout_batch(mask, pos, w, return_max_len=True)
    assert length.tolist() == [1, 5, 3] and slot.tolist() == [0, 0, 0] and longest == 5 and isinstance(longest, int)
    assert len(engine_mod.check_rollout_batch(mask, pos, w)) == 2             # as before without the flag
    assert engine_mod.check_rollout_batch(mask[:0], pos[:0], w[:0], return_max_len=True)[2] == 0
    early = pos.clone()
    early[1, 0] = 3
    with pytest.raises(ValueError, match="prepare_inference"):
        engine_mod.check_rollout_batch(mask, early, w, return_max_len=True)
