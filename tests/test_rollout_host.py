"""Multi-step roll-outs without a GPU: the restatements of tests/rollout_ref.py against prepare_inference and against a brute-force
selection, the argument checks of the two C entry points (all made before any launch) and of the Python layers."""
import ctypes as C

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, engine as engine_mod, models
from bert4rec_amd.apps import Recommender
from tests import rollout_ref as rr
from tests.test_gpu_api import make_loader

F32 = np.float32
NINF = F32(-np.inf)


# ---- advance = prepare_inference(history + [item]) ------------------------------------------------------------------------------
def test_advance_equals_prepare_inference_of_the_longer_history():
    L, P = 24, 6
    dl = make_loader()
    dl.generate_vocab()
    items = dl.create_item_list()
    tok = dl.get_tokenizer()
    V = tok.get_vocab_size()
    lengths = (0, 1, 21, 22, 23, 24, 40)
    histories = [items[7 * i:7 * i + n] for i, n in enumerate(lengths)]
    nexts = [items[100 + 5 * i:100 + 5 * i + 3] for i in range(len(lengths))]

    def prepared(hs):
        parts = [dl.prepare_inference(list(h)) for h in hs]
        return {k: np.concatenate([np.asarray(p[k]) for p in parts], axis=0) for k in ("input_word_ids", "input_mask", "masked_lm_positions")}

    cur = prepared(histories)
    assert cur["input_word_ids"].shape == (len(lengths), L) and cur["masked_lm_positions"].shape == (len(lengths), P)
    mask_id = int(cur["input_word_ids"][0, 0])                               # the empty history is the placeholder alone
    assert mask_id == engine_mod.MASK_ID
    tokens, length = cur["input_word_ids"], cur["input_mask"].sum(axis=1).astype(np.int32)
    assert length.tolist() == [1, 2, 22, 23, 24, 24, 24]
    ex = np.full((len(lengths), 3), -1, np.int64)
    path = None
    for t in range(3):
        item = np.asarray([tok.tokenize(n[t]) for n in nexts], np.int64)
        out = rr.advance(tokens, length, ex, path, None, None, item, None, 1, 1, P, 3, V, 3, mask_id, t, t)
        want = prepared([h + n[:t + 1] for h, n in zip(histories, nexts)])
        assert np.array_equal(out["tokens"], want["input_word_ids"])
        assert np.array_equal(out["mask"], want["input_mask"])
        assert np.array_equal(out["positions"], want["masked_lm_positions"])
        assert np.array_equal(out["path"][:, :t + 1], np.asarray([[tok.tokenize(x) for x in n[:t + 1]] for n in nexts]))
        tokens, length, ex, path = out["tokens"], out["len"], out["exclude"], out["path"]
    assert length.tolist() == [4, 5, 24, 24, 24, 24, 24]                     # rows 2 and 3 started to slide mid-way
    assert (ex >= 3).all()


# ---- beam_select = brute force ---------------------------------------------------------------------------------------------------
def brute_select(beam_logp, cand_ids, cand_logp, Bout):
    """Bout rounds of arg-max over the remaining live entries: another algorithm than the restatement's sort"""
    U, Bm = beam_logp.shape
    C_ = cand_ids.shape[1]
    outs = (np.full((U, Bout), -1, np.int32), np.full((U, Bout), -1, np.int64), np.full((U, Bout), NINF, F32), np.full((U, Bout), NINF, F32))
    with np.errstate(over="ignore", invalid="ignore"):
        for u in range(U):
            total = (beam_logp[u][:, None] + cand_logp[u * Bm:(u + 1) * Bm]).astype(F32)
            live = (beam_logp[u][:, None] > NINF) & (cand_ids[u * Bm:(u + 1) * Bm] >= 0) & (cand_logp[u * Bm:(u + 1) * Bm] > NINF)
            for t in range(Bout):
                best = None
                for b in range(Bm):
                    for c in range(C_):
                        if live[b, c] and (best is None or total[b, c] > total[best]):   # strict: the first of equals stays; -0.0 == 0.0
                            best = (b, c)
                if best is None:
                    break
                live[best] = False
                b, c = best
                outs[0][u, t], outs[1][u, t], outs[2][u, t], outs[3][u, t] = b, cand_ids[u * Bm + b, c], total[b, c], cand_logp[u * Bm + b, c]
    return outs


def planted_beams(U, Bm, C_, seed):
    """Random log probabilities on a coarse grid (many exact ties), plus, for user 0: an exact tie inside beam 0 and across beams 0 and
    1, totals of -0.0 against +0.0, a dead parent, -1 / -inf candidate tails; user 1 of three has two live entries, the last user of
    two or more has none."""
    rng = np.random.default_rng(seed)
    beam = (-np.round(rng.random((U, Bm)) * 8) / 4).astype(F32)
    ids = rng.integers(3, 500, size=(U * Bm, C_)).astype(np.int64)
    logp = (-np.round(rng.random((U * Bm, C_)) * 16) / 4).astype(F32)
    if C_ >= 2:
        tail = max(1, C_ // 4)
        ids[:, C_ - tail:][rng.random((U * Bm, tail)) < 0.5] = -1            # candidate tails: -1 ids ...
        logp[ids < 0] = NINF                                                 # ... with -inf
    beam[0, 0] = F32(-0.0)
    if C_ >= 2:
        logp[0, :2], ids[0, :2] = F32(-0.25), (7, 8)                         # a tie inside beam 0
    if C_ >= 4:
        logp[0, 2:4], ids[0, 2:4] = (F32(-0.0), F32(0.0)), (9, 10)           # totals -0.0 and +0.0: equal, the lower candidate first
    if Bm >= 2:
        beam[0, 1] = F32(-0.0)
        logp[1, 0], ids[1, 0] = F32(-0.25), 11                               # a tie between beams 0 and 1
        if C_ >= 2:
            logp[1, 1], ids[1, 1] = F32(0.0), 12                             # total +0.0 in beam 1 against -0.0 in beam 0
    if Bm >= 3:
        beam[0, Bm - 1] = NINF                                               # a dead parent
    if U >= 2:
        ids[(U - 1) * Bm:] = -1                                              # a user without a live entry
        logp[(U - 1) * Bm:] = NINF
    if U >= 3:
        ids[Bm:2 * Bm] = -1                                                  # a user with two live entries
        beam[1] = F32(-3.0)
        ids[Bm, 0], logp[Bm, 0] = 13, F32(-1.0)
        ids[2 * Bm - 1, C_ - 1], logp[2 * Bm - 1, C_ - 1] = 14, F32(-2.0)
    return beam, ids, logp


@pytest.mark.parametrize("U,Bm,C_,Bout", [(1, 1, 1, 1), (3, 1, 5, 4), (2, 4, 4, 4), (3, 3, 21, 5), (2, 5, 13, 64), (3, 8, 16, 8)])
def test_restated_beam_select_equals_brute_force(U, Bm, C_, Bout):
    for seed in range(3):
        beam, ids, logp = planted_beams(U, Bm, C_, seed)
        got = rr.beam_select(beam, ids, logp, Bout)
        want = brute_select(beam, ids, logp, Bout)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
        if U >= 2:
            assert (got[0][U - 1] == -1).all() and np.isneginf(got[2][U - 1]).all()
        if U >= 3 and Bout >= 3:
            assert got[1][1].tolist()[:3] == [13, 14, -1]


def test_restated_beam_select_orders_ties_and_zeros():
    beam = np.asarray([[-0.0, -1.0, -np.inf]], F32)
    ids = np.asarray([[5, 6, 7], [8, 9, -1], [10, 11, 12]], np.int64)
    logp = np.asarray([[-1.0, -0.0, -1.0], [0.0, 1.0, 5.0], [9.0, 9.0, 9.0]], F32)
    parent, item, total, step = rr.beam_select(beam, ids, logp, 6)
    # totals: beam 0: -1, -0, -1; beam 1: -1, 0, dead id; beam 2: a dead parent.  -0.0 ties with +0.0: the lower beam first
    assert item[0].tolist() == [6, 9, 5, 7, 8, -1] and parent[0].tolist() == [0, 1, 0, 0, 1, -1]
    assert np.signbit(total[0, 0]) and not np.signbit(total[0, 1]) and total[0, 2:5].tolist() == [-1.0, -1.0, -1.0]
    assert step[0, :5].tolist() == [-0.0, 1.0, -1.0, -1.0, 0.0] and np.isneginf(total[0, 5]) and np.isneginf(step[0, 5])


# ---- the C entry points check before they launch --------------------------------------------------------------------------------
def test_beam_select_argument_errors_need_no_gpu():
    f = _lib.load().b4r_beam_select
    x = C.create_string_buffer(64)                                           # never dereferenced: the checks come first
    p = C.addressof(x)
    ok = dict(U=2, Bm=4, C=8, Bout=4)
    for change, code in ((dict(Bm=0), -2), (dict(Bm=65), -2), (dict(C=0), -2), (dict(C=1025), -2), (dict(Bm=64, C=65), -2),
                         (dict(Bm=4, C=1024, Bout=4), 0), (dict(Bout=0), -2), (dict(Bout=65), -2), (dict(U=-1), -2)):
        a = {**ok, **change}
        if code == 0:
            a["U"] = 0                                                       # a legal shape: nothing to launch for no user
        assert f(p, p, p, a["U"], a["Bm"], a["C"], a["Bout"], p, p, p, p, None) == code, (change, _lib.last_error())
    assert "b4r_beam_select" in _lib.last_error()
    assert f(p, p, p, 2, 1, 4097, 4, p, p, p, p, None) == -2 and f(p, p, p, 2, 4, 1025, 4, p, p, p, p, None) == -2   # Bm * C = 4097 / 4100
    for nulls in ((None, p, p), (p, None, p), (p, p, None)):
        assert f(*nulls, 2, 4, 8, 4, p, p, p, p, None) == -1
    assert f(None, None, None, 0, 4, 8, 4, None, None, None, None, None) == 0   # U = 0


def advance_call(**change):
    x = [C.create_string_buffer(64) for _ in range(15)]
    ptr = [C.addressof(b) for b in x]
    a = dict(tokens_in=ptr[0], len_in=ptr[1], exclude_in=ptr[2], path_in=ptr[3], path_logp_in=ptr[4], parent=ptr[5], item=ptr[6],
             item_logp=ptr[7], N_in=1, N_out=1, G_in=1, G_out=1, L=2, P=1, E=1, T=1, V=10, first_item=3, mask_id=1, t=0, ex_col=0,
             tokens_out=ptr[8], input_mask_out=ptr[9], len_out=ptr[10], positions_out=ptr[11], exclude_out=ptr[12], path_out=ptr[13],
             path_logp_out=ptr[14])
    for k, v in change.items():
        a[k] = a[v] if isinstance(v, str) else v
    order = ("tokens_in", "len_in", "exclude_in", "path_in", "path_logp_in", "parent", "item", "item_logp", "N_in", "N_out", "G_in", "G_out",
             "L", "P", "E", "T", "V", "first_item", "mask_id", "t", "ex_col", "tokens_out", "input_mask_out", "len_out", "positions_out",
             "exclude_out", "path_out", "path_logp_out")
    return _lib.load().b4r_rollout_advance(*[a[k] for k in order], None), x


def test_rollout_advance_argument_errors_need_no_gpu():
    for change in (dict(L=1), dict(L=0), dict(P=0), dict(E=0), dict(T=0), dict(t=1), dict(t=-1), dict(ex_col=1), dict(ex_col=-1), dict(V=0),
                   dict(G_in=0), dict(G_out=0), dict(N_in=2, G_in=2, N_out=3, G_out=2), dict(N_in=2, N_out=4),
                   dict(parent=None, N_in=2, G_in=2, N_out=1)):
        rc, _ = advance_call(**change)
        assert rc == -2, (change, _lib.last_error())
    for name in ("tokens_in", "len_in", "exclude_in", "item", "tokens_out", "input_mask_out", "len_out", "positions_out", "exclude_out"):
        rc, _ = advance_call(**{name: None})
        assert rc == -1 and "null" in _lib.last_error(), name
    rc, _ = advance_call(item_logp=None)                                     # path_logp_out needs the items' log probabilities
    assert rc == -1
    for out, inp in (("tokens_out", "tokens_in"), ("len_out", "len_in"), ("exclude_out", "exclude_in"), ("path_out", "path_in"),
                     ("path_logp_out", "path_logp_in"), ("input_mask_out", "tokens_in")):
        rc, _ = advance_call(**{out: inp})
        assert rc == -1 and "alias" in _lib.last_error(), out
    # nothing to do: N_out = 0 succeeds whatever the pointers are
    for change in (dict(N_in=0, N_out=0), dict(N_in=0, N_out=0, tokens_in=None, item=None, tokens_out=None, parent=None)):
        rc, _ = advance_call(**change)
        assert rc == 0, _lib.last_error()


# ---- the Python layers ----------------------------------------------------------------------------------------------------------------
def test_python_layers_refuse_bad_arguments_before_any_work():
    check = engine_mod.check_rollout_args
    assert check(1) == (1, 1, 1) and check(64, 64, 64) == (64, 64, 64) and check(3, 4) == (3, 4, 4) and check(3, 4, 1024) == (3, 4, 1024)
    assert check(np.int64(5), sample_seed=(1 << 64) - 1, temperature=0.5) == (5, 1, 1)
    assert check(2, 1, None, 2.0) == (2, 1, 1) and check(2, 3, None, 2.0, None, False) == (2, 3, 3)
    for steps in (0, 65, 1.0, "3", None, True):
        with pytest.raises(ValueError, match="steps"):
            check(steps)
    for beams in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="beams"):
            check(3, beams)
    for expand in (0, 1025, 1.5):
        with pytest.raises(ValueError, match="expand"):
            check(3, 2, expand)
    with pytest.raises(ValueError, match="4096"):
        check(3, 5, 820)
    assert check(3, 4, 1024) and check(3, 64, 64)
    with pytest.raises(ValueError, match="beams"):
        check(3, 2, sample_seed=1)
    with pytest.raises(ValueError, match="sample_seed"):
        check(3, 1, sample_seed=-1)
    with pytest.raises(ValueError, match="temperature"):
        check(3, 1, None, 2.0, None, False)
    for t in (0.0, float("nan"), -1.0):
        with pytest.raises(ValueError, match="temperature"):
            check(3, 1, None, t)

    model = object.__new__(models.BERT4RecModel)            # the checks come before anything of the model is touched
    rs = models.BERT4RecModel.recommend_sequence_tensor
    for kw in (dict(steps=0), dict(steps=3, beams=65), dict(steps=3, beams=2, expand=4096), dict(steps=3, beams=2, sample_seed=1),
               dict(steps=3, temperature=2.0, return_logp=False), dict(steps=3, sample_streams=[1, 2])):
        with pytest.raises(ValueError):
            rs(model, {}, **kw)
    for name in ("diversity", "pool", "max_per_group"):
        with pytest.raises(TypeError):
            rs(model, {}, steps=3, **{name: 1})
    rec = Recommender(None, None)
    with pytest.raises(ValueError, match="steps"):
        rec.recommend_sequences([[1, 2]], steps=0)
    with pytest.raises(ValueError, match="beams"):
        rec.recommend_sequences([[1, 2]], steps=2, beams=2, sample_seed=1)
    with pytest.raises(ValueError, match="sample_seed"):
        rec.recommend_sequences([[1, 2]], steps=2, user_streams=[4])
    with pytest.raises(ValueError, match="temperature"):
        rec.recommend_sequences([[1, 2]], steps=2, temperature=2.0)


def test_the_roll_out_takes_prepare_inference_rows_only():
    L, P = 8, 3
    mask = torch.zeros((3, L), dtype=torch.int64)
    pos = torch.zeros((3, P), dtype=torch.int64)
    w = torch.zeros((3, P), dtype=torch.int64)
    for r, n in enumerate((1, 5, 8)):
        mask[r, :n] = 1
        pos[r, 0] = n - 1
        w[r, 0] = 1
    length, slot = engine_mod.check_rollout_batch(mask, pos, w)
    assert length.tolist() == [1, 5, 8] and slot.tolist() == [0, 0, 0]
    moved_pos, moved_w = pos.clone(), w.clone()                              # the one weighted slot may be any slot
    moved_pos[1], moved_w[1] = torch.tensor([0, 0, 4]), torch.tensor([0, 0, 1])
    assert engine_mod.check_rollout_batch(mask, moved_pos, moved_w)[1].tolist() == [0, 2, 0]
    assert engine_mod.check_rollout_batch(mask, pos[:, :1], None)[0].tolist() == [1, 5, 8]
    two = w.clone(); two[1, 1] = 1                                           # two weighted slots in a row
    none = w.clone(); none[2] = 0                                            # no weighted slot
    early = pos.clone(); early[1, 0] = 3                                     # the slot is not the last real token
    holes = mask.clone(); holes[1, 2] = 0                                    # the mask is no prefix
    empty = mask.clone(); empty[0] = 0
    for m, p_, w_ in ((mask, pos, two), (mask, pos, none), (mask, early, w), (holes, pos, w), (empty, pos, w), (mask, pos, None)):
        with pytest.raises(ValueError, match="prepare_inference"):
            engine_mod.check_rollout_batch(m, p_, w_)
    with pytest.raises(ValueError, match="masked_lm_positions"):
        engine_mod.check_rollout_batch(mask, pos[:, :0], None)
