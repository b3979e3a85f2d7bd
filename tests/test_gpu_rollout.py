"""Multi-step roll-outs on the GPU: b4r_beam_select and b4r_rollout_advance bit for bit against tests/rollout_ref.py, graph capture, and
the greedy / beam / sampled roll-outs of the model and the app against host loops over recommend_tensor."""
import functools
import itertools

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib
from bert4rec_amd.apps import Recommender
from tests import rollout_ref as rr
from tests.b4r_testlib import P, stream
from tests.test_gpu_api import make_loader, make_model
from tests.test_rollout_host import planted_beams

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
NINF = F32(-np.inf)
FIRST, MASK = 3, 1


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


# ---- b4r_beam_select ----------------------------------------------------------------------------------------------------------------
SELECT_OUTS = ("parent", "item", "logp", "step")


def select_outs(U, Bout):
    return dict(parent=torch.full((U, Bout), -7, dtype=torch.int32, device=DEV), item=torch.full((U, Bout), -7, dtype=torch.int64, device=DEV),
                logp=torch.full((U, Bout), 7.0, device=DEV), step=torch.full((U, Bout), 7.0, device=DEV))


def run_select(beam, ids, logp, Bout, null_out=(), outs=None, keep=None, sync=True):
    U, Bm = beam.shape
    keep = keep or [dev(beam), dev(ids), dev(logp)]
    outs = outs or select_outs(U, Bout)
    ptr = {k: (None if k in null_out else P(v)) for k, v in outs.items()}
    rc = _lib.load().b4r_beam_select(P(keep[0]), P(keep[1]), P(keep[2]), U, Bm, ids.shape[1], Bout, ptr["parent"], ptr["item"], ptr["logp"],
                                     ptr["step"], stream())
    if sync:
        torch.cuda.synchronize()
    return rc, outs, keep


def assert_select(outs, want, skip=()):
    for k, w in zip(SELECT_OUTS, want):
        got = outs[k].cpu().numpy()
        if k in skip:
            assert (got == (-7 if got.dtype.kind == "i" else 7.0)).all(), k
        else:
            assert got.dtype == w.dtype and got.tobytes() == w.tobytes(), k


SELECT_SHAPES = [(1, 1, 1, 1), (3, 1, 5, 4), (2, 4, 4, 4), (2, 8, 64, 8), (1, 64, 64, 64), (1, 4, 1024, 16), (2, 3, 21, 5), (2, 5, 13, 64)]


@pytest.mark.parametrize("U,Bm,C,Bout", SELECT_SHAPES)
def test_beam_select_against_the_restatement(U, Bm, C, Bout):
    """planted_beams: exact ties across beams and inside a beam, -0.0 against +0.0, a dead parent, -1 / -inf tails (and, from two
    users on, a user without a live entry); then the same case with its last user cut down to two live entries and to none"""
    beam, ids, logp = planted_beams(U, Bm, C, seed=Bm * C)
    few = (beam.copy(), ids.copy(), logp.copy())
    few[1][(U - 1) * Bm:] = -1
    few[2][(U - 1) * Bm:] = NINF
    none = tuple(a.copy() for a in few)
    none[0][U - 1] = NINF
    few[0][U - 1, 0], few[1][(U - 1) * Bm, 0], few[2][(U - 1) * Bm, 0] = F32(-1.5), 40, F32(-0.5)
    few[0][U - 1, Bm - 1], few[1][U * Bm - 1, C - 1], few[2][U * Bm - 1, C - 1] = F32(-1.0), 41, F32(-1.0)   # (one entry when Bm * C == 1)
    for variant in ((beam, ids, logp), few, none):
        rc, outs, _ = run_select(*variant, Bout)
        assert rc == 0, _lib.last_error()
        want = rr.beam_select(*variant, Bout)
        assert_select(outs, want)
    got = rr.beam_select(*few, Bout)
    want_items = [41] if Bm * C == 1 else [40, 41][:Bout]                    # 40 before 41: a better total (one beam) or the lower beam
    assert got[1][U - 1].tolist() == want_items + [-1] * (Bout - len(want_items))
    assert (rr.beam_select(*none, Bout)[0][U - 1] == -1).all()


def test_beam_select_null_outputs_and_argument_errors():
    beam, ids, logp = planted_beams(2, 3, 21, seed=5)
    want = rr.beam_select(beam, ids, logp, 5)
    for name in SELECT_OUTS:
        rc, outs, _ = run_select(beam, ids, logp, 5, null_out=(name,))
        assert rc == 0
        assert_select(outs, want, skip=(name,))
    for Bout in (0, 65):
        rc, outs, _ = run_select(beam, ids, logp, Bout)
        assert rc == -2
        assert_select(outs, want, skip=SELECT_OUTS)


# ---- b4r_rollout_advance ------------------------------------------------------------------------------------------------------------
ADV_IN = ("tokens", "len", "exclude", "path", "path_logp", "parent", "item", "item_logp")
ADV_OUT = ("tokens", "mask", "len", "positions", "exclude", "path", "path_logp")


def advance_case(G_in, G_out, L, Pn, E, T, use_parent, seed, users=16, V=50):
    rng = np.random.default_rng(seed)
    N_in, N_out = users * G_in, users * G_out
    lens = np.asarray([1, 2, L - 1, L, 0, L + 3], np.int32)[rng.permutation(N_in) % 6]   # (0 and L + 3 are clamped to 1 and L)
    lens[0:4 * G_in:G_in] = (1, 2, L - 1, L)                                 # the first input row of users 0 .. 3
    c = dict(tokens=rng.integers(3, V, size=(N_in, L)).astype(np.int64), len=lens, exclude=rng.integers(-1, V, size=(N_in, E)).astype(np.int64),
             path=rng.integers(3, V, size=(N_in, T)).astype(np.int64), path_logp=(-rng.random((N_in, T))).astype(F32),
             parent=rng.integers(0, G_in, size=N_out).astype(np.int32) if use_parent else None,
             item=rng.integers(FIRST, V, size=N_out).astype(np.int64), item_logp=(-rng.random(N_out)).astype(F32))
    if use_parent:
        c["parent"][:4 * G_out:G_out] = 0                                    # ... which the first output row of those users continues
        c["parent"][4 * G_out:5 * G_out] = rng.permutation(max(G_in, G_out))[:G_out] % G_in   # permuted
        c["parent"][5 * G_out:6 * G_out] = G_in - 1                          # repeated
        c["parent"][6 * G_out], c["parent"][7 * G_out] = -1, G_in            # dead by parent
    c["item"][8 * G_out], c["item"][9 * G_out], c["item"][10 * G_out] = -1, 2, V   # dead by item
    c.update(G_in=G_in, G_out=G_out, L=L, P=Pn, E=E, T=T, V=V, N_in=N_in, N_out=N_out)
    return c


def advance_outs(c):
    N, L, Pn, E, T = c["N_out"], c["L"], c["P"], c["E"], c["T"]
    return dict(tokens=torch.full((N, L), -7, dtype=torch.int64, device=DEV), mask=torch.full((N, L), -7, dtype=torch.int64, device=DEV),
                len=torch.full((N,), -7, dtype=torch.int32, device=DEV), positions=torch.full((N, Pn), -7, dtype=torch.int64, device=DEV),
                exclude=torch.full((N, E), -7, dtype=torch.int64, device=DEV), path=torch.full((N, T), -7, dtype=torch.int64, device=DEV),
                path_logp=torch.full((N, T), 7.0, device=DEV))


def run_advance(c, t, ex_col, outs=None, keep=None, sync=True, with_paths=True):
    keep = keep or {k: dev(c[k]) for k in ADV_IN}
    outs = outs or advance_outs(c)
    pin = (lambda k: P(keep[k])) if with_paths else (lambda k: None)
    rc = _lib.load().b4r_rollout_advance(
        P(keep["tokens"]), P(keep["len"]), P(keep["exclude"]), pin("path"), pin("path_logp"), P(keep["parent"]), P(keep["item"]),
        P(keep["item_logp"]), c["N_in"], c["N_out"], c["G_in"], c["G_out"], c["L"], c["P"], c["E"], c["T"], c["V"], FIRST, MASK, t, ex_col,
        P(outs["tokens"]), P(outs["mask"]), P(outs["len"]), P(outs["positions"]), P(outs["exclude"]), P(outs["path"]), P(outs["path_logp"]),
        stream())
    if sync:
        torch.cuda.synchronize()
    return rc, outs, keep


def restated_advance(c, t, ex_col, with_paths=True):
    return rr.advance(c["tokens"], c["len"], c["exclude"], c["path"] if with_paths else None, c["path_logp"] if with_paths else None,
                      c["parent"], c["item"], c["item_logp"], c["G_in"], c["G_out"], c["P"], c["T"], c["V"], FIRST, MASK, t, ex_col)


def assert_advance(outs, want):
    for k in ADV_OUT:
        got = outs[k].cpu().numpy()
        assert got.dtype == want[k].dtype and got.tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("G_in,G_out,use_parent", [(1, 1, False), (1, 3, True), (3, 3, True), (4, 2, True)])
def test_rollout_advance_against_the_restatement(G_in, G_out, use_parent):
    for i, (L, Pn, E, T) in enumerate(itertools.product((2, 4, 33), (1, 3), (1, 5), (1, 4))):
        c = advance_case(G_in, G_out, L, Pn, E, T, use_parent, seed=i)
        for t, ex_col in {(0, 0), (T - 1, E - 1)}:
            rc, outs, _ = run_advance(c, t, ex_col)
            assert rc == 0, _lib.last_error()
            want = restated_advance(c, t, ex_col)
            assert_advance(outs, want)
        # every length among the sources of the live rows, and every kind of dead row
        par = np.arange(c["N_out"]) % G_out if c["parent"] is None else c["parent"]
        live = (par >= 0) & (par < G_in) & (c["item"] >= FIRST) & (c["item"] < c["V"])
        src = np.arange(c["N_out"]) // G_out * G_in + np.where(live, par, 0)
        assert {1, 2, L - 1, L} <= set(np.clip(c["len"][src[live]], 1, L).tolist())
        assert (~live).sum() == (5 if use_parent else 3)
        dead = np.flatnonzero(~live)
        assert (want["path"][dead] == -1).all() and np.isneginf(want["path_logp"][dead]).all()
        assert all(np.array_equal(want["tokens"][n], c["tokens"][n // G_out * G_in]) for n in dead)   # a dead row never writes its item
    # without source paths: the path is -1 / -inf outside column t
    c = advance_case(G_in, G_out, 33, 3, 5, 4, use_parent, seed=99)
    rc, outs, _ = run_advance(c, 2, 1, with_paths=False)
    assert rc == 0, _lib.last_error()
    assert_advance(outs, restated_advance(c, 2, 1, with_paths=False))


def test_rollout_advance_refuses_aliased_buffers_and_leaves_them_untouched():
    c = advance_case(3, 3, 4, 1, 5, 4, True, seed=1)
    keep = {k: dev(c[k]) for k in ADV_IN}
    outs = advance_outs(c)
    outs["tokens"] = keep["tokens"]
    rc, _, _ = run_advance(c, 0, 0, outs=outs, keep=keep)
    assert rc == -1 and "alias" in _lib.last_error()
    assert np.array_equal(keep["tokens"].cpu().numpy(), c["tokens"]) and (outs["mask"] == -7).all() and (outs["exclude"] == -7).all()


# ---- graph capture, reproducibility -----------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_bits():
    beam, ids, logp = planted_beams(2, 8, 64, seed=3)
    c = advance_case(4, 2, 33, 3, 5, 4, True, seed=7)
    rc, eager_sel, _ = run_select(beam, ids, logp, 8)
    assert rc == 0
    rc, again_sel, _ = run_select(beam, ids, logp, 8)
    rc2, eager_adv, _ = run_advance(c, 3, 4)
    rc3, again_adv, _ = run_advance(c, 3, 4)
    assert rc == 0 and rc2 == 0 and rc3 == 0
    assert all(torch.equal(bits(eager_sel[k]), bits(again_sel[k])) for k in SELECT_OUTS)      # two eager runs: the same bits
    assert all(torch.equal(bits(eager_adv[k]), bits(again_adv[k])) for k in ADV_OUT)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        s_keep, s_outs = [dev(beam), dev(ids), dev(logp)], select_outs(2, 8)   # allocations and copies outside the capture
        a_keep, a_outs = {k: dev(c[k]) for k in ADV_IN}, advance_outs(c)
        torch.cuda.synchronize()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            rc, _, _ = run_select(beam, ids, logp, 8, outs=s_outs, keep=s_keep, sync=False)
            assert rc == 0
            rc, _, _ = run_advance(c, 3, 4, outs=a_outs, keep=a_keep, sync=False)
            assert rc == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert (s_outs["item"] == -7).all() and (a_outs["tokens"] == -7).all(), "a capture must not run the kernels"
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(bits(eager_sel[k]), bits(s_outs[k])) for k in SELECT_OUTS)
    assert all(torch.equal(bits(eager_adv[k]), bits(a_outs[k])) for k in ADV_OUT)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
L_MODEL, P_MODEL = 24, 6
HISTORY_LENGTHS = (3, 21, 22, 23, 30, 1, 24, 12)
HIGH_SEED = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def setting():
    dl = make_loader()
    dl.generate_vocab()
    V = dl.get_tokenizer().get_vocab_size()
    model = make_model(V, L=L_MODEL, seed=11)
    items = dl.create_item_list()
    histories = [items[37 * i:37 * i + n] for i, n in enumerate(HISTORY_LENGTHS)]
    parts = [dl.prepare_inference(list(h)) for h in histories]
    batch = {k: torch.from_numpy(np.concatenate([np.asarray(p[k]) for p in parts], axis=0)) for k in parts[0]}
    return dl, model, V, histories, batch


def host_batch(tokens, mask, positions):
    w = np.zeros_like(positions)
    w[:, 0] = 1
    return {"input_word_ids": torch.from_numpy(tokens), "input_mask": torch.from_numpy(mask), "masked_lm_positions": torch.from_numpy(positions),
            "masked_lm_weights": torch.from_numpy(w)}


def host_rollout(model, V, batch, steps, beams=1, expand=None, allow=None, row_filter=None, temperature=1.0, seed=None, streams=None):
    """The roll-out as a host loop: recommend_tensor on the rows, the restatements of the select and the advance in numpy, every step
    read back.  Returns (ids [U, beams, steps], step_logp, logp) as numpy arrays."""
    tokens, mask = batch["input_word_ids"].numpy(), batch["input_mask"].numpy()
    positions = batch["masked_lm_positions"].numpy()
    U = tokens.shape[0]
    length = mask.sum(axis=1).astype(np.int32)
    ex = np.concatenate([tokens, np.full((U, steps), -1, np.int64)], axis=1)
    E0 = tokens.shape[1]
    path = path_logp = None
    beam_logp = np.zeros((U, 1), F32)
    rf = row_filter
    for t in range(steps):
        b = host_batch(tokens, mask, positions) if t else batch
        kw = dict(exclude_seen=False, exclude=torch.from_numpy(ex), allow=allow, row_filter=rf, return_distribution=True, temperature=temperature)
        if beams > 1:
            K = max(expand, beams) if t == 0 else expand
            ids, _, _, dist = model.recommend_tensor(b, k=K, **kw)
            parent, item, beam_logp, step = rr.beam_select(beam_logp, ids.cpu().numpy(), dist["logp"].cpu().numpy(), beams)
            out = rr.advance(tokens, length, ex, path, path_logp, parent.reshape(-1), item.reshape(-1), step.reshape(-1), 1 if t == 0 else beams,
                             beams, P_MODEL, steps, V, FIRST, MASK, t, E0 + t)
            if t == 0 and rf is not None:
                rf = torch.as_tensor(rf).repeat_interleave(beams)
        else:
            if seed is not None:
                kw.update(sample_seed=(seed + t) % (1 << 64), sample_streams=streams)
            ids, _, _, dist = model.recommend_tensor(b, k=1, **kw)
            item, step = ids.cpu().numpy()[:, 0], dist["logp"].cpu().numpy()[:, 0]
            out = rr.advance(tokens, length, ex, None, None, None, item, None, 1, 1, P_MODEL, steps, V, FIRST, MASK, t, E0 + t)
            # (the restated dead row forgets its path: a greedy path keeps what it had, so it is collected here)
            path = np.full((U, steps), -1, np.int64) if path is None else path
            path_logp = np.full((U, steps), NINF, F32) if path_logp is None else path_logp
            path[:, t], path_logp[:, t] = item, step
        tokens, mask, positions, length, ex = out["tokens"], out["mask"], out["positions"], out["len"], out["exclude"]
        if beams > 1:
            path, path_logp = out["path"], out["path_logp"]
    if beams == 1:
        total = path_logp[:, 0].copy()
        for t in range(1, steps):
            total = (total + path_logp[:, t]).astype(F32)
        beam_logp = total[:, None]
    return path.reshape(U, beams, steps), path_logp.reshape(U, beams, steps), beam_logp


def same(t, a):
    got = t.cpu().numpy()
    return got.shape == a.shape and got.dtype == a.dtype and got.tobytes() == a.tobytes()


def test_greedy_rollout_equals_the_host_loop():
    dl, model, V, histories, batch = setting()
    ids, step_logp, logp, slots = model.recommend_sequence_tensor(batch, steps=3)
    w_ids, w_step, w_logp = host_rollout(model, V, batch, 3)
    assert same(ids, w_ids) and same(step_logp, w_step) and same(logp, w_logp)
    assert slots.tolist() == [u * P_MODEL for u in range(len(histories))]
    assert (ids >= FIRST).all() and torch.isfinite(step_logp).all()
    window = batch["input_word_ids"].tolist()
    for u, row in enumerate(ids[:, 0].tolist()):
        assert len(set(row)) == 3 and not set(row) & set(window[u])           # also the items that slid out of the window since
    # return_logp=False: the same ids, no distribution sweep
    plain = model.recommend_sequence_tensor(batch, steps=3, return_logp=False)
    assert torch.equal(plain[0], ids) and plain[1] is None and plain[2] is None
    # the step is recommend_tensor's top 1
    first = model.recommend_tensor(batch, k=1)[0]
    assert torch.equal(first[:, 0], ids[:, 0, 0])
    lists = model.recommend_sequence(batch, steps=3)
    assert [row[0][0] for row in lists] == ids[:, 0].tolist() and [row[0][1] for row in lists] == logp[:, 0].tolist()
    with pytest.raises(ValueError, match="prepare_inference"):
        bad = dict(batch)
        bad["masked_lm_weights"] = torch.ones_like(batch["masked_lm_weights"])
        model.recommend_sequence_tensor(bad, steps=2)


def test_greedy_rollout_honours_filters_at_every_step():
    dl, model, V, histories, batch = setting()
    rng = np.random.default_rng(3)
    allow = torch.as_tensor(rng.random(V) < 0.7)
    ids, step_logp, logp, _ = model.recommend_sequence_tensor(batch, steps=3, allow=allow)
    w_ids, w_step, w_logp = host_rollout(model, V, batch, 3, allow=allow)
    assert same(ids, w_ids) and same(step_logp, w_step) and same(logp, w_logp)
    assert allow[ids.cpu().reshape(-1)].all()
    # per-user filters: user 2 may be served two items only, and runs out at the third step
    U = len(histories)
    window = set(batch["input_word_ids"][2].tolist())
    two = [i for i in range(FIRST, V) if i not in window][:2]
    masks = torch.zeros((2, V), dtype=torch.bool)
    masks[0] = allow
    masks[1, two] = True
    rf = torch.zeros(U, dtype=torch.int32)
    rf[2] = 1
    ids2, step2, logp2, _ = model.recommend_sequence_tensor(batch, steps=3, allow=masks, row_filter=rf)
    row = ids2[2, 0].tolist()
    assert sorted(row[:2]) == two and row[2] == -1
    assert torch.isfinite(step2[2, 0, :2]).all() and step2[2, 0, 2] == float("-inf") and logp2[2, 0] == float("-inf")
    others = [u for u in range(U) if u != 2]
    assert torch.equal(ids2[others], ids[others]) and torch.equal(bits(step2[others]), bits(step_logp[others]))
    w_ids, w_step, w_logp = host_rollout(model, V, batch, 3, allow=masks, row_filter=rf)
    assert same(ids2, w_ids) and same(step2, w_step) and same(logp2, w_logp)


def test_beam_rollout_equals_the_host_loop():
    dl, model, V, histories, batch = setting()
    ids, step_logp, logp, _ = model.recommend_sequence_tensor(batch, steps=3, beams=3, expand=4)
    w_ids, w_step, w_logp = host_rollout(model, V, batch, 3, beams=3, expand=4)
    assert same(ids, w_ids) and same(step_logp, w_step) and same(logp, w_logp)
    assert (ids >= FIRST).all()
    total = step_logp[:, :, 0].clone()
    for t in range(1, 3):
        total = total + step_logp[:, :, t]
    assert torch.equal(bits(total), bits(logp))                             # the sequential fp32 sum of the steps
    assert (logp[:, 1:] <= logp[:, :-1]).all()                               # best first
    paths = ids.cpu().tolist()
    window = batch["input_word_ids"].tolist()
    for u in range(len(histories)):
        assert len({tuple(p) for p in paths[u]}) == 3
        assert all(len(set(p)) == 3 and not set(p) & set(window[u]) for p in paths[u])
    # a temperature reshapes the log probabilities the search ranks by
    warm = model.recommend_sequence_tensor(batch, steps=3, beams=3, expand=4, temperature=3.0, return_logp=False)
    w_ids, _, w_logp = host_rollout(model, V, batch, 3, beams=3, expand=4, temperature=3.0)
    assert same(warm[0], w_ids) and warm[1] is None and same(warm[2], w_logp)
    # one beam of one candidate is the greedy path
    greedy = model.recommend_sequence_tensor(batch, steps=3)
    one = model.recommend_sequence_tensor(batch, steps=3, beams=1, expand=1)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(greedy, one))
    # the best beam is at least as probable as the greedy path
    assert (logp[:, 0] >= greedy[2][:, 0]).all()


def test_beam_rollout_with_too_few_items_drops_whole_beams():
    dl, model, V, histories, batch = setting()
    U = len(histories)
    window = set(batch["input_word_ids"][1].tolist())
    three = [i for i in range(FIRST, V) if i not in window][:3]
    masks = torch.zeros((2, V), dtype=torch.bool)
    masks[0] = True
    masks[1, three] = True
    rf = torch.zeros(U, dtype=torch.int32)
    rf[1] = 1
    # 3 items: 6 ordered paths of 2 steps, of which the 4 beams keep 4; each has one item left for a third step; a fourth has none
    for steps, n_paths in ((2, 4), (3, 4), (4, 0)):
        ids, step_logp, logp, _ = model.recommend_sequence_tensor(batch, steps=steps, beams=4, expand=4, allow=masks, row_filter=rf)
        w_ids, w_step, w_logp = host_rollout(model, V, batch, steps, beams=4, expand=4, allow=masks, row_filter=rf)
        assert same(ids, w_ids) and same(step_logp, w_step) and same(logp, w_logp)
        row = ids[1].cpu().tolist()
        assert all(set(p) <= set(three) and len(set(p)) == steps for p in row[:n_paths])
        assert all(p == [-1] * steps for p in row[n_paths:]) and torch.isneginf(logp[1, n_paths:]).all()
        assert (ids[[0, 2, 3]] >= FIRST).all()


def test_sampled_rollout_equals_the_host_loop_and_follows_the_user():
    dl, model, V, histories, batch = setting()
    U = len(histories)
    streams = torch.as_tensor([(1 << 40) + 5, -3, 17, 0, 99, 4, -(1 << 62), 8], dtype=torch.int64)
    ids, step_logp, logp, _ = model.recommend_sequence_tensor(batch, steps=3, sample_seed=HIGH_SEED, sample_streams=streams, temperature=0.5)
    w_ids, w_step, w_logp = host_rollout(model, V, batch, 3, seed=HIGH_SEED, streams=streams, temperature=0.5)   # the seed wraps at step 1
    assert same(ids, w_ids) and same(step_logp, w_step) and same(logp, w_logp)
    assert (ids >= FIRST).all() and all(len(set(p)) == 3 for p in ids[:, 0].tolist())
    again = model.recommend_sequence_tensor(batch, steps=3, sample_seed=HIGH_SEED, sample_streams=streams, temperature=0.5)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((ids, step_logp, logp), again))
    other = model.recommend_sequence_tensor(batch, steps=3, sample_seed=5, sample_streams=streams, temperature=0.5)[0]
    assert (other != ids).any()
    # the same user with the same stream rolls out the same path in a batch of 3
    pick = [6, 0, 4]
    small = {k: v[pick] for k, v in batch.items()}
    ids3, step3, _, _ = model.recommend_sequence_tensor(small, steps=3, sample_seed=HIGH_SEED, sample_streams=streams[pick], temperature=0.5)
    assert torch.equal(ids3, ids[pick]) and torch.equal(bits(step3), bits(step_logp[pick]))
    # without streams the stream is the row number
    default = model.recommend_sequence_tensor(batch, steps=2, sample_seed=9)
    numbered = model.recommend_sequence_tensor(batch, steps=2, sample_seed=9, sample_streams=torch.arange(U))
    assert torch.equal(default[0], numbered[0])


# ---- the app ------------------------------------------------------------------------------------------------------------------------
def test_recommender_returns_the_detokenised_paths():
    dl, model, V, histories, batch = setting()
    tok = dl.get_tokenizer()
    rec = Recommender(model, dl)
    seen = [tok.tokenize(list(h)) for h in histories]
    width = max(len(s) for s in seen)
    exclude = torch.full((len(seen), width), -1, dtype=torch.int64)
    for i, s in enumerate(seen):
        exclude[i, :len(s)] = torch.as_tensor(s)
    ids, step_logp, logp, _ = model.recommend_sequence_tensor(batch, steps=3, exclude_seen=False, exclude=exclude)
    got = rec.recommend_sequences(histories, steps=3)
    assert got == [tok.detokenize(row) for row in ids[:, 0].tolist()]
    assert all(not set(path) & set(h) for path, h in zip(got, histories))    # also the items before the model's window
    pairs = rec.recommend_sequences(histories, steps=3, return_probabilities=True)
    assert [[item for item, _ in row] for row in pairs] == got
    want_p = torch.exp(step_logp[:, 0].to(torch.float64)).tolist()
    assert [[p for _, p in row] for row in pairs] == want_p and all(0.0 < p <= 1.0 for row in pairs for _, p in row)
    ids2, _, logp2, _ = model.recommend_sequence_tensor(batch, steps=3, beams=2, exclude_seen=False, exclude=exclude)
    beams = rec.recommend_sequences(histories, steps=3, beams=2)
    assert [[items for items, _ in row] for row in beams] == [[tok.detokenize(p) for p in row] for row in ids2.tolist()]
    assert [[lp for _, lp in row] for row in beams] == logp2.to(torch.float64).tolist()
    # allow-lists per user; a user with two allowed items gets a list of two
    catalogue = tok.detokenize(list(range(FIRST, V)))
    free = [x for x in catalogue if x not in set(histories[3])]
    per_user = [free[:40]] * len(histories)
    per_user[3] = free[5:7]
    limited = rec.recommend_sequences(histories, steps=3, allowed_items_per_user=per_user)
    assert sorted(limited[3], key=str) == sorted(free[5:7], key=str)
    assert all(len(path) == 3 and set(path) <= set(free[:40]) for u, path in enumerate(limited) if u != 3)
    limited_beams = rec.recommend_sequences(histories, steps=3, beams=2, allowed_items_per_user=per_user)
    assert limited_beams[3] == [] and all(len(row) == 2 for u, row in enumerate(limited_beams) if u != 3)
    # sampled paths follow the user's stream
    users = [5, 1 << 40, -2, 9, 3, 77, 12, 0]
    drawn = rec.recommend_sequences(histories, steps=3, sample_seed=4, user_streams=users)
    order = [4, 1, 7]
    moved = rec.recommend_sequences([histories[i] for i in order], steps=3, sample_seed=4, user_streams=[users[i] for i in order])
    assert moved == [drawn[i] for i in order] and drawn != got
    assert rec.recommend_sequences([], steps=3) == []
