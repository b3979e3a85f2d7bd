"""Occlusion explanations on the GPU: b4r_occlude_rows and b4r_attribution_select bit for bit against tests/explain_ref.py, graph
capture, and explain_tensor / Recommender.explain_batch against host loops that build every occluded batch with prepare_inference."""
import functools

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, config, models
from bert4rec_amd.apps import Recommender
from bert4rec_amd.models.components import networks
from tests import explain_ref as er
from tests.b4r_testlib import P, stream
from tests.test_explain_host import planted_attribution
from tests.test_gpu_api import make_loader, make_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
NINF = F32(-np.inf)
FIRST, MASK = 3, 1


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(t, a):
    got = t.cpu().numpy()
    return got.shape == a.shape and got.dtype == a.dtype and got.tobytes() == a.tobytes()


# ---- b4r_occlude_rows -----------------------------------------------------------------------------------------------------------------
OCC_OUT = ("tokens", "mask", "len", "positions", "live", "unit_pos", "unit_item", "unit_label", "removed")
OCC_I64 = ("tokens", "mask", "positions", "unit_item")


def occlude_case(L, U, mode, seed):
    """Rows of length 1, 2, L - 1, L (and 0 / L + 3, which are clamped) in one batch, ids outside [0, V) among the tokens, and the labels
    of the mode: None (item mode), one label for all, three labels and -1, one label per item and -1."""
    V = 500
    rng = np.random.default_rng(seed)
    tokens = rng.integers(3, V, size=(U, L)).astype(np.int64)
    wild = rng.random((U, L)) < 0.1
    tokens[wild] = rng.choice(np.asarray([V, V + 9, -1, -(1 << 40), 1 << 40, (1 << 31) + 5, 0, 2], np.int64), size=int(wild.sum()))
    tokens[0, 0] = 5                                                         # row 0 is full and starts with an item of the catalogue
    lens = np.asarray([L, 1, 2, L - 1, 0, L + 3], np.int32)[np.arange(U) % 6]
    if mode == "item":
        labels = None
    elif mode == "one":
        labels = np.zeros(V, np.int32)
    elif mode == "three":
        labels = rng.integers(-1, 3, size=V).astype(np.int32)
        labels[5] = 1
        tokens[0, ::3] = tokens[0, 0]                                        # duplicate items
    else:
        labels = rng.permutation(V).astype(np.int32) * 1000                  # labels are values, not indices
        labels[rng.random(V) < 0.2] = -1
        labels[7], labels[5] = -5, 123000                                    # any negative label is no group
    return tokens, lens, labels, V


def occlude_outs(N, L, Pn):
    return {k: torch.full({"tokens": (N, L), "mask": (N, L), "positions": (N, Pn)}.get(k, (N,)), -7,
                          dtype=torch.int64 if k in OCC_I64 else torch.int32, device=DEV) for k in OCC_OUT}


def run_occlude(keep, U, L, Pn, V, w0, Wc, outs=None, null_out=(), sync=True):
    outs = outs or occlude_outs(U * Wc, L, Pn)
    ptr = {k: (None if k in null_out else P(v)) for k, v in outs.items()}
    rc = _lib.load().b4r_occlude_rows(P(keep[0]), P(keep[1]), P(keep[2]), U, L, Pn, V, MASK, w0, Wc, *[ptr[k] for k in OCC_OUT], stream())
    if sync:
        torch.cuda.synchronize()
    return rc, outs


def assert_occlude(outs, want, skip=()):
    for k in OCC_OUT:
        got = outs[k].cpu().numpy()
        if k in skip:
            assert (got == -7).all(), k
        else:
            assert got.dtype == want[k].dtype and got.tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("U", [1, 70])
@pytest.mark.parametrize("mode", ["item", "one", "three", "many"])
@pytest.mark.parametrize("L", [2, 3, 64, 65, 256])
def test_occlude_rows_against_the_restatement(L, mode, U):
    tokens, lens, labels, V = occlude_case(L, U, mode, seed=L + U)
    keep = [dev(tokens), dev(lens), dev(labels)]
    n_live = 0
    for w0, Wc in ((0, 1), (0, 7), (5, 64), (L - 2, 3)):                     # chunks that start inside and run past every history
        for Pn in (1, 6):
            rc, outs = run_occlude(keep, U, L, Pn, V, w0, Wc)
            assert rc == 0, _lib.last_error()
            want = er.occlude_rows(tokens, lens, labels, V, MASK, Pn, w0, Wc)
            assert_occlude(outs, want)
            n_live += int(want["live"].sum())
            assert ((want["len"] >= 1) & (want["len"] <= L)).all()
    assert np.array_equal(keep[0].cpu().numpy(), tokens)                     # the input rows are read only
    assert n_live > 0
    if mode == "one" and L >= 3:                                             # a history removed whole leaves the placeholder alone
        want = er.occlude_rows(tokens, lens, labels, V, MASK, 1, 0, 1)
        whole = [u for u in range(U) if want["live"][u] and want["len"][u] == 1]
        assert whole or U == 1
        assert all(want["tokens"][u].tolist() == [MASK] + [0] * (L - 1) for u in whole)


def test_occlude_rows_null_outputs_and_argument_errors():
    tokens, lens, labels, V = occlude_case(9, 5, "three", seed=2)
    keep = [dev(tokens), dev(lens), dev(labels)]
    want = er.occlude_rows(tokens, lens, labels, V, MASK, 2, 1, 4)
    optional = ("unit_pos", "unit_item", "unit_label", "removed")
    rc, outs = run_occlude(keep, 5, 9, 2, V, 1, 4, null_out=optional)
    assert rc == 0
    assert_occlude(outs, want, skip=optional)
    for name in ("tokens", "mask", "len", "positions", "live"):
        rc, outs = run_occlude(keep, 5, 9, 2, V, 1, 4, null_out=(name,))
        assert rc == -1
        assert_occlude(outs, want, skip=OCC_OUT)
    outs = occlude_outs(5, 9, 2)
    outs["mask"] = keep[0]                                                   # an output on top of the input rows
    rc, outs = run_occlude(keep, 5, 9, 2, V, 0, 1, outs=outs)
    assert rc == -1 and "overlaps" in _lib.last_error()
    assert np.array_equal(keep[0].cpu().numpy(), tokens) and (outs["tokens"] == -7).all()


# ---- b4r_attribution_select -----------------------------------------------------------------------------------------------------------
def select_outs(U, K, m):
    return dict(w=torch.full((U, K, m), -7, dtype=torch.int32, device=DEV), delta=torch.full((U, K, m), 7.0, device=DEV))


def run_select(keep, U, W, K, m, outs=None, null_out=(), sync=True):
    outs = outs or select_outs(U, K, m)
    rc = _lib.load().b4r_attribution_select(P(keep[0]), P(keep[1]), P(keep[2]), U, W, K, m, None if "w" in null_out else P(outs["w"]),
                                            None if "delta" in null_out else P(outs["delta"]), stream())
    if sync:
        torch.cuda.synchronize()
    return rc, outs


@pytest.mark.parametrize("W,K", [(W, K) for W in (1, 63, 64, 65, 255, 256) for K in (1, 3, 1024) if K < 1024 or W <= 65])
def test_attribution_select_against_the_restatement(W, K):
    """planted_attribution: a coarse grid (exact ties are common), a planted tie between two units, -0.0 against +0.0, NaN and -inf
    among the occluded values, a -inf and a NaN base, a user with some dead units and one with none alive"""
    U = 3
    base, occ, live = planted_attribution(U, W, K, seed=W + K)
    keep = [dev(base), dev(occ), dev(live)]
    want_w, want_d = er.attribution_select(base, occ, live, W)               # the first m of the full order, for every m
    for m in sorted({1, min(2, W), W}):
        rc, outs = run_select(keep, U, W, K, m)
        assert rc == 0, _lib.last_error()
        assert same(outs["w"], np.ascontiguousarray(want_w[:, :, :m])) and same(outs["delta"], np.ascontiguousarray(want_d[:, :, :m])), m
    assert (want_w[U - 1] == -1).all() and np.isneginf(want_d[U - 1]).all()  # no live unit
    if W >= 2:
        assert want_w[0, 0, :2].tolist() == [0, 1] or want_d[0, 0, 0] > F32(0.75)   # the planted tie: the lower w first
    if W >= 4:
        at = want_w[0, K - 1].tolist()
        assert at.index(2) + 1 == at.index(3) and np.signbit(want_d[0, K - 1, at.index(2)]) and not np.signbit(want_d[0, K - 1, at.index(3)])
    if K >= 4:
        assert (want_w[0, 1:3] == -1).all()
    dead_some = live.reshape(U, W)[1] == 0
    assert not set(want_w[1].reshape(-1).tolist()) & set(np.flatnonzero(dead_some).tolist())


def test_attribution_select_null_outputs_and_argument_errors():
    base, occ, live = planted_attribution(3, 9, 4, seed=1)
    keep = [dev(base), dev(occ), dev(live)]
    want = er.attribution_select(base, occ, live, 3)
    for name, other, w in (("w", "delta", want[1]), ("delta", "w", want[0])):
        rc, outs = run_select(keep, 3, 9, 4, 3, null_out=(name,))
        assert rc == 0 and same(outs[other], w) and (outs[name] == (-7 if name == "w" else 7.0)).all()
    for m in (0, 10):
        rc, outs = run_select(keep, 3, 9, 4, m, outs=select_outs(3, 4, 3))
        assert rc == -2 and (outs["w"] == -7).all() and (outs["delta"] == 7.0).all()


# ---- graph capture, reproducibility -----------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_bits():
    tokens, lens, labels, V = occlude_case(65, 70, "three", seed=4)
    base, occ, live = planted_attribution(3, 65, 17, seed=6)
    o_keep, s_keep = [dev(tokens), dev(lens), dev(labels)], [dev(base), dev(occ), dev(live)]
    rc, eager_occ = run_occlude(o_keep, 70, 65, 6, V, 5, 7)
    rc2, again_occ = run_occlude(o_keep, 70, 65, 6, V, 5, 7)
    rc3, eager_sel = run_select(s_keep, 3, 65, 17, 5)
    rc4, again_sel = run_select(s_keep, 3, 65, 17, 5)
    assert rc == 0 and rc2 == 0 and rc3 == 0 and rc4 == 0
    assert all(torch.equal(eager_occ[k], again_occ[k]) for k in OCC_OUT)     # two eager runs: the same bits
    assert all(torch.equal(bits(eager_sel[k]), bits(again_sel[k])) for k in ("w", "delta"))
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        o_outs, s_outs = occlude_outs(70 * 7, 65, 6), select_outs(3, 17, 5)   # allocations outside the capture
        torch.cuda.synchronize()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            rc, _ = run_occlude(o_keep, 70, 65, 6, V, 5, 7, outs=o_outs, sync=False)
            assert rc == 0
            rc, _ = run_select(s_keep, 3, 65, 17, 5, outs=s_outs, sync=False)
            assert rc == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert (o_outs["tokens"] == -7).all() and (s_outs["w"] == -7).all(), "a capture must not run the kernels"
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(eager_occ[k], o_outs[k]) for k in OCC_OUT)
    assert all(torch.equal(bits(eager_sel[k]), bits(s_outs[k])) for k in ("w", "delta"))


# ---- the model ------------------------------------------------------------------------------------------------------------------------
L_MODEL, P_MODEL = 24, 6
HISTORY_LENGTHS = (1, 2, 5, 23, 30, 12, 0)
K_MODEL = 3


@functools.lru_cache(maxsize=None)
def setting(hidden=64):
    dl = make_loader()
    dl.generate_vocab()
    V = dl.get_tokenizer().get_vocab_size()
    if hidden == 64:
        model = make_model(V, L=L_MODEL, seed=11)
    else:
        cfgd = {**config.get_encoder_config("ml-1m_128"), "max_sequence_length": L_MODEL, "output_dropout": 0.0, "attention_dropout": 0.0}
        model = models.BERT4RecModel(networks.Bert4RecEncoder(V, seed=12, **cfgd))
    items = dl.create_item_list()
    histories = [items[37 * i:37 * i + n] for i, n in enumerate(HISTORY_LENGTHS)]
    batch = prepared(dl, histories)
    target = model.recommend_tensor(batch, k=K_MODEL)[0].cpu()
    target[2, 1] = -1                                                        # an entry without an item comes back dead
    return dl, model, V, histories, batch, target


def prepared(dl, histories):
    parts = [dl.prepare_inference(list(h)) for h in histories]
    return {k: torch.from_numpy(np.concatenate([np.asarray(p[k]) for p in parts], axis=0)) for k in parts[0]}


def group_labels(V):
    labels = (np.arange(V) % 5).astype(np.int32)
    labels[::7] = -1
    return labels


@functools.lru_cache(maxsize=None)
def host_explain(hidden=64, grouped=False, filtered=False, window=None, temperature=1.0):
    """The explanation as the loop a user would write: for every recency index one prepare_inference batch of every user's window
    without that unit (users without it keep their row), one score_distribution_tensor call each, everything read back; then the
    restated selection.  Returns numpy arrays under explain_tensor's names (top = 2)."""
    dl, model, V, histories, batch, target = setting(hidden)
    tok = dl.get_tokenizer()
    labels = group_labels(V) if grouped else None
    allow = allow_mask(V) if filtered else None
    B, K, W = len(histories), target.shape[1], window or L_MODEL - 1
    kw = dict(query_ids=target, exclude_seen=False, exclude=batch["input_word_ids"], allow=allow, temperature=temperature)
    out = dict(base_logp=model.score_distribution_tensor(batch, **kw)["logp"].cpu().numpy(), occluded_logp=np.full((B, W, K), NINF, F32),
               live=np.zeros((B, W), np.int32), unit_pos=np.full((B, W), -1, np.int32), unit_item=np.full((B, W), -1, np.int64),
               unit_label=np.full((B, W), -1, np.int32), removed=np.zeros((B, W), np.int32))
    windows = [list(h[-(L_MODEL - 1):]) for h in histories]
    for w in range(W):
        rows = []
        for u, win in enumerate(windows):
            p = len(win) - 1 - w
            ids = tok.tokenize(win) if win else []
            lab = [int(labels[t]) for t in ids] if grouped else [-1] * len(ids)
            live = p >= 0 and (not grouped or (lab[p] >= 0 and lab[p] not in lab[p + 1:]))
            if not live:
                rows.append(win)
                continue
            rest = [x for q, x in enumerate(win) if (lab[q] != lab[p] if grouped else q != p)]
            rows.append(rest)
            out["live"][u, w], out["unit_pos"][u, w], out["unit_item"][u, w] = 1, p, ids[p]
            out["unit_label"][u, w], out["removed"][u, w] = lab[p], len(win) - len(rest)
        lp = model.score_distribution_tensor(prepared(dl, rows), **kw)["logp"].cpu().numpy()
        out["occluded_logp"][:, w] = np.where(out["live"][:, w, None] != 0, lp, NINF)
    top_w, top_delta = er.attribution_select(out["base_logp"], out["occluded_logp"].reshape(B * W, K), out["live"].reshape(-1), 2)
    at = np.maximum(top_w, 0).reshape(B, -1)
    for name, src, dt in (("top_pos", "unit_pos", np.int32), ("top_item", "unit_item", np.int64), ("top_label", "unit_label", np.int64)):
        out[name] = np.where(top_w < 0, -1, np.take_along_axis(out[src], at, axis=1).reshape(top_w.shape)).astype(dt)
    out.update(top_w=top_w, top_delta=top_delta, target_ids=target.numpy())
    return out


def allow_mask(V):
    return torch.as_tensor(np.random.default_rng(3).random(V) < 0.7)


NAMES = ("target_ids", "base_logp", "occluded_logp", "live", "unit_pos", "unit_item", "unit_label", "removed", "top_w", "top_pos", "top_item",
         "top_label", "top_delta")


def assert_explained(got, want):
    for name in NAMES:
        assert same(got[name], want[name]), name


@pytest.mark.parametrize("hidden,grouped,filtered,window", [(64, False, False, None), (128, False, False, None), (64, False, True, None),
                                                            (64, False, False, 2), (64, True, False, None), (64, True, True, 5)])
def test_explain_tensor_equals_the_host_loop_whatever_the_chunks(hidden, grouped, filtered, window):
    dl, model, V, histories, batch, target = setting(hidden)
    want = host_explain(hidden, grouped, filtered, window)
    B = len(histories)
    kw = dict(top=2, labels=torch.from_numpy(group_labels(V)) if grouped else None, window=window, allow=allow_mask(V) if filtered else None)
    for rows in (B, 1, 3 * B + 1, 1024):
        got = model.explain_tensor(batch, target, rows_per_forward=rows, **kw)
        assert_explained(got, want)
        assert got["slot_index"].tolist() == [u * P_MODEL for u in range(B)]
    W = window or L_MODEL - 1
    seen = [min(len(h), L_MODEL - 1) for h in histories]
    if not grouped:
        assert want["live"].sum(axis=1).tolist() == [min(n, W) for n in seen]
    else:
        assert (want["live"].sum(axis=1) <= 5).all() and want["removed"].max() > 1 and (want["removed"].sum(axis=1) <= np.asarray(seen)).all()
    # the support is fixed: a finite base has finite occluded log probabilities on every live unit, and a dead target is dead throughout
    finite = np.isfinite(want["base_logp"])
    assert (np.isfinite(want["occluded_logp"]) == (finite[:, None, :] & (want["live"][:, :, None] != 0))).all()
    assert not finite[2, 1] and (want["top_w"][2, 1] == -1).all() and (filtered or finite[:, 0].all())
    assert (want["top_w"][6] == -1).all() and np.isneginf(want["top_delta"][6]).all()      # the empty history has no unit
    deltas = want["top_delta"][np.isfinite(want["top_delta"])]
    assert (deltas != 0).any()


def test_explain_tensor_follows_the_user_and_repeats_its_bits():
    dl, model, V, histories, batch, target = setting()
    full = model.explain_tensor(batch, target, top=3, temperature=0.5)
    again = model.explain_tensor(batch, target, top=3, temperature=0.5)
    assert all(torch.equal(bits(full[name]), bits(again[name])) for name in NAMES)
    cold = model.explain_tensor(batch, target, top=3)
    assert not torch.equal(bits(cold["base_logp"]), bits(full["base_logp"]))
    # short histories alone: the chunks past the longest history are skipped, the bits stay
    pick = [2, 0, 6]
    small = model.explain_tensor({k: v[pick] for k, v in batch.items()}, target[pick], top=3, temperature=0.5, rows_per_forward=6)
    for name in NAMES:
        assert torch.equal(bits(small[name]), bits(full[name][pick])), name
    # an integer instead of ids: the row's own top k, from the same base forward
    own = model.explain_tensor(batch, K_MODEL, top=3)
    ids, _, _, dist = model.recommend_tensor(batch, k=K_MODEL, return_distribution=True)
    assert torch.equal(own["target_ids"], ids) and torch.equal(bits(own["base_logp"]), bits(dist["logp"]))
    lists = model.explain(batch, target, top=3)
    assert [[e[0] for e in row] for row in lists] == target.tolist() and lists[6][0][2] == [] and len(lists[3][0][2]) == 3
    assert [r[3] for r in lists[3][0][2]] == cold["top_delta"][3, 0].tolist()
    with pytest.raises(ValueError, match="prepare_inference"):
        bad = dict(batch)
        bad["masked_lm_weights"] = torch.ones_like(batch["masked_lm_weights"])
        model.explain_tensor(bad, target)


# ---- the app ------------------------------------------------------------------------------------------------------------------------
def test_recommender_explains_its_own_recommendations():
    dl, model, V, histories, batch, target = setting()
    tok = dl.get_tokenizer()
    rec = Recommender(model, dl)
    served = rec.recommend_batch(histories, k=3, return_probabilities=True)
    got = rec.explain_batch(histories, k=3, top=2)
    assert [[(item, p) for item, p, _ in row] for row in got] == served       # the same items with the same probabilities
    assert got[6][0][2] == [] and all(len(reasons) == 2 for _, _, reasons in got[3])
    for u, row in enumerate(got):
        for _, _, reasons in row:
            assert all(h in histories[u] for h, _ in reasons) and [d for _, d in reasons] == sorted((d for _, d in reasons), reverse=True)
    alone = rec.explain(histories[4], k=3, top=2)
    assert alone == got[4]                                                   # one user of many gets the same reasons as alone
    named = rec.explain_batch(histories, items=[[item for item, _, _ in row][:2] + ["no such item"] for row in got], top=2)
    assert [row[:2] for row in named] == [row[:2] for row in got] and all(row[2] == ("no such item", 0.0, []) for row in named)
    # by category: every label once, with the number of history items it stands for
    catalogue = tok.detokenize(list(range(FIRST, V)))
    genre = {item: "genre %d" % (i % 4) for i, item in enumerate(catalogue) if i % 9}
    grouped = rec.explain_batch(histories, k=2, top=4, by_group=genre)
    assert [[(item, p) for item, p, _ in row] for row in grouped] == [row[:2] for row in served]
    for u, row in enumerate(grouped):
        window = list(histories[u][-(L_MODEL - 1):])
        for _, _, reasons in row:
            labels = [label for label, _, _ in reasons]
            assert len(set(labels)) == len(labels) and set(labels) == {genre[h] for h in window if h in genre}
            assert all(n == sum(genre.get(h) == label for h in window) for label, _, n in reasons)
    by_id = np.full(V, -1, np.int64)
    for i, item in enumerate(catalogue):
        if item in genre:
            by_id[FIRST + i] = int(genre[item][-1]) + 10
    numbered = rec.explain_batch(histories, k=2, top=4, by_group=by_id)
    assert [[[(int(label[-1]) + 10, d, n) for label, d, n in reasons] for _, _, reasons in row] for row in grouped] == \
        [[reasons for _, _, reasons in row] for row in numbered]
    # allow-lists: the explained items are recommend_batch's under the same lists
    free = [x for x in catalogue if x not in set(histories[3])]
    per_user = [free[:40]] * len(histories)
    per_user[3] = free[5:7]
    limited = rec.explain_batch(histories, k=3, top=2, allowed_items_per_user=per_user, window=4)
    assert [[(item, p) for item, p, _ in row] for row in limited] == \
        rec.recommend_batch(histories, k=3, return_probabilities=True, allowed_items_per_user=per_user)
    assert len(limited[3]) == 2 and all(h in histories[3][-4:] for _, _, reasons in limited[3] for h, _ in reasons)
