"""Category affinity on the GPU (b4r_group_mass): the op against the CPU restatement (tests/group_mass_ref.py) and the model / app
layers built on it.

Bit-exact: group_n, rest_n, sum_g group_n + rest_n = b4r_score_dist's row_n, dead rows, two runs, a captured graph, G in one call
against the same labels in two calls over disjoint label ranges, rows in another order, and a singleton group against
b4r_audience_merge's demand of one user.  group_mass / rest_mass: |device - restatement| <= group_n units (group_mass_ref: u has the
same bits on both sides, two exponentials good to 1 ulp move the rounded integer by at most 1); each test prints the largest
difference it saw.  With every allowed item labelled: |sum of the masses - 2^40| <= tol_total(row_n).

The shapes reach the sweep's boundaries: 16 rows per tile (R = 1, 17, 33), 1024 ids per chunk (V = 4, 33, 1027, 2051), the 16-float
k-block (H = 32, 100, 256) and the window of GW = 256 groups (G = 1, 2, 255, 256, 257, 515)."""
import functools

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, config, models
from bert4rec_amd.apps import Recommender
from bert4rec_amd.models.components import networks
from tests import catalogue_ref as ref
from tests import group_mass_ref as gref
from tests import score_dist_ref as sref
from tests.b4r_testlib import P, stream
from tests.test_gpu_api import make_loader, make_model
from tests.test_gpu_full_rank import make_case

pytestmark = pytest.mark.gpu

DEV = "cuda"
FIRST = 3
F32 = np.float32
GW = 256
GS = (1, 2, GW - 1, GW, GW + 1, 2 * GW + 3)
SHAPES = [(1, 32, 4), (17, 100, 33), (33, 256, 1027), (17, 32, 2051), (33, 100, 2051)]


def dev(x, dtype=None):
    if x is None:
        return None
    t = torch.as_tensor(x)
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


@functools.lru_cache(maxsize=None)
def planted(R, H, V):
    """make_case's inputs, three filters (0: a random 85 %, 1: zeros, 2: the even ids) and a row_filter that names them by row:
    r % 5 = 0 no filter (an index outside [0, 3)), 1 / 2 filter 0, 3 the even ids, 4 the filter of zeros: an empty row."""
    hidden, table, bias, ex, _ = make_case(R, H, V, seed=R * 31 + H + V % 97, E=12)
    rng = np.random.default_rng(V + R)
    masks = np.zeros((3, V), bool)
    masks[0] = rng.random(V) < 0.85
    masks[0, V - 1] = True
    masks[2, ::2] = True
    row_filter = np.array([(3, 0, 0, 2, 1)[r % 5] for r in range(R)], np.int32)
    if R > 2:
        row_filter[2] = -1
    scale = (0.5 + np.random.default_rng(V + 1).random(V)).astype(F32)
    return dict(hidden=hidden.numpy().copy(), table=table.numpy().copy(), bias=bias.numpy().copy(), ex=ex, masks=masks,
                words=ref.pack_bits(masks), row_filter=row_filter, scale=scale)


@functools.lru_cache(maxsize=None)
def chain(R, H, V, use_bias):
    c = planted(R, H, V)
    return ref.chain_scores(c["hidden"], c["table"], c["bias"] if use_bias else None)


def labels_of(pattern, V, G, seed=0):
    j = np.arange(V)
    if pattern == "one":
        return np.zeros(V, np.int32)                         # every item in group 0 (G > 1: the other groups hold nothing)
    if pattern == "each":
        return j.astype(np.int32)                            # one group per item; the ids from G on are outside [0, G)
    if pattern == "parity":
        return (j % 2).astype(np.int32)                      # every wave sees both labels (G = 1: the odd ids are outside)
    return np.random.default_rng(seed + V + G).integers(-3, G + 3, size=V).astype(np.int32)   # "mixed": labels < 0 and >= G among them


def device_inputs(c, use_bias=True, use_scale=False, filters=True, hidden=None, hidden_row=None):
    return dict(hidden=dev(c["hidden"] if hidden is None else hidden), table=dev(c["table"]), bias=dev(c["bias"]) if use_bias else None,
                ex=dev(c["ex"]), words=dev(c["words"].view(np.int32)) if filters else None, rf=dev(c["row_filter"]) if filters else None,
                scale=dev(c["scale"]) if use_scale else None, hr=dev(hidden_row, torch.int64))


def run_dist(c, d, inv_t=1.0, hidden_ld=None, R=None):
    """b4r_score_dist (gt = NULL) on the same rows: (row_n, row_lse) on the device"""
    lib = _lib.load()
    R = c["hidden"].shape[0] if R is None else R
    H, V = c["hidden"].shape[1], c["table"].shape[0]
    n = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    lse = torch.full((R,), 7.0, dtype=torch.float64, device=DEV)
    nbytes = int(lib.b4r_score_dist_scratch_bytes(R, V))
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    rc = lib.b4r_score_dist(P(d["hidden"]), hidden_ld or H, P(d["hr"]), P(d["table"]), P(d["bias"]), H, V, FIRST, R, P(d["ex"]),
                            c["ex"].shape[1], None, P(d["words"]), 0 if d["words"] is None else 3, P(d["rf"]), P(d["scale"]), inv_t, None, 0,
                            P(n), None, P(lse), None, None, P(scratch), nbytes, stream())
    assert rc == 0, _lib.last_error()
    return n, lse


def run_mass(c, d, lse_d, lab_d, G, inv_t=1.0, hidden_ld=None, R=None, outs=None, sync=True, want=(True, True, True, True)):
    """b4r_group_mass on the case; the outputs start from sentinels.  Returns (rc, dict of device tensors)."""
    lib = _lib.load()
    R = c["hidden"].shape[0] if R is None else R
    H, V = c["hidden"].shape[1], c["table"].shape[0]
    if outs is None:
        outs = sentinels(c["hidden"].shape[0], G)
    ptr = [P(outs[k]) if w else None for k, w in zip(("mass", "n", "rest_mass", "rest_n"), want)]
    rc = lib.b4r_group_mass(P(d["hidden"]), hidden_ld or H, P(d["hr"]), P(d["table"]), P(d["bias"]), H, V, FIRST, R, P(d["ex"]),
                            c["ex"].shape[1], P(d["words"]), 0 if d["words"] is None else 3, P(d["rf"]), P(d["scale"]), inv_t, P(lse_d),
                            P(lab_d), G, *ptr, stream())
    if sync:
        torch.cuda.synchronize()
    return rc, outs


def sentinels(R, G):
    return dict(mass=torch.full((R, max(G, 1)), -7, dtype=torch.int64, device=DEV), n=torch.full((R, max(G, 1)), -7, dtype=torch.int32, device=DEV),
                rest_mass=torch.full((R,), -7, dtype=torch.int64, device=DEV), rest_n=torch.full((R,), -7, dtype=torch.int32, device=DEV))


def host(outs):
    return {k: v.cpu().numpy() for k, v in outs.items()}


def allowed(c, filters=True, R=None):
    R = c["hidden"].shape[0] if R is None else R
    V = c["table"].shape[0]
    return ref.allowed_mask(V, FIRST, c["ex"][:R], None, R, c["words"] if filters else None, c["row_filter"][:R] if filters else None)


def assert_against(got, want, what):
    """counts exact, masses within one unit per item; returns the largest difference in units"""
    mass, n, rest_mass, rest_n = want
    assert np.array_equal(got["n"][:, :n.shape[1]], n), what
    assert np.array_equal(got["rest_n"], rest_n), what
    gap = np.abs(got["mass"][:, :n.shape[1]] - mass)
    rest_gap = np.abs(got["rest_mass"] - rest_mass)
    assert (gap <= gref.tol_mass(n)).all() and (rest_gap <= gref.tol_mass(rest_n)).all(), (what, int(gap.max()), int(rest_gap.max()))
    return int(max(gap.max(initial=0), rest_gap.max(initial=0)))


# ---- the op against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,H,V", SHAPES)
def test_group_mass_against_the_restatement(R, H, V):
    c = planted(R, H, V)
    d = device_inputs(c)
    n_d, lse_d = run_dist(c, d)
    row_n, lse = n_d.cpu().numpy(), lse_d.cpu().numpy()
    ok = allowed(c)
    assert np.array_equal(row_n, ok.sum(axis=1))
    t = chain(R, H, V, True)                                                 # inv_temperature = 1: t = s
    worst = 0
    for G in GS:
        for pattern in ("one", "each", "parity", "mixed"):
            lab = labels_of(pattern, V, G)
            rc, outs = run_mass(c, d, lse_d, dev(lab), G)
            assert rc == 0, _lib.last_error()
            got = host(outs)
            what = (G, pattern)
            worst = max(worst, assert_against(got, gref.group_mass(t, ok, lse, lab, G), what))
            assert np.array_equal(got["n"].sum(axis=1) + got["rest_n"], row_n), what     # b4r_score_dist's row_n
            empty = row_n == 0
            assert not got["mass"][empty].any() and not got["rest_mass"][empty].any() and (got["mass"] >= 0).all()
            if pattern == "one" and G > 1:
                assert not got["n"][:, 1:].any() and not got["mass"][:, 1:].any()   # groups without an item
            if pattern == "parity" and G >= 2:
                odd_only = c["row_filter"] == 2                              # the even ids: group 1 has no allowed item
                assert not got["n"][odd_only, 1].any() and not got["mass"][odd_only, 1].any()
    print("group_mass R=%d H=%d V=%d: largest |device - restatement| = %d units" % (R, H, V, worst))


@pytest.mark.parametrize("use_bias,use_scale,inv_t,filters,strided", [(False, False, 1.0, True, False), (True, True, 0.7, True, False),
                                                                    (True, False, 2.5, False, False), (False, True, 1.0 / 3.0, True, True)])
def test_group_mass_with_every_input_varied(use_bias, use_scale, inv_t, filters, strided):
    R, H, V = 33, 100, 2051
    c = planted(R, H, V)
    inv_t = float(F32(inv_t))
    hidden = hidden_row = hidden_ld = None
    if strided:                                                              # rows permuted inside a wider buffer
        hidden_ld = H + 12
        hidden_row = np.random.default_rng(3).permutation(R + 4)[:R].astype(np.int64)
        hidden = np.full((R + 4, hidden_ld), np.nan, F32)
        hidden[hidden_row, :H] = c["hidden"]
    d = device_inputs(c, use_bias, use_scale, filters, hidden, hidden_row)
    n_d, lse_d = run_dist(c, d, inv_t, hidden_ld)
    ok = allowed(c, filters)
    t = sref.scaled_scores(c["hidden"], c["table"], c["bias"] if use_bias else None, c["scale"] if use_scale else None, inv_t)
    worst = 0
    for G, pattern in ((2, "parity"), (GW + 1, "mixed"), (2 * GW + 3, "each")):
        lab = labels_of(pattern, V, G, seed=7)
        rc, outs = run_mass(c, d, lse_d, dev(lab), G, inv_t, hidden_ld)
        assert rc == 0, _lib.last_error()
        got = host(outs)
        worst = max(worst, assert_against(got, gref.group_mass(t, ok, lse_d.cpu().numpy(), lab, G), (G, pattern)))
        assert np.array_equal(got["n"].sum(axis=1) + got["rest_n"], n_d.cpu().numpy())
    print("largest |device - restatement| = %d units" % worst)


def test_dead_rows_the_clamp_and_null_outputs():
    R, H, V, G = 17, 32, 2051, 5
    c = planted(R, H, V)
    hidden_row = np.arange(R, dtype=np.int64)
    hidden_row[[3, 16]] = (-1, -(1 << 40))                                   # negative: dead rows
    d = device_inputs(c, hidden_row=hidden_row)
    n_d, lse_d = run_dist(c, device_inputs(c))
    lse = lse_d.cpu().numpy().copy()
    assert np.isneginf(lse[4]) and n_d[4] == 0                               # the empty row: score_dist's own -inf
    lse[5], lse[6] = np.nan, -np.inf
    lse[7] -= 3.0                                                            # too small by 3: the probabilities would sum to e^3
    lse[8] = -1e30                                                           # absurdly small: every exponent is clamped at 0
    lab = labels_of("mixed", V, G)
    t = sref.scaled_scores(c["hidden"], c["table"], c["bias"])
    ok = allowed(c)
    dead = hidden_row < 0
    rc, outs = run_mass(c, d, dev(lse), dev(lab), G)
    assert rc == 0, _lib.last_error()
    got = host(outs)
    worst = assert_against(got, gref.group_mass(t, ok, lse, lab, G, dead=dead), "dead rows")
    for r in (3, 4, 5, 6, 16):
        assert not got["mass"][r].any() and not got["n"][r].any() and got["rest_mass"][r] == 0 and got["rest_n"][r] == 0, r
    assert np.array_equal(got["mass"][8], got["n"][8].astype(np.int64) << 40) and got["rest_mass"][8] == int(got["rest_n"][8]) << 40
    total7 = got["mass"][7].sum() + got["rest_mass"][7]
    assert (1 << 40) < total7 <= int(np.exp(3.0) * 2.0 ** 40 * 1.001)
    print("largest |device - restatement| = %d units" % worst)
    # any output may be NULL: the others keep their bits, the NULL one's buffer its sentinel
    for want in ((True, False, False, False), (False, True, True, False), (False, False, False, True), (False, False, True, True)):
        rc, part = run_mass(c, d, dev(lse), dev(lab), G, want=want)
        assert rc == 0, _lib.last_error()
        for k, w in zip(("mass", "n", "rest_mass", "rest_n"), want):
            assert torch.equal(part[k], outs[k]) if w else bool((part[k] == -7).all()), (want, k)
    rc, none = run_mass(c, d, dev(lse), dev(lab), G, want=(False, False, False, False))
    assert rc == 0 and all(bool((v == -7).all()) for v in none.values())
    rc, none = run_mass(c, d, dev(lse), dev(lab), G, R=0)
    assert rc == 0 and all(bool((v == -7).all()) for v in none.values())
    rc, rest_only = run_mass(c, d, dev(lse), None, 0, want=(False, False, True, True))   # G = 0: everything is the rest
    assert rc == 0 and np.array_equal(rest_only["rest_n"].cpu().numpy(), got["n"].sum(axis=1) + got["rest_n"])
    # refused arguments leave the outputs untouched
    rc, bad = run_mass(c, d, dev(lse), dev(lab), 65537)
    assert rc == -2 and (bad["rest_n"] == -7).all()
    rc, bad = run_mass(c, d, dev(lse), dev(lab), G, inv_t=0.0)
    assert rc == -1 and (bad["mass"] == -7).all() and (bad["rest_n"] == -7).all()


def test_the_masses_of_a_fully_labelled_catalogue_sum_to_one():
    worst = 0.0
    for R, H, V in SHAPES[1:]:
        c = planted(R, H, V)
        d = device_inputs(c)
        n_d, lse_d = run_dist(c, d)
        row_n = n_d.cpu().numpy()
        for G, pattern in ((1, "one"), (2 * GW + 3, "mixed")):
            lab = np.clip(labels_of(pattern, V, G), 0, G - 1).astype(np.int32)  # every item labelled
            rc, outs = run_mass(c, d, lse_d, dev(lab), G)
            assert rc == 0, _lib.last_error()
            got = host(outs)
            live = row_n > 0
            assert not got["rest_n"].any() and not got["rest_mass"].any() and live.any()
            gap = np.abs(got["mass"].sum(axis=1) - float(1 << 40))[live]
            assert (gap <= gref.tol_total(row_n[live])).all(), (R, H, V, G, gap.max())
            worst = max(worst, float((gap / gref.tol_total(row_n[live])).max()))
    print("largest |sum of masses - 2^40| as a share of the bound: %.3f" % worst)


def test_a_singleton_group_holds_the_audience_demand_of_its_item():
    """Identity with the existing kernels, not with libm: group {q} against b4r_audience_merge's demand over b4r_score_dist's query_logp"""
    lib = _lib.load()
    R, H, V = 17, 32, 2051
    c = planted(R, H, V)
    d = device_inputs(c)
    H_, nbytes = H, int(lib.b4r_score_dist_scratch_bytes(R, V))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    for q in (7, 1030, 2050):
        query = torch.full((R, 1), q, dtype=torch.int64, device=DEV)
        lse_d = torch.empty((R,), dtype=torch.float64, device=DEV)
        logp = torch.empty((R, 1), dtype=torch.float32, device=DEV)
        rc = lib.b4r_score_dist(P(d["hidden"]), H_, None, P(d["table"]), P(d["bias"]), H, V, FIRST, R, P(d["ex"]), c["ex"].shape[1], None,
                                P(d["words"]), 3, P(d["rf"]), None, 1.0, P(query), 1, None, None, P(lse_d), None, P(logp), P(scratch), nbytes,
                                stream())
        assert rc == 0, _lib.last_error()
        demand = torch.zeros((R,), dtype=torch.int64, device=DEV)
        for r in range(R):                                                   # one user per merge: demand[r] is that user's term
            users = torch.full((1, 1), -1, dtype=torch.int64, device=DEV)
            best = torch.full((1, 1), -np.inf, dtype=torch.float32, device=DEV)
            assert lib.b4r_audience_merge(P(logp[r:r + 1]), 1, 1, 1, None, r, float("-inf"), 1, P(users), P(best), None,
                                          P(demand[r:r + 1]), stream()) == 0
        lab = np.full(V, -1, np.int32)
        lab[q] = 0
        rc, outs = run_mass(c, d, lse_d, dev(lab), 1)
        assert rc == 0, _lib.last_error()
        assert torch.equal(outs["mass"][:, 0], demand), q
        served = torch.isfinite(logp[:, 0])
        assert torch.equal(outs["n"][:, 0], served.to(torch.int32)) and served.any() and (demand[served] > 0).all()


# ---- reproducibility: runs, a graph, the split of G, the order of the rows ------------------------------------------------------------------
def same_bits(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def test_two_runs_a_graph_the_split_of_g_and_the_row_order_give_the_same_bits():
    R, H, V, G = 33, 100, 2051, 2 * GW + 3
    c = planted(R, H, V)
    d = device_inputs(c)
    n_d, lse_d = run_dist(c, d)
    lab = labels_of("mixed", V, G, seed=5)
    lab_d = dev(lab)
    rc, first = run_mass(c, d, lse_d, lab_d, G)
    rc2, again = run_mass(c, d, lse_d, lab_d, G)
    assert rc == 0 and rc2 == 0 and same_bits(first, again) and int(first["mass"].sum()) > 0

    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        outs = sentinels(R, G)                                               # allocations outside the capture
        torch.cuda.synchronize()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            rc, _ = run_mass(c, d, lse_d, lab_d, G, outs=outs, sync=False)
            assert rc == 0, _lib.last_error()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(bool((v == -7).all()) for v in outs.values()), "a capture must not run the kernel"
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(first, outs)
    graph.replay()                                                           # the replay zeroes its own outputs
    torch.cuda.synchronize()
    assert same_bits(first, outs)

    # the same labels as two calls over disjoint label ranges [0, cut) and [cut, G)
    for cut in (1, GW, GW + 7):
        low = np.where((lab >= 0) & (lab < cut), lab, -1).astype(np.int32)
        high = np.where((lab >= cut) & (lab < G), lab - cut, -1).astype(np.int32)
        _, a = run_mass(c, d, lse_d, dev(low), cut)
        _, b = run_mass(c, d, lse_d, dev(high), G - cut)
        assert torch.equal(torch.cat([a["mass"], b["mass"]], dim=1), first["mass"]) and torch.equal(torch.cat([a["n"], b["n"]], dim=1), first["n"])
        assert torch.equal(a["rest_mass"], first["rest_mass"] + b["mass"].sum(dim=1))
        assert torch.equal(b["rest_n"].to(torch.int64), first["rest_n"] + a["n"].sum(dim=1))

    # rows in another order: every row lands in another tile slot, the outputs follow the rows
    perm = np.random.default_rng(9).permutation(R)
    pc = dict(c, ex=c["ex"][perm], row_filter=c["row_filter"][perm])
    pd = device_inputs(pc, hidden_row=perm.astype(np.int64))
    _, moved = run_mass(pc, pd, lse_d[torch.as_tensor(perm, device=DEV)].contiguous(), lab_d, G)
    at = torch.as_tensor(perm, device=DEV)
    assert all(torch.equal(moved[k], first[k][at]) for k in first)


def test_the_sums_and_the_audience_state_do_not_depend_on_how_the_rows_are_cut_into_calls():
    """Given the hidden rows: one b4r_group_mass call over 1000 rows and one merge, against slices of 1, 7, 64 and 257 rows in
    shuffled order, each slice swept and merged on its own: the sums and all four outputs of the merge in every bit."""
    lib = _lib.load()
    R, H, V, G, K = 1000, 32, 2051, 9, 65
    c = planted(R, H, V)
    d = device_inputs(c)
    _, lse_d = run_dist(c, d)
    lab_d = dev(np.random.default_rng(2).integers(-1, G - 1, size=V).astype(np.int32))   # group G - 1 holds nothing
    rc, whole = run_mass(c, d, lse_d, lab_d, G)
    assert rc == 0, _lib.last_error()

    def merged(pieces):
        state = [torch.full((G, K), -1, dtype=torch.int64, device=DEV), torch.full((G, K), -np.inf, dtype=torch.float32, device=DEV),
                 torch.zeros((G,), dtype=torch.int64, device=DEV), torch.zeros((G,), dtype=torch.int64, device=DEV)]
        for b0, b1, mass in pieces:
            logp = torch.log(mass.to(torch.float64) * 2.0 ** -40).to(torch.float32)
            users = torch.arange(b0, b1, dtype=torch.int64, device=DEV)
            assert lib.b4r_audience_merge(P(logp), G, b1 - b0, G, P(users), 0, float(np.log(F32(0.05))), K, P(state[0]), P(state[1]),
                                          P(state[2]), P(state[3]), stream()) == 0
        torch.cuda.synchronize()
        return [state[0], state[1].view(torch.int32), state[2], state[3]]

    want = merged([(0, R, whole["mass"])])
    assert (want[0][:G - 1, -1] >= 0).all() and (want[0][G - 1] == -1).all() and int(want[3][G - 1]) == 0
    for size in (1, 7, 64, 257):
        cuts = [(b0, min(b0 + size, R)) for b0 in range(0, R, size)]
        pieces = []
        for i in np.random.default_rng(size).permutation(len(cuts)).tolist():
            b0, b1 = cuts[i]
            cs = dict(c, hidden=c["hidden"][b0:b1], ex=c["ex"][b0:b1])
            ds = dict(d, ex=d["ex"][b0:b1], rf=d["rf"][b0:b1], hr=torch.arange(b0, b1, dtype=torch.int64, device=DEV))
            rc, part = run_mass(cs, ds, lse_d[b0:b1], lab_d, G, sync=False)
            assert rc == 0, _lib.last_error()
            pieces.append((b0, b1, part["mass"]))
            assert all(torch.equal(part[k], whole[k][b0:b1]) for k in part), (size, b0)
        assert all(torch.equal(a, b) for a, b in zip(want, merged(pieces))), size


# ---- the model and the app ----------------------------------------------------------------------------------------------------------------
L_MODEL = 24
N_USERS = 1000
TEMPERATURE = 0.7
N_GROUPS = 9


@functools.lru_cache(maxsize=None)
def setting(hidden=64):
    dl = make_loader()
    dl.generate_vocab()
    tok = dl.get_tokenizer()
    V = tok.get_vocab_size()
    if hidden == 64:
        model = make_model(V, L=L_MODEL, seed=11)
    else:
        cfgd = {**config.get_encoder_config("ml-1m_128"), "max_sequence_length": L_MODEL, "output_dropout": 0.0, "attention_dropout": 0.0}
        model = models.BERT4RecModel(networks.Bert4RecEncoder(V, seed=12, **cfgd))
    items = dl.create_item_list()
    n = min(len(items), 200)
    histories = [items[(11 * i) % n:(11 * i) % n + 1 + (7 * i) % (L_MODEL - 1)] for i in range(N_USERS)]   # 1 .. 23 items: all in the window
    rng = np.random.default_rng(21)
    labels = rng.integers(-1, N_GROUPS - 1, size=V).astype(np.int64)         # some items without a group; group N_GROUPS - 1 holds nothing
    allow = torch.as_tensor(rng.random(V) < 0.7)
    return dl, model, V, histories, items, torch.from_numpy(labels), allow


def prepared(dl, histories):
    parts = [dl.prepare_inference(list(h)) for h in histories]
    return {k: torch.from_numpy(np.concatenate([np.asarray(p[k]) for p in parts], axis=0)) for k in parts[0]}


@pytest.mark.parametrize("hidden", [64, 128])
def test_group_affinity_tensor_equals_the_host_composition_over_score_distribution_tensor(hidden):
    dl, model, V, histories, items, labels, allow = setting(hidden)
    batch = prepared(dl, histories[:40])
    kw = dict(allow=allow, temperature=TEMPERATURE)
    got = model.group_affinity_tensor(batch, labels, N_GROUPS, **kw)
    R = 40
    ids = torch.arange(V, dtype=torch.int64)
    parts = [model.score_distribution_tensor(batch, query_ids=ids[None, c0:c0 + 1024].expand(R, -1), **kw) for c0 in range(0, V, 1024)]
    logp = np.concatenate([p["logp"].cpu().numpy() for p in parts], axis=1).astype(np.float64)          # [R, V]
    assert torch.equal(got["row_lse"], parts[0]["lse"]) and torch.equal(got["row_n"], parts[0]["n"])
    with np.errstate(under="ignore"):
        c = np.where(np.isfinite(logp), np.rint(np.exp(np.minimum(logp, 0.0)) * gref.ONE), 0.0).astype(np.int64)
    lab = labels.numpy()
    mass, n = np.zeros((R, N_GROUPS), np.int64), np.zeros((R, N_GROUPS), np.int64)
    for g in range(N_GROUPS):
        mass[:, g] = c[:, lab == g].sum(axis=1)
        n[:, g] = np.isfinite(logp[:, lab == g]).sum(axis=1)
    rest = (lab < 0) | (lab >= N_GROUPS)
    dm, dn = got["group_mass"].cpu().numpy(), got["group_n"].cpu().numpy()
    assert np.array_equal(dn, n) and np.array_equal(got["rest_n"].cpu().numpy(), np.isfinite(logp[:, rest]).sum(axis=1))
    gap = np.abs(dm - mass)
    rest_gap = np.abs(got["rest_mass"].cpu().numpy() - c[:, rest].sum(axis=1))
    print("hidden %d: largest |device - host composition| = %d units (groups), %d (rest)" % (hidden, gap.max(), rest_gap.max()))
    assert (gap <= n).all() and (rest_gap <= np.isfinite(logp[:, rest]).sum(axis=1)).all()
    assert np.array_equal(dn.sum(axis=1) + got["rest_n"].cpu().numpy(), got["row_n"].cpu().numpy())
    assert not dn[:, N_GROUPS - 1].any() and np.isneginf(got["group_logp"].cpu().numpy()[:, N_GROUPS - 1]).all()   # a group without items
    want_logp = np.log(dm.astype(np.float64) * 2.0 ** -40, where=dm > 0, out=np.full(dm.shape, -np.inf)).astype(F32)
    dl_ = got["group_logp"].cpu().numpy()
    assert np.array_equal(np.isneginf(dl_), dm == 0) and np.allclose(dl_, want_logp, rtol=0, atol=2.0 ** -19)
    total = dm.sum(axis=1) + got["rest_mass"].cpu().numpy()
    assert (np.abs(total - gref.ONE) <= gref.tol_total(got["row_n"].cpu().numpy())).all()


def state_bits(state):
    return [state["users"], state["logp"].contiguous().view(torch.int32), state["reach"], state["demand"]]


@pytest.mark.parametrize("hidden", [64, 128])
def test_group_audience_tensor_does_not_depend_on_the_slicing_nor_on_the_order(hidden):
    """One call over 1000 users against slices of 257, 64, 7 and 1 users in shuffled order: the whole state in every bit.  The sums
    and the merge are exact given the hidden rows; the hidden rows keep their bits because the forward runs on blocks of 256 rows
    with every user at the place of its id (forward_rows; DESIGN.md 6.13: without the places, demand at hidden 64 differed by up to
    61 719 units of 2^-40 between the two ways, with users, logp and reach identical)."""
    dl, model, V, histories, items, labels, allow = setting(hidden)
    kw = dict(k=65, min_probability=0.05, allow=allow, temperature=TEMPERATURE)
    names = torch.arange(N_USERS, dtype=torch.int64)
    whole = model.group_audience_tensor(prepared(dl, histories), labels, N_GROUPS, user_ids=names, **kw)
    sizes = [257, 257] + [64] * 6 + [7] * 13 + [1] * 11
    assert sum(sizes) == N_USERS
    rng = np.random.default_rng(hidden)
    order = rng.permutation(len(sizes))
    starts = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    sliced = None
    for i in order.tolist():
        b0, b1 = int(starts[i]), int(starts[i]) + sizes[i]
        sliced = model.group_audience_tensor(prepared(dl, histories[b0:b1]), labels, N_GROUPS, state=sliced, user_ids=names[b0:b1], **kw)
    for a, b, what in zip(state_bits(whole), state_bits(sliced), ("users", "logp", "reach", "demand")):
        assert torch.equal(a, b), what
    users = whole["users"].cpu().numpy()
    assert (users[:N_GROUPS - 1, -1] >= 0).all() and (users[N_GROUPS - 1] == -1).all()      # nobody is in the audience of an empty group
    assert int(whole["reach"][N_GROUPS - 1]) == 0 and int(whole["demand"][N_GROUPS - 1]) == 0
    demand = whole["demand"].cpu().numpy() / gref.ONE
    assert 0 < demand.sum() <= N_USERS and whole["next_user"] == 0
    with pytest.raises(ValueError, match="other item_ids"):
        model.group_audience_tensor(prepared(dl, histories[:2]), labels, N_GROUPS + 1, state=whole, k=65)


def test_recommender_category_calls_agree_with_the_tensor_calls_and_recommend_batch():
    dl, model, V, histories, items, labels, allow = setting()
    rec = Recommender(model, dl)
    few = histories[:24]
    tok = dl.get_tokenizer()
    vocab_items = tok.detokenize(list(range(3, V)))
    by_group = {}
    for j, item in zip(range(3, V), vocab_items):
        if 0 <= int(labels[j]) < 4:
            by_group[item] = "genre-%d" % int(labels[j])
    allowed_items = [item for j, item in zip(range(3, V), vocab_items) if bool(allow[j])]
    lists = rec.category_affinity(few, by_group, allowed_items=allowed_items, temperature=TEMPERATURE)
    assert len(lists) == len(few) and all(len(row) == 4 for row in lists)
    for row in lists:
        assert [p for _, p in row] == sorted((p for _, p in row), reverse=True) and 0.0 < sum(p for _, p in row) < 1.0
    assert rec.category_affinity(few, by_group, top=2, allowed_items=allowed_items, temperature=TEMPERATURE) == [row[:2] for row in lists]
    # the integer-label form gives the same numbers under the group indices
    index = {}
    for item in vocab_items:
        if item in by_group:
            index.setdefault(by_group[item], len(index))
    ints = np.full(V, -1, np.int64)
    for j, item in zip(range(3, V), vocab_items):
        if item in by_group:
            ints[j] = index[by_group[item]]
    assert rec.category_affinity(few, ints, allowed_items=allowed_items, temperature=TEMPERATURE) == \
        [[(index[label], p) for label, p in row] for row in lists]

    # shelves: each shelf is recommend_batch's list with the group as the allow-list
    pages = rec.recommend_shelves(few, by_group, shelves=3, k=5, allowed_items=allowed_items, temperature=TEMPERATURE)
    assert len(pages) == len(few)
    for u, page in enumerate(pages):
        assert [(label, p) for label, p, _ in page] == lists[u][:3]
    for s in range(3):
        per_user = [[item for item in allowed_items if by_group.get(item) == pages[u][s][0]] for u in range(len(few))]
        want = rec.recommend_batch(few, k=5, allowed_items_per_user=per_user)
        assert [pages[u][s][2] for u in range(len(few))] == want, s

    # the audience of the categories: the same state as the tensor call under the users' names
    got = rec.category_audience(by_group, few, k=5, batch_size=10, allowed_items=allowed_items, temperature=TEMPERATURE)
    assert [row["label"] for row in got] == list(index)
    tokens = torch.from_numpy(ints)
    mask = torch.zeros(V, dtype=torch.bool)
    mask[torch.as_tensor(tok.tokenize(allowed_items), dtype=torch.int64)] = True
    state = None
    for b0 in range(0, len(few), 10):
        part = few[b0:b0 + 10]
        ex = Recommender._padded_ids([tok.tokenize(list(seq)) for seq in part])
        state = model.group_audience_tensor(prepared(dl, part), tokens, 4, state=state, k=5, user_ids=torch.arange(b0, b0 + len(part)),
                                            exclude_seen=False, exclude=ex, allow=mask, temperature=TEMPERATURE)
    users, prob = state["users"].cpu().tolist(), torch.exp(state["logp"].to(torch.float64)).cpu().tolist()
    for g, row in enumerate(got):
        assert row["users"] == [(u, p) for u, p in zip(users[g], prob[g]) if u >= 0] and len(row["users"]) == 5
        assert row["reach"] == int(state["reach"][g]) and row["expected_demand"] == int(state["demand"][g]) / 2.0 ** 40
        # the best user of a category has the largest affinity for it (the batches differ: up to the forward's last bits)
        most = max(dict(lists[u]).get(row["label"], 0.0) for u in range(len(few)))
        assert dict(lists[row["users"][0][0]])[row["label"]] >= most * (1.0 - 1e-5)
