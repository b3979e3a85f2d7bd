"""Beyond-accuracy list metrics on the GPU (b4r_list_metrics): the kernel through ctypes against the CPU restatement
(tests/list_metrics_ref.py), and the model / app / evaluator layers built on it.

The restatement is fed the device's own rnorm (what the call leaves in its scratch when it is given none), so the integers -- row_n,
row_dist, row_nov, hit_pos, exposure, counts -- are compared bit for bit.  The double sums are compared with math.fsum of the same
per-row terms within 1e-12 relative: at most 300 terms here, each exact to 2^-53 relative whatever the order, so 300 * 2^-53 = 3e-14
bounds the difference (a derived bound, not a measurement).

Shapes: a workgroup has 256 threads (4 waves) and a thread owns 1, 2 or 4 list positions (K <= 256, <= 512, <= 1024), so K = 1, 2, 3,
63, 64, 65, 255, 256, 257, 511, 1024 cross the wave, workgroup and positions-per-thread boundaries; widths 4 (one 16-byte load), 8,
128 and 132 (no multiple of the 16-float unrolled step).  V = 300: a list longer than that repeats ids.  R = 300 gives the closing
fold more rows than its workgroup has threads."""
import functools
import math

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, evaluation
from bert4rec_amd import engine as engine_mod
from bert4rec_amd.apps import Recommender, item_self_information
from oracle import bert4rec_oracle as orc
from tests import diverse_ref as dref
from tests import list_metrics_ref as lref
from tests.b4r_testlib import P, stream
from tests.test_gpu_api import make_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
V0 = 300
FIRST = 3
ZERO_ROW = 20                      # an all-zero table row: rnorm is clamped, every sim with it is 0, every distance exactly 2^30
TWINS = ((4, 7), (11, V0 - 1))     # distinct ids with identical table rows
KS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 1024)
WIDTHS = (4, 8, 128, 132)
OUTPUTS = ("n", "dist", "nov", "hit_pos", "exposure", "sums", "counts")


def run(table_d, V, ids, gt=None, weight=None, rnorm=None, into=None, skip=(), first_item=FIRST, scratch_bytes=None):
    """One b4r_list_metrics call.  rnorm: a device tensor, or None = computed by the call.  into: a dict of accumulators (exposure, sums,
    counts) to add to, else fresh zeroed ones.  skip: names of OUTPUTS passed as NULL.  Returns (rc, out, call, read): out maps the
    names to numpy arrays (plus "rnorm": what the call left in its scratch), call repeats the call, read reads the outputs again."""
    lib = _lib.load()
    R, K = ids.shape
    width = int(table_d.shape[1])
    ids_d = torch.as_tensor(np.ascontiguousarray(ids)).to(DEV)
    gt_d = None if gt is None else torch.as_tensor(np.asarray(gt, np.int64)).to(DEV)
    w_d = None if weight is None else torch.as_tensor(np.asarray(weight, F32)).to(DEV)
    bufs = dict(n=torch.full((max(R, 1),), -7, dtype=torch.int32, device=DEV), dist=torch.full((max(R, 1),), -7, dtype=torch.int64, device=DEV),
                nov=torch.full((max(R, 1),), -7, dtype=torch.int64, device=DEV), hit_pos=torch.full((max(R, 1),), -7, dtype=torch.int32, device=DEV),
                exposure=torch.zeros(V, dtype=torch.int64, device=DEV), sums=torch.zeros(2, dtype=torch.float64, device=DEV),
                counts=torch.zeros(2, dtype=torch.int64, device=DEV))
    if into is not None:
        bufs.update(into)
    need = int(lib.b4r_list_metrics_scratch_bytes(R, K, V))
    scratch = torch.zeros(max(need, 16), dtype=torch.uint8, device=DEV)
    assert scratch.data_ptr() % 16 == 0
    nbytes = need if scratch_bytes is None else scratch_bytes
    ptr = {name: None if name in skip else P(bufs[name]) for name in OUTPUTS}

    def call():
        return lib.b4r_list_metrics(P(table_d), width, width, V, first_item, P(rnorm), P(ids_d), R, K, P(gt_d), P(w_d), ptr["n"], ptr["dist"],
                                    ptr["nov"], ptr["hit_pos"], ptr["exposure"], ptr["sums"], ptr["counts"], P(scratch), nbytes, stream())

    def read():
        torch.cuda.synchronize()
        out = {name: bufs[name].cpu().numpy()[: (R if name in OUTPUTS[:4] else None)] for name in OUTPUTS}
        out["rnorm"] = scratch[: 4 * V].view(torch.float32).cpu().numpy() if need >= 4 * V else None
        return out
    rc = call()
    return rc, read(), call, read, bufs


@functools.lru_cache(maxsize=None)
def case(width, V=V0):
    """An item table with two pairs of identical rows and an all-zero row, the rnorm the device computes for it, the restatement's
    [V, V] similarities under that rnorm, and item weights; computed once per width."""
    g = torch.Generator().manual_seed(V * 17 + width)
    table = (torch.randn(V, width, generator=g) * 0.05).numpy()
    if V == V0:
        for a, b in TWINS:
            table[b] = table[a]
        table[ZERO_ROW] = 0.0
    table_d = torch.as_tensor(table).to(DEV)
    rc, out = run(table_d, V, np.zeros((1, 1), np.int64))[:2]
    assert rc == 0, _lib.last_error()
    rnorm = out["rnorm"].copy()
    want = 1.0 / np.sqrt(np.maximum((table.astype(np.float64) ** 2).sum(axis=1), 1e-24))
    assert np.allclose(rnorm, want, rtol=2e-4)                      # (a sanity check: the fp32 chain of `width` squares, at most width * 2^-24 / 2)
    counts = np.random.default_rng(width).zipf(1.3, size=V) % 1000
    weight = item_self_information(counts)
    weight[5] = F32(-3.25)                                          # weights are the caller's: a negative one, a large one
    weight[6] = F32(2.0 ** 19 + 0.5)
    return dict(table=table, table_d=table_d, rnorm=rnorm, rnorm_d=torch.as_tensor(rnorm).to(DEV), sim=dref.sim_matrix(table, rnorm), weight=weight)


def make_lists(V, K, R, seed=0):
    """R lists of K ids (distinct where V allows it) and a ground truth per row; the first rows hold the inputs that break lazy code."""
    rng = np.random.default_rng(seed + 31 * K + R)
    ids = np.stack([rng.permutation(V)[:K] if K <= V else rng.integers(0, V, size=K) for _ in range(R)]).astype(np.int64)
    gt = ids[np.arange(R), rng.integers(0, K, size=R)].copy()        # present, somewhere
    dead = np.array([-1, V, 2 ** 40, -2 ** 40], np.int64)
    if R > 0:
        ids[0] = dead[np.arange(K) % 4]                              # an all-dead row: n = 0
    if R > 1:
        ids[1] = -1; ids[1, K // 2] = 9                              # one live entry: counted for novelty only
    if R > 2 and K >= 3:
        ids[2, 0] = V; ids[2, K // 2] = 2 ** 40; ids[2, (2 * K) // 3:] = -1    # dead at the head, in the middle, and as the whole tail
        gt[2] = ids[2, 1] if ids[2, 1] >= 0 else gt[2]
    if R > 3 and K >= 2:
        ids[3, K // 2:] = ids[3, 0]                                  # exact duplicates of one id
    if R > 4 and K >= 2:
        ids[4, 0], ids[4, K - 1] = TWINS[0]                          # two ids with identical rows: a distance of about 0, perhaps below
        if K >= 4:
            ids[4, 1], ids[4, 2] = TWINS[1][1], TWINS[1][0]
    if R > 5:
        ids[5, K // 3] = ZERO_ROW                                    # the all-zero row
        if K >= 2:
            ids[5, K - 1] = ZERO_ROW
    if R > 6 and K >= 3:
        ids[6, 1] = ids[6, K - 1] = 37; ids[6, 0] = 36; gt[6] = 37   # gt twice: the first position (2) counts
    if R > 7:
        ids[7][ids[7] == 41] = 42; gt[7] = 41                        # gt absent
    if R > 8:
        ids[8, 0] = 1; gt[8] = 1                                     # gt below first_item, though it stands in the list
    if R > 9:
        gt[9] = V + 5                                                # gt past the table
    if R > 10:
        gt[10] = -1
    return ids, gt


def assert_same(got, want, what, names=OUTPUTS):
    for name in names:
        if name == "sums":
            for g, w in zip(got["sums"].tolist(), want["sums"]):
                assert abs(g - w) <= 1e-12 * abs(w), f"{what}: sums {got['sums'].tolist()} against {want['sums']}"
        else:
            assert np.array_equal(np.asarray(got[name], np.int64), np.asarray(want[name], np.int64)), f"{what}: {name}"


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("width", WIDTHS)
def test_grid_bit_exact(width, K):
    c = case(width)
    ids, gt = make_lists(V0, K, 17)
    want = lref.list_metrics(c["table"], c["rnorm"], ids, gt, c["weight"], FIRST, c["sim"])
    rc, got = run(c["table_d"], V0, ids, gt, c["weight"], c["rnorm_d"])[:2]
    assert rc == 0, _lib.last_error()
    assert_same(got, want, f"K={K} R=17")
    assert got["n"][0] == 0 and got["dist"][0] == 0 and got["nov"][0] == 0 and got["n"][1] == 1 and got["dist"][1] == 0
    assert got["counts"][1] - got["counts"][0] >= (1 if K > 1 else 0)            # row 1 counts for novelty only
    one = lref.list_metrics(c["table"], c["rnorm"], ids[8:9], gt[8:9], c["weight"], FIRST, c["sim"])
    rc, got1 = run(c["table_d"], V0, ids[8:9], gt[8:9], c["weight"], c["rnorm_d"])[:2]
    assert rc == 0, _lib.last_error()
    assert_same(got1, one, f"K={K} R=1")


@pytest.mark.parametrize("K,width", [(2, 8), (65, 128), (257, 8), (10, 132)])
def test_more_rows_than_the_fold_has_threads(K, width):
    c = case(width)
    ids, gt = make_lists(V0, K, 300, seed=3)
    want = lref.list_metrics(c["table"], c["rnorm"], ids, gt, c["weight"], FIRST, c["sim"])
    rc, got = run(c["table_d"], V0, ids, gt, c["weight"], c["rnorm_d"])[:2]
    assert rc == 0, _lib.last_error()
    assert_same(got, want, f"K={K} R=300")
    assert want["counts"][1] > 256


def test_widest_table():
    V, width, K = 64, 4096, 8
    c = case(width, V)
    rng = np.random.default_rng(5)
    ids = np.stack([rng.permutation(V)[:K] for _ in range(17)]).astype(np.int64)
    gt = ids[:, 3].copy()
    want = lref.list_metrics(c["table"], c["rnorm"], ids, gt, c["weight"], FIRST, c["sim"])
    rc, got = run(c["table_d"], V, ids, gt, c["weight"], c["rnorm_d"])[:2]
    assert rc == 0, _lib.last_error()
    assert_same(got, want, "width 4096")


def test_inputs_that_break_lazy_code():
    """The special rows of make_lists at K = 12, looked at one by one."""
    K, width = 12, 128
    c = case(width)
    ids, gt = make_lists(V0, K, 17)
    want = lref.list_metrics(c["table"], c["rnorm"], ids, gt, c["weight"], FIRST, c["sim"])
    rc, got = run(c["table_d"], V0, ids, gt, c["weight"], c["rnorm_d"])[:2]
    assert rc == 0, _lib.last_error()
    assert_same(got, want, "special rows")
    assert got["n"][0] == 0 and got["hit_pos"][0] == 0                              # all dead: in neither count
    assert got["n"][1] == 1 and got["dist"][1] == 0 and got["nov"][1] == lref.q30(c["weight"][9])
    assert got["counts"].tolist() == [15, 16]
    assert got["n"][2] == (2 * K) // 3 - 2 and got["hit_pos"][2] == 2               # dead head, middle and tail; gt at position 2
    assert got["n"][3] == K and got["exposure"][ids[3, 0]] >= K // 2 + 1             # duplicates count once per occurrence
    assert c["rnorm"][ZERO_ROW] > 1e11 and got["n"][5] == K                       # clamped: 1 / sqrt(1e-24)
    only_zero = np.array([[ZERO_ROW, 50, ZERO_ROW, 51]], np.int64)                  # pairs with the zero row: exactly 2^30 each
    rc, z = run(c["table_d"], V0, only_zero, None, None, c["rnorm_d"])[:2]
    d_50_51 = int(lref.q30(F32(1.0) - c["sim"][50, 51]))
    assert rc == 0 and z["dist"][0] == 5 * 2 ** 30 + d_50_51
    # identical rows: about 0, sign included.  With u = 2^-24: each rnorm is within (width / 2 + 2) u of 1 / |row| (the chain of squares,
    # the square root, the reciprocal), qhat and the last product add u each, the chain width u: |1 - sim| <= (2 width + 6) u, in units
    # of 2^-30 (2 width + 6) * 64
    twins = np.array([[4, 7], [7, 4], [11, V0 - 1]], np.int64)
    rc, t = run(c["table_d"], V0, twins, None, None, c["rnorm_d"])[:2]
    assert rc == 0 and (np.abs(t["dist"]) <= (2 * width + 6) * 64).all()
    assert t["dist"].tolist() == [int(lref.q30(F32(1.0) - c["sim"][a, b])) for a, b in twins]
    assert got["hit_pos"][6] == 2 and got["hit_pos"][7] == 0 and got["hit_pos"][8] == 0 and got["hit_pos"][9] == 0 and got["hit_pos"][10] == 0
    assert got["exposure"][1] >= 1 and ids[8, 0] == 1                               # id 1 is live (below first_item only matters for gt)
    # gt NULL, item_weight NULL
    rc, g = run(c["table_d"], V0, ids, None, None, c["rnorm_d"])[:2]
    assert rc == 0 and (g["hit_pos"] == 0).all() and (g["nov"] == 0).all() and g["sums"][1] == 0.0
    assert np.array_equal(g["dist"], got["dist"]) and g["counts"].tolist() == [15, 16] and g["sums"][0] == got["sums"][0]


def test_every_output_may_be_null():
    K, width = 65, 8
    c = case(width)
    ids, gt = make_lists(V0, K, 17, seed=2)
    rc, full = run(c["table_d"], V0, ids, gt, c["weight"], c["rnorm_d"])[:2]
    assert rc == 0, _lib.last_error()
    for name in OUTPUTS:
        for rnorm in (c["rnorm_d"], None):                            # (without rnorm the call has its scratch for the fold's rows)
            rc, got = run(c["table_d"], V0, ids, gt, c["weight"], rnorm, skip=(name,))[:2]
            assert rc == 0, (name, _lib.last_error())
            untouched = got[name]
            assert (untouched == (-7 if name in OUTPUTS[:4] else 0)).all(), name
            for other in OUTPUTS:
                if other != name:
                    assert np.array_equal(got[other], full[other]), (name, other)
    # sums or counts without the per-row outputs and without a scratch: refused, not guessed
    rc = run(c["table_d"], V0, ids, gt, c["weight"], c["rnorm_d"], skip=("dist",), scratch_bytes=0)[0]
    assert rc == -5 and "scratch" in _lib.last_error()
    rc, got = run(c["table_d"], V0, ids, gt, c["weight"], c["rnorm_d"], skip=("dist", "sums", "counts"), scratch_bytes=0)[:2]
    assert rc == 0 and np.array_equal(got["n"], full["n"])


def test_accumulation_and_reproducibility():
    K, width = 63, 132
    c = case(width)
    ids_a, gt_a = make_lists(V0, K, 17, seed=4)
    ids_b, gt_b = make_lists(V0, K, 300, seed=5)
    rc, first, _, _, bufs = run(c["table_d"], V0, ids_a, gt_a, c["weight"], c["rnorm_d"])
    assert rc == 0, _lib.last_error()
    acc = {name: bufs[name] for name in ("exposure", "sums", "counts")}
    rc, both = run(c["table_d"], V0, ids_b, gt_b, c["weight"], c["rnorm_d"], into=acc)[:2]
    assert rc == 0, _lib.last_error()
    want = lref.list_metrics(c["table"], c["rnorm"], np.concatenate([ids_a, ids_b]), np.concatenate([gt_a, gt_b]), c["weight"], FIRST, c["sim"])
    assert_same(both, want, "two calls", names=("exposure", "sums", "counts"))
    assert np.array_equal(both["dist"], want["dist"][17:])
    # the same call into fresh accumulators: identical bits, the double sums included
    again = [run(c["table_d"], V0, ids_b, gt_b, c["weight"], c["rnorm_d"])[1] for _ in range(2)]
    for name in OUTPUTS:
        assert np.array_equal(again[0][name].view(np.int64 if again[0][name].dtype.itemsize == 8 else np.int32),
                              again[1][name].view(np.int64 if again[1][name].dtype.itemsize == 8 else np.int32)), name


def test_rnorm_forms_scratch_and_empty_calls():
    lib = _lib.load()
    K, width, R = 10, 128, 17
    c = case(width)
    ids, gt = make_lists(V0, K, R, seed=6)
    rc, given = run(c["table_d"], V0, ids, gt, c["weight"], c["rnorm_d"])[:2]
    assert rc == 0, _lib.last_error()
    rc, own = run(c["table_d"], V0, ids, gt, c["weight"], None)[:2]
    assert rc == 0, _lib.last_error()
    for name in OUTPUTS:
        assert np.array_equal(given[name], own[name]), name
    assert np.array_equal(own["rnorm"].view(np.uint32), c["rnorm"].view(np.uint32))
    need = int(lib.b4r_list_metrics_scratch_bytes(R, K, V0))
    assert need >= 4 * V0
    rc = run(c["table_d"], V0, ids, gt, c["weight"], None, scratch_bytes=need - 1)[0]
    assert rc == -5 and "b4r_list_metrics" in _lib.last_error()                      # B4R_E_NOMEM
    # argument errors with real pointers, and R = 0
    t = c["table_d"]
    ids_d = torch.as_tensor(ids).to(DEV)
    out = torch.full((R,), -7, dtype=torch.int32, device=DEV)

    def call(K=K, ld=width, w=width, R=R, table=t):
        return lib.b4r_list_metrics(P(table), ld, w, V0, FIRST, P(c["rnorm_d"]), P(ids_d), R, K, None, None, P(out), None, None, None, None,
                                    None, None, None, 0, stream())
    for kw, code in ((dict(K=0), -2), (dict(K=1025), -2), (dict(ld=width + 4), -2), (dict(w=6, ld=6), -2), (dict(table=None), -1)):
        assert call(**kw) == code and "b4r_list_metrics" in _lib.last_error(), kw
    assert call(R=0) == 0
    torch.cuda.synchronize()
    assert (out == -7).all()                                          # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), given["n"])


def test_in_a_captured_graph():
    K, width = 257, 128
    c = case(width)
    ids, gt = make_lists(V0, K, 17, seed=8)
    want = lref.list_metrics(c["table"], c["rnorm"], ids, gt, c["weight"], FIRST, c["sim"])
    for rnorm in (c["rnorm_d"], None):
        rc, first, call, read, bufs = run(c["table_d"], V0, ids, gt, c["weight"], rnorm)
        assert rc == 0, _lib.last_error()
        assert_same(first, want, "eager")
        for name in ("exposure", "sums", "counts"):
            bufs[name].zero_()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                assert call() == 0
        torch.cuda.current_stream().wait_stream(side)
        for _ in range(2):
            graph.replay()
        got = read()
        assert np.array_equal(got["exposure"], 2 * want["exposure"]) and got["counts"].tolist() == [2 * x for x in want["counts"]]
        assert_same(got, want, "replayed", names=OUTPUTS[:4])
        for g, w in zip(got["sums"].tolist(), want["sums"]):
            assert abs(g - 2 * w) <= 1e-12 * abs(2 * w)


# ---- the model, the app and the evaluator ---------------------------------------------------------------------------------------------
V1, L1, K1 = 500, 20, 10


@functools.lru_cache(maxsize=None)
def small_setup():
    """A hidden-64 model over V = 500, one fine-tune batch of 32 users, the item table, the device's rnorm for it and the restatement's
    similarities, item counts, and the exclusion lists under which recommend_tensor ranks what the evaluator ranks (the row's labels
    without its ground truth)."""
    model = make_model(V1, L=L1, seed=23)
    batch = orc.synthetic_batch(32, L1, 4, V1, seed=81, ragged=True, finetune=True)
    table_d = model.engine.view("word_embeddings/embeddings")
    rc, out = run(table_d, V1, np.zeros((1, 1), np.int64))[:2]
    assert rc == 0, _lib.last_error()
    table, rnorm = table_d.cpu().numpy(), out["rnorm"].copy()
    w = batch["masked_lm_weights"] != 0
    b_idx, p_idx = torch.nonzero(w, as_tuple=True)
    assert b_idx.tolist() == list(range(32))
    gt = batch["masked_lm_ids"][b_idx, p_idx]
    exclude = batch["labels"].clone()
    exclude[exclude == gt[:, None]] = -1
    counts = np.random.default_rng(1).zipf(1.2, size=V1) % 500
    return dict(model=model, batch=batch, table=table, rnorm=rnorm, sim=dref.sim_matrix(table, rnorm), gt=gt.numpy(), exclude=exclude,
                counts=counts, weight=item_self_information(counts))


def test_model_and_recommender_layers():
    s = small_setup()
    model = s["model"]
    ids, _, _ = model.recommend_tensor(s["batch"], k=K1)
    ids_h = ids.cpu().numpy()
    ids_h[3, 7:] = -1                                                 # a short list, a list of one, an empty list
    ids_h[4, 1:] = -1
    ids_h[5, :] = -1
    want = lref.list_metrics(s["table"], s["rnorm"], ids_h, s["gt"], s["weight"], FIRST, s["sim"])
    got = model.list_metrics_tensor(torch.as_tensor(ids_h), s["gt"], s["weight"])
    assert got["ild"].dtype == torch.float64 and got["novelty"].dtype == torch.float64 and got["ild"].is_cuda
    assert np.array_equal(got["n"].cpu().numpy(), want["n"]) and np.array_equal(got["hit_pos"].cpu().numpy(), want["hit_pos"])
    ild, nov = got["ild"].cpu().numpy(), got["novelty"].cpu().numpy()
    assert np.isnan(ild[4]) and np.isnan(ild[5]) and np.isnan(nov[5]) and not np.isnan(nov[4])
    for r in range(32):
        n = int(want["n"][r])
        if n >= 2:
            assert ild[r] == pytest.approx(want["dist"][r] / 2 ** 30 / (n * (n - 1) // 2), rel=1e-15)
        if n >= 1:
            assert nov[r] == pytest.approx(want["nov"][r] / 2 ** 30 / n, rel=1e-15)
    plain = model.list_metrics_tensor(ids)
    assert torch.isnan(plain["novelty"]).all() and (plain["hit_pos"] == 0).all() and (plain["n"] == K1).all()
    for bad in (ids.to(torch.int32), ids[0], torch.zeros((2, 1025), dtype=torch.int64)):
        with pytest.raises(ValueError):
            model.engine.list_metrics(bad)
    with pytest.raises(ValueError):
        model.engine.list_metrics(ids, item_weight=torch.zeros(V1 - 1))
    with pytest.raises(ValueError):
        model.engine.list_metrics(ids, exposure=torch.zeros(V1, dtype=torch.int64))   # an accumulator on the host

    class Tok:
        _extensible = False

        def tokenize(self, item):
            if isinstance(item, int) and 0 <= item < V1:
                return item
            raise ValueError(item)

        def disable_extensibility(self):
            pass

    class Loader:
        def get_tokenizer(self):
            return Tok()
    rec = Recommender(model, Loader())
    lists = [[i for i in row if i >= 0] + ["unknown item"] for row in ids_h.tolist()]
    q = rec.list_quality(lists, item_counts=s["counts"])
    assert q["ild"] == pytest.approx(want["sums"][0] / want["counts"][0], rel=1e-12)
    assert q["novelty"] == pytest.approx(want["sums"][1] / want["counts"][1], rel=1e-12)
    assert q["coverage"] == lref.coverage(want["exposure"])
    by_item = {j: int(cnt) for j, cnt in enumerate(s["counts"].tolist())}
    assert rec.list_quality(lists, item_counts=by_item) == q
    assert set(rec.list_quality(lists)) == {"ild", "coverage"} and rec.list_quality([]) == {"ild": 0.0, "coverage": 0.0}


def expected_results(s, lists, k):
    want = lref.list_metrics(s["table"], s["rnorm"], lists, s["gt"], s["weight"], FIRST, s["sim"])
    out = {f"ILD@{k}": want["sums"][0] / want["counts"][0], f"Novelty@{k}": want["sums"][1] / want["counts"][1],
           f"Coverage@{k}": lref.coverage(want["exposure"]), f"Gini@{k}": lref.gini(want["exposure"])}
    return out, want


def test_evaluator_list_evaluation():
    s = small_setup()
    model, batch = s["model"], s["batch"]
    base = evaluation.get(full_ranking=True)
    base.evaluate(model, [batch])
    base_res = base.get_metrics_results()
    ev = evaluation.get(full_ranking=True, list_k=K1, item_counts=s["counts"])
    ev.evaluate(model, [batch])
    res = ev.get_metrics_results()
    assert list(res) == list(base_res) + [f"ILD@{K1}", f"Novelty@{K1}", f"Coverage@{K1}", f"Gini@{K1}"]
    for key, v in base_res.items():
        assert res[key] == v, key                                     # the accuracy metrics come from the same gt_rank
    lists, _, _ = model.recommend_tensor(batch, k=K1, exclude_seen=False, exclude=s["exclude"])
    want, _ = expected_results(s, lists.cpu().numpy(), K1)
    for key, v in want.items():
        assert res[key] == pytest.approx(v, rel=1e-12), key
    assert 0.0 < res[f"Coverage@{K1}"] <= 1.0 and 0.0 < res[f"Gini@{K1}"] < 1.0 and res[f"ILD@{K1}"] > 0.0
    # without item counts and without a dataloader: no Novelty key
    assert f"Novelty@{K1}" not in evaluation.get(full_ranking=True, list_k=K1).get_metrics_results()
    # reset, then a second evaluation reproduces the first; without the reset the sums go on
    ev.reset_metrics()
    assert ev.get_metrics_results()[f"Coverage@{K1}"] == 0.0
    ev.evaluate(model, [batch])
    assert ev.get_metrics_results() == res
    ev.evaluate(model, [batch])
    twice = ev.get_metrics_results()
    assert twice[f"ILD@{K1}"] == pytest.approx(res[f"ILD@{K1}"], rel=1e-12) and twice[f"Coverage@{K1}"] == res[f"Coverage@{K1}"]
    assert twice["Valid Ranks"] == 2 * res["Valid Ranks"]


def test_evaluator_with_diversity():
    s = small_setup()
    model, batch = s["model"], s["batch"]
    metrics = lambda: [evaluation.Counter(name="Valid Ranks")] + [f(k) for f in (evaluation.HR, evaluation.NDCG) for k in (1, 5, 10)]
    plain = evaluation.get(full_ranking=True, list_k=K1, item_counts=s["counts"], metrics=metrics())
    plain.evaluate(model, [batch])
    zero = evaluation.get(full_ranking=True, list_k=K1, diversity=0.0, item_counts=s["counts"], metrics=metrics())
    zero.evaluate(model, [batch])
    assert zero.get_metrics_results() == plain.get_metrics_results()  # lambda = 1 keeps the sweep's order: identical, list metrics too
    pool = 60
    ev = evaluation.get(full_ranking=True, list_k=K1, diversity=0.5, candidate_pool=pool, item_counts=s["counts"], metrics=metrics())
    ev.evaluate(model, [batch])
    res = ev.get_metrics_results()
    lists, _, _ = model.recommend_tensor(batch, k=K1, exclude_seen=False, exclude=s["exclude"], diversity=0.5, pool=pool)
    lists = lists.cpu().numpy()
    cand, cand_sc, _ = model.recommend_tensor(batch, k=pool, exclude_seen=False, exclude=s["exclude"])
    lam = engine_mod.check_rerank_args(K1, pool, 0.5)[2]
    assert np.array_equal(lists, dref.rerank(s["table"], s["rnorm"], cand.cpu().numpy(), cand_sc.cpu().numpy(), lam, K1, s["sim"])[0])
    want, raw = expected_results(s, lists, K1)
    for key, v in want.items():
        assert res[key] == pytest.approx(v, rel=1e-12), key
    assert res[f"ILD@{K1}"] >= plain.get_metrics_results()[f"ILD@{K1}"]
    ranks = np.where(raw["hit_pos"] > 0, raw["hit_pos"], K1 + 1)      # the accuracy metrics come from the position in the re-ranked list
    assert res["Valid Ranks"] == 32
    for k in (1, 5, 10):
        assert res[f"HR@{k}"] == pytest.approx(float((ranks <= k).mean()), abs=1e-12)
        ndcg = [1.0 / math.log2(r + 1) if r <= k else 0.0 for r in ranks.tolist()]
        assert res[f"NDCG@{k}"] == pytest.approx(math.fsum(ndcg) / 32, abs=1e-12)
    ev.reset_metrics()
    ev.evaluate(model, [batch])
    assert ev.get_metrics_results() == res
