"""Host side of the catalogue filter and the item neighbours (no GPU): the filter packing, the restatement, the argument checks
of the Python layer and of the C ABI, and the binding of the new symbols."""
import numpy as np
import pytest
import torch

from bert4rec_amd import _lib
from bert4rec_amd import engine as engine_mod
from bert4rec_amd.apps import pack_item_filter
from tests import catalogue_ref as ref


@pytest.mark.parametrize("V", [4, 31, 32, 33, 1025])
def test_pack_item_filter_against_bit_loop(V):
    rng = np.random.default_rng(V)
    W = (V + 31) // 32
    for shape in ((V,), (3, V)):
        for dtype in (torch.bool, torch.uint8):
            mask = rng.random(shape) < 0.5
            mask[..., V - 1] = True                                  # the last id's bit: the top bit of word W-1 when V % 32 == 0
            got = pack_item_filter(torch.as_tensor(mask).to(dtype))
            assert got.dtype == torch.uint32 and tuple(got.shape) == (1 if len(shape) == 1 else 3, W)
            assert np.array_equal(got.numpy(), ref.pack_bits(mask))
    # uint8 values above 1 count as set; bits past V stay clear
    ones = pack_item_filter(torch.full((V,), 7, dtype=torch.uint8)).numpy()
    assert np.array_equal(ones, ref.pack_bits(np.ones(V, bool)))
    if V % 32:
        assert int(ones[0, -1]) >> (V % 32) == 0
    assert not pack_item_filter(torch.zeros(V, dtype=torch.bool)).numpy().any()
    for bad in (torch.zeros(V, dtype=torch.int64), torch.zeros((2, 2, V), dtype=torch.bool), torch.zeros((0,), dtype=torch.bool)):
        with pytest.raises(ValueError):
            pack_item_filter(bad)


def test_restatement_all_ones_filter_equals_unfiltered():
    rng = np.random.default_rng(0)
    R, H, V, K, first = 5, 8, 70, 12, 3
    hidden, table, bias = (rng.standard_normal(s).astype(np.float32) for s in ((R, H), (V, H), (V,)))
    table[40] = table[9]; bias[40] = bias[9]                       # a tie
    sc = ref.chain_scores(hidden, table, bias)
    gt = rng.integers(first, V, size=R)
    ex = rng.integers(-1, V, size=(R, 6))
    plain = ref.expected(sc, ref.allowed_mask(V, first, ex, gt, R), gt, K, first)
    words = ref.pack_bits(np.ones((2, V), bool))
    for rf in (None, np.array([0, 1, 0, 5, -1])):
        got = ref.expected(sc, ref.allowed_mask(V, first, ex, gt, R, words, rf), gt, K, first)
        assert all(np.array_equal(a, b) for a, b in zip(plain, got))
    # and a filter does restrict: nothing outside it but gt, scores of the ids kept
    keep = rng.random(V) < 0.3
    ids, scores, _ = ref.expected(sc, ref.allowed_mask(V, first, ex, gt, R, ref.pack_bits(keep)), gt, K, first)
    for r in range(R):
        for i, s in zip(ids[r], scores[r]):
            assert i == -1 or ((keep[i] or i == gt[r]) and i >= first and s == sc[r, i])
    # the chain with no bias is the chain with a zero bias; the scale is one multiply
    assert np.array_equal(ref.chain_scores(hidden, table).view(np.uint32), ref.chain_scores(hidden, table, np.zeros(V)).view(np.uint32))
    scale = rng.random(V).astype(np.float32)
    assert np.array_equal(ref.scaled(sc, scale), sc * scale[None, :])


def test_python_argument_validation():
    V = 70
    W = 3
    check = engine_mod.check_item_filter
    assert check(None, None, V) == (None, None)
    packed, rf = check(torch.ones(V, dtype=torch.bool), None, V)
    assert packed.dtype == torch.uint32 and tuple(packed.shape) == (1, W) and rf is None
    packed, rf = check(torch.ones((3, V), dtype=torch.uint8), torch.tensor([0, 2, 7, -4]), V, n_rows=4)
    assert tuple(packed.shape) == (3, W) and rf.dtype == torch.int32 and rf.tolist() == [0, 2, 3, -1]
    packed2, _ = check(packed, torch.tensor([1]), V)
    assert packed2 is packed
    bad = [
        (torch.ones(V + 1, dtype=torch.bool), None),                # wrong length
        (torch.ones((2, V - 1), dtype=torch.bool), torch.tensor([0])),
        (torch.ones((2, 2, V), dtype=torch.bool), None),            # rank 3
        (torch.ones(V, dtype=torch.float32), None),                 # dtype
        (torch.ones((2, W + 1), dtype=torch.int32).view(torch.uint32), torch.tensor([0])),   # packed with a wrong word count
        (torch.ones(W, dtype=torch.int32).view(torch.uint32), None),                          # packed must be 2-D
        (torch.ones(V, dtype=torch.bool), torch.tensor([0])),       # row_filter with a 1-D allow
        (None, torch.tensor([0])),                                  # row_filter without allow
        (torch.ones((2, V), dtype=torch.bool), None),               # two filters, nothing to pick them
        (torch.ones((2, V), dtype=torch.bool), torch.tensor([0.0])),
        (torch.ones((2, V), dtype=torch.bool), torch.tensor([[0]])),
    ]
    for allow, row_filter in bad:
        with pytest.raises(ValueError):
            check(allow, row_filter, V)
    with pytest.raises(ValueError):
        check(torch.ones((2, V), dtype=torch.bool), torch.tensor([0, 1, 0]), V, n_rows=4)
    assert engine_mod.check_similar_items_args(10, "cosine") == (10, 1) and engine_mod.check_similar_items_args(0, "dot") == (0, 0)
    for k, metric in ((10, "euclid"), (10, None), (1025, "dot"), (-1, "cosine"), (2.5, "dot")):
        with pytest.raises(ValueError):
            engine_mod.check_similar_items_args(k, metric)


def test_lib_binds_the_new_symbols():
    lib = _lib.load()
    for name in ("b4r_rank_full_ex", "b4r_item_neighbours", "b4r_item_neighbours_scratch_bytes"):
        assert name in _lib.PROTOTYPES, name
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert (_lib.SIM_DOT, _lib.SIM_COSINE) == (0, 1)
    # the sizing covers the sweep's scratch plus rnorm [V], the query rows [R, width] and their row indices [R]
    R, V, K, width = 17, 2051, 10, 64
    need = lib.b4r_item_neighbours_scratch_bytes(R, V, K, width)
    assert need >= lib.b4r_rank_full_scratch_bytes(R, V, K) + 4 * V + 4 * R * width + 8 * R
    assert lib.b4r_item_neighbours_scratch_bytes(0, V, K, width) == 0 and lib.b4r_item_neighbours_scratch_bytes(R, V, 1025, width) == 0


def test_c_abi_refuses_bad_arguments_before_touching_the_device():
    lib = _lib.load()
    ex = lambda R, K, H=64, n_filters=0: lib.b4r_rank_full_ex(None, H, None, None, None, H, 1000, 3, R, None, 0, None, K, None, None, None,
                                                             None, 0, None, None, n_filters, None, None)
    assert ex(4, 1025) == -2 and ex(4, -1) == -2 and ex(-1, 10) == -2 and ex(4, 10, H=30) == -2
    assert ex(4, 10) == -1 and "b4r_rank_full_ex" in _lib.last_error()
    assert ex(0, 10) == 0
    nb = lambda R, K, width=64, ld=None, metric=1: lib.b4r_item_neighbours(None, width if ld is None else ld, width, 1000, 3, None, R,
                                                                           metric, None, 0, None, K, None, None, None, 0, None)
    assert nb(4, 1025) == -2 and nb(4, -1) == -2 and nb(-1, 10) == -2        # the codes b4r_rank_full uses
    assert nb(4, 10, width=30) == -2 and nb(4, 10, width=4100) == -2 and nb(4, 10, ld=68) == -2
    assert nb(4, 10, metric=2) == -1
    assert nb(4, 10) == -1 and "b4r_item_neighbours" in _lib.last_error()
    assert nb(0, 10) == 0
