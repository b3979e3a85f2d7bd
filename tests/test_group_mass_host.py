"""Category affinity (b4r_group_mass) without a GPU: the CPU restatement (tests/group_mass_ref.py) against a brute-force fp64 softmax
grouped by label, the label and argument checks of the Python layers (raised before any work), the binding, the library's own argument
checks (they return before any launch), and the host side of category_affinity / recommend_shelves."""
import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, models
from bert4rec_amd import engine as engine_mod
from bert4rec_amd.apps import Recommender
from tests import catalogue_ref as ref
from tests import group_mass_ref as gref
from tests import score_dist_ref as sref

F32 = np.float32


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,H,G", [(1500, 32, 7), (2051, 64, 300)])
def test_restatement_against_a_brute_force_softmax_grouped_by_label(V, H, G):
    rng = np.random.default_rng(V + G)
    table = (rng.standard_normal((V, H)) * 0.05).astype(F32)
    bias = (rng.standard_normal(V) * 0.01).astype(F32)
    base = rng.standard_normal((1, H)).astype(F32)
    hidden = np.concatenate([base * s for s in (1, 20, 200)]).astype(F32)
    ex = rng.integers(0, V, size=(3, 20)).astype(np.int64)
    ok = ref.allowed_mask(V, 3, ex, None, 3)
    lab = rng.integers(-2, G + 2, size=V)                                    # some labels below 0 and at or above G
    for inv_t in (1.0, 0.5):
        t = sref.scaled_scores(hidden, table, bias, None, inv_t)
        p_g, p_rest, lse = gref.brute_force(t, ok, lab, G)
        mass, n, rest_mass, rest_n = gref.group_mass(t, ok, lse, lab, G)
        inside = (lab >= 0) & (lab < G)
        assert np.array_equal(n.sum(axis=1) + rest_n, ok.sum(axis=1))
        assert np.array_equal(rest_n, (ok & ~inside).sum(axis=1))
        for g in (0, G // 2, G - 1):
            assert np.array_equal(n[:, g], (ok & (lab == g)).sum(axis=1))
        # half a unit of rounding per item, and the rounding of u to fp32: 2^-24 |u| relative in every term (|u| <= max |t - lse|)
        umax = np.abs(np.where(ok, t.astype(np.float64) - lse[:, None], 0.0)).max(axis=1)
        rel = 2.0 ** -24 * umax + 2.0 ** -50
        assert (np.abs(mass - p_g * gref.ONE) <= n / 2.0 + p_g * gref.ONE * rel[:, None] + 1).all()
        assert (np.abs(rest_mass - p_rest * gref.ONE) <= rest_n / 2.0 + p_rest * gref.ONE * rel + 1).all()
        total = mass.sum(axis=1) + rest_mass
        assert (np.abs(total - gref.ONE) <= gref.tol_total(ok.sum(axis=1))).all()


def test_restatement_dead_rows_clamp_and_resolution():
    t = np.array([[0.0, -1.0, -2.0, -40.0]] * 5, F32)
    ok = np.ones((5, 4), bool)
    lab = np.array([0, 0, 1, 1])
    lse = np.array([0.5, -np.inf, np.nan, -30.0, 0.5])
    mass, n, rest_mass, rest_n = gref.group_mass(t, ok, lse, lab, 2, dead=[False, False, False, False, True])
    assert not mass[1].any() and not mass[2].any() and not mass[4].any() and not n[[1, 2, 4]].any()
    assert n[0].tolist() == [2, 2] and rest_n.tolist() == [0] * 5
    assert mass[0, 0] == int(np.rint(np.exp(np.float64(F32(-0.5))) * gref.ONE)) + int(np.rint(np.exp(np.float64(F32(-1.5))) * gref.ONE))
    # a row_lse that is far too small: every exponent is clamped at 0, an item counts 2^40 at the most
    assert mass[3].tolist() == [2 << 40, (1 << 40) + int(np.rint(np.exp(-10.0) * gref.ONE))]
    # an item below 2^-41 adds nothing, and is counted all the same
    assert gref.units(np.array([[-40.0]], F32), [0.0])[0, 0] == 0


# ---- the Python layers --------------------------------------------------------------------------------------------------------------------
def test_check_item_group_labels():
    check = engine_mod.check_item_group_labels
    lab, G = check(torch.tensor([0, 3, -5, 2], dtype=torch.int64), 4)
    assert lab.dtype == torch.int32 and lab.tolist() == [0, 3, -1, 2] and G == 4
    lab, G = check(np.array([0, 3, -5, 2], np.int32), 4, n_groups=2)        # labels >= n_groups stay: they count as the rest
    assert lab.tolist() == [0, 3, -1, 2] and G == 2
    assert check([1, 1, 1], 3)[1] == 2 and check([1, 1, 1], 3, n_groups=65536)[1] == 65536
    for bad, kw, match in (([0.0, 1.0], {}, "int32 / int64"), ([[0, 1]], {}, "int32 / int64"), ([True, False], {}, "int32 / int64"),
                           ([0, 1, 2], {}, "3 labels"), ([-1, -1], {}, "no item has a group"), ([0, 1], dict(n_groups=0), "n_groups"),
                           ([0, 1], dict(n_groups=65537), "n_groups"), ([0, 1], dict(n_groups=1.5), "n_groups"),
                           ([0, 1 << 31], {}, "fit int32"), ([0, 70000], {}, "n_groups")):
        with pytest.raises(ValueError, match=match):
            check(torch.as_tensor(bad), 2, **kw)
    with pytest.raises(ValueError, match="at most"):
        check(torch.zeros((1 << 22) + 1, dtype=torch.int32), (1 << 22) + 1)


def test_python_layers_refuse_bad_arguments_before_any_work():
    model = object.__new__(models.BERT4RecModel)            # the checks come before anything of the model's engine is touched
    model.vocab_size = 50
    labels = torch.arange(50, dtype=torch.int64) % 5
    one = torch.zeros((2, 6), dtype=torch.int64)
    one[:, 0] = 1
    batch = {"input_word_ids": torch.zeros((2, 24), dtype=torch.int64), "masked_lm_positions": torch.zeros((2, 6), dtype=torch.int64),
             "masked_lm_weights": one}
    two = one.clone()
    two[1, 3] = 1
    aff = models.BERT4RecModel.group_affinity_tensor
    for lab, kw, match in ((labels, dict(temperature=0.0), "temperature"), (labels[:49], {}, "49 labels"), (labels.to(torch.float32), {}, "int32 / int64"),
                           (labels, dict(n_groups=0), "n_groups"), (labels - 9, {}, "no item has a group"),
                           (labels, dict(allow=torch.ones(49, dtype=torch.bool)), "allow"),
                           (labels, dict(row_filter=torch.zeros(2, dtype=torch.int32)), "row_filter")):
        with pytest.raises(ValueError, match=match):
            aff(model, batch, lab, **kw)
    aud = models.BERT4RecModel.group_audience_tensor
    for b, lab, G, kw, match in ((batch, labels, None, {}, "n_groups"), (batch, labels, 5, dict(k=0), "k"), (batch, labels, 5, dict(k=1025), "k"),
                                 (batch, labels, 5, dict(min_probability=0.0), "min_probability"), (batch, labels, 5, dict(temperature=-1.0), "temperature"),
                                 (batch, labels[:3], 5, {}, "3 labels"), ({**batch, "masked_lm_weights": two}, labels, 5, {}, "one ranked slot"),
                                 ({}, labels, 5, {}, "group_audience_tensor takes prepare_inference"),
                                 (batch, labels, 5, dict(user_ids=torch.zeros(3, dtype=torch.int64)), "for 2 rows"),
                                 (batch, labels, 5, dict(forward_rows=0), "forward_rows"), (batch, labels, 5, dict(forward_rows=2.5), "forward_rows"),
                                 (batch, labels, 5, dict(state={"users": None}), "state")):
        with pytest.raises(ValueError, match=match):
            aud(model, b, lab, G, **kw)
    shelf = models.BERT4RecModel.recommend_shelves_tensor
    for lab, kw, match in ((labels, dict(shelves=0), "shelves"), (labels, dict(shelves=6), "shelves"), (labels, dict(k=0), "k"), (labels, dict(k=1025), "k"),
                           (labels, dict(n_groups=1025), "at most 1024 groups"), (labels, dict(allow=torch.ones((2, 50), dtype=torch.bool)), "one bool"),
                           (labels, dict(temperature=float("nan")), "temperature")):
        with pytest.raises(ValueError, match=match):
            shelf(model, batch, lab, **kw)

    class Stub:
        vocab_size = 50
    rec = Recommender(Stub(), None)
    by = labels.numpy()
    for call, kw, match in ((rec.category_affinity, dict(temperature=0.0), "temperature"), (rec.category_affinity, dict(top=0), "top"),
                            (rec.category_audience, dict(k=0), "k"), (rec.category_audience, dict(batch_size=0), "batch_size"),
                            (rec.category_audience, dict(user_ids=["a", "b"]), "user ids"),
                            (rec.category_audience, dict(min_probability=2), "min_probability"),
                            (rec.recommend_shelves, dict(temperature=-1.0), "temperature")):
        with pytest.raises(ValueError, match=match):
            call(**{"sequences": [[1, 2]], "by_group": by, **kw})
    with pytest.raises(ValueError, match="by_group"):
        rec.category_affinity([[1, 2]], by[:10])
    for kw, match in ((dict(shelves=6), "shelves"), (dict(shelves=0), "shelves"), (dict(k=0), "k")):
        with pytest.raises(ValueError, match=match):
            rec.recommend_shelves([], by, **kw)
    with pytest.raises(ValueError, match="at most 1024 groups"):
        Recommender(type("Big", (), {"vocab_size": 2000})(), None).recommend_shelves([], np.arange(2000), shelves=2, k=3)
    assert rec.category_affinity([], by) == [] and rec.recommend_shelves([], by, shelves=2, k=3) == []


# ---- the host side of the app calls -------------------------------------------------------------------------------------------------------
def test_pack_group_filters_against_bit_by_bit_packing():
    rng = np.random.default_rng(4)
    for V, G in ((33, 1), (70, 3), (1027, 70)):
        lab = rng.integers(-1, G + 1, size=V).astype(np.int32)
        allow = rng.random(V) < 0.8
        for mask in (None, allow):
            want = np.zeros((G + 1, V), bool)
            for g in range(G):
                want[g] = (lab == g) & (True if mask is None else mask)
            got = engine_mod.pack_group_filters(torch.from_numpy(lab), G, None if mask is None else torch.from_numpy(mask))
            assert got.dtype == torch.uint32 and tuple(got.shape) == (G + 1, (V + 31) // 32)
            assert np.array_equal(got.view(torch.int32).numpy().view(np.uint32), ref.pack_bits(want))
            assert not got.view(torch.int32)[G].any()                       # the last filter admits nothing


def test_affinity_lists_order_ties_and_empty_groups():
    one = 1 << 40
    mass = torch.tensor([[one // 4, one // 2, 0, one // 4, 0], [0, 0, 0, 0, 0], [5, 5, 5, 0, 7]])
    n = torch.tensor([[3, 1, 2, 9, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]])
    slots = torch.tensor([0, 6, 13])                                         # P = 6: users 0, 1, 2 (user 3 has no ranked slot)
    names = ["a", "b", "c", "d", "e"]
    lists = Recommender._affinity_lists(mass, n, slots, 6, 4, names, None)
    assert lists[0] == [("b", 0.5), ("a", 0.25), ("d", 0.25), ("c", 0.0)]    # a tie keeps the lower group first; n = 0 is left out
    assert lists[1] == [] and lists[3] == []
    assert [g for g, _ in lists[2]] == ["e", "a", "b", "c", "d"]
    assert Recommender._affinity_lists(mass, n, slots, 6, 4, None, 2)[0] == [(1, 0.5), (0, 0.25)]


def test_hidden_in_blocks_places_every_user_by_its_id():
    """The forward of group_audience_tensor: user u sits at place u mod block of a block of exactly `block` rows, whatever the batch"""
    block, seen = 8, []

    class Stub:
        device = torch.device("cpu")

        def _ranked_slot_hidden(self, part, slots=None):
            assert part["input_word_ids"].shape[0] == block and slots.tolist() == [b * 3 + 1 for b in range(block)]
            seen.append(part["input_word_ids"][:, 0].tolist())
            return part["input_word_ids"][:, :1].to(torch.float32) * 10.0, slots, None

    for users in ([0, 1, 2], [5], [13, 21, 29, 6, 7, 8, 9, 10, 11, 12, 14], [-1, 7, 15, -9], list(range(100, 119))):
        B = len(users)
        seen.clear()
        batch = {"input_word_ids": torch.arange(B)[:, None].repeat(1, 4) + 1000, "masked_lm_positions": torch.zeros((B, 3), dtype=torch.int64),
                 "other": None}
        hidden = models.BERT4RecModel._hidden_in_blocks(Stub(), batch, B, 3, torch.ones(B, dtype=torch.int64), block, torch.as_tensor(users))
        assert hidden[:, 0].tolist() == [(1000 + r) * 10.0 for r in range(B)]
        for r, u in enumerate(users):
            assert sum(rows[u % block] == 1000 + r for rows in seen) >= 1      # the row sits at its user's place in some block
        most = max(sum(1 for u in users if u % block == p) for p in range(block))
        assert len(seen) == most                                              # as many blocks as the fullest place needs
    assert len(seen) == 3                                                     # 19 consecutive ids: ceil((100 % 8 + 19) / 8) blocks, no gaps inside


def test_check_shelf_args():
    assert engine_mod.check_shelf_args(3, 10, 20) == (3, 10) and engine_mod.check_shelf_args(1024, 1024, 1024) == (1024, 1024)
    for s, k, G in ((0, 1, 5), (6, 1, 5), (1, 0, 5), (1, 1025, 5), (1, 1, 1025), (True, 1, 5)):
        with pytest.raises(ValueError):
            engine_mod.check_shelf_args(s, k, G)


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_lib_binds_the_new_symbol():
    lib = _lib.load()
    assert "b4r_group_mass" in _lib.PROTOTYPES and len(_lib.PROTOTYPES["b4r_group_mass"][1]) == 24
    assert lib.b4r_group_mass.argtypes == _lib.PROTOTYPES["b4r_group_mass"][1]


def test_c_abi_refuses_bad_arguments_before_touching_the_device():
    lib = _lib.load()
    table = np.zeros(64 * 8 + 4, F32)
    tp = (table.ctypes.data + 15) & ~15                                 # (never read: every call below returns before a launch)

    def call(R=4, H=64, ld=None, V=1000, first=3, E=0, exclude=None, inv_t=1.0, hidden=tp, tab=tp, allow=None, n_filters=0, lse=tp,
             lab=tp, G=5, mass=tp, n=tp, rest_mass=None, rest_n=None):
        return lib.b4r_group_mass(hidden, H if ld is None else ld, None, tab, None, H, V, first, R, exclude, E, allow, n_filters, None,
                                  None, inv_t, lse, lab, G, mass, n, rest_mass, rest_n, None)
    for kw in (dict(R=-1), dict(E=-1), dict(first=-1), dict(H=30), dict(H=4100), dict(ld=60), dict(V=0), dict(V=(1 << 22) + 1), dict(G=-1),
               dict(G=65537), dict(allow=tp, n_filters=0)):
        assert call(**kw) == -2 and "b4r_group_mass" in _lib.last_error(), kw
    for inv_t in (0.0, -1.0, float("nan"), float("inf")):
        assert call(inv_t=inv_t) == -1 and "inv_temperature" in _lib.last_error()
    assert call(R=0) == 0                                              # nothing to do: no launch, no pointer is looked at
    assert call(G=0) == 0 and call(mass=None, n=None) == 0             # no output to write
    assert call(G=0, hidden=None, lab=None) == 0
    assert call(hidden=None) == -1 and call(tab=None) == -1 and call(lse=None) == -1 and "null" in _lib.last_error()
    assert call(lab=None) == -1 and "item_group" in _lib.last_error()
    assert call(G=0, rest_n=tp, lse=None) == -1                        # a rest output is work: the arguments are looked at
    assert call(E=3) == -1 and "exclude" in _lib.last_error()
    assert call(tab=tp + 4) == -3
