"""What the Recommender hands to the model, without a GPU: a real dataloader and tokenizer over a vocabulary of 12 tokens, and a stub
model that records the arguments of recommend_tensor, recommend_sequence_tensor, explain_tensor and audience_tensor.  The expected
batches, exclusion matrices, filters, streams and item ids are written out by hand.

The vocabulary: [PAD] 0, [MASK] 1, [UNK] 2, "i0" .. "i8" = 3 .. 11.  The model window holds 5 tokens, 2 prediction slots."""
import pytest
import torch

from bert4rec_amd import engine as engine_mod
from bert4rec_amd.apps import Recommender
from bert4rec_amd.dataloaders.bert4rec_dataloader import BERT4RecDataloader

V, L, P = 12, 5, 2
HISTORIES = [["i0"], ["i1", "i2", "i3"], ["i1", "i2", "i3", "i4", "i5", "i6"]]     # length 1, length 3, longer than the window
TOKENS = [[3, 1, 0, 0, 0], [4, 5, 6, 1, 0], [6, 7, 8, 9, 1]]
MASK = [[1, 1, 0, 0, 0], [1, 1, 1, 1, 0], [1, 1, 1, 1, 1]]
POSITIONS = [[1, 0], [3, 0], [4, 0]]
WEIGHTS = [[1, 0], [1, 0], [1, 0]]
EXCLUDE = [[3, -1, -1, -1, -1, -1], [4, 5, 6, -1, -1, -1], [4, 5, 6, 7, 8, 9]]     # the whole history, also before the window
# users 0 and 1 give the same allow-list in another order (one filter), user 2 only items the vocabulary does not know (an empty one)
PER_USER = [["i0", "i4", "nope"], ["i4", "i0"], ["nope", "nada"]]
ROW_FILTER = [0, 0, 1]
ALLOW_ROWS = [[3, 7], []]
ALLOW_WORDS = [[(1 << 3) | (1 << 7)], [0]]                                          # the same filters packed (pack_item_filter)
SHARED = ["i8", "nope", "i1"]                                                       # allowed_items: tokens 11 and 4


def mask_rows(rows):
    m = torch.zeros((len(rows), V), dtype=torch.bool)
    for f, tokens in enumerate(rows):
        m[f, tokens] = True
    return m


class StubEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.params = torch.zeros(1)
        self.calls = []

    def audience_state(self, item_ids, k):
        return engine_mod.Engine.audience_state(self, item_ids, k)

    def list_metrics(self, ids, gt, weight, exposure=None, sums=None, counts=None):
        self.calls.append(dict(ids=ids, gt=gt, weight=weight))


class StubModel:
    """Records every call and returns results of the right shapes that recommend nothing (-1 everywhere)."""
    vocab_size = V

    def __init__(self):
        self.engine = StubEngine()
        self.calls = []

    def recommend_tensor(self, batch, **kw):
        self.calls.append(dict(kw, batch=batch))
        R, k = int((batch["masked_lm_weights"] != 0).sum()), kw["k"]
        slots = torch.nonzero((batch["masked_lm_weights"] != 0).reshape(-1)).reshape(-1)
        out = (torch.full((R, k), -1, dtype=torch.int64), torch.full((R, k), float("-inf")), slots)
        return out + ({"logp": torch.full((R, k), float("-inf"))},) if kw["return_distribution"] else out

    def recommend_sequence_tensor(self, batch, steps, **kw):
        self.calls.append(dict(kw, batch=batch, steps=steps))
        U, beams = batch["input_word_ids"].shape[0], kw["beams"]
        ids = torch.full((U, beams, steps), -1, dtype=torch.int64)
        if not kw["return_logp"]:
            return ids, None, None, None
        return ids, torch.full((U, beams, steps), float("-inf")), torch.full((U, beams), float("-inf")), None

    def explain_tensor(self, batch, target, **kw):
        self.calls.append(dict(kw, batch=batch, target=target))
        U, top = batch["input_word_ids"].shape[0], kw["top"]
        ids = torch.full((U, target), -1, dtype=torch.int64) if isinstance(target, int) else target
        K = ids.shape[1]
        return {"target_ids": ids, "base_logp": torch.zeros((U, K)), "top_item": torch.full((U, K, top), -1, dtype=torch.int64),
                "top_label": torch.full((U, K, top), -1, dtype=torch.int64), "top_delta": torch.full((U, K, top), float("-inf")),
                "top_w": torch.full((U, K, top), -1, dtype=torch.int32), "removed": torch.zeros((U, L - 1), dtype=torch.int32)}

    def audience_tensor(self, batch, item_ids, **kw):
        self.calls.append(dict(kw, batch=batch, item_ids=item_ids))
        return kw["state"]

    def similar_items_tensor(self, item_ids, **kw):
        self.calls.append(dict(kw, item_ids=item_ids))
        return torch.full((item_ids.numel(), kw["k"]), -1, dtype=torch.int64), None


@pytest.fixture
def rec():
    dl = BERT4RecDataloader(max_seq_len=L, max_predictions_per_seq=P)
    dl.generate_vocab(source=[f"i{n}" for n in range(9)])
    assert dl.get_tokenizer().get_vocab_size() == V
    yield Recommender(StubModel(), dl)
    assert dl.get_tokenizer().get_vocab_size() == V        # no unknown item of an allow-list or an item list was added


def same(got, want, dtype):
    return torch.is_tensor(got) and got.dtype == dtype and torch.equal(got, torch.as_tensor(want, dtype=dtype))


def check_batch(batch, rows=slice(None)):
    for key, want in (("input_word_ids", TOKENS), ("input_mask", MASK), ("masked_lm_positions", POSITIONS), ("masked_lm_weights", WEIGHTS)):
        assert same(batch[key], want[rows], torch.int64), key
    assert same(batch["masked_lm_ids"], [[2, 0]] * len(TOKENS[rows]), torch.int64)   # the placeholder [UNK] under the mask


def test_recommend_batch_requests(rec):
    assert rec.recommend_batch(HISTORIES, 2, allowed_items_per_user=PER_USER, sample_seed=5, user_streams=[7, 1 << 40, -9]) == [[], [], []]
    assert rec.recommend_batch(HISTORIES, 1, allowed_items=SHARED, return_probabilities=True) == [None, None, None]
    assert rec.recommend_batch(HISTORIES, 3) == [[], [], []]
    per_user, shared, plain = rec.model.calls
    for call in (per_user, shared, plain):
        check_batch(call["batch"])
        assert same(call["exclude"], EXCLUDE, torch.int64) and call["exclude_seen"] is False
    assert same(per_user["allow"], mask_rows(ALLOW_ROWS), torch.bool)
    assert same(per_user["row_filter"], ROW_FILTER, torch.int32)         # one index per ranked slot: one slot per user here
    assert same(per_user["sample_streams"], [7, 1 << 40, -9], torch.int64) and per_user["sample_seed"] == 5 and per_user["k"] == 2
    assert same(shared["allow"], mask_rows([[4, 11]])[0], torch.bool) and shared["row_filter"] is None
    assert shared["sample_streams"] is None and shared["return_distribution"] is True
    assert plain["allow"] is None and plain["row_filter"] is None and plain["sample_streams"] is None and plain["k"] == 3


def test_recommend_sequences_requests(rec):
    assert rec.recommend_sequences(HISTORIES, 3, allowed_items_per_user=PER_USER, sample_seed=5, user_streams=[7, 1 << 40, -9]) == [[], [], []]
    assert rec.recommend_sequences(HISTORIES, 2, beams=2, allowed_items=SHARED) == [[], [], []]
    assert rec.recommend_sequences(HISTORIES, 1) == [[], [], []]
    per_user, shared, plain = rec.model.calls
    for call in (per_user, shared, plain):
        check_batch(call["batch"])
        assert same(call["exclude"], EXCLUDE, torch.int64) and call["exclude_seen"] is False
    assert same(per_user["allow"], mask_rows(ALLOW_ROWS), torch.bool) and same(per_user["row_filter"], ROW_FILTER, torch.int32)
    assert same(per_user["sample_streams"], [7, 1 << 40, -9], torch.int64) and per_user["steps"] == 3 and per_user["return_logp"] is False
    assert same(shared["allow"], mask_rows([[4, 11]])[0], torch.bool) and shared["row_filter"] is None
    assert shared["sample_streams"] is None and shared["beams"] == 2 and shared["return_logp"] is True
    assert plain["allow"] is None and plain["row_filter"] is None and plain["sample_streams"] is None


def test_explain_batch_requests(rec):
    given = [["i2", "nope"], ["i5"], ["i1", "i3"]]
    got = rec.explain_batch(HISTORIES, items=given, top=2, allowed_items_per_user=PER_USER)
    assert got == [[("i2", 1.0, []), ("nope", 1.0, [])], [("i5", 1.0, [])], [("i1", 1.0, []), ("i3", 1.0, [])]]
    assert rec.explain_batch(HISTORIES, k=4, allowed_items=SHARED) == [[], [], []]
    assert rec.explain_batch(HISTORIES) == [[], [], []]
    per_user, shared, plain = rec.model.calls
    for call in (per_user, shared, plain):
        check_batch(call["batch"])
        assert same(call["exclude"], EXCLUDE, torch.int64) and call["exclude_seen"] is False
    assert same(per_user["target"], [[5, -1], [8, -1], [4, 6]], torch.int64)       # unknown items and the padding are -1
    assert same(per_user["allow"], mask_rows(ALLOW_ROWS), torch.bool) and same(per_user["row_filter"], ROW_FILTER, torch.int32)
    assert shared["target"] == 4 and same(shared["allow"], mask_rows([[4, 11]])[0], torch.bool) and shared["row_filter"] is None
    assert plain["target"] == 1 and plain["allow"] is None and plain["row_filter"] is None


def test_audience_requests_in_batches_of_two(rec):
    nobody = {"users": [], "reach": 0, "expected_demand": 0.0}
    assert rec.audience(["i2", "nope", "i8"], HISTORIES, k=4, batch_size=2, allowed_items_per_user=PER_USER) == [nobody] * 3
    first, second = rec.model.calls
    check_batch(first["batch"], slice(0, 2))
    check_batch(second["batch"], slice(2, 3))
    assert same(first["exclude"], [[3, -1, -1], [4, 5, 6]], torch.int64)            # as wide as the batch's longest history
    assert same(second["exclude"], EXCLUDE[2:], torch.int64)
    assert same(first["row_filter"], [0, 0], torch.int32) and same(second["row_filter"], [1], torch.int32)
    assert same(first["user_ids"], [0, 1], torch.int64) and same(second["user_ids"], [2], torch.int64)
    for call in (first, second):
        assert same(call["item_ids"], [5, -1, 11], torch.int64) and call["k"] == 4 and call["exclude_seen"] is False
        assert call["allow"].dtype == torch.uint32 and torch.equal(call["allow"].view(torch.int32), torch.tensor(ALLOW_WORDS, dtype=torch.int32))
    assert second["state"] is first["state"]
    rec.model.calls.clear()
    assert rec.audience(["i2"], HISTORIES, batch_size=256, allowed_items=SHARED) == [nobody]
    assert rec.audience(["i2"], HISTORIES, batch_size=3) == [nobody]
    shared, plain = rec.model.calls
    for call in (shared, plain):
        check_batch(call["batch"])
        assert same(call["exclude"], EXCLUDE, torch.int64) and same(call["user_ids"], [0, 1, 2], torch.int64) and call["row_filter"] is None
    assert torch.equal(shared["allow"].view(torch.int32), torch.tensor([[(1 << 4) | (1 << 11)]], dtype=torch.int32)) and plain["allow"] is None


def test_both_filters_or_a_wrong_number_of_lists_are_refused_and_no_sequences_give_nothing(rec):
    calls = {"recommend_batch": lambda seqs, **kw: rec.recommend_batch(seqs, 2, **kw),
             "recommend_sequences": lambda seqs, **kw: rec.recommend_sequences(seqs, 2, **kw),
             "explain_batch": lambda seqs, **kw: rec.explain_batch(seqs, **kw),
             "audience": lambda seqs, **kw: rec.audience(["i2"], seqs, **kw)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match="give allowed_items or allowed_items_per_user, not both"):
            call(HISTORIES, allowed_items=SHARED, allowed_items_per_user=PER_USER)
        with pytest.raises(ValueError, match="2 allow-lists for 3 sequences"):
            call(HISTORIES, allowed_items_per_user=PER_USER[:2])
        with pytest.raises(ValueError, match="1 allow-lists for 0 sequences"):
            call([], allowed_items_per_user=PER_USER[:1])
        if name != "audience":
            assert call([]) == [] and call([], allowed_items=SHARED) == [] and call([], allowed_items_per_user=[]) == [], name
    # an audience is per item: no users give every item an empty one, no items give nothing
    assert rec.audience(["i2", "i3"], [], allowed_items_per_user=[]) == [{"users": [], "reach": 0, "expected_demand": 0.0}] * 2
    assert rec.audience([], HISTORIES) == []
    assert rec.model.calls == []


def test_similar_items_and_list_quality_requests(rec):
    assert rec.similar_items(["i7", "nope", "i0"], k=3, allowed_items=SHARED) == [[], [], []]
    call, = rec.model.calls
    assert same(call["item_ids"], [10, -1, 3], torch.int64) and same(call["allow"], mask_rows([[4, 11]])[0], torch.bool)
    rec.list_quality([["i1", "nope", "i2"], [], ["i8"]])
    assert same(rec.model.engine.calls[0]["ids"], [[4, 5], [-1, -1], [11, -1]], torch.int64)
    assert rec.list_quality([[], ["nope"]]) == {"ild": 0.0, "coverage": 0.0} and len(rec.model.engine.calls) == 1
