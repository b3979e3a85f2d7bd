"""The inference matrix (tests/inference_matrix.py) on the CPU: every cell of tests/feature_matrix.py and tests/geometry_matrix.py has
an inference record per mode group it runs in, every form of the encoder-only forward is exercised by some cell, every item-table
width has a cell -- and the fp32 restatement passes the GPU test's own criteria (tests/inference_checks.py) against the fp64
restatement at every cell, with the bounds derived from its own error: criteria the reference failed would be wrong criteria."""
import numpy as np
import pytest
import torch

from tests import feature_matrix as fm
from tests import geometry_matrix as gm
from tests import inference_checks as ic
from tests import inference_matrix as im

FORM_NAMES = {"attn": {"Block", "SlotQuery", "Core", "Core64"}, "ffn": {"Block", "Wide", "CompactRows", "TileProducts"}}


def test_every_cell_of_both_matrices_has_an_inference_record_in_every_mode_it_runs():
    assert not set(fm.CELLS) & set(gm.CELLS), "cell names must be unique across the matrices"
    assert set(im.CELLS) == set(fm.CELLS) | set(gm.CELLS)
    for name, train in list(fm.CELLS.items()) + list(gm.CELLS.items()):
        c = im.CELLS[name]
        assert c.modes == train.modes and set(c.modes) <= set(im.MODES) and "bf16x3" in c.modes, name
        assert (c.H, c.heads, c.inner, c.L, c.P, c.E, c.acts) == (train.H, train.heads, train.inner, train.L, train.P, train.E,
                                                                 train.acts), name
        assert c.layers == getattr(train, "layers", fm.LAYERS) and c.V == getattr(train, "V", fm.VOCAB), name
        for mode in c.modes:
            f = c.forms(mode)
            assert isinstance(f, im.InferenceForms), (name, mode)
            assert len(f.attn_fwd) == len(f.ffn) == c.layers, (name, mode)
            assert set(f.attn_fwd) <= FORM_NAMES["attn"] and set(f.ffn) <= FORM_NAMES["ffn"], (name, mode)
            assert f.slotq_rows == (f.attn_fwd[-1] == "SlotQuery") and "SlotQuery" not in f.attn_fwd[:-1], (name, mode)
            assert not f.slotq_rows or f.ffn[-1] == "CompactRows", (name, mode)
            assert "CompactRows" not in f.ffn[:-1], (name, mode)
            assert f.emb_proj == (c.E is not None) and not (f.emb_proj and f.emb_fused), (name, mode)
            assert all(a == "Core64" for a in f.attn_fwd) == (c.head_dim == 64), (name, mode)
            assert not f.slot_only_last or (f.attn_fwd[-1] == "Block" and f.ffn[-1] == "Block"), (name, mode)
            if mode == "f32":   # exact fp32 runs no fused block, no slot queries and no Wide pair
                assert not {"Block", "SlotQuery"} & set(f.attn_fwd) and not {"Block", "Wide"} & set(f.ffn), name
        assert (c.f32 is None) == ("f32" not in c.modes), name
        # the evaluation batch's compact rows: 2 P <= L is the library's own condition, B * P must differ from B * L for the labels
        assert c.P < c.L, name


def test_the_rule_gives_the_pinned_records():
    for (name, group), want in im.PINNED.items():
        c = im.CELLS[name]
        assert (c.split if group == "split" else c.f32) == want, (name, group)
    # the one form an encoder-only forward plans differently: the Wide pair at hidden 256, split modes, never on the compact rows
    for name, c in im.CELLS.items():
        train = (fm.CELLS.get(name) or gm.CELLS[name])
        for mode in c.modes:
            t, f = train.forms(mode), c.forms(mode)
            assert f.attn_fwd == t.attn_fwd and (f.emb_proj, f.emb_fused, f.slot_only_last, f.slotq_rows) == \
                (t.emb_proj, t.emb_fused, t.slot_only_last, t.slotq_rows), (name, mode)
            for a, b in zip(t.ffn, f.ffn):
                assert a == b or (a == "TileProducts" and b == "Wide" and c.H == 256 and mode != "f32"), (name, mode)
            assert c.H != 256 or mode == "f32" or "TileProducts" not in f.ffn, (name, mode)


def covered(pred):
    return sorted((n, m) for n, c in im.CELLS.items() for m in c.modes if pred(c, c.forms(m), m))


def test_every_form_of_the_encoder_only_forward_is_exercised():
    need = {
        "Block with the slot-only last layer": lambda c, f, m: f.slot_only_last and not c.sweeps_every_query(m),
        "Block sweeping every query": lambda c, f, m: f.attn_fwd[-1] == "Block" and c.sweeps_every_query(m),
        "SlotQuery": lambda c, f, m: f.attn_fwd[-1] == "SlotQuery",
        "CompactRows from a gather": lambda c, f, m: f.ffn[-1] == "CompactRows" and not f.slotq_rows,
        "CompactRows from the slot-query attention": lambda c, f, m: f.ffn[-1] == "CompactRows" and f.slotq_rows,
        "Wide at hidden 128": lambda c, f, m: c.H == 128 and "Wide" in f.ffn,
        "Wide at hidden 256": lambda c, f, m: c.H == 256 and "Wide" in f.ffn,
        "Wide in the last layer": lambda c, f, m: f.ffn[-1] == "Wide",
        "TileProducts": lambda c, f, m: "TileProducts" in f.ffn,
        "TileProducts in the last layer": lambda c, f, m: f.ffn[-1] == "TileProducts",
        "Core64": lambda c, f, m: "Core64" in f.attn_fwd,
        "emb_proj": lambda c, f, m: f.emb_proj,
        "emb_fused": lambda c, f, m: f.emb_fused,
        "a single layer": lambda c, f, m: c.layers == 1,
        "32 layers": lambda c, f, m: c.layers == 32,
        "exact fp32 with a factorised table": lambda c, f, m: m == "f32" and f.emb_proj,
        "mode 2 with the Wide pair at hidden 256": lambda c, f, m: m == "bf16" and c.H == 256 and "Wide" in f.ffn,
        "a non-GELU masked-LM activation with E != H": lambda c, f, m: c.E is not None and c.acts[1] != "gelu",
    }
    for what, pred in need.items():
        assert covered(pred), f"no cell exercises: {what}"
    # every width of the item table the ranking kernels meet (hidden 32 ... 1024, E = 64 / 128 / 256)
    assert {c.width for c in im.CELLS.values()} >= {32, 64, 128, 256, 512, 1024}
    assert {m for c in im.CELLS.values() for m in c.modes} == set(im.MODES)


def test_the_shape_changes_fit_their_models():
    assert 3 <= len(im.SHAPE_CHANGES) <= 6
    for (name, mode), ((L, P), (L2, P2)) in im.SHAPE_CHANGES.items():
        c = im.CELLS[name]
        assert mode in c.modes and max(L, L2) <= c.L and (L, P) != (L2, P2) and 0 < P < L and 0 < P2 < L2, name


def test_the_edge_rows_of_the_evaluation_batch():
    b = ic.eval_batch(8, 200, 40, 1000)
    n = b["input_mask"].sum(dim=1)
    w = b["masked_lm_weights"]
    assert int(n[0]) == 1 and int(b["masked_lm_positions"][0, 0]) == 0 and int(w[0].sum()) == 1
    assert int(n[1]) == 200 and int(b["masked_lm_positions"][1, 0]) == 199
    assert int(w[2].sum()) == 1 and int(b["masked_lm_positions"][2, 0]) < int(n[2]) - 1
    assert int(w[3].sum()) == 2
    assert bool((b["masked_lm_positions"][w == 0] == 0).all()) and bool((b["masked_lm_ids"][w == 0] == 0).all())
    assert bool((w[4:].sum(dim=1) == 1).all())
    assert bool((b["input_word_ids"][w.sum(dim=1) > 0, :][b["labels"][w.sum(dim=1) > 0, :] == 0] == 0).all())
    rk = ic.ranked_slots(b)
    assert rk.rows.numel() == 9 and bool((b["input_word_ids"].reshape(-1)[rk.rows] == 1).all())
    assert bool((b["labels"].reshape(-1)[rk.rows] == rk.gt).all())


def test_the_interval_criteria_fail_a_wrong_answer():
    """a swapped pair beyond the tolerance, an excluded id, a rank off by one outside its interval"""
    ref = np.array([[0.0, 0.0, 0.0, 0.9, 0.8, 0.7, 0.6, 0.5]])
    ok = ic.allowed(8, np.array([[6, -1]]))
    ic.check_top_k(np.array([[3, 4, 5]]), ref, ok, 3, 1e-3)
    ic.check_top_k(np.array([[4, 3, 5]]), ref, ok, 3, 0.2)
    for bad in ([[4, 3, 5]], [[3, 4, 6]], [[3, 4, 7]], [[3, 3, 4]], [[3, 4, -1]], [[2, 3, 4]]):
        with pytest.raises(AssertionError):
            ic.check_top_k(np.array(bad), ref, ok, 3, 1e-3)
    assert ic.rank_interval(ref[0], 5, 1e-3, ok[0]) == (3, 3) and ic.rank_interval(ref[0], 5, 0.15, ok[0]) == (2, 3)
    ic.check_gt_ranks([3], ref, [5], 1e-3, ok)
    with pytest.raises(AssertionError):
        ic.check_gt_ranks([2], ref, [5], 1e-3, ok)


@pytest.mark.parametrize("name", list(im.CELLS))
def test_the_fp32_restatement_passes_the_criteria_against_the_fp64_one(name):
    """checks 3 - 5 of tests/test_gpu_inference_matrix.py with the fp32 restatement in the library's place, at the exact-fp32 bound"""
    c = im.CELLS[name]
    cfg_o, params = ic.cell_params(c)
    batch = ic.eval_batch(im.BATCH, c.L, c.P, c.V)
    rk = ic.ranked_slots(batch)
    ref32, ref64 = ic.restatement(params, batch, cfg_o, c.acts, torch.float32), ic.restatement(params, batch, cfg_o, c.acts, torch.float64)
    e32 = ic.e32_of(ref32, ref64)
    print(f"{name}: e32 {e32}")
    assert all(0.0 < e < 1e-4 for e in e32.values()), e32
    for q in ic.QUANTITIES:
        assert float((ref32[q].double() - ref64[q]).abs().max()) <= ic.bound("f32", e32[q])
    tol = 2 * ic.bound("f32", e32["scores"])
    s32, s64 = ref32["scores"].numpy(), ref64["scores"].numpy()
    ex_eval, ex_rec, _ = ic.exclusion_lists(batch, rk, c.V)
    for ex, gt in ((ex_eval, rk.gt.numpy()), (ex_rec, None)):
        ok = ic.allowed(c.V, ex.numpy(), gt)
        ic.check_top_k(ic.stable_top_k(s32, ok, ic.TOP_K), s64, ok, ic.TOP_K, tol, name)
        if gt is not None:
            ic.check_gt_ranks([ic.counted_rank(s32[r], int(gt[r]), ok[r]) for r in range(len(gt))], s64, gt, tol, ok, name)
    cand = ic.draw_candidates(c.V, rk.gt.numpy())
    g = cand.shape[1] - 1
    c32, c64 = np.take_along_axis(s32, cand, 1), np.take_along_axis(s64, cand, 1)
    ic.check_gt_ranks([ic.counted_rank(c32[r], g) for r in range(len(cand))], c64, [g] * len(cand), tol, None, name)
