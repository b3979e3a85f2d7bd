"""The feature-by-form matrix (tests/feature_matrix.py) covers what it claims to: every launch form of plan_step in every mode that
plan_step allows it in, every activation in both roles at a length where the long-sequence forms run, and the factorised widths at
the benchmark length.  Runs without a GPU, so the table cannot silently shrink."""
import os
import re

from bert4rec_amd import activations
from tests.feature_matrix import CELLS, EVAL_CELLS, LAYERS, MODES, REPRO_CELL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the table's names of the forms of plan_step's enums (the core's backward by its kernels, the core at head width 64 apart)
ENUM_OF = {"Core16": "Core", "Core32": "Core", "Core64": "Core"}
# (form, mode) pairs plan_step can reach in a train step: the fused blocks, the slot queries, the Wide pair and the 32-token-tile
# core need a split mode (b4r_split_mode); the exact-fp32 mode runs the cores and the tile products, compact rows gathered
SPLIT_FORMS = {("attn_fwd", f) for f in ("Block", "SlotQuery", "Core", "Core64")} | \
              {("attn_bwd", f) for f in ("Block", "BlockFolded", "SlotQuery", "Core16", "Core32", "Core64")} | \
              {("ffn", f) for f in ("Block", "Wide", "CompactRows", "TileProducts")} | \
              {("flag", f) for f in ("emb_proj", "emb_fused", "slot_only_last", "slotq_rows", "compact_rows_gathered")}
ALLOWED = {"f32": {("attn_fwd", "Core"), ("attn_fwd", "Core64"), ("attn_bwd", "Core16"), ("attn_bwd", "Core64"),
                   ("ffn", "CompactRows"), ("ffn", "TileProducts"), ("flag", "emb_proj"), ("flag", "compact_rows_gathered")},
           "bf16x3": SPLIT_FORMS, "bf16": SPLIT_FORMS}


def pairs(forms):
    out = {("attn_fwd", f) for f in forms.attn_fwd} | {("attn_bwd", f) for f in forms.attn_bwd} | {("ffn", f) for f in forms.ffn}
    for flag in ("emb_proj", "emb_fused", "slot_only_last", "slotq_rows"):
        if getattr(forms, flag):
            out.add(("flag", flag))
    if "CompactRows" in forms.ffn and not forms.slotq_rows:
        out.add(("flag", "compact_rows_gathered"))
    return out


def plan_enums():
    src = open(os.path.join(ROOT, "bert4rec_amd", "csrc", "b4r_model.hip")).read()
    return {name: {v.strip() for v in body.split(",")} for name, body in re.findall(r"enum class (\w+) \{([^}]*)\}", src)}


def test_every_cell_is_well_formed():
    for name, c in CELLS.items():
        assert c.H % c.heads == 0 and c.head_dim in (32, 64), name
        assert set(c.modes) <= set(MODES) and c.modes, name
        assert (c.f32 is not None) == ("f32" in c.modes), name
        assert c.L <= 256 and 0 < c.P <= c.L, name
        assert c.E in (None, 64, 128, 256) and (c.E is None or c.E < c.H), name
        for mode in c.modes:
            f = c.forms(mode)
            assert len(f.attn_fwd) == len(f.attn_bwd) == len(f.ffn) == LAYERS, (name, mode)
            assert f.slotq_rows == (f.attn_fwd[-1] == "SlotQuery" == f.attn_bwd[-1]), (name, mode)
            assert not f.slotq_rows or f.ffn[-1] == "CompactRows", (name, mode)
            assert f.emb_proj == (c.E is not None) and not (f.emb_proj and f.emb_fused), (name, mode)
            assert all(a.startswith("Core64") for a in f.attn_fwd + f.attn_bwd) == (c.head_dim == 64), (name, mode)
    assert set(EVAL_CELLS) <= set(CELLS) and REPRO_CELL in CELLS and "bf16" in CELLS[REPRO_CELL].modes


def test_every_form_of_plan_step_appears():
    enums = plan_enums()
    assert set(enums) >= {"AttnFwd", "AttnBwd", "FfnForm"}, enums
    seen = {"AttnFwd": set(), "AttnBwd": set(), "FfnForm": set()}
    flags = set()
    for c in CELLS.values():
        for mode in c.modes:
            f = c.forms(mode)
            seen["AttnFwd"] |= {ENUM_OF.get(a, a) for a in f.attn_fwd}
            seen["AttnBwd"] |= {ENUM_OF.get(a, a) for a in f.attn_bwd}
            seen["FfnForm"] |= set(f.ffn)
            flags |= {n for n in ("emb_proj", "emb_fused", "slot_only_last", "slotq_rows") if getattr(f, n)}
    for enum, values in seen.items():
        assert values == enums[enum], (enum, values, enums[enum])
    assert flags == {"emb_proj", "emb_fused", "slot_only_last", "slotq_rows"}
    assert {c.head_dim for c in CELLS.values()} == {32, 64}


def test_every_form_and_mode_pair_that_plan_step_allows_appears():
    for mode in MODES:
        got = set()
        for c in CELLS.values():
            if mode in c.modes:
                got |= pairs(c.forms(mode))
        assert got == ALLOWED[mode], (mode, sorted(ALLOWED[mode] - got), sorted(got - ALLOWED[mode]))
    # ... and each core backward of the split modes behind a factorised embedding (layer 0's dx0 goes into embed_proj_bwd)
    for mode in ("bf16x3", "bf16"):
        for core in ("Core16", "Core32", "Core64"):
            assert any(c.E and core in c.forms(mode).attn_bwd for c in CELLS.values() if mode in c.modes), (mode, core)


def test_every_activation_runs_in_both_roles_beyond_length_64():
    ids = sorted(set(activations.IDS.values()))
    name_of = {activations.IDS[n]: n for n in activations.NAMES}
    for role in (0, 1):
        got = {activations.IDS[c.acts[role]] for c in CELLS.values() if c.L > 64}
        assert got == set(ids), (role, sorted(name_of[i] for i in set(ids) - got))
    for mode in ("bf16x3", "bf16"):   # every feed-forward epilogue in both split modes (at one term in mode 2)
        assert {activations.IDS[c.acts[0]] for c in CELLS.values() if mode in c.modes} == set(ids), mode


def test_factorised_widths_run_at_the_benchmark_length():
    for E in (64, 128):
        assert any(c.E == E and c.L >= 200 for c in CELLS.values()), E
        assert any(c.E == E and c.L >= 200 and "bf16" in c.modes for c in CELLS.values()), E
    # E = 64 with the slot-query attention and E-wide compact rows in mode 2
    assert any(c.E == 64 and c.split.slotq_rows and "bf16" in c.modes for c in CELLS.values())
