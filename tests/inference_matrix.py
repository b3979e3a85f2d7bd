"""The inference record of every cell of tests/feature_matrix.py and tests/geometry_matrix.py (tests/test_gpu_inference_matrix.py runs
it on the GPU; tests/test_inference_matrix_host.py checks its coverage on the CPU): the launch forms plan_step
(bert4rec_amd/csrc/b4r_model.hip) picks for the evaluation path's forward, B4R_FLAG_ENCODER_ONLY | B4R_FLAG_HEAD_ROWS_ONLY
(Engine.encoder_forward(ranked_rows_only=True)), per mode group.

What plan_step does under those flags, read off its source:

* every predicate but one reads the model, (L, P), the presence of the slots and the gemm mode only -- so the attention forward of
  every layer, emb_proj, emb_fused, slot_only_last, the compact rows of the last layer and where they come from (slotq_rows) are the
  train step's forward half;
* the exception is `wide`: the one-launch feed-forward pair (b4r_ffn32w.hip: hidden 128 / 256, inner a multiple of 32 from 64, split
  modes) runs in a train step at hidden 128 only, in an encoder-only forward at hidden 256 as well.  So at hidden 256 every layer
  that is TileProducts in the train step's split-mode record is Wide here; the last layer on compact rows stays CompactRows;
* forward_impl then drops the Wide launch's stores of f and the pre-activation (keep = false) and needs the encoder's regions of the
  workspace only (ws_need = w.gath); the compact rows live inside the last layer's own regions.

slot_only_last (hidden 64, split modes, 65 <= L <= 208, P <= 64): the last layer's attention block sweeps the slots' queries only.  No
label shows it; the GPU test reads it from the rows of the last layer's context the forward wrote.  Layer 0's block carries the
embedding stage and sweeps every query even then, so a single layer runs dense (geometry_matrix.last_block_sweeps_every_query).

The records were confirmed from the launch labels on an MI355X; the GPU test parses every forward's labels into the same record and
compares.  BATCH rows per cell (the train matrices run 2 - 6; the evaluation batches here hold the four hand-made edge rows and four
drawn ones)."""
from typing import Dict, NamedTuple, Optional, Tuple

from tests import feature_matrix as fm
from tests import geometry_matrix as gm

MODES = fm.MODES
BATCH = 8


class InferenceForms(NamedTuple):
    attn_fwd: Tuple[str, ...]      # per layer: Block, SlotQuery, Core, Core64
    ffn: Tuple[str, ...]           # per layer: Block, Wide, CompactRows, TileProducts
    emb_proj: bool
    emb_fused: bool
    slot_only_last: bool
    slotq_rows: bool


class InferenceCell(NamedTuple):
    matrix: str                    # "feature" or "geometry": whose build_cell makes the model
    name: str
    H: int
    heads: int
    inner: int
    layers: int
    L: int
    P: int
    V: int
    E: Optional[int]
    acts: Tuple[str, str]
    modes: Tuple[str, ...]
    split: InferenceForms          # modes 1 and 2
    f32: Optional[InferenceForms]  # the exact-fp32 mode, where the cell runs in it

    @property
    def head_dim(self) -> int:
        return self.H // self.heads

    @property
    def width(self) -> int:
        """the item table's width"""
        return self.E or self.H

    def forms(self, mode: str) -> InferenceForms:
        return self.f32 if mode == "f32" else self.split

    def sweeps_every_query(self, mode: str) -> bool:
        """the last layer's attention block (where it runs one) sweeps every query"""
        return not (self.forms(mode).slot_only_last and self.layers > 1)


def encoder_only_forms(train: fm.Forms, H: int, inner: int, split: bool) -> InferenceForms:
    """the rule of the module docstring applied to a train step's record"""
    wide_256 = split and H == 256 and inner >= 64 and inner % 32 == 0
    ffn = tuple("Wide" if f == "TileProducts" and wide_256 else f for f in train.ffn)
    return InferenceForms(train.attn_fwd, ffn, train.emb_proj, train.emb_fused, train.slot_only_last, train.slotq_rows)


def _cell(matrix, name, c, layers, V) -> InferenceCell:
    f32 = encoder_only_forms(c.f32, c.H, c.inner, False) if "f32" in c.modes else None
    return InferenceCell(matrix, name, c.H, c.heads, c.inner, layers, c.L, c.P, V, c.E, c.acts, c.modes,
                         encoder_only_forms(c.split, c.H, c.inner, True), f32)


CELLS: Dict[str, InferenceCell] = {}
CELLS.update({n: _cell("feature", n, c, fm.LAYERS, fm.VOCAB) for n, c in fm.CELLS.items()})
CELLS.update({n: _cell("geometry", n, c, c.layers, c.V) for n, c in gm.CELLS.items()})

# Records pinned in full, one per form that exists in the encoder-only flavour alone or changes meaning there (the host test compares
# them with what the rule gives, so a slip of the rule fails without a GPU)
PINNED: Dict[Tuple[str, str], InferenceForms] = {
    # the Wide pair at hidden 256: the first layer in front of the slot-query attention's compact rows ...
    ("h256_L200_e64", "split"): InferenceForms(("Core", "SlotQuery"), ("Wide", "CompactRows"), True, False, False, True),
    # ... in both layers where the last one stays dense (inner 512 < 3 H + 8), and in front of gathered rows at head width 64
    ("h256_I512", "split"): InferenceForms(("Core", "Core"), ("Wide", "Wide"), True, False, False, False),
    ("h256hd64", "split"): InferenceForms(("Core64", "Core64"), ("Wide", "CompactRows"), True, False, False, False),
    # exact fp32 has no Wide pair at any size
    ("h256_L200_e128", "f32"): InferenceForms(("Core", "Core"), ("TileProducts", "CompactRows"), True, False, False, False),
    ("h128_L200", "split"): InferenceForms(("Core", "SlotQuery"), ("Wide", "CompactRows"), False, False, False, True),
    ("h64_L200", "split"): InferenceForms(("Block", "Block"), ("Block", "Block"), False, True, True, False),
    ("h64_L240", "split"): InferenceForms(("Block", "Block"), ("Block", "Block"), False, True, False, False),
    ("h64_1L_L200", "split"): InferenceForms(("Block",), ("Block",), False, True, True, False),
    ("h1024hd64_e256", "split"): InferenceForms(("Core64", "Core64"), ("TileProducts", "CompactRows"), True, False, False, False),
    ("h512hd64_e64", "split"): InferenceForms(("Core64", "Core64"), ("TileProducts", "TileProducts"), True, False, False, False),
}

# Shape changes on one engine (the evaluator's trim_padding changes L from batch to batch): cell -> ((L, P) first and last, (L', P')
# in between), in the modes given.  Between them every pair of forms that can alternate on one model does:
#   h128_L200      SlotQuery + its compact rows <-> Core + gathered compact rows (L' = 64: no slot queries), the Wide first layer in both
#   h256_L200_e64  SlotQuery / Wide / CompactRows <-> Core / Wide in both layers (2 P' > L': no compact rows), factorised
#   h64_L240       Block with the slot-only last layer (L = 208) <-> Block sweeping every query (L' = 240), head rows in both
#   h1024hd64_e256 Core64 with gathered compact rows <-> Core64 with TileProducts in both layers (2 P' > L')
#   h128_L200 f32  gathered compact rows <-> TileProducts in both layers, exact fp32
SHAPE_CHANGES = {
    ("h128_L200", "bf16x3"): ((200, 40), (64, 12)),
    ("h256_L200_e64", "bf16x3"): ((200, 40), (96, 49)),
    ("h64_L240", "bf16x3"): ((208, 41), (240, 48)),
    ("h1024hd64_e256", "bf16"): ((200, 40), (48, 30)),
    ("h128_L200", "f32"): ((200, 40), (96, 49)),
}
