"""The geometry matrix of train steps (tests/test_gpu_geometry.py runs it on the GPU; tests/test_geometry_host.py checks its coverage
on the CPU): the models check_cfg (bert4rec_amd/csrc/b4r_model.hip) accepts outside the shipped configurations -- hidden 32, 512 and
1024, 16 and 32 heads, inner sizes off the tile grid, a single layer, deep stacks and tiny vocabularies.

Each cell is one model -- hidden size, heads, inner size, layers, a factorised embedding width E (or none), the vocabulary size and
the activation pair -- at one batch shape (B, L, P), the arithmetic modes it runs in, and the launch forms plan_step picks for its
train step per layer.  The forms were derived by reading plan_step and confirmed from the launch labels on an MI355X; the GPU test
parses every step's labels into the same record and compares, so a moved threshold fails the cell instead of silently changing what
it checks.  Form names are tests/feature_matrix.py's."""
from typing import Dict, NamedTuple, Optional, Tuple

from tests.feature_matrix import Forms, _f

MODES = ("f32", "bf16x3", "bf16")
SPLIT_AND_F32 = ("f32", "bf16x3")
ALL = MODES


class Cell(NamedTuple):
    H: int
    heads: int
    inner: int
    layers: int
    B: int
    L: int
    P: int
    V: int
    E: Optional[int]
    acts: Tuple[str, str]          # (inner_activation, mlm_activation)
    modes: Tuple[str, ...]
    split: Forms                   # the forms of modes 1 and 2
    f32: Forms                     # the forms of the exact-fp32 mode

    @property
    def head_dim(self) -> int:
        return self.H // self.heads

    def forms(self, mode: str) -> Forms:
        return self.f32 if mode == "f32" else self.split


def _dense(n, core_bwd):
    """n layers as the cores and the tile products (the exact-fp32 mode everywhere; the split modes where no block, no Wide pair and
    no compact rows apply): the core's backward on 32-token tiles (Core32) in the split modes at 65 <= L <= 224, else Core16"""
    return _f(["Core"] * n, [core_bwd] * n, ["TileProducts"] * n)


def _slotq(n, core_bwd="Core32", ffn="TileProducts", emb_proj=False):
    """n layers: the cores, the last one SlotQuery with the compact rows it leaves"""
    return _f(["Core"] * (n - 1) + ["SlotQuery"], [core_bwd] * (n - 1) + ["SlotQuery"], [ffn] * (n - 1) + ["CompactRows"],
              emb_proj=emb_proj, slotq_rows=True)


def _f32_rows(n, core="Core", core_bwd="Core16", emb_proj=False):
    """exact fp32: the cores, the last feed-forward half on the head's rows (2 P <= L, inner >= 3 H + 8), rows gathered"""
    return _f([core] * n, [core_bwd] * n, ["TileProducts"] * (n - 1) + ["CompactRows"], emb_proj=emb_proj)


_H64_FOLDED = _f(["Block"] * 2, ["BlockFolded"] * 2, ["Block"] * 2, emb_fused=True, slot_only_last=True)
_H64_F32 = _f32_rows(2)

CELLS: Dict[str, Cell] = {
    # hidden 32, one head of 32: K = 32 tile products, the LayerNorm / slot-tail instances (8, 1), the materialising head in every
    # mode (the fused head needs an item-table width of 64 / 128 / 256); inner 128 >= 3 H + 8 = 104: SlotQuery + CompactRows
    "h32": Cell(32, 1, 128, 2, 6, 100, 20, 1000, None, ("relu", "gelu"), ALL, _slotq(2), _f32_rows(2)),
    # the compact rows exactly at inner = 3 H + 8 = 104 (off the 32 grid: the exact-fp32 fallbacks inside a split-mode step) ...
    "h32_I104": Cell(32, 1, 104, 2, 6, 96, 24, 1000, None, ("swish", "tanh"), SPLIT_AND_F32, _slotq(2), _f32_rows(2)),
    # ... and just below it: the last layer stays dense
    "h32_I100": Cell(32, 1, 100, 2, 6, 96, 24, 1000, None, ("gelu", "selu"), SPLIT_AND_F32, _dense(2, "Core32"),
                     _dense(2, "Core16")),
    # hidden 64 off inner 256: the fused attention blocks (folded backward, 65 <= L <= 208) with tile-product feed-forward halves at
    # an off-grid K; inner 100 < 3 H + 8: no compact rows, so no slot-only sweep either
    "h64_I100": Cell(64, 2, 100, 2, 4, 200, 40, 1000, None, ("elu", "softplus"), SPLIT_AND_F32,
                     _f(["Block"] * 2, ["BlockFolded"] * 2, ["TileProducts"] * 2, emb_fused=True), _dense(2, "Core16")),
    # the smallest accepted inner size; L < 65: the unfolded block backward
    "h64_I4": Cell(64, 2, 4, 2, 6, 50, 10, 1000, None, ("tanh", "relu"), SPLIT_AND_F32,
                   _f(["Block"] * 2, ["Block"] * 2, ["TileProducts"] * 2, emb_fused=True), _dense(2, "Core16")),
    # one layer at hidden 64: layer 0 is the last layer.  Its block forward carries the embedding stage (so sweeps every query), its
    # backward reads the slots' dz1 only (slot_only_last); exact fp32: layer 0's feed-forward half on the head's rows
    "h64_1L_L200": Cell(64, 2, 256, 1, 4, 200, 40, 1000, None, ("sigmoid", "swish"), SPLIT_AND_F32,
                        _f(["Block"], ["BlockFolded"], ["Block"], emb_fused=True, slot_only_last=True), _f32_rows(1)),
    "h64_1L_L65": Cell(64, 2, 256, 1, 6, 65, 13, 1000, None, ("linear", "gelu"), SPLIT_AND_F32,
                       _f(["Block"], ["BlockFolded"], ["Block"], emb_fused=True, slot_only_last=True), _f32_rows(1)),
    # 16 heads of 32: LayerNorm (64, 2), SlotQuery + CompactRows at 512 (inner 2048 >= 1544), the materialising head
    "h512hd32": Cell(512, 16, 2048, 2, 4, 100, 20, 1000, None, ("gelu", "relu"), ALL, _slotq(2), _f32_rows(2)),
    # 8 heads of 64, inner 1024 < 3 H + 8: the last layer dense; embed_proj 64 -> 512 with the fused head at E = 64
    "h512hd64_e64": Cell(512, 8, 1024, 2, 4, 200, 40, 1000, 64, ("softplus", "sigmoid"), SPLIT_AND_F32,
                         _f(["Core64"] * 2, ["Core64"] * 2, ["TileProducts"] * 2, emb_proj=True),
                         _f(["Core64"] * 2, ["Core64"] * 2, ["TileProducts"] * 2, emb_proj=True)),
    # 32 heads of 32: LayerNorm (64, 4), tile products at K = 4096, SlotQuery + CompactRows at 1024
    "h1024hd32": Cell(1024, 32, 4096, 2, 3, 96, 16, 500, None, ("selu", "elu"), SPLIT_AND_F32, _slotq(2), _f32_rows(2)),
    # 16 heads of 64, embed_proj 256 -> 1024, the fused head at E = 256; the last layer's rows gathered after its dense attention
    "h1024hd64_e256": Cell(1024, 16, 4096, 2, 2, 200, 40, 500, 256, ("gelu", "linear"), ALL,
                           _f32_rows(2, "Core64", "Core64", emb_proj=True), _f32_rows(2, "Core64", "Core64", emb_proj=True)),
    # B4R_MAX_LAYERS: 32 layers of blocks (L < 65: the unfolded block backward, no slot-only sweep), dropout streams and workspace
    # regions of every layer
    "deep32": Cell(64, 2, 256, 32, 4, 50, 10, 500, None, ("tanh", "softplus"), SPLIT_AND_F32,
                   _f(["Block"] * 32, ["Block"] * 32, ["Block"] * 32, emb_fused=True), _f32_rows(32)),
    # a deep stack on the Wide / SlotQuery forms
    "deep8_h128": Cell(128, 4, 512, 8, 4, 200, 40, 1000, 64, ("swish", "elu"), SPLIT_AND_F32,
                       _slotq(8, ffn="Wide", emb_proj=True), _f32_rows(8, emb_proj=True)),
    # one head of 64 at hidden 64: the width-64 core with the fused feed-forward block, on the head's rows in the last layer
    "h64hd64": Cell(64, 1, 256, 2, 6, 200, 40, 1000, None, ("softplus", "relu"), SPLIT_AND_F32,
                    _f(["Core64"] * 2, ["Core64"] * 2, ["Block"] * 2), _f32_rows(2, "Core64", "Core64")),
    # the other embedding widths above hidden 256 (L = 64: no slot queries; L = 48 / 130 with inner < 3 H + 8: dense)
    "h512hd32_e128": Cell(512, 16, 2048, 2, 3, 64, 12, 1000, 128, ("elu", "gelu"), SPLIT_AND_F32,
                          _f32_rows(2, emb_proj=True), _f32_rows(2, emb_proj=True)),
    "h512hd64_e256": Cell(512, 8, 512, 2, 2, 130, 26, 1000, 256, ("relu", "softplus"), SPLIT_AND_F32,
                          _f(["Core64"] * 2, ["Core64"] * 2, ["TileProducts"] * 2, emb_proj=True),
                          _f(["Core64"] * 2, ["Core64"] * 2, ["TileProducts"] * 2, emb_proj=True)),
    "h1024hd32_e64": Cell(1024, 32, 1024, 2, 2, 48, 8, 500, 64, ("sigmoid", "selu"), SPLIT_AND_F32,
                          _f(["Core"] * 2, ["Core16"] * 2, ["TileProducts"] * 2, emb_proj=True),
                          _f(["Core"] * 2, ["Core16"] * 2, ["TileProducts"] * 2, emb_proj=True)),
    # inner 3200 (a multiple of 64 off the powers of two) >= 3 H + 8: compact rows gathered after the dense width-64 attention
    "h1024hd64_e128": Cell(1024, 16, 3200, 2, 2, 80, 16, 500, 128, ("tanh", "swish"), SPLIT_AND_F32,
                           _f32_rows(2, "Core64", "Core64", emb_proj=True), _f32_rows(2, "Core64", "Core64", emb_proj=True)),
    # tiny vocabularies through the logits-free head: one real item (V = 4), one vocabulary tile plus one (V = 33)
    "tinyV4": Cell(64, 2, 256, 2, 6, 80, 16, 4, None, ("relu", "tanh"), SPLIT_AND_F32, _H64_FOLDED, _H64_F32),
    "tinyV33": Cell(64, 2, 256, 2, 6, 80, 16, 33, None, ("selu", "sigmoid"), SPLIT_AND_F32, _H64_FOLDED, _H64_F32),
}

def last_block_sweeps_every_query(c: Cell, mode: str) -> bool:
    """where the last layer runs the attention block (hidden 64, split modes): its forward sweeps every query unless the plan asks for
    the slots' queries only (slot_only_last) -- and layer 0's block, which carries the embedding stage, sweeps every query even then
    (b4r_attn32.hip: the slots-only form is not for the first layer).  So a single layer pairs a dense forward with the slots-only
    backward."""
    return not (c.forms(mode).slot_only_last and c.layers > 1)


# the cells whose evaluation forward is checked as well (logits and top-10 against the restatement; encoder-only on the ranked rows)
EVAL_CELLS = ("h32", "h512hd32", "h1024hd32")
