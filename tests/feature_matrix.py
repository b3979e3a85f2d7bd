"""The feature-by-form matrix of train steps (tests/test_gpu_feature_matrix.py runs it on the GPU; tests/test_feature_matrix_host.py
checks its coverage on the CPU).

Each cell is one model -- hidden size, heads, inner size, a factorised embedding width E (or none) and the activation pair -- at
one batch shape (L, P), the arithmetic modes it runs in, and the launch forms plan_step (bert4rec_amd/csrc/b4r_model.hip) picks for
its train step (fused head, head rows only).  The forms were derived by reading plan_step and confirmed from the launch labels
on an MI355X; the GPU test parses every step's labels into the same record and compares, so a moved threshold fails the cell
instead of silently changing what it checks.

Form names:

* attention forward per layer: Block (b4r_attn_block_fwd), SlotQuery (the last layer with the masked-LM slots as its only queries),
  Core (QKV product, the width-32 core, output projection), Core64 (the same with the width-64 core);
* attention backward per layer: Block and BlockFolded (the block's backward; folded, it also forms the half's weight gradients),
  SlotQuery, Core16 (the width-32 core's two-launch backward: dq, then dk / dv -- 16-token tiles in the split modes, the exact-fp32
  kernels in f32), Core32 (the one-launch backward on 32-token tiles, 65 <= L <= 224), Core64;
* feed-forward per layer: Block, Wide, CompactRows (the last layer on the head's rows), TileProducts;
* step flags: emb_proj (factorised embedding stage), emb_fused (the embedding stage inside layer 0's attention block),
  slot_only_last (the last layer's attention block sweeps the slots' queries only), slotq_rows (the compact rows of the last
  feed-forward half come from the SlotQuery attention; otherwise from a gather).

"f32" is B4R_GEMM_F32, "bf16x3" B4R_GEMM_BF16X3 (mode 1), "bf16" B4R_GEMM_BF16 (mode 2).  Modes 1 and 2 plan the same forms."""
from typing import Dict, NamedTuple, Optional, Tuple

MODES = ("f32", "bf16x3", "bf16")
LAYERS = 2
BATCH = 6
VOCAB = 1000


class Forms(NamedTuple):
    attn_fwd: Tuple[str, ...]
    attn_bwd: Tuple[str, ...]
    ffn: Tuple[str, ...]
    emb_proj: bool
    emb_fused: bool
    slot_only_last: bool
    slotq_rows: bool


class Cell(NamedTuple):
    H: int
    heads: int
    inner: int
    L: int
    P: int
    E: Optional[int]
    acts: Tuple[str, str]          # (inner_activation, mlm_activation)
    modes: Tuple[str, ...]
    split: Forms                   # the forms of modes 1 and 2
    f32: Optional[Forms] = None    # the forms of the exact-fp32 mode, where the cell runs in it

    @property
    def head_dim(self) -> int:
        return self.H // self.heads

    def forms(self, mode: str) -> Forms:
        return self.f32 if mode == "f32" else self.split


def _f(fwd, bwd, ffn, emb_proj=False, emb_fused=False, slot_only_last=False, slotq_rows=False) -> Forms:
    return Forms(tuple(fwd), tuple(bwd), tuple(ffn), emb_proj, emb_fused, slot_only_last, slotq_rows)


SPLIT = ("bf16x3", "bf16")
ALL = MODES

# hidden 64 (2 heads of 32, inner 256): the resident blocks.  Block forward at L <= 256 (the embedding stage inside it when not
# factorised), its backward at L <= 208: folded on 32-token tiles from L = 65, else the unfolded 16-token-tile block; above 208 the
# core's backward (32-token tiles to L = 224)
_H64_FOLDED = _f(["Block"] * 2, ["BlockFolded"] * 2, ["Block"] * 2, emb_fused=True, slot_only_last=True)
# exact fp32 at hidden 64: no blocks; the last feed-forward half on the head's rows (2 P <= L, inner >= 3 H + 8), rows gathered
_H64_F32 = _f(["Core"] * 2, ["Core16"] * 2, ["TileProducts", "CompactRows"])

CELLS: Dict[str, Cell] = {
    "h64_L200": Cell(64, 2, 256, 200, 40, None, ("swish", "relu"), ALL, _H64_FOLDED, _H64_F32),
    "h64_L240": Cell(64, 2, 256, 240, 48, None, ("elu", "tanh"), SPLIT,
                     _f(["Block"] * 2, ["Core16"] * 2, ["Block"] * 2, emb_fused=True)),
    # hidden 128, 4 heads of 32: layer 0 the core (backward on 32-token tiles) and the Wide pair; the last layer SlotQuery with the
    # compact rows it leaves
    "h128_L200": Cell(128, 4, 512, 200, 40, None, ("relu", "sigmoid"), ALL,
                      _f(["Core", "SlotQuery"], ["Core32", "SlotQuery"], ["Wide", "CompactRows"], slotq_rows=True),
                      _f(["Core"] * 2, ["Core16"] * 2, ["TileProducts", "CompactRows"])),
    "h128_L200_e64": Cell(128, 4, 512, 200, 40, 64, ("relu", "sigmoid"), ALL,
                          _f(["Core", "SlotQuery"], ["Core32", "SlotQuery"], ["Wide", "CompactRows"], emb_proj=True, slotq_rows=True),
                          _f(["Core"] * 2, ["Core16"] * 2, ["TileProducts", "CompactRows"], emb_proj=True)),
    # hidden 128, 2 heads of 64: the width-64 core; the last layer's rows gathered after its dense attention
    "h128hd64_L200": Cell(128, 2, 512, 200, 40, 64, ("softplus", "selu"), ALL,
                          _f(["Core64"] * 2, ["Core64"] * 2, ["Wide", "CompactRows"], emb_proj=True),
                          _f(["Core64"] * 2, ["Core64"] * 2, ["TileProducts", "CompactRows"], emb_proj=True)),
    # hidden 256, 8 heads: tile products (the Wide pair runs in encoder-only forwards only at 256)
    "h256_L200_e64": Cell(256, 8, 1024, 200, 40, 64, ("tanh", "linear"), SPLIT,
                          _f(["Core", "SlotQuery"], ["Core32", "SlotQuery"], ["TileProducts", "CompactRows"], emb_proj=True,
                             slotq_rows=True)),
    "h256_L200_e128": Cell(256, 8, 1024, 200, 40, 128, ("sigmoid", "swish"), ALL,
                           _f(["Core", "SlotQuery"], ["Core32", "SlotQuery"], ["TileProducts", "CompactRows"], emb_proj=True,
                              slotq_rows=True),
                           _f(["Core"] * 2, ["Core16"] * 2, ["TileProducts", "CompactRows"], emb_proj=True)),
    # inner 512 < 3 H + 8: the last layer stays dense
    "h256_I512": Cell(256, 8, 512, 200, 40, 128, ("linear", "elu"), SPLIT,
                      _f(["Core"] * 2, ["Core32"] * 2, ["TileProducts"] * 2, emb_proj=True)),
    "h256hd64": Cell(256, 4, 1024, 200, 40, 64, ("gelu", "softplus"), SPLIT,
                     _f(["Core64"] * 2, ["Core64"] * 2, ["TileProducts", "CompactRows"], emb_proj=True)),
    # L > 224: the 16-token-tile backward, no slot queries
    "h128_L240": Cell(128, 4, 512, 240, 40, 64, ("swish", "tanh"), SPLIT,
                      _f(["Core"] * 2, ["Core16"] * 2, ["Wide", "CompactRows"], emb_proj=True)),
    # 2 P > L: no compact rows, the Wide pair in both layers
    "h128_2P_gt_L": Cell(128, 4, 512, 96, 49, 64, ("relu", "linear"), SPLIT,
                         _f(["Core"] * 2, ["Core32"] * 2, ["Wide"] * 2, emb_proj=True)),
    # ---- each side of the thresholds ----
    # the 16 -> 32-token-tile threshold (65) and the slot-query limit L > 64
    "b128_L64": Cell(128, 4, 512, 64, 12, 64, ("selu", "relu"), SPLIT,
                     _f(["Core"] * 2, ["Core16"] * 2, ["Wide", "CompactRows"], emb_proj=True)),
    "b128_L65": Cell(128, 4, 512, 65, 13, 64, ("tanh", "gelu"), SPLIT,
                     _f(["Core", "SlotQuery"], ["Core32", "SlotQuery"], ["Wide", "CompactRows"], emb_proj=True, slotq_rows=True)),
    # the slot-query and 32-token-tile limit L <= 224
    "b128_L224": Cell(128, 4, 512, 224, 44, 64, ("sigmoid", "selu"), SPLIT,
                      _f(["Core", "SlotQuery"], ["Core32", "SlotQuery"], ["Wide", "CompactRows"], emb_proj=True, slotq_rows=True)),
    "b128_L225": Cell(128, 4, 512, 225, 45, 64, ("softplus", "relu"), SPLIT,
                      _f(["Core"] * 2, ["Core16"] * 2, ["Wide", "CompactRows"], emb_proj=True)),
    # the slot-query limit P <= 64 (2 P <= L on both sides)
    "b128_L128_P64": Cell(128, 4, 512, 128, 64, 64, ("elu", "swish"), SPLIT,
                          _f(["Core", "SlotQuery"], ["Core32", "SlotQuery"], ["Wide", "CompactRows"], emb_proj=True,
                             slotq_rows=True)),
    "b128_L130_P65": Cell(128, 4, 512, 130, 65, 64, ("linear", "sigmoid"), SPLIT,
                          _f(["Core"] * 2, ["Core32"] * 2, ["Wide", "CompactRows"], emb_proj=True)),
    # hidden 64: the unfolded 16-token-tile block backward at L <= 64, folded from 65; the block backward up to L = 208, then a
    # Block forward with the core's backward on 32-token tiles and no slot-only sweep
    "b64_L64": Cell(64, 2, 256, 64, 12, None, ("relu", "softplus"), SPLIT,
                    _f(["Block"] * 2, ["Block"] * 2, ["Block"] * 2, emb_fused=True)),
    "b64_L65": Cell(64, 2, 256, 65, 13, None, ("selu", "swish"), SPLIT, _H64_FOLDED),
    "b64_L208": Cell(64, 2, 256, 208, 41, None, ("tanh", "sigmoid"), SPLIT, _H64_FOLDED),
    "b64_L209": Cell(64, 2, 256, 209, 41, None, ("softplus", "elu"), SPLIT,
                     _f(["Block"] * 2, ["Core32"] * 2, ["Block"] * 2, emb_fused=True)),
}

# the cells whose evaluation forward is checked as well (full forward against the restatement; encoder-only on the ranked rows)
EVAL_CELLS = ("h128_L200_e64", "h256_L200_e64", "h256_L200_e128", "h256hd64")
# the cell of the reproducibility and graph-replay check in mode 2
REPRO_CELL = "h128_L200_e64"
