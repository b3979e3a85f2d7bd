"""The geometry matrix (tests/geometry_matrix.py) covers what the library accepts: the library is asked, without a GPU, which hidden
sizes, head widths, layer counts and embedding widths it takes (b4r_param_total_floats is a host-only query), and every accepted
(hidden size, head width) pair must have a cell here or in tests/feature_matrix.py, every accepted embedding width above hidden 256
one here.  If check_cfg widens, this fails until cells are added.  Plus the refusals of what it does not take, each an error with a
message."""
import ctypes as C

import pytest

from bert4rec_amd import _lib
from bert4rec_amd.engine import make_model_config
from bert4rec_amd.models.components.networks import Bert4RecEncoder
from tests import feature_matrix as fm
from tests import geometry_matrix as gm

HIDDEN = range(16, 2049, 16)
WIDTHS = (32, 64)
EMBEDDING_WIDTHS = (32, 64, 96, 128, 192, 256, 512)


def accepted(H, heads, layers=2, inner=None, E=0):
    lib = _lib.load()
    base = make_model_config(1000, H, layers, heads, 64, inner if inner is not None else 4 * H)
    return lib.b4r_param_total_floats_ex(C.byref(_lib.ModelConfigEx(base, E, (0, 0, 0)))) > 0


def accepted_pairs():
    return {(H, w) for H in HIDDEN for w in WIDTHS if H % w == 0 and accepted(H, H // w)}


def test_every_cell_is_well_formed():
    for name, c in gm.CELLS.items():
        assert accepted(c.H, c.heads, c.layers, c.inner, c.E or 0), (name, _lib.last_error())
        assert c.head_dim in WIDTHS and c.L <= 256 and 0 < c.P and 2 <= c.B <= 6, name
        assert c.V <= 1000 or name.startswith("tinyV"), name
        assert set(c.modes) <= set(gm.MODES) and {"f32", "bf16x3"} <= set(c.modes), name
        for mode in c.modes:
            f = c.forms(mode)
            assert len(f.attn_fwd) == len(f.attn_bwd) == len(f.ffn) == c.layers, (name, mode)
            assert f.slotq_rows == (f.attn_fwd[-1] == "SlotQuery" == f.attn_bwd[-1]), (name, mode)
            assert not f.slotq_rows or f.ffn[-1] == "CompactRows", (name, mode)
            assert f.emb_proj == (c.E is not None) and not (f.emb_proj and f.emb_fused), (name, mode)
            assert all(a == "Core64" for a in f.attn_fwd + f.attn_bwd) == (c.head_dim == 64), (name, mode)
    assert set(gm.EVAL_CELLS) <= set(gm.CELLS)
    # mode 2 where the issue of this matrix asked for it
    assert all("bf16" in gm.CELLS[n].modes for n in ("h32", "h512hd32", "h1024hd64_e256"))


def test_every_accepted_hidden_size_and_head_width_has_a_cell():
    pairs = accepted_pairs()
    assert pairs == {(H, w) for H in (32, 64, 128, 256, 512, 1024) for w in WIDTHS if H >= w}, sorted(pairs)
    cells = {(c.H, c.head_dim) for c in list(gm.CELLS.values()) + list(fm.CELLS.values())}
    assert pairs <= cells, sorted(pairs - cells)
    # ... and the sizes the shipped configurations miss have cells in this matrix, with a train step in mode 2 at hidden 32 and 1024
    assert {(c.H, c.head_dim) for c in gm.CELLS.values()} >= {(32, 32), (64, 64), (512, 32), (512, 64), (1024, 32), (1024, 64)}


def test_layer_counts_one_to_thirty_two_are_accepted_and_the_cells_reach_both_ends():
    got = {n for n in range(0, 34) if accepted(64, 2, layers=n)}
    assert got == set(range(1, 33)), sorted(got)
    assert {c.layers for c in gm.CELLS.values()} >= {1, 32}


def test_every_accepted_embedding_width_above_hidden_256_has_a_cell():
    for H in (512, 1024):
        widths = {E for E in EMBEDDING_WIDTHS if E < H and accepted(H, H // 32, E=E)}
        assert widths == {64, 128, 256}, (H, sorted(widths))
        have = {c.E for c in gm.CELLS.values() if c.H == H}
        assert widths <= have, (H, sorted(widths - have))


def test_inner_sizes_around_the_compact_rows_threshold_at_hidden_32():
    """inner = 3 H + 8 = 104 (compact rows) and 100 (dense) at hidden 32, and the smallest accepted inner size"""
    inner = {c.inner for c in gm.CELLS.values() if c.H == 32}
    assert {104, 100} <= inner
    assert accepted(64, 2, inner=4) and any(c.inner == 4 for c in gm.CELLS.values())


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs,message", [
    (dict(), "hidden_size 768"),                                               # the reference's defaults: hidden 768, 12 heads
    (dict(hidden_size=64, num_attention_heads=2, num_layers=33, inner_dim=256), "num_layers 33"),
    (dict(hidden_size=64, num_attention_heads=2, num_layers=0, inner_dim=256), "num_layers 0"),
    (dict(hidden_size=64, num_attention_heads=2, num_layers=2, inner_dim=6), "inner_dim must be a multiple of 4"),
    (dict(hidden_size=1024, num_attention_heads=16, num_layers=2, inner_dim=4096, embedding_width=512), "embedding_width 512"),
])
def test_encoder_refuses_unsupported_geometry_with_a_message(kwargs, message):
    with pytest.raises(ValueError, match=message):
        Bert4RecEncoder(vocab_size=101, max_sequence_length=64, device="cpu", **kwargs)


@pytest.mark.parametrize("H,heads,layers,inner,E,message", [
    (768, 12, 12, 3072, 0, "hidden_size 768 not supported"),
    (64, 2, 33, 256, 0, "num_layers 33 not supported"),
    (64, 2, 2, 6, 0, "inner_dim must be a multiple of 4"),
    (1024, 16, 2, 4096, 512, "embedding_width 512 not supported"),
])
def test_library_refuses_unsupported_geometry_with_an_error_code(H, heads, layers, inner, E, message):
    lib = _lib.load()
    x = _lib.ModelConfigEx(make_model_config(101, H, layers, heads, 64, inner), E, (0, 0, 0))
    assert lib.b4r_param_total_floats_ex(C.byref(x)) == -1
    assert lib.b4r_param_info_ex(C.byref(x), 0, None, 0, None, None, None, None, None) == -2   # B4R_E_SHAPE
    assert message in _lib.last_error(), _lib.last_error()
