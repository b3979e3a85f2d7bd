"""Factorised item embeddings (embedding_width E < hidden_size H), host side: the restatement against the frozen oracle, the _ex
parameter layout of the C ABI and the encoder's constructor surface.  No GPU needed."""
import ctypes as C

import pytest
import torch

from bert4rec_amd import _lib
from bert4rec_amd.engine import make_model_config, param_table
from bert4rec_amd.models.components.networks import Bert4RecEncoder
from oracle import bert4rec_oracle as orc
from tests import factorized_ref as fr


def cfg_ex(H, E, heads=None, V=1001, layers=2, reserved=(0, 0, 0)):
    base = make_model_config(V, H, layers, heads or H // 32, 64, 4 * H, 0.1, 0.1)
    return _lib.ModelConfigEx(base, E, reserved)


def table_ex(x):
    lib = _lib.load()
    n = lib.b4r_param_count_ex(C.byref(x))
    assert n > 0, _lib.last_error()
    name = C.create_string_buffer(256)
    off, rows, cols, ld, dec = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    out = []
    for i in range(n):
        _lib.check(lib.b4r_param_info_ex(C.byref(x), i, name, 256, C.byref(off), C.byref(rows), C.byref(cols), C.byref(ld),
                                         C.byref(dec)))
        out.append((name.value.decode(), off.value, rows.value, cols.value, ld.value, dec.value))
    return out


def test_restatement_at_full_width_with_identity_projection_is_the_oracle():
    """E = H, Wp = I, bp = 0: the factorised restatement computes oracle.model_forward, dropout included"""
    cfg = orc.OracleConfig(vocab_size=97, hidden_size=64, num_layers=2, num_attention_heads=2, max_sequence_length=32, inner_dim=256,
                           output_dropout=0.2, attention_dropout=0.1)
    params = orc.init_params(cfg, seed=5)
    batch = orc.synthetic_batch(4, 32, 6, 97, seed=1, ragged=True)
    fparams = dict(params)
    fparams[fr.PROJ_W] = torch.eye(64)
    fparams[fr.PROJ_B] = torch.zeros(64)
    for training in (False, True):
        ref = orc.model_forward(params, batch, cfg, training=training, rng=(7, 3))
        got = fr.model_forward(fparams, batch, cfg, training=training, rng=(7, 3))
        assert float((got["mlm_logits"] - ref["mlm_logits"]).abs().max()) < 1e-6


def test_restatement_shapes_follow_keras():
    cfg = orc.OracleConfig(vocab_size=50, hidden_size=128, num_layers=1, num_attention_heads=4, max_sequence_length=16, inner_dim=512)
    shapes = dict(fr.param_shapes(cfg, 64))
    assert shapes["word_embeddings/embeddings"] == (50, 64) and shapes[fr.PROJ_W] == (64, 128)
    assert shapes["cls/predictions/transform/dense/kernel"] == (128, 64)


@pytest.mark.parametrize("H,E", [(128, 64), (256, 64), (1024, 256)])
def test_ex_layout_names_shapes_and_decay(H, E):
    t = table_ex(cfg_ex(H, E))
    by = {n: (r, c, ld, d) for n, _, r, c, ld, d in t}
    assert by["word_embeddings/embeddings"] == (1001, E, E, 1)
    assert by["position_embedding/embeddings"] == (64, E, E, 1)
    assert by["embeddings/layer_norm/gamma"][:2] == (1, E) and by["embeddings/layer_norm/beta"][3] == 0
    assert by["embedding_projection/kernel"] == (E, H, H, 1)
    assert by["embedding_projection/bias"] == (1, H, H, 0)
    assert by["cls/predictions/transform/dense/kernel"] == (H, E, E, 1)
    for n in ("cls/predictions/transform/dense/bias", "cls/predictions/transform/LayerNorm/gamma",
              "cls/predictions/transform/LayerNorm/beta"):
        assert by[n][:2] == (1, E)
    assert by["transformer/layer_0/intermediate/kernel"][:2] == (H, 4 * H)
    # decay flags follow the reference's default exclusion list
    for n, (_, _, _, d) in by.items():
        assert d == (1 if orc.uses_weight_decay(n) else 0), n
    # the decayed prefix holds exactly the decayed entries
    lib = _lib.load()
    x = cfg_ex(H, E)
    n_decay = lib.b4r_param_decay_floats_ex(C.byref(x))
    total = lib.b4r_param_total_floats_ex(C.byref(x))
    for n, off, r, c, ld, d in t:
        end = off + (r - 1) * ld + c
        assert (end <= n_decay) if d else (off >= n_decay and end <= total), n


@pytest.mark.parametrize("H", [128, 256])
def test_ex_at_zero_or_full_width_is_the_classic_layout(H):
    lib = _lib.load()
    base = cfg_ex(H, 0).base
    classic = [(e.name, e.offset, e.rows, e.cols, e.ld, e.decay) for e in param_table(base)]
    for E in (0, H):
        x = cfg_ex(H, E)
        assert table_ex(x) == classic
        assert lib.b4r_param_total_floats_ex(C.byref(x)) == lib.b4r_param_total_floats(C.byref(base))
        assert lib.b4r_param_decay_floats_ex(C.byref(x)) == lib.b4r_param_decay_floats(C.byref(base))
        for B, L, P in ((8, 64, 12), (3, 17, 0)):
            assert lib.b4r_workspace_bytes_ex(C.byref(x), B, L, P) == lib.b4r_workspace_bytes(C.byref(base), B, L, P)
            assert lib.b4r_workspace_bytes_encoder_ex(C.byref(x), B, L, P) == lib.b4r_workspace_bytes_encoder(C.byref(base), B, L, P)


def test_ex_mlm_hidden_region_is_table_wide():
    lib = _lib.load()
    off, rows, cols, ld = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(lib.b4r_workspace_region_ex(C.byref(cfg_ex(256, 64)), 4, 32, 5, b"mlm_hidden", C.byref(off), C.byref(rows),
                                           C.byref(cols), C.byref(ld)))
    assert (rows.value, cols.value, ld.value) == (20, 64, 64)


@pytest.mark.parametrize("E", [32, 96, 512])
def test_ex_refuses_unsupported_widths(E):
    lib = _lib.load()
    x = cfg_ex(256, E)
    assert lib.b4r_param_total_floats_ex(C.byref(x)) == -1
    assert lib.b4r_param_count_ex(C.byref(x)) == -1
    assert lib.b4r_workspace_bytes_ex(C.byref(x), 4, 16, 2) == -1
    assert lib.b4r_param_info_ex(C.byref(x), 0, None, 0, None, None, None, None, None) == -2   # B4R_E_SHAPE
    assert "embedding_width" in _lib.last_error()


def test_ex_refuses_a_nonzero_reserved_word():
    lib = _lib.load()
    for r in ((1, 0, 0), (0, 0, 7)):
        x = cfg_ex(256, 64, reserved=r)
        assert lib.b4r_param_total_floats_ex(C.byref(x)) == -1
        assert lib.b4r_param_info_ex(C.byref(x), 0, None, 0, None, None, None, None, None) == -1   # B4R_E_BADARG
        assert "reserved" in _lib.last_error()


def test_encoder_accepts_a_factorised_width_on_the_host():
    enc = Bert4RecEncoder(vocab_size=301, hidden_size=256, num_layers=2, num_attention_heads=8, max_sequence_length=40,
                          inner_dim=1024, embedding_width=64, device="cpu")
    cfg = enc.get_config()
    assert cfg["embedding_width"] == 64
    again = Bert4RecEncoder.from_config({**cfg, "device": "cpu"})
    assert again.get_config() == cfg
    assert tuple(enc.get_embedding_table().shape) == (301, 64)
    w = enc.engine.export_named()
    assert tuple(w["embedding_projection/kernel"].shape) == (64, 256)
    assert tuple(w["embedding_projection/bias"].shape) == (256,)
    assert tuple(w["cls/predictions/transform/dense/kernel"].shape) == (256, 64)
    assert tuple(w["position_embedding/embeddings"].shape) == (40, 64)
    assert float(w["embedding_projection/bias"].abs().max()) == 0.0
    assert 0.0 < float(w["embedding_projection/kernel"].abs().max()) <= 0.04   # TruncatedNormal(0.02), cut at 2 sigma


@pytest.mark.parametrize("H,E", [(256, 32), (256, 96), (128, 256), (64, 64 + 64), (64, 32)])
def test_encoder_refuses_unsupported_widths(H, E):
    with pytest.raises(ValueError):
        Bert4RecEncoder(vocab_size=101, hidden_size=H, num_layers=1, num_attention_heads=H // 32, max_sequence_length=16,
                        inner_dim=4 * H, embedding_width=E, device="cpu")
