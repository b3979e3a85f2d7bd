"""Attention heads of width 64 (hidden_size = 64 * num_attention_heads): the host side -- configuration checks, parameter layout and
the Keras-shaped weight views.  No GPU needed."""
import ctypes as C
import json

import pytest
import torch

from bert4rec_amd import _lib, models
from bert4rec_amd.engine import make_model_config, param_table
from bert4rec_amd.models.components import networks

GEOMETRIES = [(64, 1), (128, 2), (256, 4), (512, 8), (1024, 16)]


@pytest.mark.parametrize("H,heads", GEOMETRIES)
def test_library_accepts_width_64(H, heads):
    lib = _lib.load()
    cfg = make_model_config(97, H, 2, heads, 32, 4 * H, 0.1, 0.1)
    assert lib.b4r_param_total_floats(C.byref(cfg)) > 0, _lib.last_error()
    assert lib.b4r_workspace_bytes(C.byref(cfg), 4, 32, 6) > 0, _lib.last_error()
    assert lib.b4r_workspace_bytes_encoder(C.byref(cfg), 4, 32, 6) > 0, _lib.last_error()
    table = {p.name: p for p in param_table(cfg)}
    q = table["transformer/layer_0/self_attention/query/kernel"]
    assert (q.rows, q.cols) == (H, H)   # the layout does not depend on the head count
    o = table["transformer/layer_1/self_attention/attention_output/kernel"]
    assert (o.rows, o.cols) == (H, H)
    # same flat layout as the width-32 model of the same hidden size (where one exists)
    if H >= 64:
        cfg32 = make_model_config(97, H, 2, H // 32, 32, 4 * H, 0.1, 0.1)
        assert lib.b4r_param_total_floats(C.byref(cfg)) == lib.b4r_param_total_floats(C.byref(cfg32))
        assert [(p.name, p.offset) for p in param_table(cfg)] == [(p.name, p.offset) for p in param_table(cfg32)]


@pytest.mark.parametrize("H,heads", GEOMETRIES)
def test_encoder_builds_and_weights_have_width_64(H, heads):
    enc = networks.Bert4RecEncoder(50, hidden_size=H, num_layers=2, num_attention_heads=heads, max_sequence_length=16,
                                   inner_dim=4 * H, device="cpu")
    model = models.BERT4RecModel(enc)
    w = model.get_weights()
    for kind in ("query", "key", "value"):
        assert w["transformer/layer_0/self_attention/%s/kernel" % kind].shape == (H, heads, 64)
        assert w["transformer/layer_1/self_attention/%s/bias" % kind].shape == (heads, 64)
    assert w["transformer/layer_1/self_attention/attention_output/kernel"].shape == (heads, 64, H)


@pytest.mark.parametrize("H,heads", [(64, 4), (32, 2), (256, 16),          # width 16
                                     (96, 2), (192, 4),                    # width 48 (hidden sizes not supported either)
                                     (128, 1), (256, 2), (1024, 8),        # width 128
                                     (768, 12)])                           # width 64 at a hidden size outside the supported set
def test_other_widths_are_refused(H, heads):
    with pytest.raises(ValueError):
        networks.Bert4RecEncoder(50, hidden_size=H, num_layers=1, num_attention_heads=heads, max_sequence_length=16,
                                 inner_dim=4 * H, device="cpu")
    lib = _lib.load()
    cfg = make_model_config(50, H, 1, heads, 16, 4 * H, 0.1, 0.1)
    assert lib.b4r_param_total_floats(C.byref(cfg)) < 0
    if H // heads in (16, 48, 128):
        assert "32 or 64" in _lib.last_error()


def test_weights_and_meta_config_roundtrip_at_width_64(tmp_path):
    kw = dict(hidden_size=128, num_layers=2, num_attention_heads=2, max_sequence_length=16, inner_dim=512)
    m1 = models.BERT4RecModel(networks.Bert4RecEncoder(40, device="cpu", seed=5, **kw))
    m2 = models.BERT4RecModel(networks.Bert4RecEncoder(40, device="cpu", seed=6, **kw))
    assert not torch.equal(m1.engine.params, m2.engine.params)
    f = tmp_path / "w.safetensors"
    m1.save_weights(f)
    m2.load_weights(f)
    assert torch.equal(m1.engine.params, m2.engine.params) and torch.equal(m1.engine.pooler, m2.engine.pooler)
    w1, w2 = m1.get_weights(), m2.get_weights()
    assert w2["transformer/layer_0/self_attention/query/kernel"].shape == (128, 2, 64)
    assert all(torch.equal(torch.as_tensor(w1[k]), torch.as_tensor(w2[k])) for k in w1)
    meta = models.BERT4RecModelWrapper(m1).get_meta_config()
    enc_cfg = json.loads(json.dumps(meta["encoder_config"]))
    assert (enc_cfg["hidden_size"], enc_cfg["num_attention_heads"]) == (128, 2)
    m3 = models.BERT4RecModel(networks.Bert4RecEncoder(device="cpu", **enc_cfg))
    m3.load_weights(f)
    assert torch.equal(m1.engine.params, m3.engine.params)
    assert m3.get_weights()["transformer/layer_1/self_attention/attention_output/kernel"].shape == (2, 64, 128)
