"""inner_activation / mlm_activation without a GPU: the restatement against the frozen oracle at GELU, the activations' fp64 values and
derivatives, the encoder's surface and the _ex host queries' activations word (include/b4r.h)."""
import ctypes as C

import numpy as np
import pytest
import torch

from bert4rec_amd import _lib, activations
from bert4rec_amd.engine import make_model_config
from bert4rec_amd.models.components.networks import Bert4RecEncoder
from oracle import bert4rec_oracle as orc
from tests import activation_ref as ar


def small_cfg():
    return orc.OracleConfig(vocab_size=61, hidden_size=64, num_layers=2, num_attention_heads=2, max_sequence_length=16,
                            inner_dim=256, output_dropout=0.1, attention_dropout=0.1)


@pytest.mark.parametrize("training", [False, True])
def test_restatement_at_gelu_is_bitwise_the_oracle(training):
    cfg = small_cfg()
    params = orc.init_params(cfg, seed=3)
    batch = orc.synthetic_batch(3, 16, 4, cfg.vocab_size, seed=1, ragged=True)
    ref = orc.model_forward(params, batch, cfg, training=training, rng=(7, 2))
    got = ar.model_forward(params, batch, cfg, "gelu", "gelu", training=training, rng=(7, 2))
    assert torch.equal(ref["mlm_logits"], got["mlm_logits"])
    l0, g0, _ = orc.loss_and_grads(params, batch, cfg, training=training, rng=(7, 2))
    l1, g1, _ = ar.loss_and_grads(params, batch, cfg, "gelu", "gelu", training=training, rng=(7, 2))
    assert torch.equal(l0, l1)
    assert set(g0) == set(g1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_restatement_changes_with_the_activations():
    cfg = small_cfg()
    params = orc.init_params(cfg, seed=3)
    batch = orc.synthetic_batch(3, 16, 4, cfg.vocab_size, seed=1)
    base = ar.model_forward(params, batch, cfg)["mlm_logits"]
    assert not torch.equal(base, ar.model_forward(params, batch, cfg, inner="relu")["mlm_logits"])
    assert not torch.equal(base, ar.model_forward(params, batch, cfg, mlm="tanh")["mlm_logits"])


def test_fp64_values_and_derivatives_of_every_activation():
    x = np.array([-88.0, -30.0, -3.0, -1.0, -1e-3, 0.0, 1e-3, 1.0, 3.0, 30.0, 88.0])
    s = 1.0 / (1.0 + np.exp(-x))
    expect = {
        "relu": (np.maximum(x, 0), (x > 0).astype(float)),
        "swish": (x * s, s * (1 + x * (1 - s))),
        "tanh": (np.tanh(x), 1 - np.tanh(x) ** 2),
        "sigmoid": (s, s * (1 - s)),
        "elu": (np.where(x > 0, x, np.expm1(np.minimum(x, 0))), np.where(x > 0, 1.0, np.exp(np.minimum(x, 0)))),
        "selu": (ar.SELU_SCALE * np.where(x > 0, x, ar.SELU_ALPHA * np.expm1(np.minimum(x, 0))),
                 np.where(x > 0, ar.SELU_SCALE, ar.SELU_SCALE * ar.SELU_ALPHA * np.exp(np.minimum(x, 0)))),
        "softplus": (np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x))), s),
        "linear": (x, np.ones_like(x)),
    }
    for name, (f, d) in expect.items():
        gf, gd = ar.value_and_grad64(name, x)
        assert np.all(np.isfinite(gf)) and np.all(np.isfinite(gd)), name
        np.testing.assert_allclose(gf, f, rtol=1e-12, atol=1e-300, err_msg=name)
        np.testing.assert_allclose(gd, d, rtol=1e-12, atol=1e-15, err_msg=name)   # expm1's backward is expm1 + 1
    # TF's ReluGrad: 0 at exactly 0
    assert ar.value_and_grad64("relu", np.array([0.0]))[1][0] == 0.0
    # the GELU is the oracle's
    gf, _ = ar.value_and_grad64("gelu", x)
    np.testing.assert_allclose(gf, orc.gelu_erf(torch.tensor(x)).numpy(), rtol=1e-15)


def test_ids_follow_the_header():
    assert [activations.IDS[n] for n in ar.NAMES] == list(range(9))
    assert activations.IDS["silu"] == activations.IDS["swish"]


@pytest.mark.parametrize("name", list(activations.NAMES))
def test_encoder_takes_every_name_and_round_trips_it(name):
    enc = Bert4RecEncoder(vocab_size=50, hidden_size=64, num_layers=1, num_attention_heads=2, max_sequence_length=16, inner_dim=256,
                          inner_activation=name, device="cpu")
    assert enc.get_config()["inner_activation"] == name
    assert enc.engine.inner_activation == activations.IDS[name]
    again = Bert4RecEncoder.from_config(enc.get_config())
    assert again.get_config() == enc.get_config()


def test_encoder_legacy_activation_kwarg_and_none():
    enc = Bert4RecEncoder(vocab_size=50, hidden_size=64, num_layers=1, num_attention_heads=2, max_sequence_length=16, inner_dim=256,
                          activation="relu", device="cpu")
    assert enc.get_config()["inner_activation"] == "relu" and enc.engine.inner_activation == activations.RELU
    # None keeps the GELU (Keras would make it linear; the package's classic behaviour stays)
    enc = Bert4RecEncoder(vocab_size=50, hidden_size=64, num_layers=1, num_attention_heads=2, max_sequence_length=16, inner_dim=256,
                          inner_activation=None, device="cpu")
    assert enc.get_config()["inner_activation"] == "gelu" and enc.engine.inner_activation == activations.GELU


@pytest.mark.parametrize("bad", ["softmax", "hard_sigmoid", "exponential", "softsign", "Relu", torch.relu, lambda x: x])
def test_encoder_refuses_other_activations(bad):
    with pytest.raises(NotImplementedError, match="supported"):
        Bert4RecEncoder(vocab_size=50, hidden_size=64, num_layers=1, num_attention_heads=2, max_sequence_length=16, inner_dim=256,
                        inner_activation=bad, device="cpu")


def test_model_refuses_other_mlm_activations():
    from bert4rec_amd.models.bert4rec_model import BERT4RecModel
    enc = Bert4RecEncoder(vocab_size=50, hidden_size=64, num_layers=1, num_attention_heads=2, max_sequence_length=16, inner_dim=256,
                          device="cpu")
    for bad in ("softmax", None, torch.tanh):
        with pytest.raises(NotImplementedError, match="supported"):
            BERT4RecModel(enc, mlm_activation=bad)


def test_model_mlm_activation_is_bound_to_the_encoder():
    from bert4rec_amd.models.bert4rec_model import BERT4RecModel
    enc = Bert4RecEncoder(vocab_size=50, hidden_size=64, num_layers=1, num_attention_heads=2, max_sequence_length=16, inner_dim=256,
                          device="cpu")
    m = BERT4RecModel(enc, mlm_activation="sigmoid")
    assert m.get_config()["mlm_activation"] == "sigmoid" and enc.engine.mlm_activation == activations.SIGMOID
    BERT4RecModel(enc, mlm_activation="sigmoid")   # the same activation again is fine
    with pytest.raises(ValueError, match="sigmoid"):
        BERT4RecModel(enc, mlm_activation="gelu")
    assert enc.engine.mlm_activation == activations.SIGMOID


def ex_cfg(words):
    base = make_model_config(211, 64, 2, 2, 32, 256, 0.1, 0.1)
    return _lib.ModelConfigEx(base, 0, tuple(words))


def test_ex_queries_take_every_activations_word():
    lib = _lib.load()
    classic = lib.b4r_param_total_floats(C.byref(make_model_config(211, 64, 2, 2, 32, 256, 0.1, 0.1)))
    for inner in range(9):
        for mlm in range(9):
            cfg = ex_cfg((0, 0, 0)).set_activations(inner, mlm)
            assert cfg.reserved[1] == inner | (mlm << 8)
            assert lib.b4r_param_total_floats_ex(C.byref(cfg)) == classic
            assert lib.b4r_workspace_bytes_ex(C.byref(cfg), 4, 32, 6) == lib.b4r_workspace_bytes_ex(C.byref(ex_cfg((0, 0, 0))), 4, 32, 6)


@pytest.mark.parametrize("words", [(0, 9, 0), (0, 9 << 8, 0), (0, 0xFF, 0), (0, 1 << 16, 0), (0, -1, 0), (1, 0, 0), (0, 0, 1),
                                   (0, 0x0102, 5)])
def test_ex_queries_refuse_bad_words_with_the_message(words):
    lib = _lib.load()
    cfg = ex_cfg(words)
    assert lib.b4r_param_total_floats_ex(C.byref(cfg)) == -1
    assert lib.b4r_param_count_ex(C.byref(cfg)) == -1
    msg = _lib.last_error()
    assert ("activations word" in msg) if words[0] == 0 and words[2] == 0 else ("reserved" in msg), msg
