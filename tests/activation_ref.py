"""Restatement of the BERT4Rec model with separate activations for the feed-forward blocks (Bert4RecEncoder inner_activation,
bert4rec_encoder.py:70,88-89,140) and the masked-LM transform (BERT4RecModel mlm_activation, bert4rec_model.py:42,77-81), built from
the frozen oracle's own pieces (and tests/factorized_ref.py's embedding stage when the parameters hold a projection).  At
("gelu", "gelu") it is oracle.model_forward / oracle.loss_and_grads (tests/test_activation_host.py pins it there)."""
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from oracle import bert4rec_oracle as orc
from tests import factorized_ref as fr

SELU_ALPHA, SELU_SCALE = 1.6732632423543772, 1.0507009873554805

# TF semantics: relu' = 0 at 0 (torch.relu's autograd agrees), softplus overflow-safe
ACT = {
    "gelu": orc.gelu_erf,
    "relu": torch.relu,
    "swish": lambda x: x * torch.sigmoid(x),
    "silu": lambda x: x * torch.sigmoid(x),
    "tanh": torch.tanh,
    "sigmoid": torch.sigmoid,
    "elu": lambda x: torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0.0))),
    "selu": lambda x: SELU_SCALE * torch.where(x > 0, x, SELU_ALPHA * torch.expm1(torch.clamp(x, max=0.0))),
    "softplus": lambda x: torch.logaddexp(x, torch.zeros_like(x)),
    "linear": lambda x: x,
}
NAMES = ("gelu", "relu", "swish", "tanh", "sigmoid", "elu", "selu", "softplus", "linear")   # ids 0..8 of include/b4r.h


def embed(params, input_word_ids, cfg: orc.OracleConfig, training=False, rng=None):
    if fr.PROJ_W in params:
        return fr.embed(params, input_word_ids, cfg, training, rng)
    L = input_word_ids.shape[1]
    x = params["word_embeddings/embeddings"][input_word_ids] + params["position_embedding/embeddings"][:L].unsqueeze(0)
    x = orc.layer_norm(x, params["embeddings/layer_norm/gamma"], params["embeddings/layer_norm/beta"], cfg.ln_eps)
    return orc._dropout(x, cfg.output_dropout, training, rng, orc.STREAM_EMB)


def encoder_forward(params, input_word_ids, input_mask, cfg: orc.OracleConfig, inner="gelu", training=False, rng=None):
    """orc.encoder_forward's layers, restated, with `inner` between the two dense layers of every feed-forward block"""
    act = ACT[inner]
    x = embed(params, input_word_ids, cfg, training, rng)
    d = cfg.head_dim
    adder = (1.0 - input_mask.to(torch.float32))[:, None, None, :] * torch.tensor(-1e9, dtype=torch.float32)
    outs = []
    for i in range(cfg.num_layers):
        p = f"transformer/layer_{i}"
        q = torch.einsum("blH,Hhd->blhd", x, params[f"{p}/self_attention/query/kernel"]) + params[f"{p}/self_attention/query/bias"]
        k = torch.einsum("blH,Hhd->blhd", x, params[f"{p}/self_attention/key/kernel"]) + params[f"{p}/self_attention/key/bias"]
        v = torch.einsum("blH,Hhd->blhd", x, params[f"{p}/self_attention/value/kernel"]) + params[f"{p}/self_attention/value/bias"]
        q = q * torch.tensor(1.0 / math.sqrt(float(d)), dtype=torch.float32)
        s = torch.einsum("bqhd,bkhd->bhqk", q, k) + adder
        a = torch.softmax(s, dim=-1)
        a = orc._dropout(a, cfg.attention_dropout, training, rng, orc.stream_attn_probs(i), orc.ATTN_PITCH)
        ctx = torch.einsum("bhqk,bkhd->bqhd", a, v)
        y = torch.einsum("bqhd,hdH->bqH", ctx, params[f"{p}/self_attention/attention_output/kernel"]) \
            + params[f"{p}/self_attention/attention_output/bias"]
        y = orc._dropout(y, cfg.output_dropout, training, rng, orc.stream_attn_out(i))
        x1 = orc.layer_norm(x + y, params[f"{p}/self_attention_layer_norm/gamma"], params[f"{p}/self_attention_layer_norm/beta"],
                            cfg.ln_eps)
        f = act(x1 @ params[f"{p}/intermediate/kernel"] + params[f"{p}/intermediate/bias"])
        g = f @ params[f"{p}/output/kernel"] + params[f"{p}/output/bias"]
        g = orc._dropout(g, cfg.output_dropout, training, rng, orc.stream_ffn_out(i))
        x = orc.layer_norm(g + x1, params[f"{p}/output_layer_norm/gamma"], params[f"{p}/output_layer_norm/beta"], cfg.ln_eps)
        outs.append(x)
    return dict(sequence_output=x, encoder_outputs=outs)


def mlm_transform(params, sequence_output, masked_lm_positions, cfg: orc.OracleConfig, mlm="gelu"):
    """orc.mlm_transform with `mlm` as the dense layer's activation: [B, P, E]"""
    B, L, H = sequence_output.shape
    offs = (torch.arange(B, dtype=torch.int64) * L)[:, None]
    g = sequence_output.reshape(B * L, H)[(masked_lm_positions.to(torch.int64) + offs).reshape(-1)]
    t = ACT[mlm](g @ params["cls/predictions/transform/dense/kernel"] + params["cls/predictions/transform/dense/bias"])
    t = orc.layer_norm(t, params["cls/predictions/transform/LayerNorm/gamma"], params["cls/predictions/transform/LayerNorm/beta"],
                       cfg.ln_eps)
    return t.reshape(B, -1, t.shape[-1])


def model_forward(params, batch, cfg: orc.OracleConfig, inner="gelu", mlm="gelu", training=False, rng=None):
    out = encoder_forward(params, batch["input_word_ids"], batch["input_mask"], cfg, inner, training, rng)
    t = mlm_transform(params, out["sequence_output"], batch["masked_lm_positions"], cfg, mlm)
    out["mlm_hidden"] = t
    out["mlm_logits"] = t @ params["word_embeddings/embeddings"].t() + params["cls/predictions/output_bias/bias"]
    return out


def loss_and_grads(params, batch, cfg: orc.OracleConfig, inner="gelu", mlm="gelu", training=True, rng=None):
    leaf = {n: p.detach().clone().requires_grad_(orc.is_trainable(n)) for n, p in params.items()}
    out = model_forward(leaf, batch, cfg, inner, mlm, training, rng)
    loss = orc.masked_sparse_categorical_crossentropy(batch["masked_lm_ids"], out["mlm_logits"])
    names = [n for n in leaf if orc.is_trainable(n)]
    gs = torch.autograd.grad(loss, [leaf[n] for n in names], allow_unused=True)
    grads = {n: (g if g is not None else torch.zeros_like(leaf[n])) for n, g in zip(names, gs)}
    out = {k: (v.detach() if torch.is_tensor(v) else [t.detach() for t in v]) for k, v in out.items()}
    return loss.detach(), grads, out


def train_step(params, m, v, batch, cfg: orc.OracleConfig, hp: orc.AdamWConfig, step: int, inner="gelu", mlm="gelu",
               training=True, rng: Optional[Tuple[int, int]] = None) -> Dict[str, float]:
    """orc.train_step with the two activations: mutates params / m / v"""
    loss, grads, out = loss_and_grads(params, batch, cfg, inner, mlm, training, rng)
    gnorm = orc.adamw_apply(params, grads, m, v, step, hp)
    return dict(loss=float(loss), grad_norm=gnorm)


def value_and_grad64(name: str, x: np.ndarray):
    """fp64 f and f' of activation `name` at the points x (autograd of the torch restatement)"""
    t = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    y = ACT[name](t)
    (d,) = torch.autograd.grad(y.sum(), t)
    return y.detach().numpy(), d.numpy()
