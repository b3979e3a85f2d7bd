"""Restatement of the factorised BERT4Rec model (Bert4RecEncoder(embedding_width=E), bert4rec_encoder.py:103-131, 198-214) built
from the frozen oracle's own pieces: the item and position tables are E wide, LayerNorm and dropout run at width E, then the learned
E -> H projection; tfm MaskedLM is built from the [V, E] table, so its transform maps H -> E.  With E = H, Wp = I and bp = 0 it is
oracle.model_forward (tests/test_factorized_host.py pins it there)."""
import math
from typing import Dict, Optional, Tuple

import torch

from oracle import bert4rec_oracle as orc

PROJ_W, PROJ_B = "embedding_projection/kernel", "embedding_projection/bias"


def param_shapes(cfg: orc.OracleConfig, E: int):
    """the Keras names and shapes of the factorised model: the oracle's list with the E-wide entries and the projection"""
    H = cfg.hidden_size
    wide_e = {"word_embeddings/embeddings": (cfg.vocab_size, E), "position_embedding/embeddings": (cfg.max_sequence_length, E),
              "embeddings/layer_norm/gamma": (E,), "embeddings/layer_norm/beta": (E,),
              "cls/predictions/transform/dense/kernel": (H, E), "cls/predictions/transform/dense/bias": (E,),
              "cls/predictions/transform/LayerNorm/gamma": (E,), "cls/predictions/transform/LayerNorm/beta": (E,)}
    out = [(n, wide_e.get(n, s)) for n, s in orc.param_names_and_shapes(cfg)]
    return out + [(PROJ_W, (E, H)), (PROJ_B, (H,))]


def init_params(cfg: orc.OracleConfig, E: int, seed: int = 3) -> Dict[str, torch.Tensor]:
    """the oracle's initialisers over the factorised shapes (projection: TruncatedNormal(0.02) kernel, zero bias), then biases,
    betas and gammas made non-trivial so that their gradients are exercised"""
    g = torch.Generator().manual_seed(seed)
    params = {}
    for name, shape in param_shapes(cfg, E):
        if name == "cls/predictions/transform/dense/kernel":
            lim = math.sqrt(6.0 / (shape[0] + shape[1]))
            t = (torch.rand(shape, generator=g) * 2 - 1) * lim
        elif name.endswith(("bias", "beta")):
            t = torch.randn(shape, generator=g) * 0.02
        elif name.endswith("gamma"):
            t = 1.0 + torch.randn(shape, generator=g) * 0.05
        else:
            t = torch.empty(shape)
            torch.nn.init.trunc_normal_(t, mean=0.0, std=0.02, a=-0.04, b=0.04, generator=g)
        params[name] = t.to(torch.float32)
    return params


def embed(params, input_word_ids, cfg: orc.OracleConfig, training: bool = False, rng: Optional[Tuple[int, int]] = None):
    """x0 [B, L, H]: item row + position row at width E, LayerNorm, dropout (element index row * E + col), projection"""
    L = input_word_ids.shape[1]
    T = params["word_embeddings/embeddings"]
    ids = torch.where((input_word_ids >= 0) & (input_word_ids < T.shape[0]), input_word_ids, torch.zeros_like(input_word_ids))
    e = T[ids] + params["position_embedding/embeddings"][:L].unsqueeze(0)
    e = orc.layer_norm(e, params["embeddings/layer_norm/gamma"], params["embeddings/layer_norm/beta"], cfg.ln_eps)
    e = orc._dropout(e, cfg.output_dropout, training, rng, orc.STREAM_EMB)
    return e @ params[PROJ_W] + params[PROJ_B]


def encoder_forward(params, input_word_ids, input_mask, cfg: orc.OracleConfig, training=False, rng=None):
    """the oracle's encoder layers (orc.encoder_forward's loop, restated) on the projected embeddings"""
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
        f = orc.gelu_erf(x1 @ params[f"{p}/intermediate/kernel"] + params[f"{p}/intermediate/bias"])
        g = f @ params[f"{p}/output/kernel"] + params[f"{p}/output/bias"]
        g = orc._dropout(g, cfg.output_dropout, training, rng, orc.stream_ffn_out(i))
        x = orc.layer_norm(g + x1, params[f"{p}/output_layer_norm/gamma"], params[f"{p}/output_layer_norm/beta"], cfg.ln_eps)
        outs.append(x)
    return dict(sequence_output=x, encoder_outputs=outs)


def model_forward(params, batch, cfg: orc.OracleConfig, training=False, rng=None):
    """logits [B, P, V] and the transform rows mlm_hidden [B, P, E]"""
    out = encoder_forward(params, batch["input_word_ids"], batch["input_mask"], cfg, training, rng)
    x = out["sequence_output"]
    B, L, H = x.shape
    offs = (torch.arange(B, dtype=torch.int64) * L)[:, None]
    g = x.reshape(B * L, H)[(batch["masked_lm_positions"].to(torch.int64) + offs).reshape(-1)]
    t = orc.gelu_erf(g @ params["cls/predictions/transform/dense/kernel"] + params["cls/predictions/transform/dense/bias"])
    t = orc.layer_norm(t, params["cls/predictions/transform/LayerNorm/gamma"], params["cls/predictions/transform/LayerNorm/beta"],
                       cfg.ln_eps)
    t = t.reshape(B, -1, t.shape[-1])
    out["mlm_hidden"] = t
    out["mlm_logits"] = t @ params["word_embeddings/embeddings"].t() + params["cls/predictions/output_bias/bias"]
    return out


def loss_and_grads(params, batch, cfg: orc.OracleConfig, training=True, rng=None, dtype=torch.float32):
    """mean masked cross-entropy and its autograd gradients wrt every trainable variable (the oracle's loss_and_grads, restated)"""
    leaf = {n: p.detach().clone().to(dtype).requires_grad_(orc.is_trainable(n)) for n, p in params.items()}
    out = model_forward(leaf, batch, cfg, training, rng)
    loss = orc.masked_sparse_categorical_crossentropy(batch["masked_lm_ids"], out["mlm_logits"])
    names = [n for n in leaf if orc.is_trainable(n)]
    gs = torch.autograd.grad(loss, [leaf[n] for n in names], allow_unused=True)
    grads = {n: (g if g is not None else torch.zeros_like(leaf[n])) for n, g in zip(names, gs)}
    return loss.detach(), {n: g.detach() for n, g in grads.items()}, {k: v for k, v in out.items() if torch.is_tensor(v)}
