"""The activations the feed-forward blocks (Bert4RecEncoder inner_activation) and the masked-LM transform (BERT4RecModel
mlm_activation) run on the device: Keras identifiers -> the ids of include/b4r.h (B4R_ACT_*), TF semantics for value and gradient."""
from __future__ import annotations

from typing import Any

GELU, RELU, SWISH, TANH, SIGMOID, ELU, SELU, SOFTPLUS, LINEAR = range(9)

IDS = {"gelu": GELU, "relu": RELU, "swish": SWISH, "silu": SWISH, "tanh": TANH, "sigmoid": SIGMOID, "elu": ELU, "selu": SELU,
       "softplus": SOFTPLUS, "linear": LINEAR}
NAMES = tuple(IDS)
COUNT = len(set(IDS.values()))   # B4R_ACT_COUNT of include/b4r.h


def activation_id(name: Any, what: str) -> int:
    """The id of the Keras activation `name`; NotImplementedError for anything else (other identifiers, callables)."""
    if isinstance(name, str) and name in IDS:
        return IDS[name]
    raise NotImplementedError(f"{what}={name!r} is not implemented; supported: {', '.join(repr(n) for n in NAMES)}")
