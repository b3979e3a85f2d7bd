"""Mixed-precision policy, modelled on keras.mixed_precision: set_global_policy / global_policy / Policy.

The policy is the library's process-wide arithmetic mode (include/b4r.h b4r_set_gemm_mode):

  "float32"         B4R_GEMM_BF16X3 (the default): every bf16 matrix-core product runs as three split terms, fp32-level results
  "mixed_bfloat16"  B4R_GEMM_BF16: the same launch plan with operands rounded once to bf16 and one MFMA per k-slice (fp32
                    accumulation); normalisation, softmax statistics, activations, loss and the optimizer stay fp32

The exact-fp32 mode (B4R_GEMM_F32) stays reachable through b4r_set_gemm_mode only and reports itself as "float32".
Deviation from Keras: outputs stay fp32 tensors (Keras would return a bf16 pooled_output under "mixed_bfloat16"), and
weights, their master copy and every stored activation keep their fp32 dtype."""
from __future__ import annotations

from dataclasses import dataclass

from . import _lib

__all__ = ["Policy", "set_global_policy", "global_policy"]

_MODES = {"float32": _lib.GEMM_BF16X3, "mixed_bfloat16": _lib.GEMM_BF16}


@dataclass(frozen=True)
class Policy:
    name: str
    compute_dtype: str
    variable_dtype: str = "float32"


def _policy(name: str) -> Policy:
    return Policy(name, "bfloat16" if name == "mixed_bfloat16" else "float32")


def set_global_policy(name) -> None:
    """Select the arithmetic of every later step: "float32" or "mixed_bfloat16" (a Policy is accepted too).  Captured train
    steps are keyed by the mode, so a graph never replays the other mode's kernels."""
    if isinstance(name, Policy):
        if name.name in _MODES and name != _policy(name.name):
            raise ValueError(f"{name!r}: the {name.name!r} policy computes in {_policy(name.name).compute_dtype} and keeps "
                             "float32 variables")
        name = name.name
    if name == "mixed_float16":
        raise NotImplementedError('"mixed_float16" needs loss scaling, which this library does not implement; '
                                  'use "mixed_bfloat16"')
    if name not in _MODES:
        raise ValueError(f'unknown policy {name!r}: "float32" or "mixed_bfloat16"')
    _lib.check(_lib.load().b4r_set_gemm_mode(_MODES[name]))


def global_policy() -> Policy:
    """The policy of the library's current mode (B4R_GEMM_F32, set through b4r_set_gemm_mode, reads as "float32")."""
    mode = _lib.load().b4r_get_gemm_mode()
    return _policy("mixed_bfloat16" if mode == _lib.GEMM_BF16 else "float32")
