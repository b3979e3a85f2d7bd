"""Host side of b4r_rank_full (no GPU): the scratch query and the argument checks of the C ABI and the Python layer."""
import numpy as np
import pytest
import torch

from bert4rec_amd import _lib
from bert4rec_amd.engine import check_rank_full_args


def test_scratch_query_without_gpu():
    lib = _lib.load()
    big = lib.b4r_rank_full_scratch_bytes(256, 335423, 100)
    assert 0 < big < 256 * 335423 * 4 // 4                       # grows with rows x chunks x K, not rows x V
    assert lib.b4r_rank_full_scratch_bytes(512, 335423, 100) > big
    assert lib.b4r_rank_full_scratch_bytes(256, 335423, 10) < big
    assert lib.b4r_rank_full_scratch_bytes(0, 335423, 100) == 0
    assert lib.b4r_rank_full_scratch_bytes(4, 335423, 1025) == 0


def test_c_abi_refuses_bad_shapes_before_touching_the_device():
    lib = _lib.load()
    args = lambda R, K, H=64, ld=64, E=0: (None, ld, None, None, None, H, 1000, 3, R, None, E, None, K, None, None, None, None, 0, None)
    assert lib.b4r_rank_full(*args(4, 1025)) == -2
    assert lib.b4r_rank_full(*args(4, -1)) == -2
    assert lib.b4r_rank_full(*args(-1, 10)) == -2
    assert lib.b4r_rank_full(*args(4, 10, H=30, ld=30)) == -2
    assert lib.b4r_rank_full(*args(4, 10, ld=32)) == -2
    assert lib.b4r_rank_full(*args(4, 10)) == -1                # null hidden / table / bias
    assert "b4r_rank_full" in _lib.last_error()
    assert lib.b4r_rank_full(*args(0, 10)) == 0                  # nothing to rank


def test_python_argument_validation():
    assert check_rank_full_args(0) == 0 and check_rank_full_args(1024) == 1024 and check_rank_full_args(np.int64(10)) == 10
    for k in (-1, 1025, 2.5, "3"):
        with pytest.raises(ValueError):
            check_rank_full_args(k)
    with pytest.raises(ValueError):
        check_rank_full_args(10, torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError):
        check_rank_full_args(10, torch.zeros(2, 3, 4, dtype=torch.int64))
    with pytest.raises(ValueError):
        check_rank_full_args(10, torch.zeros(3, 4, dtype=torch.int64), n_rows=5)
    check_rank_full_args(10, torch.zeros(5, 4, dtype=torch.int64), n_rows=5)
