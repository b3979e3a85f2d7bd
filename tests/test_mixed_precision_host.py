"""The mixed-precision policy on the host: mode 2 (B4R_GEMM_BF16) of the C ABI and the Keras-style policy module.  No compute
call is made here."""
import pytest

from bert4rec_amd import _lib
from bert4rec_amd import mixed_precision as mp


@pytest.fixture(autouse=True)
def restore_mode():
    lib = _lib.load()
    prev = lib.b4r_get_gemm_mode()
    yield lib
    _lib.check(lib.b4r_set_gemm_mode(prev))


def test_mode_two_round_trips_and_unknown_modes_are_refused(restore_mode):
    lib = restore_mode
    assert _lib.GEMM_BF16 == 2
    assert lib.b4r_set_gemm_mode(_lib.GEMM_BF16) == 0
    assert lib.b4r_get_gemm_mode() == 2
    for bad in (3, -1):
        assert lib.b4r_set_gemm_mode(bad) != 0
        assert "unknown mode" in _lib.last_error()
        assert lib.b4r_get_gemm_mode() == 2


@pytest.mark.parametrize("mode,split,terms", [(0, 0, 0), (1, 1, 3), (2, 1, 1)])
def test_split_family_helpers(restore_mode, mode, split, terms):
    lib = restore_mode
    _lib.check(lib.b4r_set_gemm_mode(mode))
    assert lib.b4r_split_mode() == split
    assert lib.b4r_gemm_terms() == terms


def test_default_mode_is_unchanged():
    assert _lib.load().b4r_get_gemm_mode() == _lib.GEMM_BF16X3
    assert mp.global_policy().name == "float32"


def test_policy_names_select_modes(restore_mode):
    lib = restore_mode
    mp.set_global_policy("mixed_bfloat16")
    assert lib.b4r_get_gemm_mode() == _lib.GEMM_BF16
    pol = mp.global_policy()
    assert (pol.name, pol.compute_dtype, pol.variable_dtype) == ("mixed_bfloat16", "bfloat16", "float32")
    mp.set_global_policy("float32")
    assert lib.b4r_get_gemm_mode() == _lib.GEMM_BF16X3
    pol = mp.global_policy()
    assert (pol.name, pol.compute_dtype, pol.variable_dtype) == ("float32", "float32", "float32")
    mp.set_global_policy(mp.Policy("mixed_bfloat16", "bfloat16"))
    assert lib.b4r_get_gemm_mode() == _lib.GEMM_BF16


def test_policy_refusals(restore_mode):
    lib = restore_mode
    with pytest.raises(NotImplementedError, match="mixed_bfloat16"):
        mp.set_global_policy("mixed_float16")
    with pytest.raises(ValueError):
        mp.set_global_policy("bfloat16")
    assert lib.b4r_get_gemm_mode() == _lib.GEMM_BF16X3


def test_global_policy_follows_the_c_switch(restore_mode):
    lib = restore_mode
    _lib.check(lib.b4r_set_gemm_mode(_lib.GEMM_BF16))
    assert mp.global_policy().name == "mixed_bfloat16"
    _lib.check(lib.b4r_set_gemm_mode(_lib.GEMM_F32))
    assert mp.global_policy().name == "float32"
    _lib.check(lib.b4r_set_gemm_mode(_lib.GEMM_BF16X3))
    assert mp.global_policy().name == "float32"


def test_a_policy_object_must_carry_its_dtypes(restore_mode):
    lib = restore_mode
    with pytest.raises(ValueError):
        mp.set_global_policy(mp.Policy("mixed_bfloat16", "float32"))
    with pytest.raises(ValueError):
        mp.set_global_policy(mp.Policy("float32", "float32", "bfloat16"))
    assert lib.b4r_get_gemm_mode() == _lib.GEMM_BF16X3
    mp.set_global_policy(mp.global_policy())
    assert lib.b4r_get_gemm_mode() == _lib.GEMM_BF16X3
