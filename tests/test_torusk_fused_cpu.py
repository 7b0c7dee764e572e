"""No-GPU checks of the fused rank-k TFHE route (csrc/torusk_fused_kernels.hpp): the host's one eligibility rule as fhe_tggswk_form_for
states it, on every bound of the rule and one step past each; the lab switch NO_RANKK_FUSED; the refusals fhe_tggswk_prepare documents;
the new exports and harness names."""
import ctypes as C

import pytest

NEW_SYMBOLS = ("fhe_tggswk_key_form", "fhe_tggswk_form_for", "fhe_tfhek_blind_rotate_tables", "fhe_tfhek_bootstrap_tables")

# (k, N, log_b, d)
X3_SHAPES = [(2, 512, 7, 3), (2, 256, 7, 2), (3, 256, 6, 2), (2, 1024, 6, 2),
             (3, 1024, 7, 4)]    # the limit: 16 limbs, 16 * 2^10 * 2^7 = 2^21 exactly
COMPOSED_SHAPES = [(3, 1024, 7, 5),   # 20 limbs
                   (2, 1024, 7, 5),   # log_b d = 35
                   (2, 512, 8, 2),    # base 2^8: a digit no longer fits a byte
                   (2, 2048, 6, 1),   # N too large
                   (2, 128, 7, 2),    # N too small
                   (4, 256, 6, 2),    # k = 4
                   (1, 1024, 7, 3)]   # k = 1 stays on the composed route


def test_new_symbols_and_harness_names(fhe):
    lib = fhe.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    for name in ("form", "blind_rotate_tables", "bootstrap_tables"):
        assert callable(getattr(fhe.TggswKeyK, name, None)), name
    assert callable(fhe.tggswk_form_for) and (fhe.TGGSWK_FORM_COMPOSED, fhe.TGGSWK_FORM_X3) == (0, 1)


def test_the_rule_on_and_past_every_bound(fhe):
    for k, n, log_b, d in X3_SHAPES:
        limbs = (k + 1) * d
        assert k in (2, 3) and 256 <= n <= 1024 and log_b <= 7 and log_b * d <= 31 and limbs <= 16 and limbs * n << log_b <= 1 << 21
        assert fhe.tggswk_form_for(k, n, log_b, d) == fhe.TGGSWK_FORM_X3, (k, n, log_b, d)
    assert 16 * 1024 << 7 == 1 << 21
    for shape in COMPOSED_SHAPES:
        assert fhe.tggswk_form_for(*shape) == fhe.TGGSWK_FORM_COMPOSED, shape
    # the product bound alone: every other condition holds, (k + 1) d N 2^log_b = 12 * 2^10 * 2^8 > 2^21 needs base 2^8 -- so one step
    # past it with byte digits is (3, 1024, 7, 4) with one limb more, the first composed row above; and one step inside:
    assert fhe.tggswk_form_for(3, 1024, 7, 3) == fhe.TGGSWK_FORM_X3 and fhe.tggswk_form_for(2, 1024, 7, 4) == fhe.TGGSWK_FORM_X3


def test_the_lab_switch_turns_every_shape_composed(fhe):
    try:
        fhe.set_option("NO_RANKK_FUSED", 1)
        for shape in X3_SHAPES + COMPOSED_SHAPES:
            assert fhe.tggswk_form_for(*shape) == fhe.TGGSWK_FORM_COMPOSED, shape
    finally:
        fhe.set_option("NO_RANKK_FUSED", 0)
    assert fhe.tggswk_form_for(*X3_SHAPES[0]) == fhe.TGGSWK_FORM_X3   # read at the call


def test_refusals_are_those_of_prepare(fhe):
    lib, form = fhe.lib(), C.c_int(-1)
    ask = lambda k, n, log_b, d: lib.fhe_tggswk_form_for(k, n, log_b, d, C.byref(form))  # noqa: E731
    assert lib.fhe_tggswk_form_for(2, 512, 7, 3, None) == 1    # no output
    assert ask(0, 512, 7, 3) == 1                                # rank 0
    assert ask(2, 48, 7, 3) == 1                                 # n not a power of two
    assert ask(2, 0, 7, 3) == 1
    assert ask(2, 512, 0, 3) == 1 and ask(2, 512, 64, 1) == 1    # log_b outside 1 .. 63
    assert ask(2, 512, 7, 0) == 1 and ask(2, 512, 1, 65) == 1    # d outside 1 .. 64
    assert ask(9, 512, 7, 3) == 6                                # rank above the build's 8
    assert ask(2, 1 << 16, 7, 3) == 6 and ask(2, 1, 7, 3) == 6   # rings outside 2 .. 2^15
    assert ask(2, 64, 62, 1) == 6                                # (k + 1) d n 2^(62 + log_b) >= 2^118 (test_torusk_gpu.py asks prepare the same)
    assert form.value == -1                                      # a refusal writes nothing
    assert ask(8, 2, 1, 1) == 0 and form.value == 0
    assert lib.fhe_tggswk_key_form(None, C.byref(form)) == 1


def test_prepare_without_a_device_still_refuses_first(fhe):
    """a host-only torus context: the shape errors that come before the device check keep their codes"""
    lib, h = fhe.lib(), C.c_void_p()
    assert lib.fhe_tggswk_prepare(None, 2, 7, 3, None, 512, 1, 0, C.byref(h)) == 1 and not h.value


def test_option_name_in_either_case(fhe):
    try:
        fhe.set_option("no_rankk_fused", 1)
        assert fhe.tggswk_form_for(2, 512, 7, 3) == fhe.TGGSWK_FORM_COMPOSED
    finally:
        fhe.set_option("NO_RANKK_FUSED", 0)
    with pytest.raises(fhe.FheError):
        fhe.set_option("NO_RANKK_FUSE", 1)
