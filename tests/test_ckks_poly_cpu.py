"""The host-only plan of the CKKS polynomial evaluation (include/fhe_ring.h fhe_ckks_poly_plan_*, fhe_ckks_scaled_constant): the
exported schedule replayed in float64 against numpy, its structural rules, the exact constants and the refusals.  No GPU."""
import ctypes as C
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ckks_poly_model as PM  # noqa: E402

INVALID = 1
DEGREES = [0, 1, 2, 3, 7, 8, 31, 63, 255]
X = np.cos(np.pi * (np.arange(64) + 0.5) / 64)  # 64 points of [-1, 1], dense near the ends where T_j swings fastest
X[0], X[-1] = 1.0, -1.0


def coefficients(degree, odd_only, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    c = rng.uniform(-1, 1, degree + 1)
    if odd_only:
        c[0::2] = 0.0
    return c


@pytest.fixture(scope="module")
def poly(fhe):
    return fhe.ckks_poly


@pytest.mark.parametrize("basis", [0, 1])
@pytest.mark.parametrize("odd_only", [False, True])
@pytest.mark.parametrize("degree", DEGREES)
def test_schedule_replays_to_the_series(fhe, poly, degree, odd_only, basis):
    """The exported ops in float64 equal chebval / polyval to 1e-11 sum |c_j|.  Why that holds: the schedule has at most 300 ops, every
    intermediate (a T_j, a power of x, a block or a quotient) is bounded on [-1, 1] by 2^4 sum |c_j| (the split doubles Chebyshev
    quotient coefficients once per giant, at most four giants), and each op adds a relative rounding of at most 17 * 2^-53, so the replay
    is within 300 * 17 * 16 * 2^-53 < 1e-11 of the exact series -- numpy's own evaluation rounds far less."""
    c = coefficients(degree, odd_only, 1000 * basis + degree)
    plan = fhe.CkksPolyPlan(c, basis)
    ops = plan.ops
    assert len(ops) == plan.n_ops <= 300
    want = np.polynomial.chebyshev.chebval(X, c) if basis == 0 else np.polynomial.polynomial.polyval(X, c)
    got = poly.replay_f64(ops, X)
    err = float(np.max(np.abs(got - want)))
    print("degree %d basis %d odd %d: %d ops, depth %d, replay error %.3g" % (degree, basis, odd_only, len(ops), plan.depth, err))
    assert err <= 1e-11 * max(float(np.sum(np.abs(c))), 1e-300)
    # structure: written once and before read, at most 16 terms, the reported depth is the deepest register and small
    written = {0}
    for o in ops:
        reads = [o["a"], o["b"]] + ([o["c"]] if o["c"] >= 0 else []) if o["kind"] == poly.MUL else [s for s, _ in o["terms"]]
        assert all(g in written for g in reads)
        assert o["dst"] not in written
        written.add(o["dst"])
        if o["kind"] == poly.LIN:
            assert 1 <= len(o["terms"]) <= 16
            assert all(v != 0.0 for _, v in o["terms"]) or (len(o["terms"]) == 1 and o["terms"][0] == (0, 0.0))
        else:
            assert o["alpha"] in (1, 2)
    d = poly.depths(ops)
    assert plan.depth == max(d.values()) == d[ops[-1]["dst"]]
    assert plan.n_regs == max(written) + 1
    assert plan.depth <= math.ceil(math.log2(degree + 1)) + 2
    for o in ops:  # a subtrahend has every limb of the product
        if o["kind"] == poly.MUL and o["c"] >= 0:
            assert d[o["c"]] <= d[o["dst"]]


def test_zero_terms_are_left_out(fhe, poly):
    """an odd series never forms an even block term; degree 0 and the zero series are the single op 0 * input + c0"""
    ops = fhe.CkksPolyPlan([0.0, 0.5, 0.0, 0.25], 0).ops
    assert [o for o in ops if o["kind"] == poly.LIN and o["mode"] == 1][0]["c0"] == 0.0
    for c in ([0.75], [0.0, 0.0, 0.0]):
        ops = fhe.CkksPolyPlan(c, 0).ops
        assert ops == [poly.lin_op(1, 1, [(0, 0.0)], c[0])]
    # trailing zeros do not raise the depth
    assert fhe.CkksPolyPlan([0.1, 0.2] + [0.0] * 30, 0).depth == 1


def test_scaled_constants_are_exact(poly):
    """trunc(c * scale) mod q against exact rational arithmetic"""
    q, scale = (1 << 55) - 55 * 64 + 1, (1 << 55) + 1234567
    cs = [2.0 ** -60, -2.0 ** -60, 1 - 2.0 ** -53, -(1 - 2.0 ** -53), 0.1, -0.1, 0.0, -0.0, 3.0, -7.0, 2.0 ** -55, 1.5, 2.0 ** 60, -2.0 ** 70 * 1.25,
             5e-324, 1.0 / 3.0]
    for sc in (scale, 1 << 55, 1, (1 << 64) - 1):
        for c in cs:
            if abs(Fraction(c) * sc) >= 1 << 126:
                continue
            for m in (q, 2147483649, (1 << 62) - 57):
                assert poly.scaled_constant(c, sc, m) == PM.scaled_constant(c, sc, m), (c, sc, m)
    assert PM.trunc_scaled(-0.1, 10) == -1 and PM.trunc_scaled(0.19, 10) == 1   # toward zero, both signs
    assert poly.scaled_constant(2.0 ** 62 * (1 - 2.0 ** -53), (1 << 64) - 1, q) == PM.scaled_constant(2.0 ** 62 * (1 - 2.0 ** -53), (1 << 64) - 1, q)


def test_refusals(fhe, poly):
    from learn_fhe_amd import _lib
    lib = _lib.lib()
    dp = lambda v: np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    h = C.c_void_p()

    def create(c, degree, basis, out=True):
        rc = lib.fhe_ckks_poly_plan_create(dp(c) if c is not None else None, degree, basis, C.byref(h) if out else None)
        assert (rc == 0) == bool(h.value) or not out
        if h.value:
            lib.fhe_ckks_poly_plan_destroy(h)
            h.value = None
        return rc

    assert create(np.ones(256), 255, 0) == 0
    assert create(np.ones(257), 256, 0) == INVALID
    assert create(np.ones(2), -1, 0) == INVALID
    assert create(np.ones(2), 1, 2) == INVALID
    assert create([1.0, float("nan")], 1, 0) == INVALID
    assert create([float("inf"), 1.0], 1, 1) == INVALID
    assert create(None, 1, 0) == INVALID
    assert create(np.ones(2), 1, 0, out=False) == INVALID
    out = C.c_uint64()
    for c in (float("nan"), float("inf"), 2.0 ** 71, -2.0 ** 71):  # 2^71 * 2^55 = 2^126
        assert lib.fhe_ckks_scaled_constant(c, 1 << 55, 97, C.byref(out)) == INVALID
    assert lib.fhe_ckks_scaled_constant(2.0 ** 71 * (1 - 2.0 ** -53), 1 << 55, 97, C.byref(out)) == 0
    assert lib.fhe_ckks_scaled_constant(1.0, 0, 97, C.byref(out)) == INVALID
    assert lib.fhe_ckks_scaled_constant(1.0, 1 << 55, 97, None) == INVALID
    assert lib.fhe_ckks_poly_plan_info(None, None, None, None) == INVALID
    # caller-made lists: a read before the write, a register written twice, a fractional integer multiplier, alpha = 3, a result that
    # is not the deepest register, a subtrahend deeper than its product
    bad = [
        [poly.mul_op(1, 0, 2)],
        [poly.mul_op(1, 0, 0), poly.mul_op(1, 0, 0)],
        [poly.lin_op(1, 0, [(0, 1.5)], 0.0)],
        [poly.mul_op(1, 0, 0, alpha=3)],
        [poly.mul_op(1, 0, 0), poly.lin_op(2, 0, [(0, 1)], 0.0)],
        [poly.mul_op(1, 0, 0), poly.mul_op(2, 1, 1), poly.mul_op(3, 0, 0, 1, 2)],
    ]
    for ops in bad:
        with pytest.raises(fhe.FheError):
            fhe.CkksPolyPlan.from_ops(ops)
    plan = fhe.CkksPolyPlan.from_ops([poly.mul_op(1, 0, 0, 2), poly.lin_op(2, 0, [(1, 1)], -1.0)])
    assert (plan.depth, plan.n_ops, plan.n_regs) == (1, 2, 3)


def test_eval_mod_recipe_in_f64(fhe, poly):
    """K = 4, r = 2, degree 31: the f64 evaluation of the recipe lies within 1e-6 of eps for t = eps + I, |eps| <= 2^-10, |I| <= 4:
    sin(2 pi eps) / (2 pi) - eps is at most (2 pi)^2 eps^3 / 6 < 7e-9, and the degree-31 interpolant of a cosine of 2 pi K / 2^r = 2 pi
    radians of half-range has an error near 1e-16, which r = 2 doublings multiply by at most 16."""
    K, r, degree = 4, 2, 31
    ops, coeffs = poly.eval_mod_ops(K, r, degree)
    plan = fhe.eval_mod_plan(K, r, degree)
    assert plan.ops == ops
    series_depth = fhe.CkksPolyPlan(coeffs, 0).depth
    assert plan.depth == 1 + series_depth + r + 1
    u = np.linspace(-1, 1, 2001)
    interp = np.polynomial.chebyshev.chebval(u, coeffs) - np.cos(2 * np.pi * (K * u - 0.25) / 2 ** r)
    assert float(np.max(np.abs(interp))) < 1e-12
    rng = np.random.Generator(np.random.PCG64(4))
    eps = rng.uniform(-2.0 ** -10, 2.0 ** -10, 512)
    t = eps + rng.integers(-K, K + 1, 512)
    t = np.clip(t, -K, K)
    eps = t - np.round(t)
    got = poly.replay_f64(ops, t)
    assert float(np.max(np.abs(got - eps))) < 1e-6
