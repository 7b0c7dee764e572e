"""The host-only parts of the CKKS bootstrap (include/fhe_ring.h fhe_ckks_eval_mod_plan_create and the refusals that return before a
device is touched) and the self-check of the big-integer model in tests/ckks_bootstrap_model.py.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ckks_bootstrap_model as BM  # noqa: E402

INVALID = 1


@pytest.fixture(scope="module")
def poly(fhe):
    return fhe.ckks_poly


@pytest.fixture(scope="module")
def boot(fhe):
    return fhe.ckks_bootstrap


def points(seed, count=4096):
    rng = np.random.Generator(np.random.PCG64(seed))
    eps = rng.uniform(-2.0 ** -10, 2.0 ** -10, count)
    whole = rng.integers(-7, 8, count).astype(np.float64)
    whole[:15] = np.arange(-7, 8)   # every integer of the range at least once
    return eps, whole


def test_plan_replays_like_the_numpy_recipe(fhe, poly, boot):
    """fhe_ckks_eval_mod_plan_create(8, 3, 31, 1, 1) and eval_mod_ops(8, 3, 31) in float64 on t = eps + I, |eps| <= 2^-10, I in [-7, 7]: the
    two agree within 1e-12 (both evaluate one formula in f64; 32 coefficients that differ by a few ulp give about 1.4e-14, so the margin
    is two orders) and each is within 1e-6 of eps, test_eval_mod_decode's bound.  Measured: 8.2e-15 between the two."""
    plan = boot.eval_mod_plan_c(8, 3, 31)
    ops_np, _ = poly.eval_mod_ops(8, 3, 31)
    ref = fhe.CkksPolyPlan.from_ops(ops_np)
    assert plan.depth == ref.depth
    ops_c = plan.ops
    # (the two schedules need not be the same list: the series' coefficients beyond degree ~20 are rounding noise near 1e-15, and a
    # coefficient that one interpolation rounds to exactly 0.0 is left out structurally)
    assert ops_c[0]["terms"] == ops_np[0]["terms"] and ops_c[-1]["terms"][0][1] == ops_np[-1]["terms"][0][1]   # pre = post = 1: the recipe's own factors
    eps, whole = points(1)
    got_c, got_np = poly.replay_f64(ops_c, eps + whole), poly.replay_f64(ops_np, eps + whole)
    between = float(np.max(np.abs(got_c - got_np)))
    print("eval_mod plan: C against numpy %.3g, against eps %.3g / %.3g" % (between, float(np.max(np.abs(got_c - eps))), float(np.max(np.abs(got_np - eps)))))
    assert between <= 1e-12
    assert float(np.max(np.abs(got_c - eps))) < 1e-6 and float(np.max(np.abs(got_np - eps))) < 1e-6


def test_plan_factors_of_a_bootstrap(fhe, poly, boot):
    """pre = D / (2 q0), post = q0 / D on a 55-bit chain: slots x = 2 t / D with t = q0 (eps + I) come out as (q0 / D) eps within 1e-6,
    on the depth of eval_mod_plan"""
    from oracle import pyref as P
    qs, _ = P.ckks_primes(5, 55, 17)
    q0, scale = qs[0], qs[-1]
    plan = boot.bootstrap_eval_mod_plan(8, 3, 31, q0, scale)
    assert plan.depth == fhe.eval_mod_plan(8, 3, 31).depth
    ops = plan.ops
    assert ops[0]["terms"] == [(0, (scale / (2.0 * q0)) / 8)] and ops[-1]["terms"][0][1] == (q0 / float(scale)) / (2.0 * 3.141592653589793)
    eps, whole = points(2)
    t = (eps + whole) * q0
    got = poly.replay_f64(ops, 2.0 * t / scale)
    err = float(np.max(np.abs(got - (q0 / float(scale)) * eps)))
    print("eval_mod plan with the bootstrap's factors: %.3g" % err)
    assert err < 1e-6


def test_plan_refusals(fhe):
    from learn_fhe_amd import _lib
    lib = _lib.lib()
    h = C.c_void_p()

    def create(K=8, r=3, degree=31, pre=1.0, post=1.0, out=True):
        h.value = None
        rc = lib.fhe_ckks_eval_mod_plan_create(K, r, degree, pre, post, C.byref(h) if out else None)
        assert (rc == 0) == bool(h.value)
        if h.value:
            lib.fhe_ckks_poly_plan_destroy(h)
        return rc

    assert create() == 0 and create(K=1, r=0, degree=1) == 0 and create(degree=255) == 0
    assert create(K=0) == INVALID and create(K=-3) == INVALID
    assert create(r=-1) == INVALID
    assert create(degree=0) == INVALID and create(degree=256) == INVALID and create(degree=-1) == INVALID
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert create(pre=bad) == INVALID and create(post=bad) == INVALID
    assert create(out=False) == INVALID


def test_null_refusals_before_any_device(fhe):
    """every entry refuses a NULL context, bootstrapper or buffer before it looks at a device (host-only contexts: device = -1)"""
    from learn_fhe_amd import _lib
    from oracle import pyref as P
    lib = _lib.lib()
    qs, ps = P.ckks_primes(5, 55, 2)
    rns = fhe.RnsContext(qs, ps[:1], device=-1)
    buf = np.zeros(4 * 32, dtype=np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    H = _lib.MEM_HOST
    assert lib.fhe_ckks_mod_raise(None, p, p, 1, p, p, 32, 1, H, None) == INVALID
    assert lib.fhe_ckks_mod_raise(rns.handle, None, p, 1, p, p, 32, 1, H, None) == INVALID
    assert lib.fhe_ckks_mod_raise(rns.handle, p, p, 1, p, None, 32, 1, H, None) == INVALID
    assert lib.fhe_ckks_mod_raise(rns.handle, p, p, 0, p, p, 32, 1, H, None) == INVALID       # in_limbs < 1
    assert lib.fhe_ckks_mod_raise(rns.handle, p, p, 1, p, p, 24, 1, H, None) == INVALID       # n is no power of two
    assert lib.fhe_ckks_conj_split(None, p, p, p, p, p, p, 32, 1, H, None) == INVALID
    assert lib.fhe_ckks_conj_split(rns.handle, p, p, None, p, p, p, 32, 1, H, None) == INVALID
    assert lib.fhe_ckks_conj_join(None, p, p, p, p, 32, 1, H, None) == INVALID
    assert lib.fhe_ckks_conj_join(rns.handle, p, None, p, p, 32, 1, H, None) == INVALID
    rng = fhe.Rng(seed=3)
    assert lib.fhe_ckks_cjk_gen(None, p, 32, rng._h, 0, p, p, H, None) == INVALID
    assert lib.fhe_ckks_cjk_gen(rns.handle, None, 32, rng._h, 0, p, p, H, None) == INVALID
    assert lib.fhe_ckks_cjk_gen(rns.handle, p, 32, None, 0, p, p, H, None) == INVALID
    h = C.c_void_p()
    lv = (C.c_void_p * 1)(rns.handle)
    assert lib.fhe_ckks_bootstrap_prepare(None, 1, 32, None, None, None, p, p, H, C.byref(h)) == INVALID and not h.value
    assert lib.fhe_ckks_bootstrap_prepare(lv, 1, 32, None, None, None, p, p, H, C.byref(h)) == INVALID and not h.value
    assert lib.fhe_ckks_bootstrap_prepare(lv, 1, 32, None, None, None, p, p, H, None) == INVALID
    assert lib.fhe_ckks_bootstrap_apply(None, p, p, 1, p, p, 1, H, None) == INVALID
    assert lib.fhe_ckks_bootstrap_info(None, None, None) == INVALID
    lib.fhe_ckks_bootstrap_destroy(None)


@pytest.mark.parametrize("n", [2, 4, 32])
def test_model_self_check(n):
    """join(split(x, conj x)) = 2 x for random polynomials (any second operand serves as `conj x`: the identity is linear algebra), the
    model's X^(n/2) equals the schoolbook negacyclic product by the monomial, and applying it twice negates (X^n = -1)"""
    rng = np.random.Generator(np.random.PCG64(n))
    for q in (97, (1 << 55) - 55 * 0 - 31, 1152921504606748673):
        x = [int(v) % q for v in rng.integers(0, 1 << 62, n)]
        cx = [int(v) % q for v in rng.integers(0, 1 << 62, n)]
        assert BM.shift_half(x, q) == BM.monomial_schoolbook(x, n // 2, q)
        assert BM.shift_half(BM.shift_half(x, q), q) == [(-v) % q for v in x]
        r, j = BM.split(x, cx, q)
        assert BM.join(r, j, q) == [2 * v % q for v in x]


def test_model_mod_raise_edges():
    q0 = 97
    got = BM.mod_raise([0, 1, 48, 49, 96], q0, [97, 7, 1009])
    assert got[0] == [0, 1, 48, 49, 96]
    assert got[1] == [0, 1, 48 % 7, (-48) % 7, 6]
    assert got[2] == [0, 1, 48, 1009 - 48, 1008]
