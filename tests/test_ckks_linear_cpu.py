"""The CKKS linear-transform plan without a GPU: the exact model's own self-check (the reference's `sfft_mat_factorization`,
scheme/ckks/src/sfft.rs:125-134), the structure a host-only plan reports against that model, and the refusals that reach no device."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ckks_encode_model as Mo  # noqa: E402
import ckks_linear_model as LM  # noqa: E402

INVALID, UNSUPPORTED = 1, 6


@pytest.mark.parametrize("log_l", range(1, 8))
def test_model_factorization_and_inverses(log_l):
    """sfft.rs:125-134 for l = 2 .. 128: the product of all factors has the bit-reversed powers of w(l)[i] as row i (the l / 2 rows
    the reference compares); every inverse factor times its factor is the identity to 2^-250"""
    l = 1 << log_l
    fm = LM.sfft_fmats(l)
    dense = LM.to_dense(LM.product(fm, l), l)
    tol = Mo.mpf(2) ** -250
    for i, t in enumerate(Mo.w(l)):
        row = Mo.bit_reverse([t ** e for e in range(l)])
        assert max(abs(a - b) for a, b in zip(dense[i], row)) < tol
    for f in fm:
        ident = LM.normalised(LM.mul(LM.inv(f, l), f, l), l)
        for d, v in ident.items():
            assert max(abs(x - (1 if d == 0 else 0)) for x in v) < tol


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("l", [2, 4, 16, 64, 256])
def test_structure_of_a_host_only_plan(fhe, l, inverse):
    """depth, diagonal index sets (mod l), the split and the rotation union for r in {1, 2, 3, 4, log2 l}"""
    log_l = l.bit_length() - 1
    enc = fhe.CkksEncoder(2 * l, device=-1)
    for r in sorted({1, 2, 3, 4, log_l}):
        plan = fhe.CkksLinearPlan(enc, r, inverse)
        mats = LM.chunked(l, r, inverse)
        assert plan.depth == len(mats) == -(-log_l // min(r, log_l))
        for k, m in enumerate(mats):
            idx, bsgs_k, split = plan.matrix(k)
            assert idx == sorted(LM.normalised(m, l))
            want_k, want_split = fhe.bsgs_split(idx)
            assert bsgs_k == want_k and split == {i: sorted(js) for i, js in want_split.items()}
            if r == 1 and inverse:  # `inv` maps 0 to l (matrix.rs:77); here it is 0
                assert l in m and 0 in idx and l not in idx
            if r >= log_l:
                assert idx == list(range(l))
        assert plan.rotations == LM.rotation_union(mats, l, fhe.bsgs_split)
    if l == 2 and not inverse:
        plan = fhe.CkksLinearPlan(enc, 1, False)
        assert plan.depth == 1 and plan.matrix(0)[0] == [0, 1] and plan.rotations == [1]


def test_refusals_without_a_device(fhe, cref):
    from learn_fhe_amd import _lib
    lib = _lib.lib()
    enc = fhe.CkksEncoder(16, device=-1)
    h = C.c_void_p()
    assert lib.fhe_ckks_linear_plan_create(enc.handle, 0, 0, C.byref(h)) == INVALID and not h.value
    assert lib.fhe_ckks_linear_plan_create(enc.handle, -3, 1, C.byref(h)) == INVALID and not h.value
    assert lib.fhe_ckks_linear_plan_create(None, 1, 0, C.byref(h)) == INVALID and not h.value
    assert lib.fhe_ckks_linear_plan_create(enc.handle, 1, 0, None) == INVALID
    assert lib.fhe_ckks_linear_plan_create(fhe.CkksEncoder(2, device=-1).handle, 1, 0, C.byref(h)) == UNSUPPORTED and not h.value  # l = 1: no factor
    big = fhe.CkksEncoder(1 << 15, device=-1)
    assert lib.fhe_ckks_linear_plan_create(big.handle, 14, 0, C.byref(h)) == UNSUPPORTED and not h.value   # a dense 2^14 x 2^14 matrix
    plan = fhe.CkksLinearPlan(enc, 2)
    assert plan.depth == 2
    out = (C.c_double * (4 * 8 * 8))()
    assert lib.fhe_ckks_linear_plan_diags(plan.handle, 0, out) == INVALID          # host-only: no values
    assert lib.fhe_ckks_linear_plan_matrix_info(plan.handle, 2, None, None, None, None) == INVALID
    assert lib.fhe_ckks_linear_plan_matrix_info(plan.handle, -1, None, None, None, None) == INVALID
    assert lib.fhe_ckks_linear_plan_rotations(plan.handle, None, len(plan.rotations) + 1) == INVALID
    assert lib.fhe_ckks_linear_plan_info(None, None, None) == INVALID
    pr = cref.two_adic_primes(60, 5, 3)
    qs, ps = pr[:2], pr[2:]
    ctxs = [fhe.RnsContext(qs[:k], ps, device=-1) for k in (2, 1)]
    lv = (C.c_void_p * 2)(*[c.handle for c in ctxs])
    assert lib.fhe_ckks_linear_transform_prepare(plan.handle, lv, 2, qs[-1], None, None, None, 0, _lib.MEM_HOST, C.byref(h)) == INVALID and not h.value
    assert lib.fhe_ckks_linear_transform_prepare(plan.handle, lv, 2, qs[-1], None, None, None, 0, _lib.MEM_HOST, None) == INVALID
    assert lib.fhe_ckks_linear_transform_apply(None, None, None, None, None, 0, _lib.MEM_HOST, None) == INVALID
    assert lib.fhe_ckks_rtk_gen(ctxs[0].handle, None, 16, 1, None, 0, None, None, _lib.MEM_HOST, None) == INVALID
