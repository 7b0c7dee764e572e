"""GPU tests of the hoisted CKKS rotations and the double-hoisted diagonal-matrix product (include/fhe_ring.h fhe_rns_automorphism_eval,
fhe_ckks_rotate_many, fhe_ckks_diag_matrix_prepare_hoisted / fhe_ckks_mul_mat_hoisted), bit for bit but for the decode-level test.

Two expected values per case, so that a disagreement tells which side moved: the model of tests/ckks_hoist_model.py over the C oracle
(two ciphertexts of the batch) and the composition from the library's public entries (learn-fhe_amd/ckks_hoist.py, the whole batch).
Operands are random limbs: exactness does not depend on what the polynomials mean."""
import ctypes as C
import math
import os
import random
import subprocess

import numpy as np
import pytest

import ckks_hoist_model as M
from ckks_hoist_model import rand_limbs

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 6
SENTINEL = 0x5a5a5a5a5a5a5a5a


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def code_of(f, *args, **kw):
    # (no pytest.raises: its ExceptionInfo would keep the contexts in `args` alive until a cyclic collection)
    from learn_fhe_amd import FheError
    try:
        f(*args, **kw)
    except FheError as err:
        return err.code
    raise AssertionError("accepted")


# ---- fhe_rns_automorphism_eval ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("log_n,batch", [(4, 2), (7, 1), (11, 1), (12, 1), (14, 1), (15, 1)])
def test_automorphism_eval_is_the_transform_of_the_automorphism(fhe, cref, torch_cuda, log_n, batch):
    """automorphism_eval(ntt_fwd(x)) == ntt_fwd(automorphism(x)) on qs and on qs ++ ps, at every transform route.  (The coefficient-domain
    automorphism takes polynomials over a context's qs: a second context whose qs are qs ++ ps serves the extended base.)"""
    n = 1 << log_n
    primes = cref.two_adic_primes(55, log_n + 1, 4)
    qs, ps = primes[:2], primes[2:3]
    rns, wide = fhe.RnsContext(qs, ps), fhe.RnsContext(qs + ps, primes[3:4])
    for extended, ctx, mods in ((False, rns, qs), (True, wide, qs + ps)):
        x = dev(torch_cuda, rand_limbs(60 + log_n, mods, n, batch))
        fx = ctx.ntt_(x.clone(), n)
        for t in (5, 25, 2 * n - 1):
            want = ctx.ntt_(ctx.automorphism(x, t, n), n)
            got = rns.automorphism_eval(fx, t, n, extended=extended)
            assert np.array_equal(host(got), host(want)), (extended, t)
    # a host-memory call, and an even t: refused, the output untouched
    hx = host(fx)
    assert np.array_equal(rns.automorphism_eval(hx.copy(), 5, n, extended=True), host(rns.automorphism_eval(fx, 5, n, extended=True)))
    out = dev(torch_cuda, np.full((batch, 3, n), SENTINEL, dtype=np.uint64))
    rc = fhe.lib().fhe_rns_automorphism_eval(rns.handle, 1, 6, C.c_void_p(fx.data_ptr()), C.c_void_p(out.data_ptr()), n, batch, 1, None)
    torch_cuda.cuda.synchronize()
    assert rc == UNSUPPORTED and (host(out) == SENTINEL).all()


# ---- fhe_ckks_rotate_many --------------------------------------------------------------------------------------------------------

class RotCase:
    def __init__(self, fhe, cref, torch, log_n, bits, big_l, big_k, batch, amounts, extreme=False):
        self.fhe, self.cref, self.torch = fhe, cref, torch
        self.n, self.batch, self.amounts = 1 << log_n, batch, list(amounts)
        primes = cref.two_adic_primes(bits, log_n + 1, big_l + big_k)
        self.qs, self.ps = primes[:big_l], primes[big_l:]
        self.rns = fhe.RnsContext(self.qs, self.ps)
        self.raw = {j: (rand_limbs(1000 + j, self.qs + self.ps, self.n), rand_limbs(2000 + j, self.qs + self.ps, self.n)) for j in self.amounts if j}
        self.keys = {j: fhe.CkksKey(self.rns, dev(torch, kb), dev(torch, ka), self.n) for j, (kb, ka) in self.raw.items()}
        if extreme:
            top = np.array(self.qs, dtype=np.uint64)[:, None] - np.uint64(1)
            self.cb = np.ascontiguousarray(np.broadcast_to(top, (batch, big_l, self.n)))
            self.ca = self.cb.copy()
        else:
            self.cb, self.ca = rand_limbs(41, self.qs, self.n, batch), rand_limbs(51, self.qs, self.n, batch)

    def run(self, on_host=False):
        keys = [self.keys.get(j) for j in self.amounts]
        if on_host:
            return self.fhe.CkksKey.rotate_many(self.rns, self.n, self.amounts, keys, self.cb.copy(), self.ca.copy())
        outs = self.fhe.CkksKey.rotate_many(self.rns, self.n, self.amounts, keys, dev(self.torch, self.cb), dev(self.torch, self.ca))
        return [(host(b), host(a)) for b, a in outs]

    def check(self, outs):
        raws = [self.raw.get(j) for j in self.amounts]
        comp = self.fhe.ckks_hoist.rotate_many_composed(self.rns, self.n, self.amounts, raws, dev(self.torch, self.cb), dev(self.torch, self.ca))
        comp_ok = all(np.array_equal(ob, host(eb)) and np.array_equal(oa, host(ea)) for (ob, oa), (eb, ea) in zip(outs, comp))
        O = M.Ops(self.cref)
        for c in range(min(self.batch, 2)):
            want = M.rotate_many(O, self.qs, self.ps, self.amounts, raws, self.cb[c], self.ca[c])
            for r, ((ob, oa), (wb, wa)) in enumerate(zip(outs, want)):
                assert np.array_equal(ob[c], wb) and np.array_equal(oa[c], wa), "ciphertext %d, rotation %d: != model (== composed: %s)" % (c, r, comp_ok)
        assert comp_ok, "== model but != the composed public entries"


ROT_SHAPES = [(4, 50, 3, 3, 2, [0, 1, 2, 5]), (4, 60, 2, 1, 1, [1, 3]), (12, 55, 3, 2, 1, [1, 3])]


@pytest.mark.parametrize("log_n,bits,big_l,big_k,batch,amounts", ROT_SHAPES, ids=lambda v: None if isinstance(v, list) else str(v))
@pytest.mark.parametrize("extreme", [False, True], ids=["random", "q-1"])
def test_rotate_many_vs_model_and_composed(fhe, cref, torch_cuda, log_n, bits, big_l, big_k, batch, amounts, extreme):
    c = RotCase(fhe, cref, torch_cuda, log_n, bits, big_l, big_k, batch, amounts, extreme)
    outs = c.run()
    c.check(outs)
    if 0 in amounts:  # amount 0 copies the input
        assert np.array_equal(outs[amounts.index(0)][0], c.cb) and np.array_equal(outs[amounts.index(0)][1], c.ca)


def test_rotate_many_equals_rotate_on_the_cleared_inputs(fhe, cref, torch_cuda):
    """On the inputs tests/test_ckks_hoist_cpu.py cleared with the reference alone, extending before sigma gives the reference's bits"""
    c = M.CLEARED
    n = 1 << c["log_n"]
    qs, ps, raw, cb, ca = M.cleared_inputs(cref.two_adic_primes(c["bits"], c["log_n"] + 1, c["L"] + c["K"]))
    rns = fhe.RnsContext(qs, ps)
    keys = [fhe.CkksKey(rns, dev(torch_cuda, raw[j][0]), dev(torch_cuda, raw[j][1]), n) for j in c["amounts"]]
    outs = fhe.CkksKey.rotate_many(rns, n, c["amounts"], keys, dev(torch_cuda, cb), dev(torch_cuda, ca))
    for (ob, oa), j, key in zip(outs, c["amounts"], keys):
        b, a = dev(torch_cuda, cb), dev(torch_cuda, ca)
        key.rotate_(pow(5, j, 2 * n), b, a)
        assert np.array_equal(host(ob), host(b)) and np.array_equal(host(oa), host(a)), j


def test_rotate_many_host_memory_and_side_stream(fhe, cref, torch_cuda):
    c = RotCase(fhe, cref, torch_cuda, 4, 50, 3, 3, 2, [0, 1, 2, 5])
    want = c.run()
    got = c.run(on_host=True)
    assert all(np.array_equal(gb, wb) and np.array_equal(ga, wa) for (gb, ga), (wb, wa) in zip(got, want))
    side = torch_cuda.cuda.Stream()
    with torch_cuda.cuda.stream(side):
        got = c.run()
    assert all(np.array_equal(gb, wb) and np.array_equal(ga, wa) for (gb, ga), (wb, wa) in zip(got, want))


def test_rotate_many_refusals_write_nothing(fhe, cref, torch_cuda):
    c = RotCase(fhe, cref, torch_cuda, 4, 50, 3, 3, 1, [1, 2])
    other = fhe.RnsContext(c.qs[:-1], c.ps)
    stranger = fhe.CkksKey(other, dev(torch_cuda, np.delete(c.raw[1][0], 2, axis=0)), dev(torch_cuda, np.delete(c.raw[1][1], 2, axis=0)), c.n)
    cb, ca = dev(torch_cuda, c.cb), dev(torch_cuda, c.ca)
    outs = [(dev(torch_cuda, np.full(c.cb.shape, SENTINEL, dtype=np.uint64)), dev(torch_cuda, np.full(c.cb.shape, SENTINEL, dtype=np.uint64))) for _ in range(2)]
    R = fhe.CkksKey.rotate_many
    assert code_of(R, c.rns, c.n, [1, 2], [c.keys[1], None], cb, ca, outs=outs) == INVALID      # a missing key
    assert code_of(R, c.rns, c.n, [1, 2], [c.keys[1], stranger], cb, ca, outs=outs) == INVALID  # a key of another context
    assert code_of(R, other, c.n, [1], [c.keys[1]], cb[:, :2].contiguous(), ca[:, :2].contiguous(), outs=outs[:1]) == INVALID  # a wrong context
    torch_cuda.cuda.synchronize()
    assert all((host(x) == SENTINEL).all() for pair in outs for x in pair)


# ---- fhe_ckks_mul_mat_hoisted ----------------------------------------------------------------------------------------------------

class Case:
    """Contexts, keys (one coefficient-domain key per non-zero index; the giant-step form is the same key without limb L-1), lifted
    diagonals over qs ++ ps and ciphertexts of one shape.  edge: the accumulator-bound form (see the test)."""

    def __init__(self, fhe, cref, torch, log_n, bits, big_l, big_k, batch, split, extreme=False, diags_on_host=False, edge=False):
        self.fhe, self.cref, self.torch = fhe, cref, torch
        self.n, self.L, self.batch, self.split = 1 << log_n, big_l, batch, {i: sorted(js) for i, js in split.items()}
        n = self.n
        primes = cref.two_adic_primes(bits, log_n + 1, big_l + big_k)
        self.qs, self.ps = primes[:big_l], primes[big_l:]
        qps = self.qs + self.ps
        self.hi, self.lo = fhe.RnsContext(self.qs, self.ps), fhe.RnsContext(self.qs[:-1], self.ps)
        self.giant = sorted(self.split)
        self.baby = sorted({j for js in self.split.values() for j in js})
        self.terms = [(i, j) for i in self.giant for j in self.split[i]]
        zero_key = np.zeros((big_l + big_k, n), dtype=np.uint64)
        self.raw = {}
        for idx in sorted(set(self.giant + self.baby) - {0}):
            self.raw[idx] = (zero_key, zero_key) if edge else (rand_limbs(1000 + idx, qps, n), rand_limbs(2000 + idx, qps, n))
        cut = lambda k: np.ascontiguousarray(np.delete(k, big_l - 1, axis=0))  # noqa: E731
        self.raw_lo = {i: (cut(self.raw[i][0]), cut(self.raw[i][1])) for i in self.giant if i}
        if edge:  # one all-zero key serves every index
            zk = fhe.CkksKey(self.hi, dev(torch, zero_key), dev(torch, zero_key), n)
            self.keys_hi = {j: zk for j in self.baby if j}
        else:
            self.keys_hi = {j: fhe.CkksKey(self.hi, dev(torch, self.raw[j][0]), dev(torch, self.raw[j][1]), n) for j in self.baby if j}
        self.keys_lo = {i: fhe.CkksKey(self.lo, dev(torch, self.raw_lo[i][0]), dev(torch, self.raw_lo[i][1]), n) for i in self.giant if i}
        top = np.array(qps, dtype=np.uint64)[:, None] - np.uint64(1)
        e0 = (np.arange(n) == 0).astype(np.uint64)[None, :]
        if edge:      # the constant polynomials m - 1: every evaluation is m - 1
            self.diags = np.ascontiguousarray(np.broadcast_to(top * e0, (len(self.terms), big_l + big_k, n)))
        elif extreme:  # every word m - 1
            self.diags = np.ascontiguousarray(np.broadcast_to(top, (len(self.terms), big_l + big_k, n)))
        else:
            self.diags = np.stack([rand_limbs(3000 + t, qps, n) for t in range(len(self.terms))])
        self.extreme, self.edge = extreme, edge
        self.mat = fhe.CkksDiagMatrixHoisted(self.hi, self.lo, n, self.split, self.diags if diags_on_host else dev(torch, self.diags), self.keys_hi,
                                             self.keys_lo)

    def ciphertexts(self, batch, seed=0):
        if self.edge:  # b the constant with P b = q - 1 (every evaluation of P b^ is q - 1, fixed by every sigma); a is met by zero keys only
            big_p = math.prod(self.ps)
            c = np.array([[(q - 1) * pow(big_p, -1, q) % q] + [0] * (self.n - 1) for q in self.qs], dtype=np.uint64)
            return np.ascontiguousarray(np.broadcast_to(c, (batch, self.L, self.n))), rand_limbs(50, self.qs, self.n, batch)
        if self.extreme:
            top = np.array(self.qs, dtype=np.uint64)[:, None] - np.uint64(1)
            c = np.ascontiguousarray(np.broadcast_to(top, (batch, self.L, self.n)))
            return c, c.copy()
        return rand_limbs(40 + seed, self.qs, self.n, batch), rand_limbs(50 + seed, self.qs, self.n, batch)

    def check(self, batch=None, seed=0, on_host=False):
        batch = self.batch if batch is None else batch
        cb, ca = self.ciphertexts(batch, seed)
        if on_host:
            ob, oa = self.mat.apply(cb.copy(), ca.copy())
        else:
            ob, oa = (host(x) for x in self.mat.apply(dev(self.torch, cb), dev(self.torch, ca)))
        assert ob.shape == oa.shape == (batch, self.L - 1, self.n)
        eb, ea = self.fhe.ckks_hoist.mul_mat_hoisted_composed(self.hi, self.lo, self.n, self.split, self.diags, self.raw, self.keys_lo, dev(self.torch, cb),
                                                              dev(self.torch, ca))
        comp_ok = np.array_equal(ob, host(eb)) and np.array_equal(oa, host(ea))
        O = M.Ops(self.cref)
        for c in range(min(batch, 2)):
            xb, xa = M.mul_mat_hoisted(O, self.qs, self.ps, self.split, self.diags, self.raw, self.raw_lo, cb[c], ca[c])
            assert np.array_equal(ob[c], xb) and np.array_equal(oa[c], xa), "ciphertext %d: != model (== composed: %s)" % (c, comp_ok)
        assert comp_ok, "== model but != the composed public entries"


FULL = lambda giant, baby: {i: list(baby) for i in giant}  # noqa: E731

SHAPES = [
    # log_n, bits, L, K, batch, split, extreme: the split shapes of tests/test_ckks_matmul_gpu.py
    (4, 50, 3, 3, 2, FULL([0, 3], [0, 1, 2]), False),
    (4, 60, 2, 1, 1, FULL([0], range(17)), True),
    (4, 61, 2, 1, 1, FULL([0], range(17)), True),
    (4, 62, 2, 1, 1, FULL([0], range(17)), True),               # the fold bound is 16 < 17 terms: the counting instantiation runs
    (7, 55, 3, 2, 2, {4: [1, 2], 8: [2]}, False),               # ragged: J differs per giant step, every step rotates
    (11, 55, 4, 4, 1, FULL([0, 2], [0, 1]), False),
    (12, 55, 3, 2, 1, FULL([0, 2], [0, 1]), False),
    (14, 60, 3, 1, 1, FULL([2], [0, 1]), False),
    (15, 60, 2, 2, 1, FULL([0, 2], [0, 1]), False),
]


@pytest.mark.parametrize("log_n,bits,big_l,big_k,batch,split,extreme", SHAPES, ids=lambda v: None if isinstance(v, (dict, bool)) else str(v))
def test_mul_mat_hoisted_vs_model_and_composed(fhe, cref, torch_cuda, log_n, bits, big_l, big_k, batch, split, extreme):
    Case(fhe, cref, torch_cuda, log_n, bits, big_l, big_k, batch, split, extreme).check()


@pytest.mark.parametrize("bits,terms", [(60, 257), (61, 65), (62, 17)])
def test_accumulator_at_its_fold_bound(fhe, cref, torch_cuda, bits, terms):
    """One term more than the fold bound F = 2^(128 - 2 bits) (csrc/ckks_hoist.hpp), every product (q - 1)^2 at every point of the b half:
    all rotation keys are zero, so u_j.b = sigma(P b^), b is the constant with P b = q - 1 and the diagonals are the constants m - 1:
    automorphisms fix them and their every evaluation is the constant.  With q just below 2^bits, F + 1 such products do not fit
    128 bits: an accumulator that folded later than F, or not at all, loses a carry here."""
    c = Case(fhe, cref, torch_cuda, 4, bits, 2, 1, 1, FULL([0], range(terms)), edge=True)
    q, widest = c.qs[0], max(c.qs + c.ps)
    assert q.bit_length() == widest.bit_length() == bits and terms - 1 == 1 << (128 - 2 * bits)
    assert (terms - 1) * (widest - 1) ** 2 < 1 << 128 <= terms * (q - 1) ** 2
    c.check()


def test_one_matrix_two_batches_and_host_diagonals(fhe, cref, torch_cuda):
    c = Case(fhe, cref, torch_cuda, 4, 50, 3, 3, 1, FULL([0, 3], [0, 1, 2]))
    c.check(batch=1, seed=1)
    c.check(batch=3, seed=2)
    like = dev(torch_cuda, np.zeros((0, 3, 16), dtype=np.uint64))
    ob, oa = c.mat.apply(like, like)  # batch == 0: FHE_OK, nothing written
    assert ob.shape == (0, 2, 16)
    Case(fhe, cref, torch_cuda, 4, 50, 3, 3, 2, FULL([0, 3], [0, 1, 2]), diags_on_host=True).check(on_host=True)


def test_mul_mat_hoisted_refusals_write_nothing(fhe, cref, torch_cuda):
    n = 16
    primes = cref.two_adic_primes(50, 5, 7)
    qs, ps = primes[:3], primes[3:6]
    hi, lo = fhe.RnsContext(qs, ps), fhe.RnsContext(qs[:-1], ps)
    mk = lambda rns, seed: fhe.CkksKey(rns, dev(torch_cuda, rand_limbs(seed, rns.qs + rns.ps, n)),  # noqa: E731
                                       dev(torch_cuda, rand_limbs(seed + 1, rns.qs + rns.ps, n)), n)
    k_hi, k_lo = mk(hi, 1), mk(lo, 3)
    diags = dev(torch_cuda, rand_limbs(5, qs + ps, n, 2))  # two terms over qs ++ ps
    split = {0: [1], 3: [1]}
    H = fhe.CkksDiagMatrixHoisted
    assert H(hi, lo, n, split, diags, {1: k_hi}, {3: k_lo}) is not None  # the accepted form of what follows
    assert code_of(H, hi, lo, n, split, diags, {}, {3: k_lo}) == INVALID         # a missing key
    assert code_of(H, hi, lo, n, split, diags, {1: k_hi}, {}) == INVALID
    assert code_of(H, hi, lo, n, split, diags, {1: k_lo}, {3: k_lo}) == INVALID  # a key of the wrong context
    assert code_of(H, hi, lo, n, split, diags, {1: k_hi}, {3: k_hi}) == INVALID
    assert code_of(H, hi, fhe.RnsContext([qs[0], qs[2]], ps), n, split, diags, {1: k_hi}, {3: k_lo}) == INVALID  # rns_lo not the prefix
    assert code_of(H, hi, lo, n, split, dev(torch_cuda, rand_limbs(5, qs, n, 2)), {1: k_hi}, {3: k_lo}) == INVALID  # diagonals on L limbs
    # no term, and a NULL matrix: the C entries directly; neither handle nor outputs are written
    from learn_fhe_amd import _lib
    h = C.c_void_p()
    one = (C.c_uint32 * 1)(0)
    nokey = (C.c_void_p * 1)(None)
    rc = _lib.lib().fhe_ckks_diag_matrix_prepare_hoisted(hi.handle, lo.handle, n, one, 1, one, 1, bytes([0]), C.c_void_p(diags.data_ptr()), nokey, nokey,
                                                         _lib.MEM_DEVICE, C.byref(h))
    assert rc == INVALID and not h.value
    bufs = [dev(torch_cuda, np.full((1, 3, n), SENTINEL, dtype=np.uint64)) for _ in range(4)]
    p = [C.c_void_p(b.data_ptr()) for b in bufs]
    assert _lib.lib().fhe_ckks_mul_mat_hoisted(None, p[0], p[1], p[2], p[3], 1, _lib.MEM_DEVICE, None) == INVALID
    torch_cuda.cuda.synchronize()
    assert all((host(b) == SENTINEL).all() for b in bufs)


# ---- decode level ------------------------------------------------------------------------------------------------------------------

def test_hoisted_product_decodes_like_the_reference_product(fhe, cref, torch_cuda):
    """The one check that is not bit for bit: n = 2^7, L = 3, K = 2, a three-diagonal matrix with genuine keys and noise, built as
    test_three_diagonal_matrix_decodes_to_the_dense_product builds its own.  Both fhe_ckks_mul_mat (the reference's bits: the yardstick)
    and fhe_ckks_mul_mat_hoisted are decoded and compared with the dense product computed here.  The hoisted route may exceed the
    yardstick's maximum slot error by at most a factor 4: the two differ only in where the roundings by P and q_last fall.
    The base: three 40-bit qs and two 61-bit ps, so that P > Q and the key switch divides its key noise away (with K < L primes of one
    size it would multiply it by Q / P); scale = q_last.  Measured on gfx950: fhe_ckks_mul_mat 2^-29.3, fhe_ckks_mul_mat_hoisted 2^-29.3."""
    from oracle import pyref as P
    torch = torch_cuda
    log_n, big_l, big_k = 7, 3, 2
    n, slots = 1 << log_n, 1 << (log_n - 1)
    qs, ps = cref.two_adic_primes(40, log_n + 1, big_l), cref.two_adic_primes(61, log_n + 1, big_k)
    ql, big_p, scale = qs[:-1], math.prod(ps), qs[-1]
    assert big_p > math.prod(qs)
    rnd = random.Random(2024)
    nrng = np.random.Generator(np.random.PCG64(7))
    w = np.exp(2j * np.pi * np.array([pow(5, k, 2 * n) for k in range(slots)]) / (2 * n))
    V = w[:, None] ** np.arange(slots)[None, :]  # V V^H = slots I

    def encode(m):  # ckks.rs:186-198 -> [n] integers
        z = V.conj().T @ m / slots
        return [int(round(float(x) * scale)) for x in list(z.real) + list(z.imag)]

    def decode(coeffs, sc):  # ckks.rs:200-213
        return V @ np.array([coeffs[c] / sc + 1j * (coeffs[slots + c] / sc) for c in range(slots)])

    lift = lambda mods, v: [[x % q for x in v] for q in mods]  # noqa: E731
    U = lambda rows: np.array(rows, dtype=np.uint64)  # noqa: E731
    sk = [rnd.choice([-1, 0, 0, 1]) for _ in range(n)]

    def encrypt(mods, pt_big):  # ckks.rs:215-225: b = -(a s) + e + pt
        a = [[rnd.randrange(q) for _ in range(n)] for q in mods]
        e = [rnd.randint(-6, 6) for _ in range(n)]
        a_s = P.rns_mul(mods, a, lift(mods, sk))
        return [[(-x + ee + p) % q for x, ee, p in zip(row, e, pt_big)] for q, row in zip(mods, a_s)], a

    def decrypt(mods, b, a):
        a_s = P.rns_mul(mods, a, lift(mods, sk))
        big_q = math.prod(mods)
        out = []
        for c in range(n):
            v = sum(((rb[c] + ra[c]) % q) * (big_q // q) * pow(big_q // q, -1, q) for q, rb, ra in zip(mods, b, a_s)) % big_q
            out.append(v - big_q if v > big_q // 2 else v)
        return out

    def rot_key(rns, mods_q, idx):  # ckks.rs:154-161, 174-184
        kb, ka = encrypt(mods_q + ps, [x * big_p for x in P.sk_automorphism(sk, pow(5, idx, 2 * n))])
        return fhe.CkksKey(rns, dev(torch, U(kb)), dev(torch, U(ka)), n)

    m_shift = 4
    diag = {d: nrng.uniform(0, 1, slots) * np.exp(2j * np.pi * nrng.uniform(0, 1, slots)) for d in (0, m_shift, slots - m_shift)}
    msg = nrng.uniform(0, 1, slots) + 1j * nrng.uniform(0, 1, slots)
    want = sum(diag[d] * np.roll(msg, -d) for d in diag)
    k, split = fhe.bsgs_split(diag.keys())
    hi, lo = fhe.RnsContext(qs, ps), fhe.RnsContext(ql, ps)
    baby = sorted({j for js in split.values() for j in js})
    keys_hi = {j: rot_key(hi, qs, j) for j in baby if j}
    keys_lo = {i: rot_key(lo, ql, i) for i in split if i}
    terms = [(i, j) for i in sorted(split) for j in sorted(split[i])]
    pts = U([lift(qs, encode(np.roll(diag[i + j], i))) for i, j in terms])
    ctb, cta = encrypt(qs, encode(msg))
    cb, ca = dev(torch, U(ctb)[None]), dev(torch, U(cta)[None])

    def error(ob, oa):
        rows = lambda t: [[int(v) for v in r] for r in host(t)[0]]  # noqa: E731
        got = decode(decrypt(ql, rows(ob), rows(oa)), scale * scale / qs[-1])
        return max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag)))

    e_ref = error(*fhe.CkksDiagMatrix(hi, lo, n, split, dev(torch, pts), keys_hi, keys_lo).apply(cb, ca))
    lifted = fhe.ckks_hoist.extend_plain(qs, ps, pts)
    e_hoisted = error(*fhe.CkksDiagMatrixHoisted(hi, lo, n, split, dev(torch, lifted), keys_hi, keys_lo).apply(cb, ca))
    print("fhe_ckks_mul_mat: max slot error 2^%.1f; fhe_ckks_mul_mat_hoisted: 2^%.1f" % (math.log2(e_ref), math.log2(e_hoisted)))
    assert e_ref < 2.0 ** -16  # the base works: a 40-bit scale leaves far less than a wrong or missing term (entries of modulus up to 1)
    assert e_hoisted <= 4 * e_ref


def test_c_program_ckks_hoist(tmp_path, fhe):
    """examples/ckks_hoist_demo.c: a three-diagonal matrix through fhe_ckks_mul_mat_hoisted from plain C against include/fhe_ring.h alone"""
    from conftest import ROOT
    lib_dir = os.path.dirname(fhe.lib_path())
    exe = tmp_path / "ckks_hoist_demo"
    cmd = ["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "ckks_hoist_demo.c"), "-o", str(exe),
           "-L", lib_dir, "-lfhe_ring", "-Wl,--allow-shlib-undefined", "-Wl,-rpath," + lib_dir, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ckks_hoist_demo ok" in r.stdout, r.stdout + r.stderr
