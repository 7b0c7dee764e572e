"""GPU tests of the CKKS diagonal-matrix product (scheme/ckks/src/bootstrapping.rs:90-108 `Bootstrapping::mul_mat`;
include/fhe_ring.h fhe_ckks_diag_matrix_prepare / fhe_ckks_mul_mat), bit-exact.

Two expected values per case, so that a disagreement tells which side moved: one composed from the C oracle (`cref.ckks_rotate`,
`cref.ckks_mul_plain`, limb-wise modular add) in the reference's order, one from the library's own entries (`CkksKey.rotate_`,
`RnsContext.mul_plain`, `RnsContext.add_`).  Operands are random limbs: exactness does not depend on what the polynomials mean.
One decode-level test at the end runs a three-diagonal matrix through the scheme and compares with the dense product."""
import math
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def rand_limbs(seed, mods, n, batch=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = [rng.integers(0, m, size=(n if batch is None else (batch, n)), dtype=np.uint64) for m in mods]
    return np.stack(rows, axis=0 if batch is None else 1)  # [limb][n] or [batch][limb][n]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def add_limbs(mods, a, b):
    qv = np.array(mods, dtype=np.uint64)[:, None]
    s = a + b  # moduli below 2^62: no wrap
    return np.where(s >= qv, s - qv, s)


class Case:
    """Contexts, keys (one coefficient-domain key per non-zero index; the giant-step form is the same key without limb L-1),
    diagonals and ciphertexts of one shape."""

    def __init__(self, fhe, cref, torch, log_n, bits, big_l, big_k, batch, split, extreme=False, diags_on_host=False, edge=False):
        self.fhe, self.cref, self.torch = fhe, cref, torch
        self.n, self.L, self.batch, self.split = 1 << log_n, big_l, batch, {i: sorted(js) for i, js in split.items()}
        n = self.n
        primes = cref.two_adic_primes(bits, log_n + 1, big_l + big_k)
        self.qs, self.ps = primes[:big_l], primes[big_l:]
        self.hi, self.lo = fhe.RnsContext(self.qs, self.ps), fhe.RnsContext(self.qs[:-1], self.ps)
        self.giant = sorted(self.split)
        self.baby = sorted({j for js in self.split.values() for j in js})
        self.terms = [(i, j) for i in self.giant for j in self.split[i]]
        self.raw = {}
        zero_key = np.zeros((big_l + big_k, n), dtype=np.uint64)
        for idx in sorted(set(self.giant + self.baby) - {0}):
            self.raw[idx] = (zero_key, zero_key) if edge else (rand_limbs(1000 + idx, self.qs + self.ps, n), rand_limbs(2000 + idx, self.qs + self.ps, n))
        cut = lambda k: np.ascontiguousarray(np.delete(k, big_l - 1, axis=0))  # noqa: E731
        self.raw_lo = {i: (cut(self.raw[i][0]), cut(self.raw[i][1])) for i in self.giant if i}
        if edge:  # one all-zero key serves every index: the key switch then returns (the rotated b, 0)
            zk = fhe.CkksKey(self.hi, dev(torch, zero_key), dev(torch, zero_key), n)
            self.keys_hi = {j: zk for j in self.baby if j}
        else:
            self.keys_hi = {j: fhe.CkksKey(self.hi, dev(torch, self.raw[j][0]), dev(torch, self.raw[j][1]), n) for j in self.baby if j}
        self.keys_lo = {i: fhe.CkksKey(self.lo, dev(torch, self.raw_lo[i][0]), dev(torch, self.raw_lo[i][1]), n) for i in self.giant if i}
        top = np.array(self.qs, dtype=np.uint64)[:, None] - np.uint64(1)
        if edge:  # constant polynomials q - 1: fixed by every automorphism, and every evaluation is q - 1
            top = top * (np.arange(n) == 0).astype(np.uint64)[None, :]
        if extreme or edge:  # every plaintext and ciphertext word q - 1 (edge: coefficient 0 only)
            self.diags = np.ascontiguousarray(np.broadcast_to(top, (len(self.terms), big_l, n)))
        else:
            self.diags = np.stack([rand_limbs(3000 + t, self.qs, n) for t in range(len(self.terms))])
        self.extreme, self.top = extreme or edge, top
        self.mat = fhe.CkksDiagMatrix(self.hi, self.lo, n, self.split, self.diags if diags_on_host else dev(torch, self.diags), self.keys_hi,
                                      self.keys_lo)

    def ciphertexts(self, batch, seed=0):
        if self.extreme:
            c = np.ascontiguousarray(np.broadcast_to(self.top, (batch, self.L, self.n)))
            return c, c.copy()
        return rand_limbs(40 + seed, self.qs, self.n, batch), rand_limbs(50 + seed, self.qs, self.n, batch)

    def expect_oracle(self, cb, ca):
        """bootstrapping.rs:95-107 for one ciphertext ([L][n] b, a) from the C oracle."""
        R, n, qs, ps, ql = self.cref, self.n, self.qs, self.ps, self.qs[:-1]
        rot = {j: (cb, ca) if j == 0 else R.ckks_rotate(qs, ps, self.raw[j][0], self.raw[j][1], pow(5, j, 2 * n), cb, ca) for j in self.baby}
        total, t = None, 0
        for i in self.giant:
            s = None
            for j in self.split[i]:
                p = R.ckks_mul_plain(qs, self.diags[t], rot[j][0], rot[j][1])
                t += 1
                s = p if s is None else (add_limbs(ql, s[0], p[0]), add_limbs(ql, s[1], p[1]))
            if i:
                s = R.ckks_rotate(ql, ps, self.raw_lo[i][0], self.raw_lo[i][1], pow(5, i, 2 * n), s[0], s[1])
            total = s if total is None else (add_limbs(ql, total[0], s[0]), add_limbs(ql, total[1], s[1]))
        return total

    def expect_entries(self, cb, ca):
        """The same composition from the library's existing entries, for the whole batch ([batch][L][n] device tensors)."""
        n, rot = self.n, {}
        for j in self.baby:
            b, a = cb.clone(), ca.clone()
            if j:
                self.keys_hi[j].rotate_(pow(5, j, 2 * n), b, a)
            rot[j] = (b, a)
        total, t = None, 0
        for i in self.giant:
            s = None
            for j in self.split[i]:
                p = self.hi.mul_plain(dev(self.torch, self.diags[t][None]), rot[j][0], rot[j][1], n)
                t += 1
                s = p if s is None else (self.lo.add_(s[0], p[0], n), self.lo.add_(s[1], p[1], n))
            if i:
                self.keys_lo[i].rotate_(pow(5, i, 2 * n), s[0], s[1])
            total = s if total is None else (self.lo.add_(total[0], s[0], n), self.lo.add_(total[1], s[1], n))
        return total

    def check(self, batch=None, seed=0, on_host=False):
        batch = self.batch if batch is None else batch
        cb, ca = self.ciphertexts(batch, seed)
        if on_host:
            ob, oa = self.mat.apply(cb.copy(), ca.copy())
        else:
            ob, oa = (host(x) for x in self.mat.apply(dev(self.torch, cb), dev(self.torch, ca)))
        assert ob.shape == oa.shape == (batch, self.L - 1, self.n)
        eb, ea = self.expect_entries(dev(self.torch, cb), dev(self.torch, ca))
        entries_ok = np.array_equal(ob, host(eb)) and np.array_equal(oa, host(ea))
        for c in range(batch):
            xb, xa = self.expect_oracle(cb[c], ca[c])
            oracle_ok = np.array_equal(ob[c], xb) and np.array_equal(oa[c], xa)
            assert oracle_ok, "ciphertext %d: != oracle (== the composed entries: %s)" % (c, entries_ok)
        assert entries_ok, "== oracle but != the composed existing entries"


FULL = lambda giant, baby: {i: list(baby) for i in giant}  # noqa: E731

SHAPES = [
    # log_n, bits, L, K, batch, split, extreme
    (4, 50, 3, 3, 2, FULL([0, 3], [0, 1, 2]), False),           # the basic case, j = 0 and i = 0 present
    # every coefficient-domain word q - 1, 17 terms, rns_lo a single limb.  (What the kernels read is pseudo-random by then -- transforms,
    # and key switches with random keys: these rows walk the 17-term paths, test_accumulator_at_its_fold_bound reaches the bounds.)
    (4, 60, 2, 1, 1, FULL([0], range(17)), True),
    (4, 61, 2, 1, 1, FULL([0], range(17)), True),               # 61-bit moduli (fold bound 64)
    (4, 62, 2, 1, 1, FULL([0], range(17)), True),               # 62-bit moduli: the fold bound is 16 < 17 terms, the fold path runs
    (7, 55, 3, 2, 2, {4: [1, 2], 8: [2]}, False),               # ragged: J differs per giant step, every step rotates
    (11, 55, 4, 4, 2, FULL([0, 2], [0, 1]), False),
    (12, 55, 3, 2, 1, FULL([0, 2], [0, 1]), False),             # the 2^12 route
    (14, 60, 3, 1, 1, FULL([2], [0, 1]), False),                # the 2^14 kernels
    (15, 60, 2, 2, 1, FULL([0, 2], [0, 1]), False),             # the edge key switch
]


@pytest.mark.parametrize("log_n,bits,big_l,big_k,batch,split,extreme", SHAPES, ids=lambda v: None if isinstance(v, (dict, bool)) else str(v))
def test_mul_mat_vs_oracle_and_entries(fhe, cref, torch_cuda, log_n, bits, big_l, big_k, batch, split, extreme):
    Case(fhe, cref, torch_cuda, log_n, bits, big_l, big_k, batch, split, extreme).check()


@pytest.mark.parametrize("bits,terms", [(60, 257), (61, 65), (62, 17)])
def test_accumulator_at_its_fold_bound(fhe, cref, torch_cuda, bits, terms):
    """One term more than the fold bound F = 2^(128 - 2 bits) (csrc/ckks_matmul_kernels.hpp), every product (q - 1)^2 in every slot of the
    b half: all rotation keys are zero, so a rotation is the automorphism of b alone, and ciphertext and diagonals are the constant
    polynomial q - 1, which automorphisms leave fixed and whose every evaluation is q - 1.  With q just below 2^bits, F + 1 such products
    do not fit 128 bits ((F + 1)(q - 1)^2 > 2^128): an accumulator that folded later than F, or not at all, loses a carry here; the
    integer sum of the last limb's lifts passes 2^64 as well."""
    c = Case(fhe, cref, torch_cuda, 4, bits, 2, 1, 1, FULL([0], range(terms)), edge=True)
    q = c.qs[0]
    assert q.bit_length() == bits and (terms - 1) * (q - 1) ** 2 < 1 << 128 <= terms * (q - 1) ** 2
    c.check()


def test_single_term_equals_mul_plain(fhe, cref, torch_cuda):
    """(i, j) = (0, 0) alone is `mul_constant`: the bits of fhe_ckks_mul_plain"""
    c = Case(fhe, cref, torch_cuda, 4, 50, 3, 3, 2, {0: [0]})
    cb, ca = c.ciphertexts(2)
    ob, oa = c.mat.apply(dev(torch_cuda, cb), dev(torch_cuda, ca))
    pb, pa = c.hi.mul_plain(dev(torch_cuda, c.diags[0][None]), dev(torch_cuda, cb), dev(torch_cuda, ca), c.n)
    assert np.array_equal(host(ob), host(pb)) and np.array_equal(host(oa), host(pa))
    c.check()


def test_host_memory_operands(fhe, cref, torch_cuda):
    Case(fhe, cref, torch_cuda, 4, 50, 3, 3, 2, FULL([0, 3], [0, 1, 2]), diags_on_host=True).check(on_host=True)


def test_two_batches_through_one_matrix(fhe, cref, torch_cuda):
    c = Case(fhe, cref, torch_cuda, 4, 50, 3, 3, 1, FULL([0, 3], [0, 1, 2]))
    c.check(batch=1, seed=1)
    c.check(batch=3, seed=2)
    like = dev(torch_cuda, np.zeros((0, 3, 16), dtype=np.uint64))
    ob, oa = c.mat.apply(like, like)  # batch == 0: FHE_OK, nothing written
    assert ob.shape == (0, 2, 16)


def test_refusals(fhe, cref, torch_cuda):
    """Status codes of fhe_ckks_diag_matrix_prepare; none of them reaches a kernel."""
    n, big_l = 16, 3
    primes = cref.two_adic_primes(50, 5, 7)
    qs, ps = primes[:3], primes[3:6]
    hi, lo = fhe.RnsContext(qs, ps), fhe.RnsContext(qs[:-1], ps)
    mk = lambda rns, seed: fhe.CkksKey(rns, dev(torch_cuda, rand_limbs(seed, rns.qs + rns.ps, n)),  # noqa: E731
                                       dev(torch_cuda, rand_limbs(seed + 1, rns.qs + rns.ps, n)), n)
    k_hi, k_lo = mk(hi, 1), mk(lo, 3)
    diags = dev(torch_cuda, rand_limbs(5, qs, n, 2))  # two terms
    split = {0: [1], 3: [1]}

    def refused(*args):
        # (no pytest.raises here: its ExceptionInfo and this frame would keep each other, and with them the contexts and keys in
        # `args`, alive until a cyclic collection that finalises them in no particular order)
        try:
            fhe.CkksDiagMatrix(*args)
        except fhe.FheError as err:
            return err.code
        raise AssertionError("accepted")

    INVALID = 1
    assert fhe.CkksDiagMatrix(hi, lo, n, split, diags, {1: k_hi}, {3: k_lo}) is not None  # the accepted form of what follows
    assert refused(hi, fhe.RnsContext([qs[0], qs[2]], ps), n, split, diags, {1: k_hi}, {3: k_lo}) == INVALID  # rns_lo not the prefix
    assert refused(hi, fhe.RnsContext(qs[:-1], [ps[0], ps[1], primes[6]]), n, split, diags, {1: k_hi}, {3: k_lo}) == INVALID  # other ps
    assert refused(hi, lo, n, split, diags, {1: k_hi}, {3: k_hi}) == INVALID  # a giant key prepared on rns_hi
    assert refused(hi, lo, n, split, diags, {1: k_lo}, {3: k_lo}) == INVALID  # a baby key prepared on rns_lo
    assert refused(hi, lo, n, split, diags, {}, {3: k_lo}) == INVALID         # a missing key for a non-zero index
    assert refused(hi, lo, n, split, diags, {1: k_hi}, {}) == INVALID
    # no term present: the binding derives `present` from the split, so this one goes to the C entry directly
    import ctypes as C
    from learn_fhe_amd import _lib
    h = C.c_void_p()
    one = (C.c_uint32 * 1)(0)
    nokey = (C.c_void_p * 1)(None)
    rc = _lib.lib().fhe_ckks_diag_matrix_prepare(hi.handle, lo.handle, n, one, 1, one, 1, bytes([0]), C.c_void_p(diags.data_ptr()), nokey, nokey,
                                                 _lib.MEM_DEVICE, C.byref(h))
    assert rc == INVALID and not h.value
    # L = 1: every term's rescale would leave no limb
    one_limb = fhe.RnsContext(qs[:1], ps)
    assert refused(one_limb, one_limb, n, {0: [0]}, dev(torch_cuda, rand_limbs(6, qs[:1], n, 1)), {}, {}) == INVALID


def test_three_diagonal_matrix_decodes_to_the_dense_product(fhe, torch_cuda):
    """Decode level, as the reference tests its linear transforms (bootstrapping.rs:121-141): its parameters (log_qi = 55, L = 8) at
    log_n = 5, a matrix with the diagonals {0, m, l - m} of `sfft_fmats` (sfft.rs:75-94) and entries of modulus <= 1, slots in [0, 1);
    `decode(decrypt(mul_mat(ct)))` against the dense product (matrix.rs:86-92) within the reference's bound for this operation,
    2^-30 absolute per component (`assert_eq_complex!(.., 30)`).  Encode and decode are complex128 evaluations at the 5^k-ordered
    roots.  The same body runs through the composed existing entries first: they are unchanged by the fused entry, so that run says
    whether this f64 encoder meets the bound by itself."""
    from oracle import pyref as P
    torch = torch_cuda
    log_n, bits, big_l = 5, 55, 8
    n, slots = 1 << log_n, 1 << (log_n - 1)
    qs, ps = P.ckks_primes(log_n, bits, big_l)
    ql, qps, big_p, scale = qs[:-1], qs + ps, math.prod(ps), qs[-1]
    rnd = random.Random(2024)
    nrng = np.random.Generator(np.random.PCG64(7))
    # slot k is the plaintext at w_k = zeta^(5^k), zeta = exp(2 pi i / 2n); p(X) = sum_c z_c X^c with X^slots = i
    w = np.exp(2j * np.pi * np.array([pow(5, k, 2 * n) for k in range(slots)]) / (2 * n))
    V = w[:, None] ** np.arange(slots)[None, :]  # V V^H = slots I

    def encode(m):  # ckks.rs:186-198 -> [n] integers
        z = V.conj().T @ m / slots
        return [int(round(float(x) * scale)) for x in list(z.real) + list(z.imag)]

    def decode(coeffs, sc):  # ckks.rs:200-213
        z = np.array([coeffs[c] / sc + 1j * (coeffs[slots + c] / sc) for c in range(slots)])
        return V @ z

    lift = lambda mods, v: [[x % q for x in v] for q in mods]  # noqa: E731
    U = lambda rows: np.array(rows, dtype=np.uint64)  # noqa: E731
    sk = [rnd.choice([-1, 0, 0, 1]) for _ in range(n)]  # zo(0.5), ckks.rs:139-141

    def encrypt(mods, pt_big):  # ckks.rs:215-225: b = -(a s) + e + pt
        a = [[rnd.randrange(q) for _ in range(n)] for q in mods]
        e = [rnd.randint(-6, 6) for _ in range(n)]
        a_s = P.rns_mul(mods, a, lift(mods, sk))
        return [[(-x + ee + p) % q for x, ee, p in zip(row, e, pt_big)] for q, row in zip(mods, a_s)], a

    def decrypt(mods, b, a):  # ckks.rs:240-248, then the centred integer by CRT
        a_s = P.rns_mul(mods, a, lift(mods, sk))
        big_q = math.prod(mods)
        out = []
        for c in range(n):
            v = sum(((rb[c] + ra[c]) % q) * (big_q // q) * pow(big_q // q, -1, q) for q, rb, ra in zip(mods, b, a_s)) % big_q
            out.append(v - big_q if v > big_q // 2 else v)
        return out

    def rot_key(rns, mods_q, idx):  # ckks.rs:154-161, 174-184: ksk_gen(sk, sk(X^(5^idx))) over mods_q ++ ps
        sk_t = P.sk_automorphism(sk, pow(5, idx, 2 * n))
        kb, ka = encrypt(mods_q + ps, [x * big_p for x in sk_t])
        return fhe.CkksKey(rns, dev(torch, U(kb)), dev(torch, U(ka)), n)

    m_shift = 4
    diag = {d: nrng.uniform(0, 1, slots) * np.exp(2j * np.pi * nrng.uniform(0, 1, slots)) for d in (0, m_shift, slots - m_shift)}
    msg = nrng.uniform(0, 1, slots) + 1j * nrng.uniform(0, 1, slots)
    want = sum(diag[d] * np.roll(msg, -d) for d in diag)  # dense[i][(d + i) % slots] = diag_d[i]
    k, split = fhe.bsgs_split(diag.keys())
    hi, lo = fhe.RnsContext(qs, ps), fhe.RnsContext(ql, ps)
    baby = sorted({j for js in split.values() for j in js})
    keys_hi = {j: rot_key(hi, qs, j) for j in baby if j}
    keys_lo = {i: rot_key(lo, ql, i) for i in split if i}
    # diag_rot(i, j) = diag(i + j).rot_iter(-i) (bootstrapping.rs:101), encoded
    terms = [(i, j) for i in sorted(split) for j in sorted(split[i])]
    pts = U([lift(qs, encode(np.roll(diag[i + j], i))) for i, j in terms])
    ctb, cta = encrypt(qs, encode(msg))
    cb, ca = dev(torch, U(ctb)[None]), dev(torch, U(cta)[None])
    assert np.max(np.abs(decode(decrypt(qs, ctb, cta), scale) - msg)) < 2.0 ** -40

    def composed():
        total, t = None, 0
        for i in sorted(split):
            s = None
            for j in sorted(split[i]):
                b, a = cb.clone(), ca.clone()
                if j:
                    keys_hi[j].rotate_(pow(5, j, 2 * n), b, a)
                p = hi.mul_plain(dev(torch, pts[t][None]), b, a, n)
                t += 1
                s = p if s is None else (lo.add_(s[0], p[0], n), lo.add_(s[1], p[1], n))
            if i:
                keys_lo[i].rotate_(pow(5, i, 2 * n), s[0], s[1])
            total = s if total is None else (lo.add_(total[0], s[0], n), lo.add_(total[1], s[1], n))
        return total

    def error(ob, oa):
        rows = lambda t: [[int(v) for v in r] for r in host(t)[0]]  # noqa: E731
        got = decode(decrypt(ql, rows(ob), rows(oa)), scale * scale / qs[-1])
        return max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag)))

    e_composed = error(*composed())
    print("composed entries: max error 2^%.1f" % math.log2(e_composed))
    assert e_composed < 2.0 ** -30
    mat = fhe.CkksDiagMatrix(hi, lo, n, split, dev(torch, pts), keys_hi, keys_lo)
    ob, oa = mat.apply(cb, ca)
    e_fused = error(ob, oa)
    print("fused entry: max error 2^%.1f" % math.log2(e_fused))
    assert e_fused < 2.0 ** -30
    eb, ea = composed()
    assert np.array_equal(host(ob), host(eb)) and np.array_equal(host(oa), host(ea))
