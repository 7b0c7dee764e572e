"""The inverse wave-local transforms (csrc/ntt14w.hpp) leave every product unfolded, take their differences by offsets m q and fold a
sum only where a compile-time schedule (csrc/arith.hpp, DsGsLazy) finds that it could not enter the next butterfly.  Bit-exact
against the oracle (oracle/cref.py) where a bound that is too optimistic would show: N = 2^12 .. 2^15 (every R0) and 2^16 (the
sub-transform form), three polynomials, on the moduli tests/test_lazy_products_gpu.py picks
  * the 2^60 - 98303 prime of the headline workload (N <= 2^14: it has no larger root of unity),
  * of the first 16 primes of two_adic_primes(60, .) the one with the largest c,
  * the 60-bit prime with the largest c the pseudo-Mersenne path admits at all (c <= 2^27),
  * the first 54-bit and 55-bit prime of the family and, where the ring size has one, the one with the largest admitted c,
with the patterns applied DIRECTLY as the inverse's input (the evaluation domain is where its bounds bite): all zero, all q - 1,
alternating 0 / q - 1 at stride 1, in blocks of 8 (the pass-3 blocks) and in blocks of 2^11 (the waves), a single q - 1 at index 0
and at index N - 1, and seeded random values.  The ring product runs the same patterns as either operand (its inverse half takes the
products of the pointwise multiplication, not canonical values), and one CKKS key switch at N = 2^15 with every ciphertext limb at
q_i - 1 runs the sub-transform inverse that multiplies on its load."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q_CFG2 = 1152921504606748673  # 2^60 - 98303
BATCH = 3


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


def is_prime(n):
    """deterministic Miller-Rabin below 2^64"""
    if n < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in small:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in small:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def largest_admitted_c_prime(bits, k):
    """the prime 2^bits - c = 1 (mod 2^k) with the largest c <= 2^(bits - 33), the pseudo-Mersenne eligibility bound; None if there is none"""
    j = (1 << (bits - 33)) >> k
    while j > 0:
        q = (1 << bits) - (j << k) + 1
        if is_prime(q):
            return q
        j -= 1
    return None


def moduli(cref, log_n):
    k = max(16, log_n + 1)
    first16 = cref.two_adic_primes(60, k, 16)
    out = [max(first16, key=lambda q: (1 << 60) - q), largest_admitted_c_prime(60, log_n + 1)]
    if log_n <= 14:
        out.insert(0, Q_CFG2)
    for q in out:
        assert q.bit_length() == 60 and (1 << 60) - q <= 1 << 27  # on the two-operand (lazy) path
    for bits in (54, 55):
        out.append(cref.two_adic_primes(bits, log_n + 1, 1)[0])
        lazy = largest_admitted_c_prime(bits, log_n + 1)
        if lazy is not None and lazy != out[-1]:
            out.append(lazy)
    return out


def blocks(n, size, top):
    """0 / top alternating in blocks of `size`, BATCH polynomials"""
    one = np.where((np.arange(n) // size) % 2 == 1, top, np.uint64(0)).astype(np.uint64)
    return np.tile(one, BATCH)


def inputs(q, n, seed):
    """(name, BATCH polynomials)"""
    top = np.uint64(q - 1)
    zero = np.zeros(n * BATCH, dtype=np.uint64)
    first = zero.copy(); first[0::n] = top
    last = zero.copy(); last[n - 1::n] = top
    rng = np.random.Generator(np.random.PCG64(seed))
    return (("zero", zero), ("all q-1", np.full(n * BATCH, top, dtype=np.uint64)), ("alternating", blocks(n, 1, top)),
            ("blocks of 8", blocks(n, 8, top)), ("blocks of 2^11", blocks(n, 1 << 11, top)), ("q-1 at 0", first), ("q-1 at N-1", last),
            ("random", rng.integers(0, q, size=n * BATCH, dtype=np.uint64)))


def same(got, exp, n, what):
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, "%s: %d mismatches, first at (polynomial, coefficient) %s: got %s, expected %s" % (
        what, bad.size, [(int(i) // n, int(i) % n) for i in bad[:8]], got[bad[:8]].tolist(), exp[bad[:8]].tolist())


@pytest.mark.parametrize("log_n", (12, 13, 14, 15, 16))
def test_inverse_bit_exact_at_the_bounds(fhe, cref, torch_cuda, log_n):
    n = 1 << log_n
    for q in moduli(cref, log_n):
        ctx = fhe.NttContext(q)
        cases = inputs(q, n, 2000 * log_n + q % 997)
        rnd = cases[-1][1]
        for name, ev in cases:
            what = "N=2^%d q=2^%d-%d %s" % (log_n, q.bit_length(), (1 << q.bit_length()) - q, name)
            d = to_dev(torch_cuda, ev)
            ctx.intt_(d, n)
            same(to_host(d), cref.ntt_inv(q, ev, n, threads=8), n, "inverse " + what)
            for x, y in ((ev, rnd), (rnd, ev)):
                dx, dy = to_dev(torch_cuda, x), to_dev(torch_cuda, y)
                ctx.mul_(dx, dy, n)
                same(to_host(dx), cref.ntt_mul(q, x, y, n), n, "product " + what)


def test_key_switch_2p15_all_limbs_at_their_maximum(fhe, cref, torch_cuda):
    """two q-limbs, two p-limbs, two ciphertexts, every ciphertext limb q_i - 1, seeded random keys: the inverse of the 2^14
    sub-transforms with the key product fused into its load"""
    n, batch = 1 << 15, 2
    primes = cref.two_adic_primes(60, 16, 4)
    qs, ps = primes[:2], primes[2:]
    rns = fhe.RnsContext(qs, ps)
    rng = np.random.Generator(np.random.PCG64(77))
    kb = np.stack([rng.integers(0, m, size=n, dtype=np.uint64) for m in qs + ps])
    ka = np.stack([rng.integers(0, m, size=n, dtype=np.uint64) for m in qs + ps])
    cb = np.stack([np.stack([np.full(n, m - 1, dtype=np.uint64) for m in qs])] * batch)
    ca = cb.copy()
    key = fhe.CkksKey(rns, to_dev(torch_cuda, kb), to_dev(torch_cuda, ka), n)
    b, a = to_dev(torch_cuda, cb), to_dev(torch_cuda, ca)
    key.key_switch_(b, a)
    for i in range(batch):
        eb, ea = cref.ckks_key_switch(qs, ps, kb, ka, cb[i], ca[i])
        assert np.array_equal(to_host(b)[i], eb) and np.array_equal(to_host(a)[i], ea), i
