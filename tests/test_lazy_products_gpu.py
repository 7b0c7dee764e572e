"""The forward wave-local transforms (csrc/ntt14w.hpp) leave every twiddle product unfolded and fold only the additive operand of a
butterfly, by a compile-time schedule (csrc/arith.hpp, DsLazy).  Bit-exact against the oracle (oracle/cref.py) where a bound that
is too optimistic would show: N = 2^12 .. 2^15 (every R0) and 2^16 (the sub-transform form), three polynomials, on
  * the 2^60 - 98303 prime of the headline workload (N <= 2^14: it has no larger root of unity),
  * of the first 16 primes of two_adic_primes(60, .) the one with the largest c,
  * the 60-bit prime of the family with the largest c the pseudo-Mersenne path admits at all (c <= 2^27: the proof's own limit,
    so there is no modulus that takes these kernels outside it -- anything above runs Shoup arithmetic as before),
  * the first 54-bit and 55-bit prime of the same family and, where the ring size has one (54 bits: N <= 2^14, 55 bits: N <= 2^15),
    the 54- / 55-bit prime with the largest admitted c (c <= 2^21 / 2^22),
with inputs all zero, all q - 1, alternating 0 / q - 1, a single q - 1 at index 0 and at index N - 1, and seeded random values:
forward, inverse (on the oracle's evaluations), round trip and the ring product."""
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
    return torch.from_numpy(a.view(np.int64)).cuda()


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
        # the family's first prime of the width (from 2^15 / 2^16 on its c is above 2^(bits - 33): Shoup arithmetic) and, where the
        # width has one at this ring size (54 bits: N <= 2^14, 55 bits: N <= 2^15), the eligible prime with the largest c
        out.append(cref.two_adic_primes(bits, log_n + 1, 1)[0])
        lazy = largest_admitted_c_prime(bits, log_n + 1)
        if lazy is not None and lazy != out[-1]:
            out.append(lazy)
    return out


def inputs(q, n, seed):
    """(name, BATCH polynomials)"""
    top = np.uint64(q - 1)
    zero = np.zeros(n * BATCH, dtype=np.uint64)
    alt = zero.copy(); alt[1::2] = top
    first = zero.copy(); first[0::n] = top
    last = zero.copy(); last[n - 1::n] = top
    rng = np.random.Generator(np.random.PCG64(seed))
    return (("zero", zero), ("all q-1", np.full(n * BATCH, top, dtype=np.uint64)), ("alternating", alt), ("q-1 at 0", first),
            ("q-1 at N-1", last), ("random", rng.integers(0, q, size=n * BATCH, dtype=np.uint64)))


def same(got, exp, n, what):
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, "%s: %d mismatches, first at (polynomial, coefficient) %s: got %s, expected %s" % (
        what, bad.size, [(int(i) // n, int(i) % n) for i in bad[:8]], got[bad[:8]].tolist(), exp[bad[:8]].tolist())


@pytest.mark.parametrize("log_n", (12, 13, 14, 15, 16))
def test_bit_exact_at_the_bounds(fhe, cref, torch_cuda, log_n):
    n = 1 << log_n
    for q in moduli(cref, log_n):
        ctx = fhe.NttContext(q)
        cases = inputs(q, n, 1000 * log_n + q % 997)
        rnd = cases[-1][1]
        for name, a in cases:
            what = "N=2^%d q=2^%d-%d %s" % (log_n, q.bit_length(), (1 << q.bit_length()) - q, name)
            ev = cref.ntt_fwd(q, a, n, threads=8)
            d = to_dev(torch_cuda, a)
            ctx.ntt_(d, n)
            same(to_host(d), ev, n, "forward " + what)
            ctx.intt_(d, n)
            same(to_host(d), a, n, "round trip " + what)
            d = to_dev(torch_cuda, ev)
            ctx.intt_(d, n)
            same(to_host(d), a, n, "inverse " + what)
            for x, y in ((a, rnd), (rnd, a)):
                dx, dy = to_dev(torch_cuda, x), to_dev(torch_cuda, y)
                ctx.mul_(dx, dy, n)
                same(to_host(dx), cref.ntt_mul(q, x, y, n), n, "product " + what)
