"""GPU parity tests for the order in which the wave-local inverse (learn-fhe_amd/csrc/ntt14w.hpp: ntt14w_inv_kernel,
sub_of_block_inv) walks a batch: block b transforms polynomial count - 1 - b, and with several moduli the 2-D grid is taken from its
far corner.  The map must stay a bijection onto the sub-polynomials with descriptor, sub-transform prefix, source and multiplier
following the same index, so: the inverse alone and forward then inverse, bit-equal to the oracle, at N = 2^12, 2^13, 2^14 on 60-,
55- and 54-bit pseudo-Mersenne moduli and on the largest admitted c, with batches of 1, 3 and 5 (a single block, odd counts) in which
EVERY polynomial differs from every other (all zero, all q - 1, random ones), so that a polynomial transformed twice, skipped, or
stored in another one's place cannot pass; RNS transforms at 2^15 and 2^16 over 3 limbs and a batch of 2 (whole 2^15 rings over
several moduli, and the 2^14 sub-transforms of a larger ring: PFX, several descriptors); and the CKKS key switch, whose inverse
launches read a broadcast source and a multiplier."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POOL = 5  # polynomials per (q, N): all zero, all q - 1, three random ones


def pm_eligible(q):
    """ring_api.hip ctx_build_host: q = 2^B - c with 34 <= B <= 60 and c <= 2^(B-33), B the bit length of q"""
    b = q.bit_length()
    return 34 <= b <= 60 and (1 << b) - q <= 1 << (b - 33)


# q = 2^60 - c, the largest c <= 2^27 with 2^15 | q - 1 (tests/test_modulus_edges_gpu.py PM_BOUNDARY, the (60, 14) entry)
LARGEST_C_60 = (1 << 60) - 133398527


def moduli(cref):
    qs = cref.two_adic_primes(60, 15, 2) + cref.two_adic_primes(55, 15, 1) + cref.two_adic_primes(54, 15, 1) + [LARGEST_C_60]
    assert len(qs) == 5 and all(pm_eligible(q) for q in qs), qs  # every one runs the 16-byte (ArithDS) wave-local kernels
    return qs


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


_cases = {}


def case(cref, qi, log_n):
    """the pool of one (modulus, ring size) with its oracle transforms, computed once and shared, never written to"""
    key = (qi, log_n)
    if key not in _cases:
        q, n = moduli(cref)[qi], 1 << log_n
        rng = np.random.Generator(np.random.PCG64(1000 * qi + log_n))
        pool = rng.integers(0, q, size=(POOL, n), dtype=np.uint64)
        pool[0, :] = 0
        pool[1, :] = q - 1
        fwd = cref.ntt_fwd(q, pool.reshape(-1), n, threads=8).reshape(POOL, n)
        inv = cref.ntt_inv(q, pool.reshape(-1), n, threads=8).reshape(POOL, n)
        for arr in (pool, fwd, inv):
            arr.setflags(write=False)
        # the pool's members, their evaluations and their inverses are pairwise different (all zero maps to all zero; nothing else does)
        for arr in (pool, fwd, inv):
            assert len({arr[i].tobytes() for i in range(POOL)}) == POOL
        _cases[key] = (q, n, pool, fwd, inv)
    return _cases[key]


# batches of 1 (each kind of input on its own), 3 and 5: rows of the pool
BATCHES = [[0], [1], [2], [0, 1, 2], [0, 1, 2, 3, 4], [4, 3, 2, 1, 0]]


@pytest.mark.parametrize("log_n", [12, 13, 14])
@pytest.mark.parametrize("qi", range(5), ids=["q60a", "q60b", "q55", "q54", "q60-largest-c"])
def test_inverse_alone_and_round_trip(fhe, cref, torch_cuda, qi, log_n):
    q, n, pool, fwd, inv = case(cref, qi, log_n)
    ctx = fhe.NttContext(q)
    for rows in BATCHES:
        d = dev(torch_cuda, pool[rows])  # the pool as evaluations: the inverse alone
        ctx.intt_(d, n)
        assert np.array_equal(host(d), inv[rows]), (rows, "inverse")
        d = dev(torch_cuda, pool[rows])
        ctx.ntt_(d, n)
        assert np.array_equal(host(d), fwd[rows]), (rows, "forward")
        ctx.intt_(d, n)
        assert np.array_equal(host(d), pool[rows]), (rows, "round trip")


@pytest.mark.parametrize("log_n", [15, 16])
def test_rns_transforms_three_limbs(fhe, cref, torch_cuda, log_n):
    """fhe_rns_ntt_fwd / fhe_rns_ntt_inv on [batch 2][3 limbs][N]: 2^15 whole rings over three descriptors, 2^16 = a radix-2 pass and
    2^14 sub-transforms (PFX); every limb of every polynomial against the oracle"""
    n, batch = 1 << log_n, 2
    primes = cref.two_adic_primes(60, log_n + 1, 4)
    qs = primes[:3]
    rns = fhe.RnsContext(qs, primes[3:])
    rng = np.random.Generator(np.random.PCG64(log_n))
    a = np.stack([rng.integers(0, q, size=(batch, n), dtype=np.uint64) for q in qs], axis=1)  # [batch][limb][n]
    a[0, 0, :] = qs[0] - 1
    d = dev(torch_cuda, a)
    rns.ntt_(d, n, inverse=True)  # a as evaluations: the inverse alone
    got = host(d)
    for b in range(batch):
        for l, q in enumerate(qs):
            assert np.array_equal(got[b, l], cref.ntt_inv(q, a[b, l], n)), (b, l, "inverse")
    d = dev(torch_cuda, a)
    rns.ntt_(d, n)
    got = host(d)
    for b in range(batch):
        for l, q in enumerate(qs):
            assert np.array_equal(got[b, l], cref.ntt_fwd(q, a[b, l], n)), (b, l, "forward")
    rns.ntt_(d, n, inverse=True)
    assert np.array_equal(host(d), a)


# the smallest shape of tests/test_rns_gpu.py test_ckks_key_switch_vs_oracle, and its smallest one whose inverse is a wave-local launch
@pytest.mark.parametrize("log_n,bits,big_l", [(4, 50, 3), (13, 60, 2)])
def test_ckks_key_switch(fhe, cref, torch_cuda, log_n, bits, big_l):
    n, batch = 1 << log_n, 2
    primes = cref.two_adic_primes(bits, log_n + 1, 2 * big_l)
    qs, ps = primes[:big_l], primes[big_l:]
    rns = fhe.RnsContext(qs, ps)

    def rand_limbs(seed, mods, bt=None):
        rng = np.random.Generator(np.random.PCG64(seed))
        return np.stack([rng.integers(0, m, size=(n if bt is None else (bt, n)), dtype=np.uint64) for m in mods], axis=0 if bt is None else 1)

    kb, ka = rand_limbs(1, qs + ps), rand_limbs(2, qs + ps)
    cb, ca = rand_limbs(3, qs, batch), rand_limbs(4, qs, batch)
    key = fhe.CkksKey(rns, dev(torch_cuda, kb), dev(torch_cuda, ka), n)
    b, a = dev(torch_cuda, cb), dev(torch_cuda, ca)
    key.key_switch_(b, a)
    for i in range(batch):
        eb, ea = cref.ckks_key_switch(qs, ps, kb, ka, cb[i], ca[i])
        assert np.array_equal(host(b)[i], eb) and np.array_equal(host(a)[i], ea), i
