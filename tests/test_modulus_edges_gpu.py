"""GPU parity tests at the edges of the accepted moduli (ring_api.hip ctx_build_host): the top of the range (62-bit primes, where
ArithShoup's [0, 4q) and the composed FHEW MAC's sum + r < 4q <= 2^64 have almost no slack), and both sides of the pseudo-Mersenne
eligibility bound c <= 2^(B-33) (arith.hpp ArithPM / ArithDS, the FHEW policies of fhew_api.hip fhew_pm).  Transforms, ring
products and FHEW gadget products, bit-exact against the oracle on random inputs and on the extreme patterns that drive the lazy
reductions to their stated bounds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (B, log_n, c_pm, c_shoup): q = 2^B - c prime with 2^(log_n + 1) | q - 1; c_pm the largest such c <= 2^(B-33) (pseudo-Mersenne
# eligible), c_shoup the smallest above it (must route to Shoup).  Found with a Miller-Rabin search; test_oracle_cpu.py re-checks it.
PM_BOUNDARY = [
    (44, 0, 2045, 2049), (44, 3, 1695, 2367),
    (48, 6, 31743, 34559), (48, 10, 16383, 73727),
    (52, 10, 460799, 532479), (52, 12, 245759, 532479),
    (54, 9, 2082815, 2098175), (54, 10, 2082815, 2107391), (54, 11, 1867775, 2179071),
    (55, 9, 4179967, 4195327), (55, 10, 4179967, 4200447), (55, 11, 4087807, 4222975),
    (56, 14, 6946815, 8912895),
    (60, 14, 133398527, 134774783), (60, 15, 132972543, 135725055), (60, 16, 131989503, 136052735), (60, 17, 127401983, 136052735),
]
# the largest 62-bit primes of two_adic_primes(62, log_n + 1): c = 2^62 - q
TOP_62 = [(0, 57), (10, 22527), (14, 65535), (17, 1572863)]

# (B, log_n, c): q = 2^B - c with c just below 2^(B/2), so that 2^(2B) mod q = c^2 mod q is within 0.3 % of q.  The Barrett quotient
# of dev_arith.hpp (mu = floor(2^(2B) / q)) then falls short by 2 for about one product in eight against q-1: mulmod_barrett_lazy
# reaches [2q, 3q), and the composed FHEW MAC's sum + r (fhew_composed_kernels.hpp) reaches [3q, 4q) -- at 62 bits up to 2^64.  The
# primes of two_adic_primes (c small) never get there: their mu has no fractional part to lose.
BARRETT_WORST = [(62, 15, 2147418111), (60, 13, 1073496063), (54, 11, 134090751)]

# (q, log_n, route): log_n = the largest ring the entry was chosen for; route = what ctx_build_host must pick
EDGE_PRIMES = ([((1 << b) - cp, ln, "pm") for b, ln, cp, _ in PM_BOUNDARY]
               + [((1 << b) - cs, ln, "shoup") for b, ln, _, cs in PM_BOUNDARY]
               + [((1 << 62) - c, ln, "shoup") for ln, c in TOP_62]
               + [((1 << b) - c, ln, "shoup") for b, ln, c in BARRETT_WORST]
               + [(65537, 15, "shoup"), (12289, 11, "shoup")])


def pm_eligible(q):
    """ring_api.hip ctx_build_host: q = 2^B - c with 34 <= B <= 60 and c <= 2^(B-33), B the bit length of q"""
    b = q.bit_length()
    return 34 <= b <= 60 and (1 << b) - q <= 1 << (b - 33)


def two_adicity(q):
    return ((q - 1) & -(q - 1)).bit_length() - 1


def edge_id(e):
    q, ln, route = e
    b = q.bit_length()
    return "B%d-c%d-ln%d-%s" % (b, (1 << b) - q, ln, route) if b > 20 else "q%d-ln%d" % (q, ln)


def rand_u64(seed, q, shape):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, q, size=shape, dtype=np.uint64)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def patterns(q, n):
    """the extremes of test_ntt_gpu.py test_extreme_values_2p14: all q-1, all zero, alternating q-1 / 0, all q >> 1"""
    p = np.zeros((4, n), dtype=np.uint64)
    p[0, :] = q - 1
    p[2, 0::2] = q - 1
    p[3, :] = q >> 1
    return p


def sizes_of(ln):
    """the entry's own ring and the smaller ones that reach every transform kernel family (generic < 2^10, ArithPM 2^10 / 2^11,
    wave-local 2^12 / 2^13, 2^14)"""
    return sorted({ln} | {s for s in (3, 10, 11, 12, 13, 14) if s < ln})


def batch_of(log_n):
    return 67 if log_n <= 9 else 13 if log_n <= 13 else 5  # ragged: not a multiple of the polynomials per workgroup


@pytest.mark.parametrize("entry", EDGE_PRIMES, ids=edge_id)
def test_transforms_at_edge_primes(fhe, cref, torch_cuda, entry):
    """forward, inverse on oracle evaluations and the round trip, every kernel family up to the prime's own ring size"""
    q, ln, route = entry
    assert pm_eligible(q) == (route == "pm")
    ctx = fhe.NttContext(q)
    for log_n in sizes_of(ln):
        n, batch = 1 << log_n, batch_of(log_n)
        a = rand_u64(q % 1000003 + log_n, q, (batch, n))
        a[:4] = patterns(q, n)
        exp = cref.ntt_fwd(q, a.reshape(-1), n, threads=8).reshape(batch, n)
        d = dev(torch_cuda, a)
        ctx.ntt_(d, n)
        assert np.array_equal(host(d), exp), (log_n, "forward")
        ctx.intt_(d, n)
        assert np.array_equal(host(d), a), (log_n, "round trip")
        ev = exp.copy()  # inverse alone on evaluations: the same extremes in the evaluation domain, then oracle outputs
        ev[:4] = patterns(q, n)
        d = dev(torch_cuda, ev)
        ctx.intt_(d, n)
        assert np.array_equal(host(d), cref.ntt_inv(q, ev.reshape(-1), n, threads=8).reshape(batch, n)), (log_n, "inverse")


@pytest.mark.parametrize("entry", EDGE_PRIMES, ids=edge_id)
def test_products_at_edge_primes(fhe, cref, torch_cuda, entry):
    """mul_ (the fused forward-multiply-inverse kernels at 2^13 .. 2^15) against the oracle's product and, up to 2^10, the schoolbook
    product; pointwise_mul_; one operand all q-1 in each"""
    q, ln, _ = entry
    ctx = fhe.NttContext(q)
    for log_n in sorted({ln, min(ln, 10)} | {s for s in (13, 14) if s < ln}):
        n, batch = 1 << log_n, 3
        a, b = rand_u64(q % 999983 + log_n, q, (batch, n)), rand_u64(q % 999979 + log_n, q, (batch, n))
        a[0, :] = q - 1
        b[1, :] = q - 1
        a[2, :] = q - 1
        b[2, :] = q - 1
        da = dev(torch_cuda, a)
        ctx.mul_(da, dev(torch_cuda, b), n)
        out = host(da)
        for i in range(batch):
            assert np.array_equal(out[i], cref.ntt_mul(q, a[i], b[i], n)), (log_n, i)
            if n <= 1024:
                assert np.array_equal(out[i], cref.schoolbook_mul(q, a[i], b[i])), (log_n, i)
    x, y = rand_u64(q % 7919, q, 4099), np.full(4099, q - 1, dtype=np.uint64)
    for u, v in ((x, y), (y, x), (y, y)):
        du = dev(torch_cuda, u)
        ctx.pointwise_mul_(du, dev(torch_cuda, v))
        assert np.array_equal(host(du), cref.pointwise_mul(q, u, v))


# ---- FHEW gadget products (fhew_api.hip): the fused kernels at 2^9 .. 2^11 (ArithDS<54 / 55> where fhew_pm picks it, Shoup
# otherwise) and the composed route (fhew_composed_kernels.hpp) at 2^12 / 2^13 --------------------------------------------------

class Composed:
    """FHEW keys prepared inside the block run the composed route at every size (lab switch FHEW_COMPOSED)"""

    def __init__(self, fhe):
        self.fhe = fhe

    def __enter__(self):
        self.fhe.set_option("FHEW_COMPOSED", 1)

    def __exit__(self, *exc):
        self.fhe.set_option("FHEW_COMPOSED", 0)


def decomps(q):
    """two (log_b, d) pairs make_decomp accepts: rb = log_q - log_b d = 0 (every bit decomposed) and rb > 0 (rounded low bits)"""
    log_q = (q - 1).bit_length()
    d0 = -(-log_q // 6)
    return [(6, d0), (5, 4)]


def rb_of(q, log_b, d):
    return max(0, (q - 1).bit_length() - log_b * d)


def gadget_inputs(q, n, log_b, d, seed):
    """key entry 0: random; key entry 1: adversarial, every row the constant polynomial q-1 (its evaluations are all q-1).
    Ciphertexts: three random, then one all q-1."""
    ra, rb = rand_u64(seed, q, (2, 2 * d, n)), rand_u64(seed + 1, q, (2, 2 * d, n))
    ka, kb = rand_u64(seed + 2, q, (2, d, n)), rand_u64(seed + 3, q, (2, d, n))
    for rows in (ra, rb, ka, kb):
        rows[1] = 0
        rows[1, :, 0] = q - 1
    ca, cb = rand_u64(seed + 4, q, (4, n)), rand_u64(seed + 5, q, (4, n))
    ca[3] = q - 1
    cb[3] = q - 1
    return ra, rb, ka, kb, ca, cb


OPS = [("ep", 1), ("ks", 1), ("auto", 5), ("auto", -5)]


def run_gadget(fhe, torch, ctx, n, log_b, d, keys, ca, cb):
    ra, rb, ka, kb = keys
    rgsw = fhe.GadgetKey(ctx, log_b, d, dev(torch, ra), dev(torch, rb), n, rgsw=True)
    ksk = fhe.GadgetKey(ctx, log_b, d, dev(torch, ka), dev(torch, kb), n, rgsw=False)
    out = {}
    for idx in (0, 1):
        for kind, t in OPS:
            a, b = dev(torch, ca), dev(torch, cb)
            if kind == "ep":
                rgsw.external_product_(idx, a, b)
            elif kind == "ks":
                ksk.key_switch_(idx, a, b)
            else:
                ksk.automorphism_(idx, t, a, b)
            out[idx, kind, t] = (host(a), host(b))
    return out


def oracle_gadget(cref, q, log_b, d, keys, ca, cb, idx, kind, t, i):
    ra, rb, ka, kb = keys
    if kind == "ep":
        return cref.external_product(q, log_b, d, ra[idx], rb[idx], ca[i], cb[i])
    if kind == "ks":
        return cref.rlwe_key_switch(q, log_b, d, ka[idx], kb[idx], ca[i], cb[i])
    return cref.rlwe_automorphism(q, log_b, d, t, ka[idx], kb[idx], ca[i], cb[i])


def _by_bits(bits, ln=None):
    return [e for e in EDGE_PRIMES if e[0].bit_length() == bits and (ln is None or e[1] == ln)]


# (entry, ring sizes): the PM54 / PM55 boundary on both sides at their own fused size (and the 54-bit Barrett worst case); 62-bit
# primes (the largest at 2^15, the Barrett worst case) at fused sizes and a composed one; composed rings on a 60-bit boundary prime
# (ArithDS<60> transforms) and a 52-bit one (eligible, Shoup transforms)
GADGET_CASES = ([(e, [e[1]]) for e in _by_bits(54) + _by_bits(55)]
                + [(e, [9, 11, 13]) for e in _by_bits(62, 14) + _by_bits(62, 15)]
                + [(e, [13]) for e in _by_bits(60, 14)]
                + [(_by_bits(52, 12)[0], [12])])


@pytest.mark.parametrize("entry,log_ns", GADGET_CASES, ids=[edge_id(c[0]) for c in GADGET_CASES])
def test_gadget_products_at_edge_primes(fhe, cref, torch_cuda, entry, log_ns):
    """external product, RLWE key switch, automorphism t = 5 / -5 against the oracle, random and adversarial keys and ciphertexts"""
    q = entry[0]
    ctx = fhe.NttContext(q)
    pairs = decomps(q)
    assert rb_of(q, *pairs[0]) == 0 and rb_of(q, *pairs[1]) > 0
    for log_n in log_ns:
        n = 1 << log_n
        for log_b, d in pairs:
            ra, rb, ka, kb, ca, cb = gadget_inputs(q, n, log_b, d, seed=log_n * 100 + log_b)
            keys = (ra, rb, ka, kb)
            out = run_gadget(fhe, torch_cuda, ctx, n, log_b, d, keys, ca, cb)
            for (idx, kind, t), (ha, hb) in out.items():
                for i in range(4):
                    ea, eb = oracle_gadget(cref, q, log_b, d, keys, ca, cb, idx, kind, t, i)
                    assert np.array_equal(ha[i], ea) and np.array_equal(hb[i], eb), (log_n, log_b, d, idx, kind, t, i)


@pytest.mark.parametrize("entry", _by_bits(54, 11) + _by_bits(55, 11) + _by_bits(62, 15), ids=edge_id)
def test_gadget_composed_equals_fused_at_pm_boundary(fhe, cref, torch_cuda, entry):
    """N = 2^11 at the PM54 / PM55 boundary and at the 62-bit Barrett worst case: keys prepared under FHEW_COMPOSED give the fused
    route's bits, adversarial inputs included"""
    q = entry[0]
    n = 1 << 11
    ctx = fhe.NttContext(q)
    log_b, d = decomps(q)[0]
    ra, rb, ka, kb, ca, cb = gadget_inputs(q, n, log_b, d, seed=77)
    keys = (ra, rb, ka, kb)
    fused = run_gadget(fhe, torch_cuda, ctx, n, log_b, d, keys, ca, cb)
    with Composed(fhe):
        composed = run_gadget(fhe, torch_cuda, ctx, n, log_b, d, keys, ca, cb)
    for k, (fa, fb) in fused.items():
        ca_, cb_ = composed[k]
        assert np.array_equal(fa, ca_) and np.array_equal(fb, cb_), k
    ea, eb = oracle_gadget(cref, q, log_b, d, keys, ca, cb, 1, "ep", 1, 3)  # the adversarial corner, once against the oracle too
    assert np.array_equal(fused[1, "ep", 1][0][3], ea) and np.array_equal(fused[1, "ep", 1][1][3], eb)
