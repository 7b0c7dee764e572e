"""GPU parity tests of the RNS conversions (rns_api.hip, rns_kernels.hpp, pm_dot.hpp) at the edges of the limb counts and of the
correction u = round(sum_i frac_i vs_i): every register bound MAXA = 1 / 4 / 8 / 16 / 32 of with_limb_bound up to RNS_MAX_LIMBS = 32 on
both sides, target bases longer than MAXA, bases of pseudo-Mersenne primes of one width, of Shoup primes and of mixed widths, and
residues built from chosen CRT integers: u = 0, u = la, and exact sums within 2^-900 of k + 1/2, where only the f64 rounding of the
reference's sequential sum decides u.  Bit-exact against the oracle (oracle/cref.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LIMB_COUNTS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32]
# the other side of each extend / switch context: below and above MAXA of the source count (lb > MAXA: the Shoup route's chains)
OTHER_SIDE = {1: 17, 2: 17, 7: 9, 8: 8, 9: 7, 15: 17, 16: 16, 17: 2, 31: 32, 32: 31}
RESCALE_SHAPES = [(32, 1), (17, 2), (2, 17), (15, 32), (32, 32)]  # (L, K)
N = 1024  # coefficients per polynomial; two polynomials carry 2048 consecutive deltas


def pm_eligible(q):
    b = q.bit_length()
    return 34 <= b <= 60 and (1 << b) - q <= 1 << (b - 33)


def primes(cref, bits, two_adicity, count, pm):
    """count primes of `bits` bits that are (pm) or are not pseudo-Mersenne eligible"""
    out = [q for q in cref.two_adic_primes(bits, two_adicity, 4 * count + 64) if pm_eligible(q) == pm][:count]
    assert len(out) == count
    return out


def bases(cref, two_adicity=11):
    """(qs pool, ps pool) of 32 primes each: PM 60-bit; Shoup 45-bit and 62-bit; mixed widths 62 / 31 bits and the reverse"""
    pm60 = primes(cref, 60, two_adicity, 64, True)
    sh45 = primes(cref, 45, two_adicity, 64, False)
    sh62 = primes(cref, 62, two_adicity, 64, False)
    sh31 = primes(cref, 31, two_adicity, 32, False)
    return {"pm60": (pm60[:32], pm60[32:]), "shoup45": (sh45[:32], sh45[32:]), "shoup62": (sh62[:32], sh62[32:]),
            "mixed62_31": (sh62[:32], sh31), "mixed31_62": (sh31, sh62[:32])}


BASES = ["pm60", "shoup45", "shoup62", "mixed62_31", "mixed31_62"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def pools(cref):
    return bases(cref)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def prod(mods):
    r = 1
    for m in mods:
        r *= m
    return r


def residues(mods, xs):
    """[len(mods)][len(xs)] residues of the integers xs (any sign)"""
    return np.array([[x % m for x in xs] for m in mods], dtype=np.uint64)


def with_vs(mods, vs):
    """inputs v_i whose conversion state vs_i = v_i (A / a_i)^-1 mod a_i is vs[i] (rns.rs:331-345): v_i = vs_i (A / a_i) mod a_i"""
    A = prod(mods)
    return [(int(s) * (A // m)) % m for s, m in zip(vs, mods)]


def conv_inputs(mods, seed, shift=0):
    """[3][la][N] source limbs over `mods`, each value X + shift read modulo A = prod(mods):
    polys 0, 1: X = floor(A/2) + delta for delta in [-1024, 1024) -- the exact sum sits within 2^-900 of k + 1/2 for multi-limb A;
    poly 2: coefficients 0..15 vs_i = a_i - 1 (u = la), 16..31 vs_i = 0 (u = 0), 32.. random"""
    A, la = prod(mods), len(mods)
    xs = [A // 2 + d - shift for d in range(-N, N)]
    out = np.zeros((3, la, N), dtype=np.uint64)
    r = residues(mods, xs)
    out[0], out[1] = r[:, :N], r[:, N:]
    rng = np.random.Generator(np.random.PCG64(seed))
    out[2] = np.stack([rng.integers(0, m, size=N, dtype=np.uint64) for m in mods])
    top = with_vs(mods, [m - 1 for m in mods])
    shifted = [(v - shift) % m for v, m in zip(top, mods)]
    out[2, :, :16] = np.array(shifted, dtype=np.uint64)[:, None]
    out[2, :, 16:32] = np.array([(-shift) % m for m in mods], dtype=np.uint64)[:, None]
    return out


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("la", LIMB_COUNTS)
def test_extend_switch_at_limb_edges(fhe, cref, torch_cuda, pools, base, la):
    """extend_bases and switch_bases in both directions, source bases of every limb count and every route, u at its extremes and
    decided by the f64 rounding alone"""
    qpool, ppool = pools[base]
    lb = OTHER_SIDE[la]
    qs, ps = qpool[:la], ppool[:lb]
    rns = fhe.RnsContext(qs, ps)
    xq, xp = conv_inputs(qs, la), conv_inputs(ps, lb + 100)
    ext = host(rns.extend_bases(dev(torch_cuda, xq), N))
    to_p = host(rns.switch_bases(dev(torch_cuda, xq), N))
    to_q = host(rns.switch_bases(dev(torch_cuda, xp), N, to_qs=True))
    assert np.array_equal(ext, to_p)
    for b in range(3):
        assert np.array_equal(to_p[b], cref.rns_extend_bases(qs, ps, xq[b])), (b, "qs -> ps")
        assert np.array_equal(to_q[b], cref.rns_extend_bases(ps, qs, xp[b])), (b, "ps -> qs")
    # independently of the oracle: vs_i = a_i - 1 gives u = la and sum_i vs_i (A / a_i) - la A = -sum_i A / a_i; vs_i = 0 gives 0
    A = prod(qs)
    top = [(-sum(A // m for m in qs)) % p for p in ps]
    assert all([int(v) for v in to_p[2, :, i]] == top for i in range(16))
    assert not to_p[2, :, 16:32].any()


def rescale_inputs(qs, ps, seed):
    """[3][L+K][N]: q-limbs random (poly 2: q-1 in every limb); p-limbs such that the value `round` hands to the conversion
    (rns.rs:120-125: + floor(P/2)) is floor(P/2) + delta (polys 0, 1), vs_j = p_j - 1 (poly 2, coefficients 0..15), vs_j = 0 (16..31)"""
    P = prod(ps)
    rng = np.random.Generator(np.random.PCG64(seed))
    L, K = len(qs), len(ps)
    out = np.zeros((3, L + K, N), dtype=np.uint64)
    for b in range(3):
        out[b, :L] = np.stack([rng.integers(0, q, size=N, dtype=np.uint64) for q in qs])
    out[2, :L, :] = np.array([q - 1 for q in qs], dtype=np.uint64)[:, None]
    xp = conv_inputs(ps, seed + 1, shift=P // 2)
    out[:, L:] = xp
    return out


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("big_l,big_k", RESCALE_SHAPES)
def test_rescale_k_at_limb_edges(fhe, cref, torch_cuda, pools, base, big_l, big_k):
    """rescale_k(K) for K = 1 (the reference's shortcut; on mixed bases a wide dropped limb reduced into narrow ones), 2, 17 and 32,
    target bases longer than MAXA, u of the round step at its extremes and decided by the f64 rounding alone"""
    qpool, ppool = pools[base]
    qs, ps = qpool[:big_l], ppool[:big_k]
    rns = fhe.RnsContext(qs, ps)
    full = rescale_inputs(qs, ps, 7 * big_l + big_k)
    out = host(rns.rescale_k(dev(torch_cuda, full), N))
    for b in range(3):
        assert np.array_equal(out[b], cref.rns_rescale_k(qs + ps, big_k, full[b])), b


@pytest.mark.parametrize("base", ["pm60", "shoup45", "mixed31_62"])
def test_rescale_wide_last_limb(fhe, cref, torch_cuda, pools, base):
    """`rescale()` (rns.rs:99-101): drops the last q-limb; here that limb is wider than the rest (62 bits over 31- / 45- / 60-bit
    limbs), so the reduction of the dropped limb into the others has no slack"""
    qpool, ppool = pools[base]
    wide = pools["shoup62"][1][-1]
    for big_l in (2, 9, 32):
        qs = qpool[:big_l - 1] + [wide]
        rns = fhe.RnsContext(qs, ppool[:1])
        limbs = rescale_inputs(qs[:-1], [wide], big_l)[:, :big_l]
        limbs[2, -1, 32:64] = wide - 1
        out = host(rns.rescale(dev(torch_cuda, limbs), N))
        for b in range(3):
            assert np.array_equal(out[b], cref.rns_rescale_k(qs, 1, limbs[b])), (big_l, b)


def test_rns_ctx_limb_limits(fhe, cref, pools):
    """RNS_MAX_LIMBS = 32 on each side: 32 + 32 is accepted, 33 on either side is FHE_ERR_INVALID"""
    qs, ps = pools["pm60"]
    fhe.RnsContext(qs, ps)
    extra = primes(cref, 60, 11, 65, True)[64]
    for a, b in ((qs + [extra], ps), (qs, ps + [extra])):
        with pytest.raises(fhe.FheError) as e:
            fhe.RnsContext(a, b)
        assert e.value.code == 1


def rand_limbs(seed, mods, n, batch=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = [rng.integers(0, m, size=(n if batch is None else (batch, n)), dtype=np.uint64) for m in mods]
    return np.stack(rows, axis=0 if batch is None else 1)


@pytest.mark.parametrize("route", ["pm60", "shoup45"])
@pytest.mark.parametrize("log_n,limbs", [(10, 17), (12, 32)])
def test_ckks_key_switch_and_mul_at_limb_edges(fhe, cref, torch_cuda, route, log_n, limbs):
    """`Ckks::key_switch` and `Ckks::mul` at 17 + 17 and 32 + 32 limbs: bit-exact against the oracle, or the documented
    FHE_ERR_UNSUPPORTED (fhe_ring.h); any other status fails"""
    n, batch = 1 << log_n, 2
    pool = primes(cref, 60 if route == "pm60" else 45, log_n + 1, 2 * limbs, route == "pm60")
    qs, ps = pool[:limbs], pool[limbs:]
    rns = fhe.RnsContext(qs, ps)
    kb, ka = rand_limbs(1, qs + ps, n), rand_limbs(2, qs + ps, n)
    kb[:, 0] = [m - 1 for m in qs + ps]
    cts = [rand_limbs(3 + i, qs, n, batch) for i in range(4)]
    cts[1][0] = np.array([q - 1 for q in qs], dtype=np.uint64)[:, None]  # one ciphertext's a: every limb all q-1
    try:
        key = fhe.CkksKey(rns, dev(torch_cuda, kb), dev(torch_cuda, ka), n)
        b, a = dev(torch_cuda, cts[0]), dev(torch_cuda, cts[1])
        key.key_switch_(b, a)
    except fhe.FheError as e:
        assert e.code == 6, str(e)
        return
    for i in range(batch):
        eb, ea = cref.ckks_key_switch(qs, ps, kb, ka, cts[0][i], cts[1][i])
        assert np.array_equal(host(b)[i], eb) and np.array_equal(host(a)[i], ea), ("key switch", i)
    try:
        ob, oa = key.mul(*[dev(torch_cuda, c) for c in cts])
    except fhe.FheError as e:
        assert e.code == 6, str(e)
        return
    for i in range(batch):
        eb, ea = cref.ckks_mul(qs, ps, kb, ka, *[c[i] for c in cts])
        assert np.array_equal(host(ob)[i], eb) and np.array_equal(host(oa)[i], ea), ("mul", i)
