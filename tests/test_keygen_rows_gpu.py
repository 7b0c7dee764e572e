"""Every row of every device-made key, exactly.  The decrypt-level tests of test_keygen_gpu.py / test_rns_gpu.py / test_torusk_gpu.py
cannot see noise that is a few bits too wide, noise shared by two rows, a gadget term that is off in one digit or one limb, or a
grid-stride tail that goes wrong: all of those still decode.  Here the secret key is known, the exact oracle (oracle/cref.py)
gives a s and the gadget term, and so the noise of EVERY coefficient of EVERY row is recovered as an integer and held against
(a) the sampler's hard support, (b) its law on the pooled residuals, (c) tests/keygen_checks.py `rows_independent`, with (d) the
mask checked for range and repeats and (e) the host-memory call compared bit for bit at the smallest shape.  One fixed generator key
and explicit stream ids: every run sees the same draws.  Nothing here models the keystream.

Bounds (tests/keygen_checks.py, confirmed on numpy's own draws in test_keygen_checks_cpu.py): dg(3.2, 6) has |e| <= 19 and is
tested by chi-square on >= 2^16 residuals, X^2 <= dof + 6 sqrt(2 dof); tdg is Box-Muller on u1 >= 2^-53, so
|e| <= sqrt(106 ln 2) std_dev = 8.572 std_dev (asserted as 8.58 std_dev 2^64 + 1), tested by Kolmogorov distance on >= 2^18
residuals, D <= 3 / sqrt(N)."""
import numpy as np
import pytest

import keygen_checks as K

pytestmark = pytest.mark.gpu

U = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731
SD, NS, DG_MAX = 3.2, 6, 19
DG_POOL, TDG_POOL = 1 << 16, 1 << 18
T64 = 2.0 ** 64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def rng(fhe):
    return fhe.Rng(key=bytes(range(32)))


@pytest.fixture(scope="module")
def like(torch_cuda):
    return dev(torch_cuda, U([0]))


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def prime(cref, bits, log_n):
    return cref.two_adic_primes(bits, log_n + 1, 1)[0]


def check_dg(name, res):
    """(a), (b), (c) for dg(3.2, 6) noise; res [rows][n] centred integers"""
    res = np.asarray(res)
    assert int(np.abs(res).max()) <= DG_MAX, (name, int(np.abs(res).max()))
    assert res.size >= DG_POOL, (name, res.size)
    x2, dof = K.chi2_dg(res, SD, NS)
    corr = K.rows_independent(K.as_rows(res.reshape(-1, res.shape[-1])))
    print("FIG %s: pool %d, X^2 = %.1f (dof %d, bound %.1f), worst |corr| %.3f" % (name, res.size, x2, dof, K.chi2_bound(dof), corr))
    assert K.chi2_ok(x2, dof), (name, x2, dof)


def check_tdg(name, res, sd):
    """(a), (b), (c) for tdg(sd) noise; res [rows][n] int64 torus differences"""
    res = np.asarray(res)
    worst = float(np.abs(res.astype(np.float64)).max())
    assert worst <= 8.58 * sd * T64 + 1, (name, worst / (sd * T64))
    assert res.size >= TDG_POOL, (name, res.size)
    dist = K.ks_normal(res.astype(np.float64), sd * T64)
    corr = K.rows_independent(K.as_rows(res.reshape(-1, res.shape[-1])))
    print("FIG %s: pool %d, D = %.2e (bound %.2e), max |e| = %.2f sd, worst |corr| %.3f" % (name, res.size, dist, K.ks_bound(res.size), worst / (sd * T64), corr))
    assert K.ks_ok(dist, res.size), (name, dist)


def check_mask(torch, a, q=None):
    """(d): every value below q; no value twice where the modulus leaves no room for a chance repeat: the torus, and q >= 2^44 --
    the "45-bit" primes of two_adic_primes lie just below 2^45, where 2^16 values repeat by chance with probability 2^-14"""
    if q is not None:
        assert int(a.min()) >= 0 and int(a.max()) < q
    if q is None or q >= 1 << 44:
        assert torch.unique(a).numel() == a.numel()


def rand_mod(seed, q, shape):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, q, size=shape, dtype=np.uint64)


def rand64(seed, shape):
    g = np.random.Generator(np.random.PCG64(seed))
    return g.integers(0, 1 << 63, size=shape, dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, size=shape, dtype=np.uint64)


def terms_of(q, pt, bases):
    """[count][n] plaintexts -> [count][d][n]: pt base_j mod q"""
    return np.stack([np.stack([K.scalar_mul_mod(q, p, g) for g in bases]) for p in pt])


# ---- RLWE -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_pt", [True, False])
@pytest.mark.parametrize("bits", [45, 62])
@pytest.mark.parametrize("log_n", [0, 1, 6, 10, 12])
def test_rlwe_sk_encrypt_rows(fhe, cref, torch_cuda, rng, like, log_n, bits, with_pt):
    """rlwe.rs:146-156 at the sizes where the product under it changes route (one product per ciphertext at n = 1, the generic
    transforms, the pseudo-Mersenne ones from 2^10, the wave-local ones at 2^12), a 45-bit prime and the largest 62-bit one"""
    n = 1 << log_n
    q = prime(cref, bits, log_n)
    batch = DG_POOL // n
    sid = 1000 + 100 * log_n + 10 * (bits == 62) + with_pt
    ctx = fhe.NttContext(q)
    sk = fhe.sample_dg(q, SD, NS, rng, sid, like, (n,))
    pt = rand_mod(sid, q, (batch, n)) if with_pt else None
    a, b = fhe.rlwe_sk_encrypt(ctx, sk, dev(torch_cuda, pt) if with_pt else None, n, batch, rng, sid)
    check_mask(torch_cuda, a, q)
    check_dg("rlwe_sk_encrypt n=%d q~2^%d pt=%d" % (n, bits, with_pt), K.rlwe_residual(q, host(sk), host(a), host(b), pt))
    if log_n <= 1:  # (e)
        ha, hb = fhe.rlwe_sk_encrypt(ctx, host(sk), pt, n, batch, rng, sid)
        assert np.array_equal(ha, host(a)) and np.array_equal(hb, host(b))


@pytest.mark.parametrize("which", [0, 1])
def test_rgsw_encrypt_rows(fhe, cref, torch_cuda, rng, like, which):
    """rgsw.rs:84-105: rows j < d carry pt base_j on a (e = b - (a - base_j pt) s), rows d + j on b (e = b - a s - base_j pt);
    a gadget that decomposes every bit and one that rounds low bits away; monomials of either sign and dense plaintexts"""
    n, log_n = 256, 8
    q = prime(cref, 45, log_n)
    log_b, d = [(6, -(-45 // 6)), (5, 4)][which]
    bases = K.gadget_bases(q, log_b, d)
    assert (bases[0] == 1) == (which == 0)
    count = DG_POOL // (2 * d * n)
    sid = 2000 + which
    ctx = fhe.NttContext(q)
    sk = fhe.sample_dg(q, SD, NS, rng, sid, like, (n,))
    pt = rand_mod(sid, q, (count, n))
    for c in range(0, count, 2):        # every other plaintext a monomial +-X^k, as the blind rotation's are
        pt[c] = 0
        pt[c, (37 * c + 5) % n] = 1 if c % 4 == 0 else q - 1
    ra, rb = fhe.rgsw_encrypt(ctx, log_b, d, sk, dev(torch_cuda, pt), n, rng, sid)
    check_mask(torch_cuda, ra[:, d:], q)          # the first d rows' masks carry the message: checked through the residual instead
    ha, hb, t = host(ra).reshape(count, 2 * d, n), host(rb).reshape(count, 2 * d, n), terms_of(q, pt, bases)
    s = host(sk)
    top = K.rlwe_residual(q, s, ha[:, :d].reshape(-1, n), hb[:, :d].reshape(-1, n), on_a=t.reshape(-1, n)).reshape(count, d, n)
    bot = K.rlwe_residual(q, s, ha[:, d:].reshape(-1, n), hb[:, d:].reshape(-1, n), pt=t.reshape(-1, n)).reshape(count, d, n)
    check_dg("rgsw_encrypt (%d, %d)" % (log_b, d), np.concatenate([top, bot], axis=1).reshape(-1, n))
    if which == 1:  # (e), the smaller call
        xa, xb = fhe.rgsw_encrypt(ctx, log_b, d, s, pt, n, rng, sid)
        assert np.array_equal(xa.reshape(ha.shape), ha) and np.array_equal(xb.reshape(hb.shape), hb)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("t", [0, 5, -5, 2 * 1024 + 3])
def test_rlwe_ksk_gen_rows(fhe, cref, torch_cuda, rng, like, t, which):
    """rlwe.rs:109-132: row j encrypts -sk1 base_j (t = 0, a second key) or -sk0(X^t) base_j (automorphism keys, t odd, negative,
    beyond 2n) under sk0; one call makes d rows, so a pool is several calls on consecutive stream ids"""
    n, log_n = 1024, 10
    q = prime(cref, 45, log_n)
    log_b, d = [(6, -(-45 // 6)), (5, 4)][which]
    calls = DG_POOL // (d * n)
    ctx = fhe.NttContext(q)
    base_sid = 3000 + 100 * which + (t % 89) * 1000
    sk0 = fhe.sample_dg(q, SD, NS, rng, base_sid, like, (n,))
    sk1 = fhe.sample_dg(q, SD, NS, rng, base_sid + 1, like, (n,)) if t == 0 else None
    keys = [fhe.rlwe_ksk_gen(ctx, log_b, d, sk0, sk1, t, n, rng, base_sid + i) for i in range(calls)]
    a, b = torch_cuda.stack([k[0] for k in keys]), torch_cuda.stack([k[1] for k in keys])
    check_mask(torch_cuda, a, q)
    src = host(sk1) if t == 0 else cref.automorphism(q, t, host(sk0))
    neg = K.sub_mod(q, np.zeros(n, dtype=np.uint64), src)
    term = np.tile(terms_of(q, neg[None], K.gadget_bases(q, log_b, d))[0], (calls, 1, 1)).reshape(-1, n)
    check_dg("rlwe_ksk_gen t=%d (%d, %d)" % (t, log_b, d), K.rlwe_residual(q, host(sk0), host(a).reshape(-1, n), host(b).reshape(-1, n), pt=term))
    if t == 0 and which == 1:  # (e)
        xa, xb = fhe.rlwe_ksk_gen(ctx, log_b, d, host(sk0), host(sk1), 0, n, rng, base_sid)
        assert np.array_equal(xa, host(keys[0][0])) and np.array_equal(xb, host(keys[0][1]))


@pytest.mark.parametrize("a_rows_one", [True, False])
def test_rlwe_share_encrypt_rows(fhe, cref, torch_cuda, rng, like, a_rows_one):
    """rlwe.rs:237-249: the mask is the caller's -- one polynomial for every row, or one per row"""
    n, log_n, rows = 256, 8, 256
    q = prime(cref, 45, log_n)
    sid = 3900 + a_rows_one
    ctx = fhe.NttContext(q)
    sk = fhe.sample_dg(q, SD, NS, rng, sid, like, (n,))
    a = fhe.sample_uniform(q, rng, sid, like, (1 if a_rows_one else rows, n))
    pt = rand_mod(sid, q, (rows, n))
    b = fhe.rlwe_share_encrypt(ctx, a, sk, dev(torch_cuda, pt), n, rows, rng, sid)
    ha = np.tile(host(a), (rows, 1)) if a_rows_one else host(a)
    check_dg("rlwe_share_encrypt a_rows=%s" % ("1" if a_rows_one else "rows"), K.rlwe_residual(q, host(sk), ha, host(b), pt))
    if a_rows_one:
        z = fhe.rlwe_share_encrypt(ctx, a, sk, None, n, 2, rng, sid)      # pt NULL: the same noise, no plaintext
        assert np.array_equal(K.rlwe_residual(q, host(sk), ha[:2], host(z)), K.rlwe_residual(q, host(sk), ha[:2], host(b)[:2], pt[:2]))
        assert np.array_equal(fhe.rlwe_share_encrypt(ctx, host(a), host(sk), pt[:2].copy(), n, 2, rng, sid), host(b)[:2])   # (e)


def test_rlwe_and_rgsw_pk_encrypt_rows(fhe, cref, torch_cuda, rng, like):
    """rlwe.rs:158-170 / rgsw.rs:75-83: under sk the phase is e u + e1 - e0 s, bounded as test_reference_multi_key_encrypt_decrypt
    bounds it; no two ciphertexts share it; the RGSW rows carry base_j pt exactly where rgsw.rs:100-103 puts it"""
    n, log_n, batch, log_b, d, count = 256, 8, 16, 5, 4, 2
    q = prime(cref, 45, log_n)
    bound = DG_MAX * DG_MAX * n + DG_MAX + DG_MAX * n
    ctx = fhe.NttContext(q)
    sk = fhe.sample_dg(q, SD, NS, rng, 4000, like, (n,))
    za, zb = fhe.rlwe_sk_encrypt(ctx, sk, None, n, 1, rng, 4000)
    pk_a, pk_b = za[0].contiguous(), zb[0].contiguous()
    pt = rand_mod(4000, q, (batch, n))
    a, b = fhe.rlwe_pk_encrypt(ctx, pk_a, pk_b, dev(torch_cuda, pt), n, batch, rng, 4001)
    check_mask(torch_cuda, a, q)
    ph = K.rlwe_residual(q, host(sk), host(a), host(b), pt)
    assert 0 < int(np.abs(ph).max()) <= bound
    corr = K.rows_independent(ph)
    gpt = rand_mod(4002, q, (count, n))
    gpt[0] = 0
    gpt[0, 3] = q - 1
    ra, rb = fhe.rgsw_pk_encrypt(ctx, log_b, d, pk_a, pk_b, dev(torch_cuda, gpt), n, rng, 4002)
    ha, hb, t = host(ra).reshape(count, 2 * d, n), host(rb).reshape(count, 2 * d, n), terms_of(q, gpt, K.gadget_bases(q, log_b, d))
    top = K.rlwe_residual(q, host(sk), ha[:, :d].reshape(-1, n), hb[:, :d].reshape(-1, n), on_a=t.reshape(-1, n))
    bot = K.rlwe_residual(q, host(sk), ha[:, d:].reshape(-1, n), hb[:, d:].reshape(-1, n), pt=t.reshape(-1, n))
    both = np.concatenate([top, bot])
    assert 0 < int(np.abs(both).max()) <= bound
    print("FIG rlwe_pk_encrypt / rgsw_pk_encrypt: max |phase| %d, %d (bound %d), worst |corr| %.3f, %.3f"
          % (np.abs(ph).max(), np.abs(both).max(), bound, corr, K.rows_independent(both)))
    xa, xb = fhe.rlwe_pk_encrypt(ctx, host(pk_a), host(pk_b), pt, n, batch, rng, 4001)   # (e)
    assert np.array_equal(xa, host(a)) and np.array_equal(xb, host(b))
    xa, xb = fhe.rgsw_pk_encrypt(ctx, log_b, d, host(pk_a), host(pk_b), gpt, n, rng, 4002)
    assert np.array_equal(xa.reshape(ha.shape), ha) and np.array_equal(xb.reshape(hb.shape), hb)


# ---- LWE over Z_q -----------------------------------------------------------------------------------------------------------

LWE_N = 33
LWE_MODULI = [(1 << 16, 4, 4), (12289, 4, 3), (None, 7, 4)]   # (q, log_b, d): rounding bits 0, 2, 0; None = a 28-bit prime


def lwe_q(cref, q):
    return q if q is not None else cref.two_adic_primes(28, 10, 1)[0]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_lwe_sk_encrypt_rows(fhe, cref, torch_cuda, rng, like, which):
    """lwe.rs:128-139 over a power of two, a small prime and a 28-bit prime; one noise value per row"""
    q, n, rows, sid = lwe_q(cref, LWE_MODULI[which][0]), LWE_N, DG_POOL, 5000 + which
    sk = fhe.sample_dg(q, SD, NS, rng, sid, like, (n,))
    pt = rand_mod(sid, q, (rows,))
    a, b = fhe.lwe_sk_encrypt(q, sk, dev(torch_cuda, pt), n, rows, rng, sid)
    check_mask(torch_cuda, a, q)
    check_dg("lwe_sk_encrypt q=%d" % q, K.lwe_residual(q, host(sk), host(a), host(b), pt).reshape(-1, 1))
    if which == 1:  # pt NULL and (e), at 64 rows
        za, zb = fhe.lwe_sk_encrypt(q, sk, None, n, 64, rng, sid)
        da, db = fhe.lwe_sk_encrypt(q, sk, dev(torch_cuda, pt[:64]), n, 64, rng, sid)
        assert np.array_equal(host(za), host(da)) and np.array_equal(K.lwe_residual(q, host(sk), host(za), host(zb)), K.lwe_residual(q, host(sk), host(da), host(db), pt[:64]))
        xa, xb = fhe.lwe_sk_encrypt(q, host(sk), pt[:64].copy(), n, 64, rng, sid)
        assert np.array_equal(xa, host(da)) and np.array_equal(xb, host(db))


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_lwe_ksk_gen_rows(fhe, cref, torch_cuda, rng, like, which, share):
    """lwe.rs:108-119 / 214-226: digit-major rows r = j n1 + i carrying -sk1[i] base_j, the base by repeated doubling -- every
    (r / n1, r % n1) term; `share`: the same on the caller's masks (fhe_lwe_ksk_share_gen)"""
    q0, log_b, d = LWE_MODULI[which]
    q, n0, sid = lwe_q(cref, q0), LWE_N, 5100 + 10 * which + share
    n1 = -(-DG_POOL // d)
    sk0 = fhe.sample_dg(q, SD, NS, rng, sid, like, (n0,))
    sk1 = fhe.sample_dg(q, SD, NS, rng, sid + 100, like, (n1,))
    if share:
        a = fhe.sample_uniform(q, rng, sid, like, (n1 * d, n0))
        b = fhe.lwe_ksk_share_gen(q, log_b, d, a, sk0, sk1, rng, sid)
    else:
        a, b = fhe.lwe_ksk_gen(q, log_b, d, sk0, sk1, rng, sid)
        check_mask(torch_cuda, a, q)
    res = K.lwe_residual(q, host(sk0), host(a), host(b), K.lwe_ksk_terms(q, log_b, d, host(sk1)))
    check_dg("lwe_ksk_%sgen q=%d (%d, %d)" % ("share_" if share else "", q, log_b, d), res.reshape(d, n1))
    if which == 1:  # (e), at n1 = 8
        s1 = sk1[:8].contiguous()
        if share:
            crs = a[:8 * d].contiguous()
            assert np.array_equal(fhe.lwe_ksk_share_gen(q, log_b, d, host(crs), host(sk0), host(s1), rng, sid), host(fhe.lwe_ksk_share_gen(q, log_b, d, crs, sk0, s1, rng, sid)))
        else:
            (xa, xb), (da, db) = fhe.lwe_ksk_gen(q, log_b, d, host(sk0), host(s1), rng, sid), fhe.lwe_ksk_gen(q, log_b, d, sk0, s1, rng, sid)
            assert np.array_equal(xa, host(da)) and np.array_equal(xb, host(db))


def test_lwe_share_encrypt_rows(fhe, cref, torch_cuda, rng, like):
    """lwe.rs:169-183 on the caller's masks"""
    q, n, rows, sid = 1 << 16, LWE_N, DG_POOL, 5200
    sk = fhe.sample_dg(q, SD, NS, rng, sid, like, (n,))
    a = fhe.sample_uniform(q, rng, sid, like, (rows, n))
    pt = rand_mod(sid, q, (rows,))
    b = fhe.lwe_share_encrypt(q, a, sk, dev(torch_cuda, pt), n, rng, sid)
    check_dg("lwe_share_encrypt", K.lwe_residual(q, host(sk), host(a), host(b), pt).reshape(-1, 1))
    small = fhe.lwe_share_encrypt(q, a[:64].contiguous(), sk, dev(torch_cuda, pt[:64]), n, rng, sid)
    assert np.array_equal(fhe.lwe_share_encrypt(q, host(a)[:64].copy(), host(sk), pt[:64].copy(), n, rng, sid), host(small))   # (e)


# ---- CKKS -------------------------------------------------------------------------------------------------------------------

def ckks_shape(cref, small):
    if small:    # n = 64, 3 + 2 limbs of mixed widths
        return 64, [prime(cref, 60, 6), prime(cref, 50, 6), prime(cref, 45, 6)], [prime(cref, 62, 6), prime(cref, 55, 6)]
    p60 = cref.two_adic_primes(60, 13, 3)
    return 4096, p60[:2], p60[2:]


def check_ckks(name, torch, mods, a, res):
    """one integer noise on every limb; (d) per limb; (a) .. (c) on that integer"""
    for l, m in enumerate(mods):
        check_mask(torch, a[:, l], m)
        assert np.array_equal(res[l], res[0]), (name, "limb %d disagrees with limb 0" % l)
    check_dg(name, res[0])


@pytest.mark.parametrize("extended", [0, 1])
@pytest.mark.parametrize("small", [True, False])
def test_ckks_sk_encrypt_rows(fhe, cref, torch_cuda, rng, like, small, extended):
    """ckks.rs:215-225: b + a s - pt is the same small integer polynomial on every limb of qs (and of qs ++ ps)"""
    n, qs, ps = ckks_shape(cref, small)
    mods = qs + ps if extended else qs
    batch, sid = DG_POOL // n, 6000 + 10 * small + extended
    rns = fhe.RnsContext(qs, ps)
    sk = fhe.sample_zo(0.5, rng, sid, like, n)
    pt = np.stack([rand_mod(sid + l, m, (batch, n)) for l, m in enumerate(mods)], axis=1)
    b, a = rns.sk_encrypt(sk, dev(torch_cuda, pt), n, batch, rng, sid, extended=bool(extended))
    check_ckks("ckks_sk_encrypt n=%d extended=%d" % (n, extended), torch_cuda, mods, a, K.ckks_residual(mods, host(sk).view(np.int64), host(b), host(a), pt))
    if small and not extended:  # (e)
        xb, xa = rns.sk_encrypt(host(sk), pt, n, batch, rng, sid)
        assert np.array_equal(xb, host(b)) and np.array_equal(xa, host(a))


@pytest.mark.parametrize("form", ["square", "rotated", "given"])
@pytest.mark.parametrize("small", [True, False])
def test_ckks_ksk_gen_rows(fhe, cref, torch_cuda, rng, like, small, form):
    """ckks.rs:154-183: an encryption of P sk' over qs ++ ps -- sk' the square of sk (NULL), sk(X^5), or any polynomial given; the
    gadget term is (P mod q_l) sk' on the q-limbs and exactly zero on the p-limbs; one call makes one ciphertext, so a pool is
    many calls on consecutive stream ids"""
    n, qs, ps = ckks_shape(cref, small)
    mods, calls = qs + ps, DG_POOL // n
    base_sid = 6100 + 10000 * (1 + ["square", "rotated", "given"].index(form)) + 100000 * small
    rns = fhe.RnsContext(qs, ps)
    sk = fhe.sample_zo(0.5, rng, base_sid, like, n)
    s = host(sk).view(np.int64)
    big = prime(cref, 62, 13)
    if form == "square":
        spr, arg = K.centre(K.rq_mul_rows(big, np.mod(s, big).astype(np.uint64)[None], np.mod(s, big).astype(np.uint64))[0], big), None
    elif form == "rotated":
        spr = K.centre(cref.automorphism(big, 5, np.mod(s, big).astype(np.uint64)), big)
        arg = dev(torch_cuda, spr.view(np.uint64))
    else:
        spr = np.random.Generator(np.random.PCG64(base_sid)).integers(-(1 << 20), 1 << 20, size=n)
        arg = dev(torch_cuda, spr.view(np.uint64))
    keys = [rns.ksk_gen(sk, arg, n, rng, base_sid + i) for i in range(calls)]
    b, a = torch_cuda.stack([k[0] for k in keys]), torch_cuda.stack([k[1] for k in keys])
    big_p = 1
    for p in ps:
        big_p *= p
    term = np.stack([K.scalar_mul_mod(m, np.mod(spr, m).astype(np.uint64), big_p % m) for m in mods])
    assert not term[len(qs):].any() and term[:len(qs)].any(axis=1).all()
    pt = np.tile(term[None], (calls, 1, 1))
    check_ckks("ckks_ksk_gen n=%d sk'=%s" % (n, form), torch_cuda, mods, a, K.ckks_residual(mods, s, host(b), host(a), pt))
    if small and form == "given":  # (e)
        xb, xa = rns.ksk_gen(host(sk), spr.view(np.uint64), n, rng, base_sid)
        assert np.array_equal(xb, host(keys[0][0])) and np.array_equal(xa, host(keys[0][1]))


# ---- the torus --------------------------------------------------------------------------------------------------------------

GADGETS = [(7, 3), (23, 1)]
TN = 512


@pytest.mark.parametrize("sd", [2.0 ** -30, 2.0 ** -20])
def test_tlwe_sk_encrypt_rows(fhe, torch_cuda, rng, like, sd):
    """tlwe.rs:122-132 at n = 512: one noise value per row, so the pool is 16 calls of 2^14 rows on consecutive stream ids"""
    n, rows, calls = TN, 1 << 14, TDG_POOL >> 14
    sid = 7000 + (sd > 2.0 ** -25) * 100
    sk = fhe.sample_binary(rng, sid, like, n)
    s, res = host(sk), []
    for c in range(calls):
        pt = rand64(sid + c, (rows,))
        a, b = fhe.tlwe_sk_encrypt(sk, dev(torch_cuda, pt), n, rows, sd, rng, sid + c)
        check_mask(torch_cuda, a)
        res.append(K.tlwe_residual(s, host(a), host(b), pt))
    check_tdg("tlwe_sk_encrypt sd=2^%d" % int(np.log2(sd)), np.stack(res), sd)
    pt = rand64(sid, (64,))
    xa, xb = fhe.tlwe_sk_encrypt(s, pt, n, 64, sd, rng, sid + 50)               # (e)
    da, db = fhe.tlwe_sk_encrypt(sk, dev(torch_cuda, pt), n, 64, sd, rng, sid + 50)
    assert np.array_equal(xa, host(da)) and np.array_equal(xb, host(db))


@pytest.mark.parametrize("log_b,d", GADGETS)
def test_tlwe_ksk_gen_rows(fhe, torch_cuda, rng, like, log_b, d):
    """tlwe.rs:100-111 under a 512-bit key: row r = j n1 + i carries -sk1[i] 2^(64 - log_b d + j log_b)"""
    n0, sd = TN, 2.0 ** -25
    n1 = -(-8192 // d)
    calls = -(-TDG_POOL // (n1 * d))
    sid = 7200 + log_b
    sk0 = fhe.sample_binary(rng, sid, like, n0)
    res = []
    for c in range(calls):
        sk1 = fhe.sample_binary(rng, sid + 1 + c, like, n1)
        a, b = fhe.tlwe_ksk_gen(log_b, d, sk0, sk1, sd, rng, sid + c)
        check_mask(torch_cuda, a)
        res.append(K.tlwe_residual(host(sk0), host(a), host(b), K.tlwe_ksk_terms(log_b, d, host(sk1))).reshape(d, n1))
    check_tdg("tlwe_ksk_gen (%d, %d)" % (log_b, d), np.concatenate(res), sd)
    s1 = sk1[:8].contiguous()   # (e), at n1 = 8
    (xa, xb), (da, db) = fhe.tlwe_ksk_gen(log_b, d, host(sk0), host(s1), sd, rng, sid), fhe.tlwe_ksk_gen(log_b, d, sk0, s1, sd, rng, sid)
    assert np.array_equal(xa, host(da)) and np.array_equal(xb, host(db))


def test_tglwe_sk_encrypt_rows(fhe, torch_cuda, rng, like):
    """tglwe.rs:91-103 (k = 1) at n = 512, with and without a plaintext"""
    n, rows, sd, sid = TN, TDG_POOL // TN, 2.0 ** -30, 7400
    t = fhe.TorusContext()
    sk = fhe.sample_binary(rng, sid, like, n)
    pt = rand64(sid, (rows, n))
    a, b = fhe.tglwe_sk_encrypt(t, sk, dev(torch_cuda, pt), n, rows, sd, rng, sid)
    check_mask(torch_cuda, a)
    res = K.tglwe_residual(host(sk), host(a), host(b), pt)
    check_tdg("tglwe_sk_encrypt", res, sd)
    za, zb = fhe.tglwe_sk_encrypt(t, sk, None, n, 2, sd, rng, sid)            # pt NULL: the same draws without a plaintext
    da, db = fhe.tglwe_sk_encrypt(t, sk, dev(torch_cuda, pt[:2]), n, 2, sd, rng, sid)
    assert np.array_equal(host(za), host(da)) and np.array_equal(K.tglwe_residual(host(sk), host(za), host(zb)), K.tglwe_residual(host(sk), host(da), host(db), pt[:2]))
    xa, xb = fhe.tglwe_sk_encrypt(t, host(sk), pt[:2].copy(), n, 2, sd, rng, sid)   # (e)
    assert np.array_equal(xa, host(da)) and np.array_equal(xb, host(db))


@pytest.mark.parametrize("log_b,d", GADGETS)
def test_tggsw_encrypt_rows(fhe, torch_cuda, rng, like, log_b, d):
    """tggsw.rs:73-88 (k = 1): rows j < d carry pt 2^(64 - log_b d + j log_b) on a, rows d + j on b"""
    n, sd, sid = TN, 2.0 ** -20, 7500 + log_b
    count = -(-TDG_POOL // (2 * d * n))
    t = fhe.TorusContext()
    sk = fhe.sample_binary(rng, sid, like, n)
    pt = rand64(sid, (count, n))
    pt[0] = 0
    pt[0, 0] = 1                                                                # the constant 1 a bootstrapping key encrypts
    ra, rb = fhe.tggsw_encrypt(t, log_b, d, sk, dev(torch_cuda, pt), n, sd, rng, sid)
    check_mask(torch_cuda, ra[:, d:])
    ha, hb = host(ra).reshape(count, 2 * d, n), host(rb).reshape(count, 2 * d, n)
    term = np.stack([K.torus_shift(pt, 64 - log_b * d + j * log_b) for j in range(d)], axis=1)   # [count][d][n]
    top = K.tglwe_residual(host(sk), ha[:, :d].reshape(-1, n), hb[:, :d].reshape(-1, n), on_a=term.reshape(-1, n)).reshape(count, d, n)
    bot = K.tglwe_residual(host(sk), ha[:, d:].reshape(-1, n), hb[:, d:].reshape(-1, n), pt=term.reshape(-1, n)).reshape(count, d, n)
    check_tdg("tggsw_encrypt (%d, %d)" % (log_b, d), np.concatenate([top, bot], axis=1).reshape(-1, n), sd)
    xa, xb = fhe.tggsw_encrypt(t, log_b, d, host(sk), pt[:1].copy(), n, sd, rng, sid)     # (e), one plaintext
    da, db = fhe.tggsw_encrypt(t, log_b, d, sk, dev(torch_cuda, pt[:1]), n, sd, rng, sid)
    assert np.array_equal(xa, host(da)) and np.array_equal(xb, host(db))


@pytest.mark.parametrize("k,n,log_b,d", [(1, 512, 7, 3), (2, 512, 23, 1), (3, 64, 7, 3)])
def test_rank_k_rows(fhe, torch_cuda, rng, like, k, n, log_b, d):
    """tglwe.rs:91-103 and tggsw.rs:73-88 at rank k: ciphertexts [k + 1][n]; TGGSW rows [(k + 1) d][k + 1][n], the message on
    component row / d and every other mask component of that row a pure mask (distinct uniform words the exact product consumes
    as they are: a stray term on any of them would leave the noise far outside its support)"""
    sd, sid = 2.0 ** -25, 7700 + 10 * k
    t = fhe.TorusContext()
    sk = fhe.sample_binary(rng, sid, like, k * n)
    s = host(sk).reshape(k, n)
    rows = TDG_POOL // n
    pt = rand64(sid, (rows, n))
    ct = fhe.tglwek_sk_encrypt(t, k, sk, dev(torch_cuda, pt), n, rows, sd, rng, sid)
    check_mask(torch_cuda, ct[:, :k])
    check_tdg("tglwek_sk_encrypt k=%d n=%d" % (k, n), K.tglwek_residual(k, s, host(ct), pt), sd)
    xct = fhe.tglwek_sk_encrypt(t, k, host(sk), pt[:2].copy(), n, 2, sd, rng, sid)   # (e)
    assert np.array_equal(xct, host(fhe.tglwek_sk_encrypt(t, k, sk, dev(torch_cuda, pt[:2]), n, 2, sd, rng, sid)))
    count = -(-TDG_POOL // ((k + 1) * d * n))
    gpt = rand64(sid + 1, (count, n))
    gpt[0] = 0
    gpt[0, 0] = 1
    g = fhe.tggswk_encrypt(t, k, log_b, d, sk, dev(torch_cuda, gpt), n, sd, rng, sid + 1)
    hg = host(g).reshape(count, k + 1, d, k + 1, n)
    term = np.stack([K.torus_shift(gpt, 64 - log_b * d + j * log_b) for j in range(d)], axis=1).reshape(-1, n)   # [count d][n]
    res = []
    for col in range(k + 1):
        cts = hg[:, col].reshape(-1, k + 1, n)
        res.append(K.tglwek_residual(k, s, cts, pt=term) if col == k else K.tglwek_residual(k, s, cts, skip=(col, term)))
        pure = [c for c in range(k) if c != col]
        if pure:
            check_mask(torch_cuda, g.reshape(count, k + 1, d, k + 1, n)[:, col][:, :, pure])
    check_tdg("tggswk_encrypt k=%d n=%d (%d, %d)" % (k, n, log_b, d), np.concatenate(res), sd)
    xg = fhe.tggswk_encrypt(t, k, log_b, d, host(sk), gpt[:1].copy(), n, sd, rng, sid + 1)   # (e), one plaintext
    assert np.array_equal(xg, host(fhe.tggswk_encrypt(t, k, log_b, d, sk, dev(torch_cuda, gpt[:1]), n, sd, rng, sid + 1)))


# ---- the samplers' tails, edge moduli, and the grid-stride loops ------------------------------------------------------------

SENTINEL = 0x5EA15EA15EA15EA1
TAIL_COUNTS = [1, 3, 4, 5, 7, 8, 9, 511, 512, 513]


@pytest.mark.parametrize("name", ["uniform", "torus", "dg", "zo", "tdg", "binary"])
def test_sampler_tails(fhe, torch_cuda, rng, like, name):
    """a draw of `count` values is the prefix of a longer draw under the same (generator, stream id), whatever `count` leaves of
    the last generator block (4, 8 or 512 values per block), and writes nothing behind its last value"""
    q = 18014398509404161
    draw = {"uniform": lambda c, out: fhe.sample_uniform(q, rng, 8000, like, (c,), out=out),
            "torus": lambda c, out: fhe.sample_torus(rng, 8000, like, (c,), out=out),
            "dg": lambda c, out: fhe.sample_dg(q, SD, NS, rng, 8000, like, (c,), out=out),
            "zo": lambda c, out: fhe.sample_zo(0.5, rng, 8000, like, c, out=out),
            "tdg": lambda c, out: fhe.sample_tdg(2.0 ** -25, rng, 8000, like, c, out=out),
            "binary": lambda c, out: fhe.sample_binary(rng, 8000, like, c, out=out)}[name]
    full = host(draw(4096, None))
    assert len(np.unique(full)) > 1
    for count in TAIL_COUNTS:
        buf = dev(torch_cuda, np.full(count + 8, SENTINEL, dtype=np.uint64))
        got = host(draw(count, buf))
        assert np.array_equal(got[:count], full[:count]), (name, count)
        assert (got[count:] == np.uint64(SENTINEL)).all(), (name, count)
        hbuf = np.full(count + 8, SENTINEL, dtype=np.uint64)                    # host memory: the same values, the same tail
        draw(count, hbuf)
        assert np.array_equal(hbuf, got), (name, count)


def top_buckets(torch, x, q):
    """16 equal-width buckets of [0, q) on the leading bits (the last one takes what the width leaves): counts, probabilities"""
    width = q // 16 + 1
    counts = torch.bincount(torch.div(x.reshape(-1), width, rounding_mode="floor"), minlength=16).cpu().numpy()
    return counts, [width / q] * 15 + [(q - 15 * width) / q]


@pytest.mark.parametrize("q", [2, 3, 1 << 16, (1 << 62) - 57])
def test_sample_uniform_edge_moduli(fhe, cref, torch_cuda, rng, like, q):
    """the smallest moduli, a power of two and the largest prime below 2^62: in range, and flat"""
    assert q in (2, 1 << 16) or cref.is_prime(q)
    x = fhe.sample_uniform(q, rng, 8100, like, (DG_POOL,))
    assert int(x.min()) >= 0 and int(x.max()) < q
    if q <= 3:
        counts, probs = torch_cuda.bincount(x, minlength=q).cpu().numpy(), [1.0 / q] * q
    else:
        counts, probs = top_buckets(torch_cuda, x, q)
    x2, dof = K.chi2_counts(counts, probs)
    print("FIG sample_uniform q=%d: X^2 = %.1f (dof %d, bound %.1f)" % (q, x2, dof, K.chi2_bound(dof)))
    assert dof == min(q, 16) - 1 and K.chi2_ok(x2, dof)


def test_beyond_the_grid_cap(fhe, cref, torch_cuda, rng, like):
    """Every kernel of keygen_kernels.hpp caps its grid at 16384 x 256 threads and strides: draws of more than twice what one sweep
    covers (4 values per thread for uniform and tdg, 8 for the others), evaluated on the device.  The second sweep alone passes the
    law checks of the first, differs from it, and no value of the whole draw repeats.  The element-wise kernels under the
    encryptions stride as well: two encryptions of more than 4 194 304 elements, exact residuals around the wrap.  One buffer of
    about 0.5 GB at a time.  fhe_sample_binary makes 512 values per thread and would need 2^31 of them to stride: left out."""
    torch = torch_cuda
    sweep4, sweep8 = 16384 * 256 * 4, 16384 * 256 * 8
    q = (1 << 62) - 57

    def halves(x, sweep):
        assert x.numel() > 2 * sweep
        first, second = x[:sweep], x[sweep:2 * sweep]
        assert not torch.equal(first, second)
        return first, second

    x = fhe.sample_uniform(q, rng, 9000, like, (2 * sweep4 + 3,))
    assert int(x.min()) >= 0 and int(x.max()) < q and torch.unique(x).numel() == x.numel()
    for part in halves(x, sweep4):
        x2, dof = K.chi2_counts(*top_buckets(torch, part, q))
        print("FIG beyond cap, uniform: X^2 = %.1f (bound %.1f)" % (x2, K.chi2_bound(dof)))
        assert K.chi2_ok(x2, dof)
    del x, part
    torch.cuda.empty_cache()

    x = fhe.sample_torus(rng, 9001, like, (2 * sweep8 + 5,))
    assert torch.unique(x).numel() == x.numel()
    for part in halves(x, sweep8):
        x2, dof = K.chi2_counts(torch.bincount((part >> 60) & 15, minlength=16).cpu().numpy(), [1 / 16.0] * 16)
        print("FIG beyond cap, torus: X^2 = %.1f (bound %.1f)" % (x2, K.chi2_bound(dof)))
        assert K.chi2_ok(x2, dof)
    del x, part
    torch.cuda.empty_cache()

    x = fhe.sample_dg(0, SD, NS, rng, 9002, like, (2 * sweep8 + 5,))
    assert int(x.abs().max()) <= DG_MAX
    for part in halves(x, sweep8):
        x2, dof = K.chi2_dg(part, SD, NS)
        print("FIG beyond cap, dg: X^2 = %.1f (dof %d, bound %.1f)" % (x2, dof, K.chi2_bound(dof)))
        assert K.chi2_ok(x2, dof)
    del x, part
    torch.cuda.empty_cache()

    x = fhe.sample_zo(0.5, rng, 9003, like, 2 * sweep8 + 5)
    assert int(x.abs().max()) == 1
    for part in halves(x, sweep8):
        x2, dof = K.chi2_counts(torch.bincount(part + 1, minlength=3).cpu().numpy(), [0.25, 0.5, 0.25])
        print("FIG beyond cap, zo: X^2 = %.1f (bound %.1f)" % (x2, K.chi2_bound(dof)))
        assert K.chi2_ok(x2, dof)
    del x, part
    torch.cuda.empty_cache()

    sd = 2.0 ** -25
    x = fhe.sample_tdg(sd, rng, 9004, like, 2 * sweep8 + 5)
    assert float(x.abs().max()) <= 8.58 * sd * T64 + 1
    for part in halves(x, sweep8):
        dist = K.ks_normal(part.to(torch.float64), sd * T64)
        print("FIG beyond cap, tdg: D = %.2e (bound %.2e)" % (dist, K.ks_bound(part.numel())))
        assert K.ks_ok(dist, part.numel())
    del x, part
    torch.cuda.empty_cache()

    def around(total_rows, per_row):
        wrap = (16384 * 256) // per_row
        return sorted({0, 1, wrap, total_rows - 2, total_rows - 1})

    n, batch = 2048, 2100
    q45 = prime(cref, 45, 11)
    ctx = fhe.NttContext(q45)
    sk = fhe.sample_dg(q45, SD, NS, rng, 9005, like, (n,))
    pt = dev(torch, rand_mod(9005, q45, (batch, n)))
    a, b = fhe.rlwe_sk_encrypt(ctx, sk, pt, n, batch, rng, 9005)
    assert n * batch > 16384 * 256 and int(a.max()) < q45
    pick = around(batch, n)
    res = K.rlwe_residual(q45, host(sk), host(a[pick]), host(b[pick]), host(pt[pick]))
    assert int(np.abs(res).max()) <= DG_MAX
    K.rows_independent(res)
    del a, b, pt

    n, batch = 4096, 350
    qs = cref.two_adic_primes(60, 13, 4)
    rns = fhe.RnsContext(qs[:3], qs[3:])
    sk = fhe.sample_zo(0.5, rng, 9006, like, n)
    pt = torch.stack([dev(torch, rand_mod(9006 + l, m, (batch, n))) for l, m in enumerate(qs[:3])], dim=1).contiguous()
    b, a = rns.sk_encrypt(sk, pt, n, batch, rng, 9006)
    assert 3 * n * batch > 16384 * 256
    pick = around(batch, 3 * n)
    res = K.ckks_residual(qs[:3], host(sk).view(np.int64), host(b[pick]), host(a[pick]), host(pt[pick]))
    assert int(np.abs(res).max()) <= DG_MAX and np.array_equal(res[1], res[0]) and np.array_equal(res[2], res[0])
    K.rows_independent(res[0])
