"""tests/keygen_checks.py against itself: every check passes on numpy's own draws from the law it tests, seed after seed, and every
check rejects each of the faults it exists for.  No GPU.

Worst honest figures over the 1000 seeds below (PCG64(seed), seed = 0 .. 999):
  chi2_dg, 2^16 draws of dg(3.2, 6), dof 24, bound 65.57:     X^2 = 48.3
  ks_normal, 2^18 draws of N(0, 2^34), bound 3/sqrt(N) 5.86e-3: D = 3.56e-3 (D sqrt(N) = 1.82; the asymptotic tail
      2 exp(-2 * 3^2) = 3.0e-8 of the bound is the derivation, this is the measurement that it is not tight the wrong way)
  rows_independent, 66 rows of 256 dg draws, bound 6/sqrt(256) = 0.375: |corr| = 0.31
"""
import numpy as np
import pytest

import keygen_checks as K

SD, NS = 3.2, 6
SEEDS = 1000


def dg_draw(rng, count, std_dev=SD, n_sigma=NS):
    mx = K.dg_max(std_dev, n_sigma)
    return rng.choice(np.arange(-mx, mx + 1, dtype=np.int64), size=count, p=K.dg_weights(std_dev, n_sigma))


def gen(seed):
    return np.random.Generator(np.random.PCG64(seed))


def test_dg_weights_are_the_reference_table():
    w = K.dg_weights(SD, NS)
    assert len(w) == 39 and abs(w.sum() - 1.0) < 1e-15 and np.allclose(w, w[::-1], rtol=0, atol=1e-12)
    assert abs(w[19] - 0.12419) < 1e-4 and abs(float((w * np.arange(-19, 20) ** 2).sum()) - (SD * SD + 1 / 12.0)) < 0.02


def test_chi2_passes_on_honest_draws():
    worst = 0.0
    for seed in range(SEEDS):
        x2, dof = K.chi2_dg(dg_draw(gen(seed), 1 << 16), SD, NS)
        assert dof == 24
        worst = max(worst, x2)
        assert K.chi2_ok(x2, dof), (seed, x2)
    print("worst honest X^2 over %d seeds: %.1f (bound %.1f)" % (SEEDS, worst, K.chi2_bound(24)))


def test_chi2_rejects_the_named_mutants():
    rng = gen(12345)
    count = 1 << 16
    narrow = dg_draw(rng, count, std_dev=3.1)                       # dg(3.1) in place of dg(3.2)
    shifted = dg_draw(rng, count) + 1                                # every residual off by one
    shifted = shifted[np.abs(shifted) <= 19]
    doubled = dg_draw(rng, count) + dg_draw(rng, count)             # two draws added: variance x 2
    doubled = doubled[np.abs(doubled) <= 19]
    for name, s in (("dg(3.1)", narrow), ("shifted", shifted), ("sum of two", doubled)):
        x2, dof = K.chi2_dg(s, SD, NS)
        print("%s: X^2 = %.0f, bound %.1f" % (name, x2, K.chi2_bound(dof)))
        assert not K.chi2_ok(x2, dof), name
    with pytest.raises(AssertionError):                              # and outside the support nothing is counted at all
        K.chi2_dg(np.array([0, 20] * 100), SD, NS)


def test_chi2_counts_on_uniform_buckets():
    rng = gen(7)
    counts = np.bincount(rng.integers(0, 16, size=1 << 16), minlength=16)
    assert K.chi2_ok(*K.chi2_counts(counts, [1 / 16.0] * 16))
    skew = np.bincount(rng.integers(0, 1 << 20, size=1 << 16) % 15, minlength=16)   # one bucket never hit
    assert not K.chi2_ok(*K.chi2_counts(skew, [1 / 16.0] * 16))
    assert K.chi2_counts([100, 200, 100], [0.25, 0.5, 0.25]) == (0.0, 2)


def test_ks_passes_on_honest_draws():
    count, sd = 1 << 18, 2.0 ** 34
    worst = 0.0
    for seed in range(SEEDS):
        d = K.ks_normal(gen(seed).normal(0.0, sd, size=count), sd)
        worst = max(worst, d)
        assert K.ks_ok(d, count), (seed, d)
    print("worst honest D over %d seeds: %.3e (bound %.3e)" % (SEEDS, worst, K.ks_bound(count)))


def test_ks_rejects_the_named_mutants():
    count, sd = 1 << 18, 2.0 ** 34
    rng = gen(999)
    wide = rng.normal(0.0, 1.03 * sd, size=count)                    # std_dev x 1.03
    doubled = rng.normal(0.0, sd, size=count) + rng.normal(0.0, sd, size=count)
    moved = rng.normal(0.0, sd, size=count) + 0.05 * sd
    for name, s in (("1.03 sd", wide), ("sum of two", doubled), ("shifted", moved)):
        d = K.ks_normal(s, sd)
        print("%s: D = %.4f, bound %.4f" % (name, d, K.ks_bound(count)))
        assert not K.ks_ok(d, count), name
    import torch
    x = rng.normal(0.0, sd, size=4096)
    assert K.ks_normal(torch.from_numpy(x), sd) == K.ks_normal(x, sd)   # tensors take the same path


def test_rows_independent_passes_on_honest_rows():
    worst = 0.0
    for seed in range(SEEDS):
        worst = max(worst, K.rows_independent(dg_draw(gen(seed), 66 * 256).reshape(66, 256)))
    print("worst honest |corr| over %d seeds: %.3f (bound %.3f)" % (SEEDS, worst, 6 / 16.0))
    big = dg_draw(gen(1), 200 * 1024).reshape(200, 1024)              # more than 64 rows: the subsample, still every row compared for equality
    assert 0 < K.rows_independent(big) < 6 / 32.0
    assert K.rows_independent(dg_draw(gen(2), 512 * 64).reshape(512, 64)) == 0.0   # short rows: equality and zero only
    assert K.as_rows(np.arange(1024).reshape(1024, 1)).shape == (4, 256)


def test_rows_independent_rejects_the_named_mutants():
    base = dg_draw(gen(3), 200 * 256).reshape(200, 256)
    dup = base.copy(); dup[131] = dup[7]                              # noqa: E702  a cursor that did not move
    with pytest.raises(AssertionError, match="same noise"):
        K.rows_independent(dup)
    zero = base.copy(); zero[199] = 0                                 # noqa: E702
    with pytest.raises(AssertionError, match="all-zero"):
        K.rows_independent(zero)
    mixed = base[:32].copy(); mixed[9] = mixed[4] + dg_draw(gen(4), 256)   # noqa: E702  half of a row's noise shared
    with pytest.raises(AssertionError, match="correlate"):
        K.rows_independent(mixed)
    short = dg_draw(gen(5), 4096).reshape(4096, 1)                    # scalar noise: regrouped, then a repeated stretch shows
    short[512:768] = short[0:256]
    with pytest.raises(AssertionError, match="same noise"):
        K.rows_independent(K.as_rows(short))


def test_residuals_are_exact_and_a_wrong_gadget_base_shows(cref):
    """every residual function returns exactly the noise a ciphertext was built with (built here from the oracle's products), and a
    residual computed with a gadget base off by one bit leaves the support"""
    rng = gen(11)
    n, rows, log_b, d = 64, 8, 5, 4
    q = cref.two_adic_primes(45, 7, 1)[0]
    sk = np.mod(dg_draw(rng, n), q).astype(np.uint64)
    a = rng.integers(0, q, size=(rows, n), dtype=np.uint64)
    e = dg_draw(rng, rows * n).reshape(rows, n)
    pt = rng.integers(0, q, size=n, dtype=np.uint64)
    bases = K.gadget_bases(q, log_b, d)
    assert bases == [pow(2, 45 - 20 + 5 * j, q) for j in range(d)]
    terms = np.stack([K.scalar_mul_mod(q, pt, bases[r % d]) for r in range(rows)])
    add = lambda x, y: (x.astype(object) + y.astype(object)) % q      # noqa: E731
    b = add(add(K.rq_mul_rows(q, a, sk), np.mod(e, q).astype(np.uint64)), terms).astype(np.uint64)
    assert np.array_equal(K.rlwe_residual(q, sk, a, b, pt=terms), e)
    a_on = add(a, terms).astype(np.uint64)                             # the same term on the mask: b = (a' - term) s + e
    b_on = add(K.rq_mul_rows(q, a, sk), np.mod(e, q).astype(np.uint64)).astype(np.uint64)
    assert np.array_equal(K.rlwe_residual(q, sk, a_on, b_on, on_a=terms), e)
    wrong = np.stack([K.scalar_mul_mod(q, pt, 2 * bases[r % d] % q) for r in range(rows)])   # base off by one bit
    assert np.abs(K.rlwe_residual(q, sk, a, b, pt=wrong)).max() > 19
    for small_n in (1, 2, 4):                                          # the schoolbook routes agree with Python integers
        s2, a2 = sk[:small_n], a[:, :small_n]
        want = [[sum((1 if j <= i else -1) * int(a2[r][j]) * int(s2[(i - j) % small_n]) for j in range(small_n)) % q for i in range(small_n)] for r in range(rows)]
        assert K.rq_mul_rows(q, a2, s2).tolist() == want
    # LWE over a power of two and a prime; digit-major key-switching terms
    for ql in (1 << 16, 12289, cref.two_adic_primes(28, 10, 1)[0]):
        nl, n1, kb, kd = 33, 5, 4, 3
        s0 = rng.integers(0, ql, size=nl, dtype=np.uint64)
        s1 = np.mod(dg_draw(rng, n1), ql).astype(np.uint64)
        al = rng.integers(0, ql, size=(n1 * kd, nl), dtype=np.uint64)
        el = dg_draw(rng, n1 * kd)
        t = K.lwe_ksk_terms(ql, kb, kd, s1)
        assert int(t[n1 + 2]) == (-int(s1[2]) * K.gadget_bases(ql, kb, kd)[1]) % ql
        bl = np.array([(sum(int(x) * int(y) for x, y in zip(al[r], s0)) + int(el[r]) + int(t[r])) % ql for r in range(n1 * kd)], dtype=np.uint64)
        assert np.array_equal(K.lwe_residual(ql, s0, al, bl, pt=t), el)
        assert np.abs(K.lwe_residual(ql, s0, al, bl, pt=K.scalar_mul_mod(ql, t, 2))).max() > 19      # every base off by one bit
    # torus, rank 2: the body and a term on one mask
    k, nt = 2, 16
    skt = rng.integers(0, 2, size=(k, nt), dtype=np.uint64)
    ct = rng.integers(0, 1 << 63, size=(3, k + 1, nt), dtype=np.uint64) * np.uint64(2)
    et = rng.normal(0, 2.0 ** 40, size=(3, nt)).astype(np.int64)
    msg = rng.integers(0, 1 << 62, size=(3, nt), dtype=np.uint64)
    body = et.view(np.uint64) + msg
    for c in range(k):
        for r in range(3):
            body[r] += cref.torus_mul_exact(ct[r, c], skt[c])
    ct[:, k] = body
    assert np.array_equal(K.tglwek_residual(k, skt, ct, pt=msg), et)
    on1 = ct.copy(); on1[:, 1] += msg; on1[:, k] -= msg               # noqa: E702
    assert np.array_equal(K.tglwek_residual(k, skt, on1, skip=(1, msg)), et)
    assert np.abs(K.tglwek_residual(k, skt, on1, skip=(0, msg))).max() > 2.0 ** 50
    # CKKS: one integer noise on every limb
    mods = cref.two_adic_primes(50, 7, 2) + cref.two_adic_primes(36, 7, 1)
    skc = rng.integers(-1, 2, size=n)
    ac = np.stack([rng.integers(0, m, size=(2, n), dtype=np.uint64) for m in mods], axis=1)
    ec = dg_draw(rng, 2 * n).reshape(2, n)
    ptc = np.stack([rng.integers(0, m, size=(2, n), dtype=np.uint64) for m in mods], axis=1)
    sl = cref.rns_from_i64(mods, skc)
    bc = np.stack([np.stack([(np.mod(ec[r], m).astype(object) + ptc[r, l].astype(object) - cref.ntt_mul(m, ac[r, l], sl[l], n).astype(object)) % m
                             for l, m in enumerate(mods)]) for r in range(2)]).astype(np.uint64)
    res = K.ckks_residual(mods, skc, bc, ac, ptc)
    assert res.shape == (3, 2, n) and all(np.array_equal(res[l], ec) for l in range(3))
