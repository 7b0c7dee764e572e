"""FHEW gadget products and blind rotation at every ring size (the composed route, fhew_composed_kernels.hpp): bit-exact against
the oracle outside N = 128 .. 2048, bit-identical to the fused kernels inside it (lab switch FHEW_COMPOSED), and the reference's
RGSW / RLWE tests (rgsw.rs:164-227, rlwe.rs:379-416: testing_n_q(0..10, 45)) replayed at decrypt level."""
import random
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = lambda x: [int(v) for v in np.asarray(x).ravel()]  # noqa: E731
WS_BYTES = 256 << 20  # fhew_api.hip COMPOSED_WS_BYTES: the composed route's workspace per call


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


def chunk_of(rows, n):
    """ciphertexts per chunk of the composed route (fhew_api.hip composed_run)"""
    return max(1, WS_BYTES // ((rows + 3) * n * 8))


def step_bound(n, n_lwe, w):
    """the host loop's step count of a composed blind rotation (fhew_api.hip fhe_blind_rotate)"""
    lv = n // 2 - 1
    return min(n_lwe + 2 * (min(n_lwe, lv) + lv // w + 1) + 1, n_lwe + n + 2)


class Composed:
    """FHEW keys prepared inside the block run the composed route at every size"""

    def __init__(self, fhe):
        self.fhe = fhe

    def __enter__(self):
        self.fhe.set_option("FHEW_COMPOSED", 1)

    def __exit__(self, *exc):
        self.fhe.set_option("FHEW_COMPOSED", 0)


def _keys(fhe, torch, q, n, log_b, d, count, seed, mem="dev"):
    ctx = fhe.NttContext(q)
    ra, rb = rand_u64(seed, q, (count, 2 * d, n)), rand_u64(seed + 1, q, (count, 2 * d, n))
    ka, kb = rand_u64(seed + 2, q, (count, d, n)), rand_u64(seed + 3, q, (count, d, n))
    put = (lambda x: dev(torch, x)) if mem == "dev" else (lambda x: x)
    rgsw = fhe.GadgetKey(ctx, log_b, d, put(ra), put(rb), n, rgsw=True)
    ksk = fhe.GadgetKey(ctx, log_b, d, put(ka), put(kb), n, rgsw=False)
    return ctx, rgsw, ksk, ra, rb, ka, kb


SIZES = [0, 1, 2, 3, 4, 5, 6, 12, 13, 14, 17]


@pytest.mark.parametrize("log_n", SIZES)
@pytest.mark.parametrize("bits,log_b,d", [(45, 5, 9), (61, 12, 5)])
def test_gadget_products_vs_oracle(fhe, cref, torch_cuda, log_n, bits, log_b, d):
    """external / internal product, key switch, automorphism (t = 5, -5, 2N + 3) at N outside 128 .. 2048, batches 1, 3 and 37,
    device and host memory, every ciphertext (large N: the first, middle and last of each batch) against the oracle"""
    torch = torch_cuda
    n = 1 << log_n
    q = cref.two_adic_primes(bits, log_n + 1, 1)[0]
    ctx, rgsw, ksk, ra, rb, ka, kb = _keys(fhe, torch, q, n, log_b, d, 2, seed=10 * log_n + bits)
    ctx_h, rgsw_h, ksk_h, *_ = _keys(fhe, torch, q, n, log_b, d, 2, seed=10 * log_n + bits, mem="host")
    for batch in (1, 3, 37):
        ca, cb = rand_u64(batch, q, (batch, n)), rand_u64(batch + 1, q, (batch, n))
        ca[0, :min(n, 4)] = [0, q - 1, q >> 1, (q >> 1) + 1][:min(n, 4)]
        check = range(batch) if n <= 64 else (sorted({0, batch // 2, batch - 1}) if log_n <= 14 else [batch - 1])
        want = {}
        for kind, t in [("ep", 1), ("ks", 1), ("auto", 5), ("auto", -5), ("auto", 2 * n + 3)]:
            idx = 1 if kind != "ks" else 0
            for mem in (("dev", "host") if batch == 3 else ("dev",)):
                if mem == "dev":
                    a, b = dev(torch, ca), dev(torch, cb)
                    key = rgsw if kind == "ep" else ksk
                else:
                    a, b = ca.copy(), cb.copy()
                    key = rgsw_h if kind == "ep" else ksk_h
                if kind == "ep":
                    key.external_product_(idx, a, b)
                elif kind == "ks":
                    key.key_switch_(idx, a, b)
                else:
                    key.automorphism_(idx, t, a, b)
                ha, hb = (host(a), host(b)) if mem == "dev" else (a, b)
                for i in check:
                    if (kind, t, i) not in want:
                        if kind == "ep":
                            want[kind, t, i] = cref.external_product(q, log_b, d, ra[idx], rb[idx], ca[i], cb[i])
                        elif kind == "ks":
                            want[kind, t, i] = cref.rlwe_key_switch(q, log_b, d, ka[idx], kb[idx], ca[i], cb[i])
                        else:
                            want[kind, t, i] = cref.rlwe_automorphism(q, log_b, d, t, ka[idx], kb[idx], ca[i], cb[i])
                    ea, eb = want[kind, t, i]
                    assert np.array_equal(ha[i], ea) and np.array_equal(hb[i], eb), (kind, t, batch, mem, i)
    # internal product: one external product of rgsw[0] per row of a right-hand RGSW ciphertext (two of them in one call)
    r1a, r1b = rand_u64(7, q, (2, 2 * d, n)), rand_u64(8, q, (2, 2 * d, n))
    a, b = dev(torch, r1a), dev(torch, r1b)
    rgsw.internal_product_(0, a, b)
    ha, hb = host(a).reshape(2, 2 * d, n), host(b).reshape(2, 2 * d, n)
    for c, r in ([(0, r) for r in range(2 * d)] + [(1, 0), (1, 2 * d - 1)]) if n <= 64 else [(0, 0), (1, 2 * d - 1)]:
        ea, eb = cref.external_product(q, log_b, d, ra[0], rb[0], r1a[c, r], r1b[c, r])
        assert np.array_equal(ha[c, r], ea) and np.array_equal(hb[c, r], eb), (c, r)


def test_batch_across_workspace_chunks(fhe, cref, torch_cuda):
    """N = 2^15: batches that span several chunks of the composed route's fixed workspace; the ciphertexts on both sides of every
    chunk boundary against the oracle"""
    torch = torch_cuda
    log_n, log_b, d = 15, 2, 30
    n = 1 << log_n
    q = cref.two_adic_primes(61, log_n + 1, 1)[0]
    ctx, rgsw, ksk, ra, rb, ka, kb = _keys(fhe, torch, q, n, log_b, d, 1, seed=150)
    ch_ep, ch_ks = chunk_of(2 * d, n), chunk_of(d, n)
    batch = ch_ks + 3
    assert batch > 2 * ch_ep  # external products: three chunks; key switches: two
    ca, cb = rand_u64(151, q, (batch, n)), rand_u64(152, q, (batch, n))
    a, b = dev(torch, ca), dev(torch, cb)
    rgsw.external_product_(0, a, b)
    ha, hb = host(a), host(b)
    for i in (0, ch_ep - 1, ch_ep, 2 * ch_ep - 1, 2 * ch_ep, batch - 1):
        ea, eb = cref.external_product(q, log_b, d, ra[0], rb[0], ca[i], cb[i])
        assert np.array_equal(ha[i], ea) and np.array_equal(hb[i], eb), i
    a, b = dev(torch, ca), dev(torch, cb)
    ksk.automorphism_(0, -5, a, b)
    ha, hb = host(a), host(b)
    for i in (ch_ks - 1, ch_ks, batch - 1):
        ea, eb = cref.rlwe_automorphism(q, log_b, d, -5, ka[0], kb[0], ca[i], cb[i])
        assert np.array_equal(ha[i], ea) and np.array_equal(hb[i], eb), i


def _make_bk(fhe, torch, q, n, log_b, d, ks_log_b, ks_d, w, n_lwe, seed):
    from oracle import pyref as P
    brk = rand_u64(seed, q, (n_lwe, 2, 2 * d, n))
    ak = rand_u64(seed + 1, q, (w + 1, 2, ks_d, n))
    ctx = fhe.NttContext(q)
    gk = fhe.GadgetKey(ctx, log_b, d, dev(torch, brk[:, 0]), dev(torch, brk[:, 1]), n, rgsw=True)
    ga = fhe.GadgetKey(ctx, ks_log_b, ks_d, dev(torch, ak[:, 0]), dev(torch, ak[:, 1]), n, rgsw=False)
    ts = P.ak_t(n, w)
    return ctx, fhe.BootstrapKey(ctx, gk, ga, ts, w), brk, ak, ts


@pytest.mark.parametrize("log_n", [7, 8, 9, 10, 11])
def test_route_identity_gadget_products(fhe, cref, torch_cuda, log_n):
    """N = 128 .. 2048: keys prepared with FHEW_COMPOSED give bit-identical products to the fused kernels, at a Shoup prime, cfg3's
    54-bit modulus (N >= 512: the pseudo-Mersenne policy) and a batch in every small_shape range"""
    torch = torch_cuda
    n = 1 << log_n
    primes = [(cref.two_adic_primes(45, log_n + 1, 1)[0], 5, 9), (18014398509404161, 6, 9)]
    batches = {10: (5, 800, 1100), 11: (5, 600)}.get(log_n, (5, 37))
    for q, log_b, d in primes:
        keys = {}
        for route in ("fused", "composed"):
            if route == "composed":
                with Composed(fhe):
                    keys[route] = _keys(fhe, torch, q, n, log_b, d, 2, seed=300 + log_n)
            else:
                keys[route] = _keys(fhe, torch, q, n, log_b, d, 2, seed=300 + log_n)
        for batch in batches:
            ca, cb = rand_u64(batch, q, (batch, n)), rand_u64(batch + 7, q, (batch, n))
            for kind, t in [("ep", 1), ("ks", 1), ("auto", -5)]:
                outs = []
                for route in ("fused", "composed"):
                    _, rgsw, ksk, *_ = keys[route]
                    a, b = dev(torch, ca), dev(torch, cb)
                    if kind == "ep":
                        rgsw.external_product_(1, a, b)
                    elif kind == "ks":
                        ksk.key_switch_(0, a, b)
                    else:
                        ksk.automorphism_(1, t, a, b)
                    outs.append((a, b))
                assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (q, batch, kind)
            if batch == batches[0]:
                _, _, _, ra, rb, _, _ = keys["fused"]
                a, b = dev(torch, ca), dev(torch, cb)
                keys["composed"][1].external_product_(1, a, b)
                ea, eb = cref.external_product(q, log_b, d, ra[1], rb[1], ca[0], cb[0])
                assert np.array_equal(host(a)[0], ea) and np.array_equal(host(b)[0], eb)


@pytest.mark.parametrize("q,log_n,batches", [(18014398509404161, 10, (1, 64, 800, 1100)), (35184372060161, 11, (3, 600)),
                                             (None, 7, (5,)), (None, 9, (5,))])
def test_route_identity_blind_rotate(fhe, cref, torch_cuda, q, log_n, batches):
    """blind rotations on a composed bootstrapping key are bit-identical to the fused kernel's (cfg3's ring and key shape at
    N = 1024), and the composed walk matches the oracle's"""
    torch = torch_cuda
    n, lb, d, w, n_lwe = 1 << log_n, 6, 9, 10, 12
    if q is None:
        q = cref.two_adic_primes(45, log_n + 1, 1)[0]
    ctx, bk, brk, ak, ts = _make_bk(fhe, torch, q, n, lb, d, lb, d, w, n_lwe, seed=400 + log_n)
    with Composed(fhe):
        ctx2, bk2, _, _, _ = _make_bk(fhe, torch, q, n, lb, d, lb, d, w, n_lwe, seed=400 + log_n)
        ak_c = fhe.GadgetKey(ctx, lb, d, dev(torch, ak[:, 0]), dev(torch, ak[:, 1]), n, rgsw=False)
    with pytest.raises(fhe.FheError) as e:  # brk and ak of different routes
        fhe.BootstrapKey(ctx, bk.brk, ak_c, ts, w)
    assert e.value.code == 1  # FHE_ERR_INVALID
    for batch in batches:
        rng = np.random.Generator(np.random.PCG64(batch))
        lwe_a = rng.integers(0, n, size=(batch, n_lwe), dtype=np.uint64) * 2 + 1
        lwe_a[0, :3] = 0
        lwe_b = rng.integers(0, 2 * n, size=batch, dtype=np.uint64)
        f = dev(torch, rand_u64(batch + 1, q, n))
        da, db = dev(torch, lwe_a), dev(torch, lwe_b)
        o1 = bk.blind_rotate(da, db, f)
        o2 = bk2.blind_rotate(da, db, f)
        assert torch.equal(o1[0], o2[0]) and torch.equal(o1[1], o2[1]), batch
        bk2.check(da)
    ea, eb = cref.blind_rotate(q, n, w, lb, d, lb, d, brk, ak, ts, host(f), lwe_a[-1], int(lwe_b[-1]))
    assert np.array_equal(host(o2[0])[-1], ea) and np.array_equal(host(o2[1])[-1], eb)


@pytest.mark.parametrize("log_n,w", [(1, 1), (2, 1), (3, 3), (4, 10), (5, 1), (6, 3), (6, 10), (12, 10), (13, 512), (14, 4096)])
def test_blind_rotate_vs_oracle(fhe, cref, torch_cuda, log_n, w):
    """the composed blind rotation against cref.blind_rotate: per-ciphertext and shared LUTs (f_stride N and 0), zero coefficients,
    the walk (ops_out) against the oracle's"""
    torch = torch_cuda
    n, lb, d, ks_lb, ks_d, n_lwe = 1 << log_n, 6, 3, 5, 4, 6
    q = cref.two_adic_primes(54, log_n + 1, 1)[0]
    batch = 5 if n <= 64 else 2
    ctx, bk, brk, ak, ts = _make_bk(fhe, torch, q, n, lb, d, ks_lb, ks_d, w, n_lwe, seed=500 + log_n)
    rng = np.random.Generator(np.random.PCG64(log_n))
    lwe_a = rng.integers(0, n, size=(batch, n_lwe), dtype=np.uint64) * 2 + 1
    lwe_a[0, 1] = 0
    lwe_a[-1, :] = lwe_a[-1, 0]
    lwe_b = rng.integers(0, 2 * n, size=batch, dtype=np.uint64)
    fs = rand_u64(501, q, (batch, n))
    for f_stride in (n, 0):
        f = fs if f_stride else fs[0]
        oa, ob, sched = bk.blind_rotate(dev(torch, lwe_a), dev(torch, lwe_b), dev(torch, f), want_schedule=True)
        ha, hb = host(oa), host(ob)
        for i in range(batch):
            assert sched[i] == cref.blind_rotate_schedule(n, w, lwe_a[i]), i
            assert len(sched[i]) <= step_bound(n, n_lwe, w)
            ea, eb = cref.blind_rotate(q, n, w, lb, d, ks_lb, ks_d, brk, ak, ts, f[i] if f_stride else f, lwe_a[i], int(lwe_b[i]))
            assert np.array_equal(ha[i], ea) and np.array_equal(hb[i], eb), (f_stride, i)
    ha2, hb2 = bk.blind_rotate(lwe_a[:1], lwe_b[:1], fs[0])  # host memory
    assert np.array_equal(ha2[0], ha[0]) and np.array_equal(hb2[0], hb[0])


@pytest.mark.parametrize("w", [1, 3, 64])
def test_blind_rotate_longest_walk(fhe, cref, torch_cuda, w):
    """every a_i on a level of its own, signs alternating: both halves of the walk have an occupied level at every step, the most
    automorphisms a walk can have -- the host loop's step bound must cover it"""
    torch = torch_cuda
    log_n, lb, d, ks_lb, ks_d = 6, 6, 3, 5, 4
    n = 1 << log_n
    half = n // 2
    n_lwe = 2 * (half - 1)
    q = cref.two_adic_primes(54, log_n + 1, 1)[0]
    ctx, bk, brk, ak, ts = _make_bk(fhe, torch, q, n, lb, d, ks_lb, ks_d, w, n_lwe, seed=600 + w)
    a = []
    for i in range(n_lwe):
        v = pow(5, i // 2 + 1, 2 * n)
        a.append(v if i % 2 == 0 else 2 * n - v)
    lwe_a = np.array([a, a[::-1]], dtype=np.uint64)
    lwe_b = np.array([3, 2 * n - 1], dtype=np.uint64)
    f = rand_u64(601, q, n)
    oa, ob, sched = bk.blind_rotate(dev(torch, lwe_a), dev(torch, lwe_b), dev(torch, f), want_schedule=True)
    for i in range(2):
        assert sched[i] == cref.blind_rotate_schedule(n, w, lwe_a[i])
        n_ak = sum(1 for k, _ in sched[i] if k == "ak")
        assert n_ak == 2 * (half - 1) + 1 and len(sched[i]) <= step_bound(n, n_lwe, w)
        ea, eb = cref.blind_rotate(q, n, w, lb, d, ks_lb, ks_d, brk, ak, ts, f, lwe_a[i], int(lwe_b[i]))
        assert np.array_equal(host(oa)[i], ea) and np.array_equal(host(ob)[i], eb), i


def test_bootstrap_key_needs_two_coefficients(fhe, cref, torch_cuda):
    """N = 1: gadget products work, a bootstrapping key does not (the reference panics: bootstrapping.rs:191, 215)"""
    torch = torch_cuda
    q = cref.two_adic_primes(45, 1, 1)[0]
    ctx, rgsw, ksk, *_ = _keys(fhe, torch, q, 1, 5, 9, 2, seed=700)
    with pytest.raises(fhe.FheError) as e:
        fhe.BootstrapKey(ctx, rgsw, ksk, [1, 1], 1)
    assert e.value.code == 1  # FHE_ERR_INVALID


def test_fhew_bootstrap_4096_vs_oracle(fhe, cref, torch_cuda):
    """bootstrapping.rs:149-155 at N = 4096 on the composed route, bit-exact against the oracle's steps"""
    torch = torch_cuda
    n, lb, d, w, n_lwe, batch = 4096, 6, 3, 64, 8, 2
    q = cref.two_adic_primes(54, 13, 1)[0]
    q_ks, kb, kd = 1 << 16, 4, 4
    ctx, bk, brk, ak, ts = _make_bk(fhe, torch, q, n, lb, d, 5, 4, w, n_lwe, seed=800)
    ksk_a, ksk_b = rand_u64(801, q_ks, (kd * n, n_lwe)), rand_u64(802, q_ks, kd * n)
    ct_a, ct_b = rand_u64(803, q, (batch, n)), rand_u64(804, q, batch)
    f = rand_u64(805, q, n)
    addend = q // 8
    oa, ob = bk.bootstrap(q_ks, kb, kd, dev(torch, ksk_a), dev(torch, ksk_b), dev(torch, f), dev(torch, ct_a), dev(torch, ct_b),
                          addend=addend)
    bk.check(oa)
    for i in range(batch):
        a1 = np.array([cref.mod_switch(q, int(x), q_ks) for x in ct_a[i]], dtype=np.uint64)
        b1 = cref.mod_switch(q, int(ct_b[i]), q_ks)
        a2, b2 = cref.lwe_key_switch(q_ks, kb, kd, ksk_a, ksk_b, a1, b1)
        a3 = np.array([cref.mod_switch_odd(q_ks, int(x), 2 * n) for x in a2], dtype=np.uint64)
        b3 = cref.mod_switch_odd(q_ks, int(b2), 2 * n)
        ra, rb = cref.blind_rotate(q, n, w, lb, d, 5, 4, brk, ak, ts, f, a3, b3)
        ea, eb = cref.sample_extract(q, ra, rb, 0)
        assert np.array_equal(host(oa)[i], ea) and int(host(ob)[i]) == (eb + addend) % q, i


def test_blind_rotate_4096_is_asynchronous(fhe, cref, torch_cuda):
    """device-memory blind rotations on the composed route return once their launches are enqueued (the step count is a bound
    known on the host, no device read); an even LWE coefficient reaches the key's status word, not the return value"""
    torch = torch_cuda
    n, lb, d, w, n_lwe, batch = 4096, 6, 9, 10, 16, 256
    q = cref.two_adic_primes(54, 13, 1)[0]
    ctx, bk, brk, ak, ts = _make_bk(fhe, torch, q, n, lb, d, lb, d, w, n_lwe, seed=900)
    rng = np.random.Generator(np.random.PCG64(901))
    lwe_a = dev(torch, rng.integers(0, n, size=(batch, n_lwe), dtype=np.uint64) * 2 + 1)
    lwe_b = dev(torch, rng.integers(0, 2 * n, size=batch, dtype=np.uint64))
    f = dev(torch, rand_u64(902, q, n))
    ref_a, ref_b = bk.blind_rotate(lwe_a, lwe_b, f)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    oa, ob = bk.blind_rotate(lwe_a, lwe_b, f)
    t_call = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_one = time.perf_counter() - t0
    assert t_call < 0.5 * t_one, (t_call, t_one)
    assert torch.equal(oa, ref_a) and torch.equal(ob, ref_b)
    bk.check(lwe_a)
    bad = lwe_a.clone()
    bad[1, 3] = 4
    bk.blind_rotate(bad, lwe_b, f)  # returns without an error: the check is asynchronous
    with pytest.raises(fhe.FheError):
        bk.check(bad)
    bk.check(bad)  # cleared by the previous query


# ---- the reference's RGSW / RLWE tests at decrypt level: testing_n_q(0..10, 45), p = 16, log_b 5, d 9 -------------------------


def _ref_sweep_case(fhe, torch, P, log_n, q, rnd, seed):
    p, log_b, d = 16, 5, 9
    n = 1 << log_n
    dec = P.Base2Decomposor(q, log_b, d)
    delta = q / p
    enc = lambda m: [P.zq_from_f64(q, float(x) * delta) for x in m]  # noqa: E731
    decd = lambda pt: [P.zq_from_f64(p, float(P.zq_to_i64(q, x)) / delta) for x in pt]  # noqa: E731
    U = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731
    ctx = fhe.NttContext(q)
    m0, m1, m2 = ([rnd.randrange(p) for _ in range(n)] for _ in range(3))
    if n >= 2:  # the device producers
        like = dev(torch, U([0]))
        sk_z = fhe.sample_dg(q, 3.2, 6, seed, 0, like, (n,))
        sk2_z = fhe.sample_dg(q, 3.2, 6, seed, 1, like, (n,))
        sk = [P.zq_to_i64(q, v) for v in L(host(sk_z))]
        rga, rgb = fhe.rgsw_encrypt(ctx, log_b, d, sk_z, dev(torch, U([m0, m2])), n, seed + 1, 0)
        ca, cb = fhe.rlwe_sk_encrypt(ctx, sk_z, dev(torch, U([enc(m1)])), n, 1, seed + 2, 0)
        kka, kkb = fhe.rlwe_ksk_gen(ctx, log_b, d, sk_z, sk2_z, 0, n, seed + 3, 0)
        c2a, c2b = fhe.rlwe_sk_encrypt(ctx, sk2_z, dev(torch, U([enc(m1)])), n, 1, seed + 4, 0)
        aks = [fhe.rlwe_ksk_gen(ctx, log_b, d, sk_z, None, t, n, seed + 5, i) for i, t in enumerate((5, -5))]
        rga, rgb, ca, cb, kka, kkb, c2a, c2b = (host(x) for x in (rga, rgb, ca, cb, kka, kkb, c2a, c2b))
        aks = [(host(a), host(b)) for a, b in aks]
    else:  # n = 1: the oracle's producers
        sk = [rnd.randint(-3, 3) for _ in range(n)]
        sk2 = [rnd.randint(-3, 3) for _ in range(n)]
        r0, r2 = P.rgsw_encrypt(q, dec, sk, m0, rnd), P.rgsw_encrypt(q, dec, sk, m2, rnd)
        rga, rgb = U([r0[0], r2[0]]), U([r0[1], r2[1]])
        ca, cb = (U([x]) for x in P.rlwe_sk_encrypt(q, sk, enc(m1), rnd))
        kka, kkb = (U(x) for x in P.rlwe_ksk_gen(q, dec, sk, sk2, rnd))
        c2a, c2b = (U([x]) for x in P.rlwe_sk_encrypt(q, sk2, enc(m1), rnd))
        aks = [tuple(U(x) for x in P.rlwe_ak_gen(q, dec, t, sk, rnd)) for t in (5, -5)]
    rgsw = fhe.GadgetKey(ctx, log_b, d, dev(torch, rga), dev(torch, rgb), n, rgsw=True)
    # rgsw.rs external_product: decrypt(rgsw(m0) x rlwe(m1)) == m0 m1
    a, b = dev(torch, ca), dev(torch, cb)
    rgsw.external_product_(0, a, b)
    assert decd(P.rlwe_decrypt(q, sk, L(host(a)), L(host(b)))) == P.nega_cyclic_schoolbook_mul(p, m0, m1), ("external", log_n, q)
    # rgsw.rs internal_product: rgsw(m0) x rgsw(m2), the last row decrypted at its base
    a, b = dev(torch, rga[1]), dev(torch, rgb[1])
    rgsw.internal_product_(0, a, b)
    ha, hb = host(a).reshape(2 * d, n), host(b).reshape(2 * d, n)
    last = dec.rounding_bits + (d - 1) * log_b
    phase = P.rlwe_decrypt(q, sk, L(ha[-1]), L(hb[-1]))
    got = [(((v + ((1 << last) >> 1)) % q) >> last) % p for v in phase]
    assert got == P.nega_cyclic_schoolbook_mul(p, m0, m2), ("internal", log_n, q)
    # rlwe.rs key_switch: a ciphertext under sk2 decrypts under sk afterwards
    ksk = fhe.GadgetKey(ctx, log_b, d, dev(torch, kka), dev(torch, kkb), n, rgsw=False)
    a, b = dev(torch, c2a), dev(torch, c2b)
    ksk.key_switch_(0, a, b)
    assert decd(P.rlwe_decrypt(q, sk, L(host(a)), L(host(b)))) == m1, ("key_switch", log_n, q)
    # rlwe.rs automorphism
    for (aa, ab), t in zip(aks, (5, -5)):
        ak = fhe.GadgetKey(ctx, log_b, d, dev(torch, aa), dev(torch, ab), n, rgsw=False)
        a, b = dev(torch, ca), dev(torch, cb)
        ak.automorphism_(0, t, a, b)
        assert decd(P.rlwe_decrypt(q, sk, L(host(a)), L(host(b)))) == P.automorphism(p, m1, t), ("automorphism", t, log_n, q)


@pytest.mark.parametrize("log_n", list(range(10)))
def test_reference_rgsw_rlwe_sweep(fhe, torch_cuda, log_n):
    """rgsw.rs:164-227 (external_product, internal_product) and rlwe.rs:379-416 (key_switch, automorphism) over testing_n_q(0..10, 45):
    every log_n 0 .. 9 with all ten 45-bit primes"""
    from oracle import pyref as P
    rnd = random.Random(1000 + log_n)
    primes = P.two_adic_primes(45, log_n + 1)
    for k in range(10):
        _ref_sweep_case(fhe, torch_cuda, P, log_n, next(primes), rnd, seed=2000 + 100 * log_n + 10 * k)
