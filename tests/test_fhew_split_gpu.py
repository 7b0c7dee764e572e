"""GPU tests of the split FHEW blind rotation (learn-fhe_amd/csrc/fhew_split_kernels.hpp): a cluster of G = 2, 4, 8 workgroups
per ciphertext.  Bit-exact throughout: against the one-workgroup shape (BR_SPLIT = 0) and against the oracle.  Every test puts
BR_SPLIT back to -1.  No test provokes the kernel's give-up path: a cluster waiting for a member that never arrives would be a
deliberate hang."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q54 = 18014398509404161   # cfg3's modulus: the 54-bit two-operand policy
Q_SHOUP = 35184372060161  # 45 bits: ArithShoup


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


def cu_count(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _make_bk(fhe, torch_cuda, q, n, log_b, d, ks_log_b, ks_d, w, n_lwe, seed):
    from oracle import pyref as P
    brk = rand_u64(seed, q, (n_lwe, 2, 2 * d, n))          # [key][a|b][row][n] as the oracle takes it
    ak = rand_u64(seed + 1, q, (w + 1, 2, ks_d, n))
    ctx = fhe.NttContext(q)
    gk = fhe.GadgetKey(ctx, log_b, d, dev(torch_cuda, brk[:, 0]), dev(torch_cuda, brk[:, 1]), n, rgsw=True)
    ga = fhe.GadgetKey(ctx, ks_log_b, ks_d, dev(torch_cuda, ak[:, 0]), dev(torch_cuda, ak[:, 1]), n, rgsw=False)
    ts = P.ak_t(n, w)
    return ctx, fhe.BootstrapKey(ctx, gk, ga, ts, w), brk, ak, ts


def _lwe(seed, n, n_lwe, batch):
    rng = np.random.Generator(np.random.PCG64(seed))
    lwe_a = rng.integers(0, n, size=(batch, n_lwe), dtype=np.uint64) * 2 + 1
    lwe_b = rng.integers(0, 2 * n, size=batch, dtype=np.uint64)
    return lwe_a, lwe_b


def _q(cref, name):
    return {"q54": Q54, "q55": cref.two_adic_primes(55, 12, 1)[0], "shoup": Q_SHOUP}[name]


@pytest.mark.parametrize("qname", ["q54", "q55", "shoup"])
@pytest.mark.parametrize("log_n", [10, 11])
@pytest.mark.parametrize("g", [2, 4, 8])
def test_split_equals_one_workgroup_and_oracle(fhe, cref, torch_cuda, g, log_n, qname):
    """forced G against BR_SPLIT = 0 at batch 1, 3 and CUs / G (the largest admissible batch); one ciphertext per case against
    the oracle; the query reports G there and 1 one past it, where the call still gives the right result"""
    q, n, lb, d, w, n_lwe = _q(cref, qname), 1 << log_n, 6, 3, 3, 3
    assert cref.is_prime(q) and (q - 1) % (2 * n) == 0
    cus = cu_count(torch_cuda)
    top = cus // g
    ctx, bk, brk, ak, ts = _make_bk(fhe, torch_cuda, q, n, lb, d, 5, 4, w, n_lwe, seed=200 + log_n)
    lwe_a, lwe_b = _lwe(201, n, n_lwe, top + 1)
    f = rand_u64(202, q, n)
    da, db, df = dev(torch_cuda, lwe_a), dev(torch_cuda, lwe_b), dev(torch_cuda, f)
    try:
        fhe.set_option("BR_SPLIT", 0)
        assert bk.split(1) == 1 and bk.split(top) == 1
        ra, rb = bk.blind_rotate(da, db, df)
        bk.check(da)
        ra, rb = host(ra), host(rb)
        fhe.set_option("BR_SPLIT", g)
        for batch in (1, 3, top):
            assert bk.split(batch) == g, batch
            oa, ob = bk.blind_rotate(da[:batch], db[:batch], df)
            bk.check(da)  # no wait gave up
            assert np.array_equal(host(oa), ra[:batch]) and np.array_equal(host(ob), rb[:batch]), batch
        assert bk.split(top + 1) == 1
        oa, ob = bk.blind_rotate(da, db, df)
        bk.check(da)
        assert np.array_equal(host(oa), ra) and np.array_equal(host(ob), rb)
        i = top - 1
        ea, eb = cref.blind_rotate(q, n, w, lb, d, 5, 4, brk, ak, ts, f, lwe_a[i], int(lwe_b[i]))
        assert np.array_equal(ra[i], ea) and np.array_equal(rb[i], eb)
    finally:
        fhe.set_option("BR_SPLIT", -1)


@pytest.mark.parametrize("g,lb,d,ks_lb,ks_d", [(8, 6, 3, 5, 4), (2, 6, 9, 6, 9), (4, 6, 9, 6, 9), (8, 6, 9, 6, 9)])
def test_split_gadgets_that_do_not_divide(fhe, cref, torch_cuda, g, lb, d, ks_lb, ks_d):
    """(6, 3) with (5, 4) under G = 8: 6 and 4 digits on 8 members, some hold none and publish zeros; d = 9 (18 and 9 digits)
    under every G: members with different numbers of digits"""
    q, n, w, n_lwe, batch = Q54, 1024, 5, 4, 3
    ctx, bk, brk, ak, ts = _make_bk(fhe, torch_cuda, q, n, lb, d, ks_lb, ks_d, w, n_lwe, seed=210 + g + d)
    lwe_a, lwe_b = _lwe(211, n, n_lwe, batch)
    f = rand_u64(212, q, n)
    try:
        fhe.set_option("BR_SPLIT", g)
        assert bk.split(batch) == g
        oa, ob = bk.blind_rotate(dev(torch_cuda, lwe_a), dev(torch_cuda, lwe_b), dev(torch_cuda, f))
        bk.check(oa)
        for i in (0, batch - 1):
            ea, eb = cref.blind_rotate(q, n, w, lb, d, ks_lb, ks_d, brk, ak, ts, f, lwe_a[i], int(lwe_b[i]))
            assert np.array_equal(host(oa)[i], ea) and np.array_equal(host(ob)[i], eb), i
    finally:
        fhe.set_option("BR_SPLIT", -1)


@pytest.mark.parametrize("g", [2, 4, 8])
def test_split_uneven_clusters_in_one_launch(fhe, cref, torch_cuda, g):
    """op lists of very different lengths side by side (no LWE coefficient at all, all in one bucket, dense), per-ciphertext
    LUTs: clusters run independently, each to the end of its own list"""
    q, n, lb, d, w, n_lwe, batch = Q54, 1024, 6, 3, 7, 12, 5
    ctx, bk, brk, ak, ts = _make_bk(fhe, torch_cuda, q, n, lb, d, 5, 4, w, n_lwe, seed=220)
    lwe_a, lwe_b = _lwe(221, n, n_lwe, batch)
    lwe_a[0, :] = 0                      # automorphisms only
    lwe_a[1, :] = lwe_a[1, 0]            # everything in one bucket
    lwe_a[3, ::2] = 0                    # half of it skipped
    f = rand_u64(222, q, (batch, n))     # f_stride = N
    try:
        fhe.set_option("BR_SPLIT", g)
        assert bk.split(batch) == g
        oa, ob, sched = bk.blind_rotate(dev(torch_cuda, lwe_a), dev(torch_cuda, lwe_b), dev(torch_cuda, f), want_schedule=True)
        for i in range(batch):
            assert sched[i] == cref.blind_rotate_schedule(n, w, lwe_a[i]), i
            ea, eb = cref.blind_rotate(q, n, w, lb, d, 5, 4, brk, ak, ts, f[i], lwe_a[i], int(lwe_b[i]))
            assert np.array_equal(host(oa)[i], ea) and np.array_equal(host(ob)[i], eb), i
        assert len({len(s) for s in sched}) > 1  # the lists do differ in length
    finally:
        fhe.set_option("BR_SPLIT", -1)


def test_split_repeated_calls_and_two_streams(fhe, cref, torch_cuda):
    """the same call twice in a row on one stream, then on two streams at once: identical outputs (flags, timeout word and slabs
    are re-initialised per call and belong to the call)"""
    torch = torch_cuda
    q, n, lb, d, w, n_lwe, batch, g = Q54, 1024, 6, 3, 3, 3, 8, 8
    ctx, bk, brk, ak, ts = _make_bk(fhe, torch_cuda, q, n, lb, d, 5, 4, w, n_lwe, seed=230)
    lwe_a, lwe_b = _lwe(231, n, n_lwe, batch)
    f = rand_u64(232, q, n)
    da, db, df = dev(torch, lwe_a), dev(torch, lwe_b), dev(torch, f)
    try:
        fhe.set_option("BR_SPLIT", 0)
        ra, rb = bk.blind_rotate(da, db, df)
        fhe.set_option("BR_SPLIT", g)
        assert bk.split(batch) == g
        o1 = bk.blind_rotate(da, db, df)
        o2 = bk.blind_rotate(da, db, df)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            p1 = bk.blind_rotate(da, db, df)
        with torch.cuda.stream(s2):
            p2 = bk.blind_rotate(da, db, df)
        s1.synchronize()
        s2.synchronize()
        torch.cuda.synchronize()
        bk.check(da)
        for o in (o1, o2, p1, p2):
            assert torch.equal(o[0], ra) and torch.equal(o[1], rb)
    finally:
        fhe.set_option("BR_SPLIT", -1)


def test_split_cfg3_full_length(fhe, cref, torch_cuda):
    """BASELINE config 3 at full length (N = 1024, d = 9, n_lwe = 100, w = 10), batch 2, G = 8, both ciphertexts against the oracle"""
    q, n, lb, d, w, n_lwe, batch = Q54, 1024, 6, 9, 10, 100, 2
    ctx, bk, brk, ak, ts = _make_bk(fhe, torch_cuda, q, n, lb, d, lb, d, w, n_lwe, seed=60)
    lwe_a, lwe_b = _lwe(10, n, n_lwe, batch)
    f = rand_u64(78, q, n)
    try:
        fhe.set_option("BR_SPLIT", 8)
        assert bk.split(batch) == 8
        oa, ob, sched = bk.blind_rotate(dev(torch_cuda, lwe_a), dev(torch_cuda, lwe_b), dev(torch_cuda, f), want_schedule=True)
        for i in range(batch):
            assert sched[i] == cref.blind_rotate_schedule(n, w, lwe_a[i]) and len(sched[i]) > 200
            ea, eb = cref.blind_rotate(q, n, w, lb, d, lb, d, brk, ak, ts, f, lwe_a[i], int(lwe_b[i]))
            assert np.array_equal(host(oa)[i], ea) and np.array_equal(host(ob)[i], eb), i
    finally:
        fhe.set_option("BR_SPLIT", -1)


def test_split_gate_and_async_error_path(fhe, cref, torch_cuda):
    """the whole gate (bk.bootstrap) at batch 4 under G = 8 against the gate oracle; an even LWE coefficient under the split shape is
    reported as under the one-workgroup shape: by the call itself from host memory, by the key's status word from device memory"""
    q, n, lb, d, w, n_lwe, batch = Q54, 1024, 6, 3, 3, 6, 4
    q_ks, kb, kd = 1 << 16, 4, 4
    ctx, bk, brk, ak, ts = _make_bk(fhe, torch_cuda, q, n, lb, d, 5, 4, w, n_lwe, seed=240)
    ksk_a, ksk_b = rand_u64(241, q_ks, (kd * n, n_lwe)), rand_u64(242, q_ks, kd * n)
    ct_a, ct_b = rand_u64(243, q, (batch, n)), rand_u64(244, q, batch)
    f = rand_u64(245, q, n)
    addend = q // 8
    try:
        fhe.set_option("BR_SPLIT", 8)
        assert bk.split(batch) == 8
        oa, ob = bk.bootstrap(q_ks, kb, kd, dev(torch_cuda, ksk_a), dev(torch_cuda, ksk_b), dev(torch_cuda, f), dev(torch_cuda, ct_a),
                              dev(torch_cuda, ct_b), addend=addend)
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
        lwe_a, lwe_b = _lwe(246, n, n_lwe, batch)
        bad = lwe_a.copy()
        bad[0, 0] = 4
        bk.check(dev(torch_cuda, lwe_b))                       # nothing wrong so far
        with pytest.raises(fhe.FheError):                      # host memory: the call itself reports it
            bk.blind_rotate(bad, lwe_b, f)
        d_bad = dev(torch_cuda, bad)
        bk.blind_rotate(d_bad, dev(torch_cuda, lwe_b), dev(torch_cuda, f))  # device memory: asynchronous, the status word records it
        with pytest.raises(fhe.FheError):
            bk.check(d_bad)
        bk.check(d_bad)                                        # cleared by the previous query
    finally:
        fhe.set_option("BR_SPLIT", -1)


def test_rule_never_splits_beyond_the_compute_units(fhe, cref, torch_cuda):
    """under the library's own rule (BR_SPLIT = -1) a split launch never exceeds one cluster member per compute unit, and the
    throughput batches keep the one-workgroup shape"""
    q, n, lb, d, w, n_lwe = Q54, 1024, 6, 3, 3, 3
    ctx, bk, brk, ak, ts = _make_bk(fhe, torch_cuda, q, n, lb, d, 5, 4, w, n_lwe, seed=250)
    cus = cu_count(torch_cuda)
    for batch in (1, 2, 7, 32, 64, 100, 128, 129, 256, 1024, 4096):
        g = bk.split(batch)
        assert g in (1, 2, 4, 8) and (g == 1 or batch * g <= cus), batch
    assert bk.split(1024) == 1 and bk.split(4096) == 1
