"""The fused rank-k TFHE route (csrc/torusk_fused_kernels.hpp: k = 2, 3 at N = 256 .. 1024, three key pieces through f64 transforms) through
the rank-k entries of the C ABI: every entry bit-equal to the exact oracle (oracle/cref.py) at shapes on every team shape of the kernels, at
the eligibility limit with worst-case operands, against the composed route of the same build, with one table per ciphertext on both key
forms, and the reference's gate at decode level.  Every test first asks the key which form it took."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = lambda x: [int(v) for v in np.asarray(x).ravel()]  # noqa: E731
U = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731
KS = (4, 5)  # the gate's key switch (log_b, d)

# (k, log_n, log_b, d, n_lwe, batch): one-wave teams of two slots a lane (log_n 8), of four (log_n 9), one four-wave team (log_n 10);
# batches 5 and 3 leave idle teams behind the team set-up of a four-team workgroup
SHAPES = [(2, 9, 7, 3, 6, 5), (2, 8, 7, 2, 5, 3), (3, 8, 6, 2, 5, 3), (2, 10, 6, 2, 4, 2)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).cuda()  # a copy: the shared inputs are read-only


def host(t):
    return t.cpu().numpy().view(np.uint64)


def r64(rng, *s):
    return rng.integers(0, 1 << 63, size=s, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=s, dtype=np.uint64)


def extreme_digits(log_b, d):
    """the torus value whose every digit is -2^(log_b - 1), the most negative balanced digit (test_tfhe_forms_gpu.py)"""
    half = 1 << (log_b - 1)
    return (-sum(half << (64 - log_b * (j + 1)) for j in range(d))) % (1 << 64)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """brk [n_lwe][(k+1)d][k+1][n], v [n], mod-switched a~ [batch][n_lwe] with one 0 (the CMUX short-circuits) and one N (a pure sign flip)
    and b~ [batch], raw TLWE inputs of the gate, its key-switching key, two ciphertext batches.  Made once per shape and left unchanged."""
    from oracle import cref
    k, log_n, log_b, d, n_lwe, batch = shape
    n, k1 = 1 << log_n, k + 1
    rng = np.random.Generator(np.random.PCG64([7100, k, log_n, log_b, d]))
    brk, v = r64(rng, n_lwe, k1 * d, k1, n), r64(rng, n)
    brk[1, 0] = np.uint64(1 << 63)                       # the most negative key words
    a_raw, b_raw = r64(rng, batch, n_lwe), r64(rng, batch)
    at, bt = cref.tfhe_mod_switch(a_raw, n).copy(), cref.tfhe_mod_switch(b_raw, n).copy()
    at[0, 0], at[1, 1] = 0, n
    ksa, ksb = r64(rng, k * n * KS[1], n_lwe), r64(rng, k * n * KS[1])
    ct0, ct1 = r64(rng, batch, k1, n), r64(rng, batch, k1, n)
    ct0[0, :, : n // 2] = np.uint64(extreme_digits(log_b, d))
    ct0[1, 0, :5] = [0, (1 << 64) - 1, 1 << 63, (1 << 63) - 1, 1]
    return frozen(brk, v, at, bt, a_raw, b_raw, ksa, ksb, ct0, ct1)


@functools.lru_cache(maxsize=None)
def oracle(shape):
    """the exact oracle's accumulators, gate outputs, external products under entry 1 and CMUXes under entry 0, once per shape"""
    from oracle import cref
    k, log_n, log_b, d, n_lwe, batch = shape
    brk, v, at, bt, a_raw, b_raw, ksa, ksb, ct0, ct1 = inputs(shape)
    acc = cref.tfhek_blind_rotate(k, log_b, d, brk, v, at, bt, threads=8)
    ga, gb = cref.tfhek_bootstrap(k, log_b, d, KS[0], KS[1], brk, ksa, ksb, v, a_raw, b_raw, threads=8)
    ext = np.stack([cref.tggswk_external_product(k, log_b, d, brk[1], ct0[i]) for i in range(batch)])
    mux = np.stack([cref.tggswk_cmux(k, log_b, d, brk[0], ct0[i], ct1[i]) for i in range(batch)])
    return frozen(acc, ga, gb, ext, mux)


def raw_cmux(fhe, torch, t, key, a0, a1, tgt, batch):
    from learn_fhe_amd import _lib as LL
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    LL.check(LL.lib().fhe_tggswk_cmux(t.handle, key._h, 0, C.c_void_p(a0.data_ptr()), C.c_void_p(a1.data_ptr()), C.c_void_p(tgt.data_ptr()), batch,
                                      LL.MEM_DEVICE, st), "fhe_tggswk_cmux")


@pytest.mark.parametrize("shape", SHAPES, ids=["k%d-n%d-b%dd%d" % (s[0], 1 << s[1], s[2], s[3]) for s in SHAPES])
def test_entries_vs_oracle(fhe, torch_cuda, shape):
    """blind rotation (bootstrapping.rs:84-96), the whole gate (78-82) with key switch (4, 5), external product (tggsw.rs:100-112) under
    entry 1 (a wrong entry stride reads another entry), cmux (114-121) with `out` aliasing ct0 and then ct1: device and host memory"""
    k, log_n, log_b, d, n_lwe, batch = shape
    n = 1 << log_n
    brk, v, at, bt, a_raw, b_raw, ksa, ksb, ct0, ct1 = inputs(shape)
    acc, ga, gb, ext, mux = oracle(shape)
    D = lambda a: dev(torch_cuda, a)  # noqa: E731
    t = fhe.TorusContext()
    assert fhe.tggswk_form_for(k, n, log_b, d) == fhe.TGGSWK_FORM_X3
    key = fhe.TggswKeyK(t, k, log_b, d, D(brk), n)
    assert key.form() == fhe.TGGSWK_FORM_X3, "the host's rule moved this shape: %r" % (shape,)
    assert np.array_equal(host(key.blind_rotate(D(at), D(bt), D(v))), acc)
    oa, ob = key.bootstrap(KS[0], KS[1], D(ksa), D(ksb), D(v), D(a_raw), D(b_raw))
    assert np.array_equal(host(oa), ga) and np.array_equal(host(ob), gb)
    x = D(ct0)
    key.external_product_(1, x)
    assert np.array_equal(host(x), ext)
    assert np.array_equal(host(key.cmux(0, D(ct0), D(ct1))), mux)
    for alias in (0, 1):
        a0, a1 = D(ct0), D(ct1)
        tgt = a1 if alias else a0
        raw_cmux(fhe, torch_cuda, t, key, a0, a1, tgt, batch)
        assert np.array_equal(host(tgt), mux), alias
        assert np.array_equal(host(a0 if alias else a1), ct0 if alias else ct1), alias   # the other input is untouched
    # FHE_MEM_HOST
    hkey = fhe.TggswKeyK(t, k, log_b, d, brk.copy(), n)
    assert hkey.form() == fhe.TGGSWK_FORM_X3
    assert np.array_equal(hkey.blind_rotate(at.copy(), bt.copy(), v.copy()), acc)
    ha, hb = hkey.bootstrap(KS[0], KS[1], ksa.copy(), ksb.copy(), v.copy(), a_raw.copy(), b_raw.copy())
    assert np.array_equal(ha, ga) and np.array_equal(hb, gb)
    hx = ct0.copy()
    hkey.external_product_(1, hx)
    assert np.array_equal(hx, ext)
    assert np.array_equal(hkey.cmux(0, ct0.copy(), ct1.copy()), mux)


def test_the_eligibility_limit_with_worst_case_operands(fhe, cref, torch_cuda):
    """(k, log_n, log_b, d) = (3, 10, 7, 4): 16 limbs, 16 * 2^10 * 2^7 = 2^21, where the error bound of the f64 products (0.04) is tightest.
    Key words from {-2^63, 2^63 - 1, 2^63 - 2^21, 2^63 - 2^42 - 2^21 (pieces -2^21, -2^20, 2^20: each at its largest magnitude), random};
    entry 0 is all of the fourth kind.  The external product runs on ciphertexts whose every digit is -2^(log_b - 1); in the blind rotation
    ciphertext 0 has b~ = 0 and a~_0 = N with v = -(that word) / 2, so that the first CMUX decomposes acc X^N - acc = -2 v: the same digits."""
    k, log_n, log_b, d, n_lwe, batch = 3, 10, 7, 4, 3, 2
    n, k1 = 1 << log_n, k + 1
    assert k1 * d == 16 and (k1 * d * n) << log_b == 1 << 21
    rng = np.random.Generator(np.random.PCG64(7200))
    special = U([1 << 63, (1 << 63) - 1, (1 << 63) - (1 << 21), (1 << 63) - (1 << 42) - (1 << 21)])
    brk = r64(rng, n_lwe, k1 * d, k1, n)
    kind = rng.integers(0, 5, size=brk.shape)
    brk = np.where(kind < 4, special[np.minimum(kind, 3)], brk)
    brk[0] = special[3]
    ext_word = extreme_digits(log_b, d)
    assert ext_word % 2 == 0
    ct = np.full((batch, k1, n), ext_word, dtype=np.uint64)
    ct[1, :, n // 2:] = r64(rng, k1, n // 2)
    v = np.full(n, ((1 << 64) - ext_word) >> 1, dtype=np.uint64)
    at = rng.integers(0, 2 * n, size=(batch, n_lwe), dtype=np.uint64)
    bt = rng.integers(0, 2 * n, size=batch, dtype=np.uint64)
    at[0, 0], bt[0] = n, 0
    t = fhe.TorusContext()
    key = fhe.TggswKeyK(t, k, log_b, d, dev(torch_cuda, brk), n)
    assert key.form() == fhe.TGGSWK_FORM_X3
    for index in (0, 1):
        x = dev(torch_cuda, ct)
        key.external_product_(index, x)
        for i in range(batch):
            assert np.array_equal(host(x)[i], cref.tggswk_external_product(k, log_b, d, brk[index], ct[i])), (index, i)
    acc = key.blind_rotate(dev(torch_cuda, at), dev(torch_cuda, bt), dev(torch_cuda, v))
    assert np.array_equal(host(acc), cref.tfhek_blind_rotate(k, log_b, d, brk, v, at, bt, threads=8))


def test_both_routes_give_the_same_bits(fhe, torch_cuda):
    """a second key of the same rows prepared under NO_RANKK_FUSED = 1 is COMPOSED; all four entries agree with the fused key bit for bit"""
    shape = SHAPES[0]
    k, log_n, log_b, d, n_lwe, batch = shape
    n = 1 << log_n
    brk, v, at, bt, a_raw, b_raw, ksa, ksb, ct0, ct1 = inputs(shape)
    D = lambda a: dev(torch_cuda, a)  # noqa: E731
    t = fhe.TorusContext()
    fused = fhe.TggswKeyK(t, k, log_b, d, D(brk), n)
    try:
        fhe.set_option("NO_RANKK_FUSED", 1)
        composed = fhe.TggswKeyK(t, k, log_b, d, D(brk), n)
        assert composed.form() == fhe.TGGSWK_FORM_COMPOSED
    finally:
        fhe.set_option("NO_RANKK_FUSED", 0)
    assert fused.form() == fhe.TGGSWK_FORM_X3 and composed.form() == fhe.TGGSWK_FORM_COMPOSED   # a key keeps the form it was made in
    outs = []
    for key in (fused, composed):
        x = D(ct0)
        key.external_product_(1, x)
        oa, ob = key.bootstrap(KS[0], KS[1], D(ksa), D(ksb), D(v), D(a_raw), D(b_raw))
        outs.append((key.blind_rotate(D(at), D(bt), D(v)), oa, ob, x, key.cmux(0, D(ct0), D(ct1))))
    for name, f, c in zip(("blind_rotate", "bootstrap a", "bootstrap b", "external_product", "cmux"), *outs):
        assert torch_cuda.equal(f, c), name


TABLE_OF = [2, 0, 1, 2, 0]


@pytest.mark.parametrize("k,log_n,log_b,d,form", [(2, 9, 7, 3, 1), (2, 8, 8, 2, 0)], ids=["fused", "composed"])
def test_a_table_per_ciphertext(fhe, cref, torch_cuda, k, log_n, log_b, d, form):
    """fhe_tfhek_blind_rotate_tables / fhe_tfhek_bootstrap_tables, three tables over batch 5, on a key of either form: each ciphertext
    against the oracle's rotation and gate with ITS table (one oracle call per table); no indices = the shared-table entries; device and
    host indices; a host index >= n_tables is FHE_ERR_INVALID; an empty batch is FHE_OK"""
    n, k1, n_lwe, batch, n_tables = 1 << log_n, k + 1, 4, 5, 3
    rng = np.random.Generator(np.random.PCG64([7300, log_n, log_b]))
    brk, tables = r64(rng, n_lwe, k1 * d, k1, n), r64(rng, n_tables, n)
    a_raw, b_raw = r64(rng, batch, n_lwe), r64(rng, batch)
    at, bt = cref.tfhe_mod_switch(a_raw, n), cref.tfhe_mod_switch(b_raw, n)
    ksa, ksb = r64(rng, k * n * KS[1], n_lwe), r64(rng, k * n * KS[1])
    D = lambda a: dev(torch_cuda, a)  # noqa: E731
    t = fhe.TorusContext()
    key = fhe.TggswKeyK(t, k, log_b, d, D(brk), n)
    assert key.form() == form
    want_acc = [cref.tfhek_blind_rotate(k, log_b, d, brk, tables[j], at, bt, threads=8) for j in range(n_tables)]
    want_gate = [cref.tfhek_bootstrap(k, log_b, d, KS[0], KS[1], brk, ksa, ksb, tables[j], a_raw, b_raw, threads=8) for j in range(n_tables)]
    idx_dev = torch_cuda.tensor(TABLE_OF, dtype=torch_cuda.int32, device="cuda")
    idx_host = np.array(TABLE_OF, dtype=np.uint32)
    hkey = fhe.TggswKeyK(t, k, log_b, d, brk.copy(), n)
    runs = [(host(key.blind_rotate_tables(D(at), D(bt), D(tables), idx_dev)),
             [host(o) for o in key.bootstrap_tables(KS[0], KS[1], D(ksa), D(ksb), D(tables), idx_dev, D(a_raw), D(b_raw))]),
            (hkey.blind_rotate_tables(at.copy(), bt.copy(), tables.copy(), idx_host),
             hkey.bootstrap_tables(KS[0], KS[1], ksa.copy(), ksb.copy(), tables.copy(), idx_host, a_raw.copy(), b_raw.copy()))]
    for where, (acc, (oa, ob)) in zip(("device", "host"), runs):
        for i, tb in enumerate(TABLE_OF):
            assert np.array_equal(acc[i], want_acc[tb][i]), (where, i, tb)
            assert np.array_equal(oa[i], want_gate[tb][0][i]) and int(ob[i]) == int(want_gate[tb][1][i]), (where, i, tb)
    # no indices, and indices all zero: the shared-table entries with tables[0]
    shared = key.blind_rotate(D(at), D(bt), D(tables[0]))
    sa, sb = key.bootstrap(KS[0], KS[1], D(ksa), D(ksb), D(tables[0]), D(a_raw), D(b_raw))
    assert np.array_equal(host(shared), want_acc[0])
    zeros = torch_cuda.zeros(batch, dtype=torch_cuda.int32, device="cuda")
    for idx in (None, zeros):
        assert torch_cuda.equal(key.blind_rotate_tables(D(at), D(bt), D(tables), idx), shared)
        oa, ob = key.bootstrap_tables(KS[0], KS[1], D(ksa), D(ksb), D(tables), idx, D(a_raw), D(b_raw))
        assert torch_cuda.equal(oa, sa) and torch_cuda.equal(ob, sb)
    bad = idx_host.copy()
    bad[3] = n_tables
    for call in (lambda: hkey.blind_rotate_tables(at.copy(), bt.copy(), tables.copy(), bad),
                 lambda: hkey.bootstrap_tables(KS[0], KS[1], ksa.copy(), ksb.copy(), tables.copy(), bad, a_raw.copy(), b_raw.copy())):
        with pytest.raises(fhe.FheError) as e:
            call()
        assert e.value.code == 1
    lib, p = fhe.lib(), lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert lib.fhe_tfhek_blind_rotate_tables(t.handle, hkey._h, None, None, p(tables), n_tables, None, None, 0, 0, None) == 0
    assert lib.fhe_tfhek_bootstrap_tables(t.handle, hkey._h, KS[0], KS[1], p(ksa), p(ksb), p(tables), n_tables, None, None, None, None, None, 0, 0, None) == 0
    assert lib.fhe_tfhek_blind_rotate_tables(t.handle, hkey._h, None, None, p(tables), 0, None, None, 0, 0, None) == 1     # no table at all


def test_rank2_gate_decode_level_one_call_three_tables(fhe, torch_cuda):
    """The rank-2 gate of tests/test_torusk_gpu.py::test_rank2_gate_bootstrap_decode_level at its parameters (big_n = 512, k = 2, n_lwe =
    256, base 2^7 x 3, key switch (4, 5), log_p 3, padding 1; keys from the device producers), now on the fused route: the LUTs identity /
    double / parity are ONE table set, every message under every LUT is one ciphertext of ONE fhe_tfhek_bootstrap_tables call, decoded on
    the host."""
    from oracle import pyref as P
    k, n, n_lwe, log_p, padding, log_b, d, ks_lb, ks_d = 2, 512, 256, 3, 1, 7, 3, 4, 5
    sd_lwe, sd_glwe = 2.0 ** -22, 2.0 ** -40
    p, log_delta = 1 << log_p, 64 - (log_p + padding)
    like = dev(torch_cuda, U([0]))
    t = fhe.TorusContext()
    z, s = fhe.sample_binary(910, 0, like, n_lwe), fhe.sample_binary(910, 1, like, k * n)
    zh = L(host(z))
    pt = np.zeros((n_lwe, n), dtype=np.uint64)
    pt[:, 0] = host(z)
    key = fhe.TggswKeyK(t, k, log_b, d, fhe.tggswk_encrypt(t, k, log_b, d, s, dev(torch_cuda, pt), n, sd_glwe, 911, 0), n)
    assert key.form() == fhe.TGGSWK_FORM_X3
    ksa, ksb = fhe.tlwe_ksk_gen(ks_lb, ks_d, z, s, sd_lwe, 912, 0)

    def table(f):
        m_ = n >> log_p
        tt = [f(v) % p for v in range(p)]
        out = [tt[0]] * (m_ // 2)
        for x in tt[1:]:
            out += [x] * m_
        return out + [(-tt[0]) % p] * (m_ // 2)

    funcs = (lambda v: v, lambda v: 2 * v, lambda v: v % 2)
    tables = dev(torch_cuda, U([[(x << log_delta) % P.M64 for x in table(f)] for f in funcs]))
    msgs = dev(torch_cuda, U([(m << log_delta) % P.M64 for _ in funcs for m in range(p)]))
    table_of = torch_cuda.tensor([li for li in range(len(funcs)) for _ in range(p)], dtype=torch_cuda.int32, device="cuda")
    ca, cb = fhe.tlwe_sk_encrypt(z, msgs, n_lwe, len(funcs) * p, sd_lwe, 913, 0)
    oa, ob = key.bootstrap_tables(ks_lb, ks_d, ksa, ksb, tables, table_of, ca, cb)
    ha, hb = host(oa), host(ob)
    for li, f in enumerate(funcs):
        for m in range(p):
            i = li * p + m
            mu = ((P.tlwe_phase(zh, L(ha[i]), int(hb[i])) + (1 << (log_delta - 1))) % P.M64) >> log_delta
            assert mu % p == f(m) % p, (li, m, mu)
