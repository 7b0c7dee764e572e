"""GPU tests of the TGLWE automorphism key switch, trace and ring packing (k = 1): fhe_tglwe_automorphism, fhe_tglwe_trace and
fhe_tlwe_ring_pack bit-exact against the model of tests/tfhe_trace_model.py and against their compositions from public entries, in both
memory kinds and at every ring; the device-made keys against fhe_tglwe_sk_encrypt; rejections, aliasing, odd alignment, a side stream;
a pack with noisy keys and matvec at decode level; the C demo.  Every comparison of ciphertext words is exact equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tfhe_mul_model as MM
import tfhe_trace_model as M

pytestmark = pytest.mark.gpu

M64 = 1 << 64
U = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731
GADGETS_256 = [(7, 5), (4, 2), (16, 3), (31, 2)]
OTHER_RINGS = [512, 1024, 2048]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def tctx(fhe, torch_cuda):
    return fhe.TorusContext()


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def r64(rng, *shape):
    return rng.integers(0, 1 << 63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)


def edge_words(log_b, d):
    """0, 2^63, 2^63 - 1, 2^64 - 1, values whose digits are all +2^(log_b - 1) resp. -2^(log_b - 1) (a carry through every level), and the
    rounding ties of the decomposition: half a unit of the last digit above and just below"""
    rb, half = 64 - log_b * d, 1 << (log_b - 1)
    up = sum(half << (rb + j * log_b) for j in range(d)) % M64
    tie = (1 << rb) // 2
    return [0, 1 << 63, (1 << 63) - 1, M64 - 1, up, (-up) % M64, (up + tie - (1 if rb else 0)) % M64, tie, (tie - 1) % M64, (M64 - tie) % M64]


def random_key(rng, gs, d, n):
    """random words for key rows: the bits of the entries do not depend on what the rows encrypt"""
    ka, kb = r64(rng, len(gs), d, n), r64(rng, len(gs), d, n)
    ka[:, :, 0], kb[:, :, n - 1] = np.uint64(1 << 63), np.uint64(M64 - 1)
    return ka, kb


def model_autks(log_b, d, key, g, ca, cb):
    outs = [M.u64(M.autks(log_b, d, key, g, (ca[i], cb[i]))) for i in range(ca.shape[0])]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def model_trace(log_b, d, key, ca, cb, lo, hi):
    outs = [M.u64(M.trace(log_b, d, key, (ca[i], cb[i]), lo, hi)) for i in range(ca.shape[0])]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def check_automorphism(fhe, torch, t, log_b, d, n, batch, gs, seed):
    X = fhe.tfhe_trace
    rng = np.random.Generator(np.random.PCG64(seed))
    ka, kb = random_key(rng, gs, d, n)
    key = M.key_dict(gs, ka, kb, d, n)
    ca, cb = r64(rng, batch, n), r64(rng, batch, n)
    e = U(edge_words(log_b, d))
    ca[0, :e.size] = e
    ca[batch - 1, n - e.size:] = e
    dkey = X.AutoKey(t, log_b, d, dev(torch, ka), dev(torch, kb), n, gs)
    hkey = X.AutoKey(t, log_b, d, ka, kb, n, gs)
    da, db = dev(torch, ca), dev(torch, cb)
    for g in gs:
        want_a, want_b = model_autks(log_b, d, key, g, ca, cb)
        ga, gb = X.automorphism(dkey, g, da, db)
        assert np.array_equal(host(ga), want_a) and np.array_equal(host(gb), want_b), ("device memory", g)
        ha, hb = X.automorphism(hkey, g, ca, cb)
        assert np.array_equal(ha, want_a) and np.array_equal(hb, want_b), ("host memory", g)
    g = gs[0]
    want_a, want_b = model_autks(log_b, d, key, g, ca, cb)
    # every word -2^63, every word 2^63 - 1 (one row of the model, every row the same)
    for w in (1 << 63, (1 << 63) - 1):
        fa = np.full((batch, n), w, dtype=np.uint64)
        wa, wb = model_autks(log_b, d, key, g, fa[:1], fa[:1])
        ga, gb = X.automorphism(dkey, g, dev(torch, fa), dev(torch, fa.copy()))
        assert np.array_equal(host(ga), np.repeat(wa, batch, axis=0)) and np.array_equal(host(gb), np.repeat(wb, batch, axis=0)), hex(w)
    # out = in
    xa, xb = da.clone(), db.clone()
    X.automorphism(dkey, g, xa, xb, out=(xa, xb))
    assert np.array_equal(host(xa), want_a) and np.array_equal(host(xb), want_b), "out = in"
    # every pointer 8 but not 16 bytes past an allocation's start
    odd = [torch.empty(batch * n + 1, dtype=torch.int64, device="cuda")[1:] for _ in range(4)]
    odd[0].copy_(da.reshape(-1))
    odd[1].copy_(db.reshape(-1))
    assert all(o.data_ptr() % 16 == 8 for o in odd)
    X.automorphism(dkey, g, odd[0], odd[1], out=(odd[2], odd[3]))
    assert np.array_equal(host(odd[2]).reshape(batch, n), want_a) and np.array_equal(host(odd[3]).reshape(batch, n), want_b), "odd alignment"
    # a side stream: the inputs are made on it, the call follows them there
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    mask = 0x5555555555555555
    with torch.cuda.stream(side):
        sa, sb = X.automorphism(dkey, g, (da ^ mask) ^ mask, (db ^ mask) ^ mask)
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(host(sa), want_a) and np.array_equal(host(sb), want_b), "side stream"
    dkey.destroy()
    hkey.destroy()


@pytest.mark.parametrize("batch", [1, 5])
def test_automorphism_bit_exact_n256(fhe, torch_cuda, tctx, batch):
    """n = 256: four one-wave teams a block, batch 5 leaves the second block one team"""
    n = 256
    check_automorphism(fhe, torch_cuda, tctx, 7, 5, n, batch, [3, 5, n + 1, 2 * n - 1], 9800 + batch)


@pytest.mark.parametrize("log_b,d", GADGETS_256[1:])
def test_automorphism_gadgets_n256(fhe, torch_cuda, tctx, log_b, d):
    check_automorphism(fhe, torch_cuda, tctx, log_b, d, 256, 5, [3, 511], 9810 + log_b)


@pytest.mark.parametrize("n", OTHER_RINGS)
def test_automorphism_bit_exact_every_ring(fhe, torch_cuda, tctx, n):
    check_automorphism(fhe, torch_cuda, tctx, 7, 5, n, 2, [3, n + 1], 9820 + n)


def check_trace(fhe, torch, t, n, batch, ranges, seed, log_b=7, d=5):
    X = fhe.tfhe_trace
    rng = np.random.Generator(np.random.PCG64(seed))
    gs = M.galois_set(n)
    ka, kb = random_key(rng, gs, d, n)
    key = M.key_dict(gs, ka, kb, d, n)
    ca, cb = r64(rng, batch, n), r64(rng, batch, n)
    dkey = X.AutoKey(t, log_b, d, dev(torch, ka), dev(torch, kb), n, gs)
    da, db = dev(torch, ca), dev(torch, cb)
    for lo, hi in ranges:
        want_a, want_b = model_trace(log_b, d, key, ca, cb, lo, hi)
        ga, gb = X.trace(dkey, da, db, lo, hi)
        assert np.array_equal(host(ga), want_a) and np.array_equal(host(gb), want_b), ("fused", lo, hi)
        xa, xb = X.trace_composed(dkey, da, db, lo, hi)
        assert np.array_equal(host(xa), want_a) and np.array_equal(host(xb), want_b), ("composed", lo, hi)
    lo, hi = ranges[-1]  # want_a, want_b are this range's
    ha, hb = X.trace(dkey, ca, cb, lo, hi)
    assert np.array_equal(ha, want_a) and np.array_equal(hb, want_b), "host memory"
    xa, xb = da.clone(), db.clone()
    X.trace(dkey, xa, xb, lo, hi, out=(xa, xb))
    assert np.array_equal(host(xa), want_a) and np.array_equal(host(xb), want_b), "out = in"
    dkey.destroy()


def test_trace_bit_exact_n256(fhe, torch_cuda, tctx):
    check_trace(fhe, torch_cuda, tctx, 256, 5, [(0, 8), (6, 8), (0, 1)], 9830)


@pytest.mark.parametrize("n", OTHER_RINGS)
def test_trace_full_every_ring(fhe, torch_cuda, tctx, n):
    check_trace(fhe, torch_cuda, tctx, n, 1, [(0, M.log2(n))], 9840 + n)


def model_pack(log_b, d, key, ca, cb, count, n):
    ca, cb = ca.reshape(-1, count, n), cb.reshape(-1, count)
    outs = [M.u64(M.ring_pack(log_b, d, key, [(ca[p, r], cb[p, r]) for r in range(count)])) for p in range(ca.shape[0])]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


@pytest.mark.parametrize("count,packs", [(1, 3), (2, 1), (8, 3), (256, 1)])
def test_ring_pack_bit_exact_n256(fhe, torch_cuda, tctx, count, packs):
    """count 1: embed + full trace; 2: one level; 8: three levels through both scratch buffers; 256: the whole tree, no trace.  packs 3
    also in slabs of 2 (a full slab and a partly filled one)"""
    X = fhe.tfhe_trace
    n, log_b, d = 256, 7, 5
    rng = np.random.Generator(np.random.PCG64(9850 + count))
    gs = M.galois_set(n)
    ka, kb = random_key(rng, gs, d, n)
    key = M.key_dict(gs, ka, kb, d, n)
    ca, cb = r64(rng, packs, count, n), r64(rng, packs, count)
    want_a, want_b = model_pack(log_b, d, key, ca, cb, count, n)
    dkey = X.AutoKey(tctx, log_b, d, dev(torch_cuda, ka), dev(torch_cuda, kb), n, gs)
    da, db = dev(torch_cuda, ca), dev(torch_cuda, cb)
    ga, gb = X.ring_pack(dkey, da, db, count)
    assert np.array_equal(host(ga), want_a) and np.array_equal(host(gb), want_b), "device memory"
    ha, hb = X.ring_pack(dkey, ca, cb, count)
    assert np.array_equal(ha, want_a) and np.array_equal(hb, want_b), "host memory"
    xa, xb = X.ring_pack_composed(dkey, da, db, count)
    assert np.array_equal(host(xa), want_a) and np.array_equal(host(xb), want_b), "composed"
    if packs > 1:
        fhe.set_option("PACK_SLAB", 2)
        try:
            sa, sb = X.ring_pack(dkey, da, db, count)
        finally:
            fhe.set_option("PACK_SLAB", 0)
        assert np.array_equal(host(sa), want_a) and np.array_equal(host(sb), want_b), "slabs of 2"
    ea, eb = X.embed(da.reshape(-1, n), db.reshape(-1), n)
    ba, bb = fhe.tglwe_sample_extract(ea, eb, n, 0)
    assert np.array_equal(host(ba), ca.reshape(-1, n)) and np.array_equal(host(bb), cb.reshape(-1)), "sample_extract(embed(x), 0) = x"
    dkey.destroy()


@pytest.mark.parametrize("n", [1024, 2048])
def test_ring_pack_equals_composed_large_rings(fhe, torch_cuda, tctx, n):
    X = fhe.tfhe_trace
    log_b, d, count, packs = 7, 5, 8, 2
    rng = np.random.Generator(np.random.PCG64(9860 + n))
    gs = M.galois_set(n)
    ka, kb = random_key(rng, gs, d, n)
    dkey = X.AutoKey(tctx, log_b, d, dev(torch_cuda, ka), dev(torch_cuda, kb), n, gs)
    da, db = dev(torch_cuda, r64(rng, packs, count, n)), dev(torch_cuda, r64(rng, packs, count))
    ga, gb = X.ring_pack(dkey, da, db, count)
    xa, xb = X.ring_pack_composed(dkey, da, db, count)
    assert np.array_equal(host(ga), host(xa)) and np.array_equal(host(gb), host(xb))
    dkey.destroy()


@pytest.mark.parametrize("n,log_b,d", [(256, 7, 5), (1024, 16, 4)])
def test_atk_gen_rows(fhe, torch_cuda, tctx, n, log_b, d):
    """the rows are fhe_tglwe_sk_encrypt's on the plaintext rows -h_j sigma_g(S) for the same generator and stream_id, bit for bit; at
    std_dev = 0 every row's phase is that plaintext exactly"""
    X = fhe.tfhe_trace
    like = dev(torch_cuda, U([0]))
    sk = fhe.sample_binary(9870, 0, like, n)
    gs = [3, n + 1, 2 * n - 1]
    plain = M.atk_plain(log_b, d, host(sk), gs)
    for std_dev in (0.0, 2.0 ** -40):
        ra, rb = X.atk_gen(tctx, log_b, d, sk, n, gs, std_dev, 9871, 7)
        ea, eb = fhe.tglwe_sk_encrypt(tctx, sk, dev(torch_cuda, plain), n, len(gs) * d, std_dev, 9871, 7)
        assert np.array_equal(host(ra).reshape(-1, n), host(ea)) and np.array_equal(host(rb).reshape(-1, n), host(eb)), std_dev
    ha, hb = X.atk_gen(tctx, log_b, d, host(sk).copy(), n, gs, 0.0, 9871, 7)  # host memory
    ra, rb = X.atk_gen(tctx, log_b, d, sk, n, gs, 0.0, 9871, 7)
    assert np.array_equal(ha, host(ra)) and np.array_equal(hb, host(rb))
    for q in (0, 2):
        for j in (0, d - 1):
            assert MM.phase(ha[q, j], hb[q, j], host(sk)) == [int(v) for v in plain[q, j]], (q, j)


def test_rejections_write_nothing(fhe, torch_cuda):
    torch = torch_cuda
    n, log_b, d = 256, 7, 5
    t, other = fhe.TorusContext(), fhe.TorusContext()
    rng = np.random.Generator(np.random.PCG64(9880))
    gs = [3, 5, 257]  # u = 1, 2, 8: no key for u = 3 .. 7
    ka, kb = random_key(rng, gs, d, n)
    key = fhe.tfhe_trace.AutoKey(t, log_b, d, dev(torch, ka), dev(torch, kb), n, gs)
    ins = [dev(torch, r64(rng, 4, n)) for _ in range(2)]
    sentinel = 0x6b6b6b6b6b6b6b6b
    outs = [torch.full((4, n), sentinel, dtype=torch.int64, device="cuda") for _ in range(2)]
    lib = fhe.lib()
    P = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    i, o = [P(x) for x in ins], [P(x) for x in outs]
    INVALID, UNSUPPORTED = 1, 6
    for g in (2, 512, 513, 9):  # even, 2n, beyond 2n, no key
        assert lib.fhe_tglwe_automorphism(t.handle, key._h, g, i[0], i[1], o[0], o[1], 1, 1, None) == INVALID, g
    assert lib.fhe_tglwe_automorphism(other.handle, key._h, 3, i[0], i[1], o[0], o[1], 1, 1, None) == INVALID  # a key of another context
    assert lib.fhe_tglwe_automorphism(t.handle, key._h, 3, i[0], None, o[0], o[1], 1, 1, None) == INVALID
    assert lib.fhe_tglwe_automorphism(t.handle, key._h, 3, i[0], i[1], o[0], o[0], 1, 1, None) == INVALID
    part = C.c_void_p(ins[0].data_ptr() + 64)  # eight words into ct_a: a partial overlap
    assert lib.fhe_tglwe_automorphism(t.handle, key._h, 3, i[0], i[1], part, o[1], 1, 1, None) == INVALID
    assert lib.fhe_tglwe_automorphism(t.handle, key._h, 3, i[0], i[1], i[1], o[1], 1, 1, None) == INVALID  # out_a is ct_b
    for lo, hi in ((0, 0), (1, 0), (-1, 1), (7, 9), (0, 8), (2, 3)):  # lo >= hi, lo < 0, hi > log2 n, steps without a key
        assert lib.fhe_tglwe_trace(t.handle, key._h, lo, hi, i[0], i[1], o[0], o[1], 1, 1, None) == INVALID, (lo, hi)
    assert lib.fhe_tglwe_trace(other.handle, key._h, 0, 2, i[0], i[1], o[0], o[1], 1, 1, None) == INVALID
    assert lib.fhe_tglwe_trace(t.handle, key._h, 0, 2, i[0], i[1], None, o[1], 1, 1, None) == INVALID
    for count in (0, 3, 512, 8):  # not a power of two, > n, a level without a key
        assert lib.fhe_tlwe_ring_pack(t.handle, key._h, i[0], i[1], count, 1, o[0], o[1], 1, None) == INVALID, count
    full = fhe.tfhe_trace.AutoKey(t, log_b, d, dev(torch, np.repeat(ka, 3, axis=0)[:8]), dev(torch, np.repeat(kb, 3, axis=0)[:8]), n, M.galois_set(n))
    assert lib.fhe_tlwe_ring_pack(t.handle, full._h, i[0], i[1], 2, 1, i[0], o[1], 1, None) == INVALID  # out_a is ct_a
    assert lib.fhe_tlwe_ring_pack(t.handle, full._h, i[0], i[1], 2, 1, o[0], o[0], 1, None) == INVALID
    assert lib.fhe_tlwe_ring_pack(other.handle, full._h, i[0], i[1], 2, 1, o[0], o[1], 1, None) == INVALID
    # batch or packs = 0: FHE_OK, nothing touched
    assert lib.fhe_tglwe_automorphism(t.handle, key._h, 3, i[0], i[1], o[0], o[1], 0, 1, None) == 0
    assert lib.fhe_tglwe_trace(t.handle, key._h, 0, 2, i[0], i[1], o[0], o[1], 0, 1, None) == 0
    assert lib.fhe_tlwe_ring_pack(t.handle, full._h, i[0], i[1], 2, 0, o[0], o[1], 1, None) == 0
    h = C.c_void_p()
    g3 = (C.c_uint32 * 1)(3)
    assert lib.fhe_tglwe_atk_prepare(t.handle, 13, 5, i[0], i[1], n, g3, 1, 1, None, C.byref(h)) == UNSUPPORTED and not h.value
    assert lib.fhe_tglwe_atk_prepare(t.handle, 7, 5, i[0], i[1], 128, g3, 1, 1, None, C.byref(h)) == INVALID and not h.value
    sk, gen = fhe.sample_binary(9881, 0, ins[0], n), fhe.Rng(seed=1)
    assert lib.fhe_tglwe_atk_gen(t.handle, 0, 5, P(sk), n, g3, 1, 0.0, gen._h, 0, o[0], o[1], 1, None) == UNSUPPORTED
    assert lib.fhe_tglwe_atk_gen(t.handle, 7, 5, P(sk), n, (C.c_uint32 * 1)(4), 1, 0.0, gen._h, 0, o[0], o[1], 1, None) == INVALID
    torch.cuda.synchronize()
    for x in outs:
        assert bool((x == sentinel).all()), "a refused call wrote"
    key.destroy()
    full.destroy()


# ---- decode level -------------------------------------------------------------------------------------------------------------

def test_ring_pack_with_noisy_keys_is_inside_the_bound(fhe, torch_cuda, tctx):
    """n = 256, gadget (7, 5), keys and inputs at std_dev = 2^-50 (about 2^14 on the torus), 8 inputs at scale 2^50 with 3-bit signed
    messages (the top 8 bits of the message space empty).  The model on the same rows must decode and stay inside
    trace_error_bound with the measured noise maxima; the library's bits are the model's."""
    X = fhe.tfhe_trace
    n, log_b, d, count, p, std = 256, 7, 5, 8, 50, 2.0 ** -50
    like = dev(torch_cuda, U([0]))
    s = fhe.sample_binary(9890, 0, like, n)
    sh = host(s)
    gs = M.galois_set(n)
    atk = X.atk_gen(tctx, log_b, d, s, n, gs, std, 9891, 1)
    key = X.AutoKey(tctx, log_b, d, atk[0], atk[1], n, gs)
    rng = np.random.Generator(np.random.PCG64(9892))
    ms = [int(v) for v in rng.integers(-4, 4, size=count)]
    ct = fhe.tlwe_sk_encrypt(s, dev(torch_cuda, U([(m << p) % M64 for m in ms])), n, count, std, 9893, 0)
    ha, hb = host(ct[0]), host(ct[1])
    # the noise that is really there: the keys' rows against their plaintexts, the inputs against their messages
    plain = M.atk_plain(log_b, d, sh, gs)
    ka, kb = host(atk[0]), host(atk[1])
    e_key = max(abs(MM.centred((x - int(y)) % M64)) for q in range(len(gs)) for j in range(d)
                for x, y in zip(MM.phase(ka[q, j], kb[q, j], sh), plain[q, j]))
    e_in = max(abs(MM.centred((MM.phase(*M.embed(ha[r], hb[r]), sh)[0] - (ms[r] << p)) % M64)) for r in range(count))
    bound = M.trace_error_bound(n, log_b, d, M.log2(n), e_in, e_key)
    assert bound < 1 << (p + 8 - 1), "the bound itself must leave the message readable"
    ma, mb = M.ring_pack(log_b, d, M.key_dict(gs, ka, kb, d, n), [(ha[r], hb[r]) for r in range(count)])
    ph = MM.phase(ma, mb, sh)
    want = [0] * n
    for r, m in enumerate(ms):
        want[r * (n // count)] = n * (m << p)
    errs = [abs(MM.centred((ph[i] - want[i]) % M64)) for i in range(n)]
    assert max(errs) <= bound, (max(errs), bound)
    for r, m in enumerate(ms):  # the model itself decodes at n 2^p
        assert MM.s64((ph[r * (n // count)] + (1 << (p + 7))) % M64) >> (p + 8) == m, r
    ga, gb = X.ring_pack(key, ct[0].reshape(1, count, n), ct[1].reshape(1, count), count)
    assert np.array_equal(host(ga)[0], M.u64((ma, mb))[0]) and np.array_equal(host(gb)[0], M.u64((ma, mb))[1])
    key.destroy()


def test_matvec_decodes(fhe, torch_cuda, tctx):
    """a 4 x 8 matrix and a vector of 8, entries in [-3, 3], n = 256, n_in = 8, noise-free keys and inputs, p = 44; packing gadget
    (16, 4) and trace gadget (8, 8) are exact (log_b d = 64), relinearisation gadget (8, 7): coefficient i < 4 of the result decodes to
    (M x)_i at scale n 2^p, the other coefficients to zero"""
    X, XM = fhe.tfhe_trace, fhe.tfhe_mul
    n, n_in, p, r, m = 256, 8, 44, 4, 8
    like = dev(torch_cuda, U([0]))
    z, s = fhe.sample_binary(9900, 0, like, n_in), fhe.sample_binary(9900, 1, like, n)
    pfksk = fhe.tfhe_cbs.pfksk_gen(tctx, 16, 4, z, s, fhe.pack_funcs(n, like), 0.0, 9901, 2)
    pk = fhe.PackKey(tctx, 16, 4, pfksk, n_in, n)
    rlk = XM.rlk_gen(tctx, 8, 7, s, n, 0.0, 9902, 3)
    rk = XM.RelinKey(tctx, 8, 7, rlk[0], rlk[1], n)
    gs = M.galois_set(n)
    atk = X.atk_gen(tctx, 8, 8, s, n, gs, 0.0, 9903, 4)
    ak = X.AutoKey(tctx, 8, 8, atk[0], atk[1], n, gs)
    rng = np.random.Generator(np.random.PCG64(9904))
    mat, vec = rng.integers(-3, 4, size=(r, m)), rng.integers(-3, 4, size=m)
    enc = lambda vals, seed: fhe.tlwe_sk_encrypt(z, dev(torch_cuda, U([(int(v) << p) % M64 for v in vals])), n_in, len(vals), 0.0, seed, 0)  # noqa: E731
    rows = enc(mat.reshape(-1), 9905)
    xs = enc(vec, 9906)
    oa, ob = X.matvec(pk, rk, ak, (rows[0].reshape(r, m, n_in), rows[1].reshape(r, m)), xs, p)
    want = X.matvec_plain(mat.tolist(), vec.tolist())
    assert want == [int(v) for v in mat @ vec]
    ph = MM.phase(host(oa)[0], host(ob)[0], host(s))
    got = [MM.s64((v + (1 << (p + 7))) % M64) >> (p + 8) for v in ph]
    assert got == want + [0] * (n - r)
    for k in (pk, rk, ak):
        k.destroy()


def test_c_program_tfhe_trace(tmp_path, fhe):
    """examples/tfhe_trace_demo.c: eight TLWE ciphertexts ring-packed into one TGLWE ciphertext and decrypted in the program, from plain C
    against include/fhe_ring.h alone"""
    from conftest import ROOT
    lib_dir = os.path.dirname(fhe.lib_path())
    exe = tmp_path / "tfhe_trace_demo"
    cmd = ["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "tfhe_trace_demo.c"), "-o", str(exe),
           "-L", lib_dir, "-lfhe_ring", "-Wl,--allow-shlib-undefined", "-Wl,-rpath," + lib_dir, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tfhe_trace_demo ok" in r.stdout, r.stdout + r.stderr
