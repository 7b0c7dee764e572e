"""GPU tests of the TGLWE ciphertext product (k = 1): fhe_tglwe_tensor, fhe_tglwe_relin and fhe_tglwe_mul bit-exact against the model of
tests/tfhe_mul_model.py in both memory kinds and at every ring, the relinearisation also against the external-product route, the
device-made key against fhe_tglwe_sk_encrypt, rejections, aliasing, odd alignment, a side stream, the helpers lwe_mul and dot at decode
level, and the C demo.  Every comparison of ciphertext words is exact equality."""
import os
import subprocess

import numpy as np
import pytest

import tfhe_mul_model as M

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


def operand_sets(rng, n, batch, p):
    """name -> (a1, b1, a2, b2) [batch][n]: random words; every word -2^63 (the largest magnitude: the piece integers reach n 2^94 and
    the middle term 2 n 2^126 -- the 128-bit recombination carries); every word 2^63 - 1; operands whose products land on rounding
    ties: ct0 = (1, -1) as constants, so that T = a2, R = b2 - a2, B = -b2, with a2 = 2^(p - 1) mod 2^p everywhere and b2 = 2^(p - 1) or
    0 mod 2^p in turn (random bits above: ties of both signs)"""
    full = lambda w: np.full((batch, n), w, dtype=np.uint64)  # noqa: E731
    sets = {"random": tuple(r64(rng, batch, n) for _ in range(4)), "min": (full(1 << 63),) * 4, "max": (full((1 << 63) - 1),) * 4}
    one, minus = np.zeros((batch, n), dtype=np.uint64), np.zeros((batch, n), dtype=np.uint64)
    one[:, 0], minus[:, 0] = 1, M64 - 1
    hi_mask = np.uint64((M64 - 1) ^ ((1 << p) - 1))
    a2 = (r64(rng, batch, n) & hi_mask) | np.uint64(1 << (p - 1))
    b2 = r64(rng, batch, n) & hi_mask
    b2[:, ::2] |= np.uint64(1 << (p - 1))
    sets["ties"] = (one, minus, a2, b2)
    return sets


def model_tensor(ops, n, p):
    a1, b1, a2, b2 = ops
    if all((x == x[0, 0]).all() for x in ops):  # every row the same: one row of the model
        c = M.tensor(a1[:1], b1[:1], a2[:1], b2[:1], n, p)
        return tuple(np.repeat(x, a1.shape[0], axis=0) for x in c)
    return M.tensor(a1, b1, a2, b2, n, p)


def check_tensor(fhe, torch, t, n, batch, p, seed):
    X = fhe.tfhe_mul
    rng = np.random.Generator(np.random.PCG64(seed))
    for name, ops in operand_sets(rng, n, batch, p).items():
        want = model_tensor(ops, n, p)
        if name == "ties":
            half = np.uint64(1 << (p - 1))
            mask = np.uint64((1 << p) - 1)
            assert ((ops[2] & mask) == half).all() and (((ops[3] - ops[2]) & mask)[:, 1::2] == half).all()  # T and half of R are ties
        got = X.tensor(t, *(dev(torch, np.array(x)) for x in ops), n, p)
        for i in range(3):
            assert np.array_equal(host(got[i]), want[i]), ("device memory", name, "c%d" % i)
        goth = X.tensor(t, *(np.array(x) for x in ops), n, p)
        for i in range(3):
            assert np.array_equal(goth[i], want[i]), ("host memory", name, "c%d" % i)


@pytest.mark.parametrize("p", [1, 32, 56, 63])
@pytest.mark.parametrize("batch", [1, 5])
def test_tensor_bit_exact_n256(fhe, torch_cuda, tctx, batch, p):
    """n = 256: four teams a block, batch 5 leaves the second block one team"""
    check_tensor(fhe, torch_cuda, tctx, 256, batch, p, 9500 + 10 * p + batch)


@pytest.mark.parametrize("n,p", [(512, 56), (1024, 32), (2048, 63)])
def test_tensor_bit_exact_every_ring(fhe, torch_cuda, tctx, n, p):
    """one wave of 8 coefficients a lane (512), four and eight waves of 4 a lane (1024, 2048)"""
    check_tensor(fhe, torch_cuda, tctx, n, 2, p, 9520 + n)


def edge_words(log_b, d):
    """0, 2^63, 2^63 - 1, 2^64 - 1, values whose digits are all +2^(log_b - 1) resp. -2^(log_b - 1) (a carry through every level), and the
    rounding ties of the decomposition: half a unit of the last digit above and just below"""
    rb, half = 64 - log_b * d, 1 << (log_b - 1)
    up = sum(half << (rb + j * log_b) for j in range(d)) % M64
    tie = (1 << rb) // 2
    return [0, 1 << 63, (1 << 63) - 1, M64 - 1, up, (-up) % M64, (up + tie - (1 if rb else 0)) % M64, tie, (tie - 1) % M64, (M64 - tie) % M64]


def relin_inputs(rng, log_b, d, n, batch):
    rlk_a, rlk_b = r64(rng, d, n), r64(rng, d, n)
    rlk_a[:, 0], rlk_b[:, n - 1] = np.uint64(1 << 63), np.uint64(M64 - 1)
    c0, c1, c2 = r64(rng, batch, n), r64(rng, batch, n), r64(rng, batch, n)
    e = U(edge_words(log_b, d))
    c2[0, :e.size] = e
    c2[batch - 1, n - e.size:] = e
    return rlk_a, rlk_b, c0, c1, c2


def check_relin(fhe, torch, t, log_b, d, n, batch, seed):
    X = fhe.tfhe_mul
    rng = np.random.Generator(np.random.PCG64(seed))
    rlk_a, rlk_b, c0, c1, c2 = relin_inputs(rng, log_b, d, n, batch)
    want_a, want_b = M.relin(log_b, d, rlk_a, rlk_b, c0, c1, c2, n)
    dka, dkb, d0, d1, d2 = (dev(torch, x) for x in (rlk_a, rlk_b, c0, c1, c2))
    key = X.RelinKey(t, log_b, d, dka, dkb, n)
    ga, gb = X.relin(key, d0, d1, d2)
    assert np.array_equal(host(ga), want_a) and np.array_equal(host(gb), want_b), "device memory"
    ca, cb = X.relin_composed(t, log_b, d, dka, dkb, d0, d1, d2, n)
    assert np.array_equal(host(ca), want_a) and np.array_equal(host(cb), want_b), "external-product route"
    hkey = X.RelinKey(t, log_b, d, rlk_a, rlk_b, n)
    ha, hb = X.relin(hkey, c0, c1, c2)
    assert np.array_equal(ha, want_a) and np.array_equal(hb, want_b), "host memory"
    X.relin(key, d0, d1, d2, out=(d1, d0))  # out aliases (c1, c0)
    assert np.array_equal(host(d1), want_a) and np.array_equal(host(d0), want_b), "out = (c1, c0)"
    key.destroy()
    hkey.destroy()


@pytest.mark.parametrize("log_b,d", GADGETS_256)
def test_relin_bit_exact_n256(fhe, torch_cuda, tctx, log_b, d):
    check_relin(fhe, torch_cuda, tctx, log_b, d, 256, 5, 9540 + log_b)


@pytest.mark.parametrize("n", OTHER_RINGS)
def test_relin_bit_exact_every_ring(fhe, torch_cuda, tctx, n):
    check_relin(fhe, torch_cuda, tctx, 7, 5, n, 2, 9550 + n)


def check_mul(fhe, torch, t, log_b, d, n, batch, p, seed):
    """mul == relin(tensor) == model; then a square (ct0 is ct1), out = ct0, pointers 8 but not 16 bytes aligned, a side stream"""
    X = fhe.tfhe_mul
    rng = np.random.Generator(np.random.PCG64(seed))
    rlk_a, rlk_b = r64(rng, d, n), r64(rng, d, n)
    ops = [r64(rng, batch, n) for _ in range(4)]
    ops[0][0, :4], ops[3][batch - 1, -4:] = U([1 << 63, (1 << 63) - 1, 0, M64 - 1]), U([1 << 63, (1 << 63) - 1, 0, M64 - 1])
    want_a, want_b = M.mul(log_b, d, rlk_a, rlk_b, *ops, n, p)
    key = X.RelinKey(t, log_b, d, dev(torch, rlk_a), dev(torch, rlk_b), n)
    dops = [dev(torch, x) for x in ops]
    ga, gb = X.mul(key, *dops, p)
    assert np.array_equal(host(ga), want_a) and np.array_equal(host(gb), want_b), "fused, device memory"
    ra, rb = X.relin(key, *X.tensor(t, *dops, n, p))
    assert np.array_equal(host(ra), want_a) and np.array_equal(host(rb), want_b), "relin(tensor)"
    ha, hb = X.mul(key, *ops, p)
    assert np.array_equal(ha, want_a) and np.array_equal(hb, want_b), "fused, host memory"
    # a square, written over its input
    sq_a, sq_b = M.mul(log_b, d, rlk_a, rlk_b, ops[0], ops[1], ops[0], ops[1], n, p)
    xa, xb = dops[0].clone(), dops[1].clone()
    X.mul(key, xa, xb, xa, xb, p, out=(xa, xb))
    assert np.array_equal(host(xa), sq_a) and np.array_equal(host(xb), sq_b), "square, out = ct0"
    # out = ct1
    ya, yb = dops[2].clone(), dops[3].clone()
    X.mul(key, dops[0], dops[1], ya, yb, p, out=(ya, yb))
    assert np.array_equal(host(ya), want_a) and np.array_equal(host(yb), want_b), "out = ct1"
    # every pointer 8 but not 16 bytes past an allocation's start
    odd = [torch.empty(batch * n + 1, dtype=torch.int64, device="cuda")[1:] for _ in range(6)]
    for o, x in zip(odd, dops):
        o.copy_(x.reshape(-1))
    assert all(o.data_ptr() % 16 == 8 for o in odd)
    X.mul(key, odd[0], odd[1], odd[2], odd[3], p, out=(odd[4], odd[5]))
    assert np.array_equal(host(odd[4]).reshape(batch, n), want_a) and np.array_equal(host(odd[5]).reshape(batch, n), want_b), "odd alignment"
    # a side stream: the inputs are made on it, the call follows them there
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    mask = 0x5555555555555555
    with torch.cuda.stream(side):
        sops = [(x ^ mask) ^ mask for x in dops]
        sa, sb = X.mul(key, *sops, p)
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(host(sa), want_a) and np.array_equal(host(sb), want_b), "side stream"
    key.destroy()


@pytest.mark.parametrize("log_b,d,p", [(7, 5, 56), (4, 2, 1), (16, 3, 32), (31, 2, 63)])
def test_mul_bit_exact_n256(fhe, torch_cuda, tctx, log_b, d, p):
    check_mul(fhe, torch_cuda, tctx, log_b, d, 256, 5, p, 9560 + log_b)


@pytest.mark.parametrize("n,p", [(512, 56), (1024, 56), (2048, 32)])
def test_mul_bit_exact_every_ring(fhe, torch_cuda, tctx, n, p):
    check_mul(fhe, torch_cuda, tctx, 7, 5, n, 2, p, 9570 + n)


@pytest.mark.parametrize("n,log_b,d", [(256, 7, 5), (1024, 16, 4)])
def test_rlk_gen_rows(fhe, torch_cuda, tctx, n, log_b, d):
    """the rows are fhe_tglwe_sk_encrypt's on the plaintext rows h_j S^2 for the same generator and stream_id, bit for bit; at
    std_dev = 0 every row's phase is h_j S^2 exactly"""
    X = fhe.tfhe_mul
    like = dev(torch_cuda, U([0]))
    sk = fhe.sample_binary(9580, 0, like, n)
    plain = M.rlk_plain(log_b, d, host(sk))
    for std_dev in (0.0, 2.0 ** -40):
        ra, rb = X.rlk_gen(tctx, log_b, d, sk, n, std_dev, 9581, 7)
        ea, eb = fhe.tglwe_sk_encrypt(tctx, sk, dev(torch_cuda, plain), n, d, std_dev, 9581, 7)
        assert np.array_equal(host(ra), host(ea)) and np.array_equal(host(rb), host(eb)), std_dev
    ra, rb = X.rlk_gen(tctx, log_b, d, sk, n, 0.0, 9581, 7)
    ha, hb = X.rlk_gen(tctx, log_b, d, host(sk).copy(), n, 0.0, 9581, 7)  # host memory
    assert np.array_equal(ha, host(ra)) and np.array_equal(hb, host(rb))
    for j in range(d):
        assert M.phase(ha[j], hb[j], host(sk)) == [int(v) for v in plain[j]], j


def test_rejections_write_nothing(fhe, torch_cuda):
    import ctypes as C
    torch = torch_cuda
    n, log_b, d = 256, 7, 5
    t, other = fhe.TorusContext(), fhe.TorusContext()
    rng = np.random.Generator(np.random.PCG64(9590))
    key = fhe.tfhe_mul.RelinKey(t, log_b, d, dev(torch, r64(rng, d, n)), dev(torch, r64(rng, d, n)), n)
    ins = [dev(torch, r64(rng, 1, n)) for _ in range(4)]
    sentinel = 0x6b6b6b6b6b6b6b6b
    outs = [torch.full((1, n), sentinel, dtype=torch.int64, device="cuda") for _ in range(3)]
    lib = fhe.lib()
    P = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    i, o = [P(x) for x in ins], [P(x) for x in outs]
    INVALID, UNSUPPORTED = 1, 6
    for p in (0, 64):
        assert lib.fhe_tglwe_tensor(t.handle, i[0], i[1], i[2], i[3], n, p, o[0], o[1], o[2], 1, 1, None) == INVALID
        assert lib.fhe_tglwe_mul(t.handle, key._h, i[0], i[1], i[2], i[3], p, o[0], o[1], 1, 1, None) == INVALID
    assert lib.fhe_tglwe_tensor(t.handle, i[0], i[1], i[2], i[3], 384, 32, o[0], o[1], o[2], 1, 1, None) == INVALID
    assert lib.fhe_tglwe_tensor(t.handle, i[0], i[1], i[2], i[3], n, 32, o[0], None, o[2], 1, 1, None) == INVALID
    assert lib.fhe_tglwe_tensor(t.handle, i[0], i[1], i[2], i[3], n, 32, o[0], o[1], i[0], 1, 1, None) == INVALID     # an output is an input
    part = C.c_void_p(outs[0].data_ptr() + 64)  # eight words into c0: a partial overlap
    assert lib.fhe_tglwe_tensor(t.handle, i[0], i[1], i[2], i[3], n, 32, o[0], part, o[2], 1, 1, None) == INVALID
    assert lib.fhe_tglwe_mul(other.handle, key._h, i[0], i[1], i[2], i[3], 32, o[0], o[1], 1, 1, None) == INVALID     # a key of another context
    assert lib.fhe_tglwe_relin(other.handle, key._h, i[0], i[1], i[2], o[0], o[1], 1, 1, None) == INVALID
    assert lib.fhe_tglwe_relin(t.handle, None, i[0], i[1], i[2], o[0], o[1], 1, 1, None) == INVALID
    assert lib.fhe_tglwe_mul(t.handle, key._h, i[0], i[1], i[2], None, 32, o[0], o[1], 1, 1, None) == INVALID
    h = C.c_void_p()
    assert lib.fhe_tglwe_rlk_prepare(t.handle, 13, 5, i[0], i[1], n, 1, None, C.byref(h)) == UNSUPPORTED and not h.value
    assert lib.fhe_tglwe_rlk_prepare(t.handle, 46, 1, i[0], i[1], n, 1, None, C.byref(h)) == UNSUPPORTED and not h.value
    assert lib.fhe_tglwe_rlk_prepare(t.handle, 7, 5, i[0], i[1], 128, 1, None, C.byref(h)) == INVALID and not h.value
    sk, gen = fhe.sample_binary(9591, 0, ins[0], n), fhe.Rng(seed=1)
    assert lib.fhe_tglwe_rlk_gen(t.handle, 0, 5, P(sk), n, 0.0, gen._h, 0, o[0], o[1], 1, None) == UNSUPPORTED
    assert lib.fhe_tglwe_rlk_gen(t.handle, 7, 5, P(sk), 100, 0.0, gen._h, 0, o[0], o[1], 1, None) == INVALID
    torch.cuda.synchronize()
    for x in outs:
        assert bool((x == sentinel).all()), "a refused call wrote"
    key.destroy()


# ---- decode level -------------------------------------------------------------------------------------------------------------

def make_keys(fhe, torch, t, n, n_in, pf, rl, std_dev, seed):
    """z (TLWE, n_in), s (TGLWE, n); the packing key z -> s under gadget pf, the relinearisation key of s under gadget rl"""
    like = dev(torch, U([0]))
    z, s = fhe.sample_binary(seed, 0, like, n_in), fhe.sample_binary(seed, 1, like, n)
    pfksk = fhe.tfhe_cbs.pfksk_gen(t, pf[0], pf[1], z, s, fhe.pack_funcs(n, like), std_dev, seed + 1, 2)
    rlk = fhe.tfhe_mul.rlk_gen(t, rl[0], rl[1], s, n, std_dev, seed + 2, 3)
    return z, s, fhe.PackKey(t, pf[0], pf[1], pfksk, n_in, n), fhe.tfhe_mul.RelinKey(t, rl[0], rl[1], rlk[0], rlk[1], n)


def encrypt_msgs(fhe, torch, z, msgs, n_in, p, std_dev, seed):
    return fhe.tlwe_sk_encrypt(z, dev(torch, U([(m << p) % M64 for m in msgs])), n_in, len(msgs), std_dev, seed, 0)


def lwe_phase_err(s, ct, want, p):
    """centred phase error of one TLWE ciphertext (a [n], b) under s against want 2^p"""
    from oracle import pyref as P
    ph = P.tlwe_phase([int(x) for x in s], [int(x) for x in ct[0]], int(ct[1]))
    return P.t64_to_i64((ph - (want << p)) % M64)


def test_lwe_mul_and_dot_noise_free(fhe, torch_cuda, tctx):
    """n = 256, n_in = 8, keys and inputs at std_dev = 0, packing gadget (16, 4) (log_b d = 64: the pack is exact), relinearisation gadget
    (7, 5), p = 48.  lwe_mul on a batch of pairs and dot on 8 and on 256 entries decrypt to the plain helpers' values; the phase error
    is inside tfhe_mul_model.mul_error_bound with e = 0 (the roundings of C0, C1, C2 and of the digits)"""
    X = fhe.tfhe_mul
    n, n_in, p, rl = 256, 8, 48, (7, 5)
    z, s, pk, rk = make_keys(fhe, torch_cuda, tctx, n, n_in, (16, 4), rl, 0.0, 9600)
    sh = host(s)
    rng = np.random.Generator(np.random.PCG64(9601))
    xs, ys = [int(v) for v in rng.integers(-100, 101, size=6)] + [127, -128], [int(v) for v in rng.integers(-100, 101, size=6)] + [-128, -128]
    cx, cy = encrypt_msgs(fhe, torch_cuda, z, xs, n_in, p, 0.0, 9602), encrypt_msgs(fhe, torch_cuda, z, ys, n_in, p, 0.0, 9603)
    oa, ob = X.lwe_mul(pk, rk, cx, cy, p)
    want = X.lwe_mul_plain(xs, ys)
    ha, hb = host(oa).reshape(len(xs), n), host(ob).reshape(-1)
    for r in range(len(xs)):
        bound = M.mul_error_bound(n, rl[0], rl[1], p, max(abs(xs[r]), abs(ys[r])), 0)
        err = lwe_phase_err(sh, (ha[r], hb[r]), want[r], p)
        assert abs(err) <= bound and bound < 1 << (p - 1), (r, err, bound)
    for m in (8, 256):
        xs, ys = [int(v) for v in rng.integers(-7, 8, size=m)], [int(v) for v in rng.integers(-7, 8, size=m)]
        cx, cy = encrypt_msgs(fhe, torch_cuda, z, xs, n_in, p, 0.0, 9604 + m), encrypt_msgs(fhe, torch_cuda, z, ys, n_in, p, 0.0, 9605 + m)
        oa, ob = X.dot(pk, rk, cx, cy, p)
        want = X.dot_plain(xs, ys)
        bound = M.mul_error_bound(n, rl[0], rl[1], p, 7 * m, 0)
        err = lwe_phase_err(sh, (host(oa).reshape(n), host(ob).reshape(-1)[0]), want, p)
        assert abs(err) <= bound and bound < 1 << (p - 1), (m, err, bound)
    pk.destroy()
    rk.destroy()


def test_dot_with_noisy_keys_decodes(fhe, torch_cuda, tctx):
    """n = 256, n_in = 8, every key and input at std_dev = 2^-55 (about 2^9 on the torus), gadgets (8, 7) and (7, 7), p = 52, 16
    entries in [-3, 3].  The parameters are chosen so that the model decodes: the test runs tfhe_mul_model.mul on the packed operands
    first and asserts that its phase rounds to the inner product, then asserts that the library's bits are the model's."""
    X = fhe.tfhe_mul
    n, n_in, p, rl, m, std = 256, 8, 52, (7, 7), 16, 2.0 ** -55
    z, s, pk, rk = make_keys(fhe, torch_cuda, tctx, n, n_in, (8, 7), rl, std, 9620)
    rng = np.random.Generator(np.random.PCG64(9621))
    xs, ys = [int(v) for v in rng.integers(-3, 4, size=m)], [int(v) for v in rng.integers(-3, 4, size=m)]
    cx, cy = encrypt_msgs(fhe, torch_cuda, z, xs, n_in, p, std, 9622), encrypt_msgs(fhe, torch_cuda, z, ys, n_in, p, std, 9623)
    want = X.dot_plain(xs, ys)
    # the model on the same packed operands and the same key rows
    full = n
    ya, yb = torch_cuda.zeros((full, n_in), dtype=torch_cuda.int64, device="cuda"), torch_cuda.zeros((full,), dtype=torch_cuda.int64, device="cuda")
    ya[0], yb[0] = cy[0][0], cy[1][0]
    ya[full - m + 1:], yb[full - m + 1:] = -cy[0][1:].flip(0), -cy[1][1:].flip(0)
    px = fhe.pack(pk, cx[0].reshape(1, m, n_in).contiguous(), cx[1].reshape(1, m).contiguous(), m, 1)
    py = fhe.pack(pk, ya.reshape(1, full, n_in), yb.reshape(1, full), full, 1)
    rlk = X.rlk_gen(tctx, rl[0], rl[1], s, n, std, 9622, 3)  # make_keys' draw: seed + 2, stream 3
    ma, mb = M.mul(rl[0], rl[1], host(rlk[0]), host(rlk[1]), host(px[0]), host(px[1]), host(py[0]), host(py[1]), n, p)
    ph0 = M.phase(ma[0], mb[0], host(s))[0]
    assert M.s64((ph0 + (1 << (p - 1))) % M64) >> p == want, "the model itself must decode at these parameters"
    oa, ob = X.dot(pk, rk, cx, cy, p)
    ea, eb = fhe.tglwe_sample_extract(dev(torch_cuda, ma), dev(torch_cuda, mb), n, 0)
    assert np.array_equal(host(oa), host(ea)) and np.array_equal(host(ob), host(eb)), "dot == sample_extract(model mul)"
    err = lwe_phase_err(host(s), (host(oa).reshape(n), host(ob).reshape(-1)[0]), want, p)
    assert abs(err) < 1 << (p - 1)
    pk.destroy()
    rk.destroy()


def test_c_program_tfhe_mul(tmp_path, fhe):
    """examples/tfhe_mul_demo.c: two short vectors encrypted as TLWE, packed, multiplied, extracted and decrypted in the program, from
    plain C against include/fhe_ring.h alone"""
    from conftest import ROOT
    lib_dir = os.path.dirname(fhe.lib_path())
    exe = tmp_path / "tfhe_mul_demo"
    cmd = ["gcc", "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "tfhe_mul_demo.c"), "-o", str(exe),
           "-L", lib_dir, "-lfhe_ring", "-Wl,--allow-shlib-undefined", "-Wl,-rpath," + lib_dir, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tfhe_mul_demo ok" in r.stdout, r.stdout + r.stderr
