"""GPU tests of the CKKS encoder (include/fhe_ring.h fhe_ckks_encoder_* / fhe_ckks_sifft / fhe_ckks_sfft / fhe_ckks_encode /
fhe_ckks_decode: scheme/ckks/src/ckks.rs:186-213 over scheme/ckks/src/sfft.rs:7-72 in double-double arithmetic) against the exact
model of tests/ckks_encode_model.py.  Batches of 1 and 3 throughout, so that a batch stride error shows.

Bounds.  Transforms: 2^-95 max|z| (the issue's; dd carries 2^-106 per operation and a transform is at most 14 butterflies deep).
Encode: every coefficient within 1 of the model's integer, and equal wherever the model's exact z scale lies farther than 2^-30 from
an integer -- dd unit roundoff 2^-105 x about 2^4 operations deep x a scale below 2^61 gives about 2^-40 integer units, 2^-30 leaves
room -- an exemption the model alone decides and that may cover at most 1 coefficient in 1000.  Decode: 2^-95 of the largest value."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import ckks_encode_model as Mo

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = Mo.mpf(2) ** -95
INVALID = 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def log2(x):
    return float(Mo.M.log(Mo.mpf(x) + Mo.mpf(2) ** -300, 2))


def cerr(got, want):
    return max(max(abs(g.real - t.real), abs(g.imag - t.imag)) for g, t in zip(got, want))


_MSG = {}


def messages(l):
    """Three messages [3][l] (high words, low words) and the model's sifft of each, computed once per size.  Above l = 1024 the second
    and third are exact multiples of the first (x / 2, -x / 4), for which the model's answer is the same multiple."""
    if l not in _MSG:
        rng = np.random.Generator(np.random.PCG64(100 + l))
        draw = lambda: (rng.uniform(-1, 1, l) + 1j * rng.uniform(-1, 1, l), (rng.uniform(-1, 1, l) + 1j * rng.uniform(-1, 1, l)) * 2.0 ** -55)  # noqa: E731
        h0, l0 = draw()
        if l <= 1024:
            (h1, l1), (h2, l2) = draw(), draw()
            hi, lo = np.stack([h0, h1, h2]), np.stack([l0, l1, l2])
            want = [Mo.sifft(Mo.cfrom(hi[b], lo[b])) for b in range(3)]
        else:
            hi, lo = np.stack([h0, h0 / 2, -h0 / 4]), np.stack([l0, l0 / 2, -l0 / 4])
            w0 = Mo.sifft(Mo.cfrom(h0, l0))
            want = [w0, [v / 2 for v in w0], [-v / 4 for v in w0]]
        _MSG[l] = (hi, lo, want)
    return _MSG[l]


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dd") / "dd_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "dd_host_test.cpp")])
    return exe


# log_n = 1 .. 10; l = 4096 is the largest size of the LDS route, l = 8192 the only size with one register stage in front of it
# (S = 1), l = 16384 (n = 2^15) the size with two (S = 2)
@pytest.mark.parametrize("log_n", list(range(1, 11)) + [13, 14, 15])
def test_transforms_against_the_model(fhe, torch_cuda, log_n):
    n, l = 1 << log_n, 1 << (log_n - 1)
    enc = fhe.CkksEncoder(n)
    hi, lo, want = messages(l)
    scale = [max(max(abs(v.real), abs(v.imag)) for v in Mo.cfrom(hi[b], lo[b])) for b in range(3)]
    zh, zl = dev(torch_cuda, hi), dev(torch_cuda, lo)
    enc.sifft(zh, zl)
    gh, gl = host(zh), host(zl)
    for b in range(3):
        e = cerr(Mo.cfrom(gh[b], gl[b]), want[b])
        print("n=2^%d message %d: sifft error 2^%.1f max|z|" % (log_n, b, log2(e / scale[b])))
        assert e <= BOUND * scale[b]
    enc.sfft(zh, zl)
    bh, bl = host(zh), host(zl)
    for b in range(3):
        e = cerr(Mo.cfrom(bh[b], bl[b]), Mo.cfrom(hi[b], lo[b]))
        print("n=2^%d message %d: sfft(sifft) error 2^%.1f max|z|" % (log_n, b, log2(e / scale[b])))
        assert e <= BOUND * scale[b]
    # batch 1: the bits of message 0 of the batch of 3
    z1h, z1l = dev(torch_cuda, hi[:1]), dev(torch_cuda, lo[:1])
    enc.sifft(z1h, z1l)
    assert np.array_equal(host(z1h)[0], gh[0]) and np.array_equal(host(z1l)[0], gl[0])
    # no low words: zeros in, only the f64-rounded value out -- the high words of the same transform
    z0 = dev(torch_cuda, hi[:1])
    enc.sifft(z0)
    zz_h, zz_l = dev(torch_cuda, hi[:1]), dev(torch_cuda, np.zeros_like(lo[:1]))
    enc.sifft(zz_h, zz_l)
    assert np.array_equal(host(z0), host(zz_h))
    # host memory
    nh, nl = hi.copy(), lo.copy()
    enc.sifft(nh, nl)
    assert np.array_equal(nh, gh) and np.array_equal(nl, gl)
    enc.status(zh)


def test_device_and_host_header_agree_bit_for_bit(fhe, torch_cuda, host_exe):
    """Sizes the host loops of csrc/dd.hpp serve as well: both run the same operations on the same values in the same order (DESIGN.md
    section 4.9), so every word is equal."""
    for l in (1, 2, 8, 64, 1024):
        hi, lo, _ = messages(l)
        text = "F %d\n" % l + "".join("%s %s %s %s\n" % (float(h.real).hex(), float(o.real).hex(), float(h.imag).hex(), float(o.imag).hex())
                                      for h, o in zip(hi[1], lo[1]))
        out = subprocess.run([host_exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        rows = np.array([[float.fromhex(t) for t in line.split()] for line in out.stdout.split("\n")[:2 * l]])
        enc = fhe.CkksEncoder(2 * l)
        zh, zl = dev(torch_cuda, hi[1:2]), dev(torch_cuda, lo[1:2])
        for op, part in ((enc.sifft, rows[:l]), (enc.sfft, rows[l:])):
            op(zh, zl)
            gh, gl = host(zh)[0], host(zl)[0]
            got = np.stack([gh.real, gl.real, gh.imag, gl.imag], axis=1)
            assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(part).view(np.uint64)), l


def primes(cref, bits, log_n, count):
    return cref.two_adic_primes(bits, log_n + 1, count)


def check_encode(fhe, torch, enc, rns, qs, scale, hi, lo, exact_ints_only=False, want=None):
    """encode [batch][l] on the device against the model (want: the model's sifft of each message, where the caller has it already);
    returns (coefficients, coefficients the model exempts from equality)"""
    n, l, batch = enc.n, enc.l, hi.shape[0]
    pt = host(enc.encode(rns, scale, dev(torch, hi), None if lo is None else dev(torch, lo)))
    assert pt.shape == (batch, len(qs), n)
    exempt = total = 0
    margin = Mo.mpf(2) ** -30
    for b in range(batch):
        if want is None:
            exact = Mo.encode_exact(Mo.cfrom(hi[b], None if lo is None else lo[b]), scale)
        else:
            exact = [v.real * scale for v in want[b]] + [v.imag * scale for v in want[b]]
        for c in range(n):
            v = Mo.to_bigint(exact[c])
            near = exact_ints_only or abs(exact[c] - Mo.M.nint(exact[c])) <= margin
            exempt += bool(near) and not exact_ints_only
            total += 1
            row = pt[b, :, c]
            for j, q in enumerate(qs):
                d = (int(row[j]) - v) % q
                assert d in ((0, 1, q - 1) if near else (0,)), (b, j, c, d)
    return total, exempt


ENCODE_CASES = [
    # log_n, (bits of the moduli, L), scale: "last" = qs[-1] of P.ckks_primes(log_n, 55, 8), else the bit length of a prime
    (5, (55, 8), "last"),
    (1, (55, 8), "last"),
    (9, (55, 8), "last"),
    (10, (61, 2), 61),
    (4, (30, 1), 30),
    (7, (61, 8), 30),
    (6, (30, 2), 55),
    (3, (55, 1), 61),
    (14, (55, 2), 61),   # l = 8192: the two-pass route (one register stage) with the tail behind its LDS kernel
    (15, (61, 2), 55),   # l = 16384, the cfg4 size: two register stages in front
]


@pytest.mark.parametrize("log_n,mods,scale_kind", ENCODE_CASES)
def test_encode_against_the_models_integers(fhe, cref, torch_cuda, log_n, mods, scale_kind):
    from oracle import pyref as P
    n, l = 1 << log_n, 1 << (log_n - 1)
    bits, big_l = mods
    if (bits, big_l) == (55, 8):
        qs, ps = P.ckks_primes(log_n, 55, 8)
    else:
        pr = primes(cref, bits, log_n, big_l + 1)
        qs, ps = pr[:big_l], pr[big_l:]
    scale = P.ckks_primes(log_n, 55, 8)[0][-1] if scale_kind == "last" else primes(cref, scale_kind, log_n, 1)[0]
    assert scale.bit_length() == (55 if scale_kind == "last" else scale_kind)
    rns, enc = fhe.RnsContext(qs, ps), fhe.CkksEncoder(n)
    hi, lo, want = messages(l)
    total, exempt = check_encode(fhe, torch_cuda, enc, rns, qs, scale, hi, lo, want=want)  # batch 3, with low words
    if l <= 1024:
        t1, e1 = check_encode(fhe, torch_cuda, enc, rns, qs, scale, hi[:1], None)           # batch 1, no low words
    else:  # (the model's transform of another input would cost seconds: batch 1 keeps its low words)
        t1, e1 = check_encode(fhe, torch_cuda, enc, rns, qs, scale, hi[:1], lo[:1], want=want[:1])
    total, exempt = total + t1, exempt + e1
    assert exempt * 1000 <= max(total, 1000), "%d of %d coefficients within 2^-30 of an integer" % (exempt, total)
    # worst |device - exact| of the sifft entry, in integer units of this scale
    zh, zl = dev(torch_cuda, hi), dev(torch_cuda, lo)
    enc.sifft(zh, zl)
    worst = max(cerr(Mo.cfrom(host(zh)[b], host(zl)[b]), want[b]) for b in range(3)) * scale
    print("n=2^%d scale %d bits: worst |device - exact| of z scale = 2^%.1f integer units; %d of %d coefficients exempt" % (
        log_n, scale.bit_length(), log2(worst), exempt, total))
    # structured inputs: all slots 1 (z = (1, 0, ..): z scale is the integer `scale` exactly, where truncation is least forgiving) and a
    # single non-zero slot; for both only +-1 is required
    ones = np.ones((1, l), dtype=np.complex128)
    check_encode(fhe, torch_cuda, enc, rns, qs, scale, ones, None, exact_ints_only=True)
    single = np.zeros((3, l), dtype=np.complex128)
    single[0, 0], single[1, l - 1], single[2, l // 2] = 1, -1, 1j
    check_encode(fhe, torch_cuda, enc, rns, qs, scale, single, None, exact_ints_only=True)
    enc.status(zh)


@pytest.mark.parametrize("big_l,bits", [(1, 55), (2, 55), (8, 55), (16, 55), (32, 30), (3, 61)])
def test_decode_head_on_known_centred_integers(fhe, cref, torch_cuda, big_l, bits):
    """Plaintexts built on the host from centred integers: message 0 holds the small ones (0, +-1, +-2^54, random 60-bit values, as a
    decryption leaves them: an inexact lift would lose them against Q), message 1 +-(Q - 1) / 2 and full-range values, message 2
    full-range values.  L = 32 = RNS_MAX_LIMBS runs on 30-bit moduli (Q below the f64 range)."""
    import random
    log_n = 4
    n, l = 1 << log_n, 1 << (log_n - 1)
    pr = primes(cref, bits, log_n, big_l + 1)
    qs, ps = pr[:big_l], pr[big_l:]
    big_q = math.prod(qs)
    half = (big_q - 1) // 2
    scale = primes(cref, 55, log_n, 1)[0]
    rnd = random.Random(big_l)
    fit = lambda v: v if abs(v) <= half else v % big_q - big_q * (v % big_q > half)  # noqa: E731
    small = [0, 1, -1, 2 ** 54, -2 ** 54] + [rnd.getrandbits(60) * rnd.choice([1, -1]) for _ in range(n - 5)]
    edge = [half, -half] + [rnd.randrange(-half, half + 1) for _ in range(n - 2)]
    full = [rnd.randrange(-half, half + 1) for _ in range(n)]
    vals = [[fit(v) for v in small], edge, full]
    pt = np.array([[[v % q for v in row] for q in qs] for row in vals], dtype=np.uint64)
    rns, enc = fhe.RnsContext(qs, ps), fhe.CkksEncoder(n)
    want = [Mo.decode(row, scale) for row in vals]
    for batch in (3, 1):
        gh, gl = enc.decode(rns, scale, dev(torch_cuda, pt[:batch]), want_lo=True)
        only = host(enc.decode(rns, scale, dev(torch_cuda, pt[:batch])))
        gh, gl = host(gh), host(gl)
        for b in range(batch):
            top = max(max(abs(v.real), abs(v.imag)) for v in want[b])
            e = cerr(Mo.cfrom(gh[b], gl[b]), want[b])
            print("L=%d message %d: decode error 2^%.1f of the largest value" % (big_l, b, log2(e / top) if top else 0.0))
            assert e <= BOUND * top
            for g, w in zip(only[b], want[b]):  # m_lo = NULL: the f64 value within one ulp of the model rounded to f64
                for x, y in ((g.real, Mo.rn(w.real)), (g.imag, Mo.rn(w.imag))):
                    assert abs(x - y) <= np.spacing(abs(y)), (x, y)
    hh = enc.decode(rns, scale, pt.copy())  # host memory
    assert np.array_equal(hh, host(enc.decode(rns, scale, dev(torch_cuda, pt))))
    enc.status(dev(torch_cuda, pt))


def test_decode_on_the_two_pass_route(fhe, cref, torch_cuda):
    """n = 2^14 (l = 8192): the decode head in front of the LDS kernel's bit-reversed loads, its output through the workspace and the
    register stage.  Decode is linear in the integers, so messages 1 and 2 are exact multiples of message 0 (2 v, -v) and the model
    runs once."""
    import random
    log_n, big_l = 14, 2
    n = 1 << log_n
    pr = primes(cref, 55, log_n, big_l + 1)
    qs, ps = pr[:big_l], pr[big_l:]
    quarter = (math.prod(qs) - 1) // 4
    scale = pr[0]
    rnd = random.Random(14)
    v0 = [0, 1, -1, 2 ** 54, -2 ** 54, quarter, -quarter] + [rnd.randrange(-quarter, quarter + 1) for _ in range(n - 7)]
    vals = [v0, [2 * v for v in v0], [-v for v in v0]]
    pt = np.array([[[v % q for v in row] for q in qs] for row in vals], dtype=np.uint64)
    rns, enc = fhe.RnsContext(qs, ps), fhe.CkksEncoder(n)
    w0 = Mo.decode(v0, scale)
    want = [w0, [2 * v for v in w0], [-v for v in w0]]
    gh, gl = enc.decode(rns, scale, dev(torch_cuda, pt), want_lo=True)
    gh, gl = host(gh), host(gl)
    for b in range(3):
        top = max(max(abs(v.real), abs(v.imag)) for v in want[b])
        e = cerr(Mo.cfrom(gh[b], gl[b]), want[b])
        print("n=2^14 message %d: decode error 2^%.1f of the largest value" % (b, log2(e / top)))
        assert e <= BOUND * top
    one = host(enc.decode(rns, scale, dev(torch_cuda, pt[:1])))  # batch 1, m_lo = NULL: the high words of message 0
    assert np.array_equal(one[0], gh[0])
    enc.status(dev(torch_cuda, pt))


@pytest.mark.parametrize("log_n", range(1, 10))
def test_reference_encrypt_decrypt_and_mul_constant_on_device_entries(fhe, torch_cuda, log_n):
    """scheme/ckks/src/ckks.rs:303-319 `encrypt_decrypt` (2^-40 absolute per component) and one step of ckks.rs:340-357 `mul_constant`
    (2^-32) at the reference's parameters (log_qi = 55, L = 8), every operation a device entry of this library."""
    from oracle import pyref as P
    n, l = 1 << log_n, 1 << (log_n - 1)
    qs, ps = P.ckks_primes(log_n, 55, 8)
    scale = qs[-1]
    hi_ctx, lo_ctx, enc = fhe.RnsContext(qs, ps), fhe.RnsContext(qs[:-1], ps), fhe.CkksEncoder(n)
    rng = np.random.Generator(np.random.PCG64(log_n))
    m = rng.uniform(0, 1, (3, l)) + 1j * rng.uniform(0, 1, (3, l))  # `Standard`: [0, 1)
    like = dev(torch_cuda, np.zeros(1, dtype=np.uint64))
    sk = fhe.sample_zo(0.5, 77, log_n, like, n)
    pk_b, pk_a = hi_ctx.sk_encrypt(sk, None, n, 1, 78, log_n)
    pt = enc.encode(hi_ctx, scale, dev(torch_cuda, m))
    for batch in (3, 1):
        cb, ca = hi_ctx.pk_encrypt(pk_b[0].contiguous(), pk_a[0].contiguous(), pt[:batch].contiguous(), n, batch, 79, log_n)
        got = host(enc.decode(hi_ctx, scale, hi_ctx.decrypt(sk, cb, ca, n)))
        e = max(np.max(np.abs(got.real - m[:batch].real)), np.max(np.abs(got.imag - m[:batch].imag)))
        print("n=2^%d batch %d: encrypt_decrypt error 2^%.1f" % (log_n, batch, math.log2(e)))
        assert e < 2.0 ** -40
    # mul_constant: encode a second message, multiply, rescale; the scale stays qs[-1] (scale^2 / q_last)
    m1 = rng.uniform(0, 1, (3, l)) + 1j * rng.uniform(0, 1, (3, l))
    cb, ca = hi_ctx.pk_encrypt(pk_b[0].contiguous(), pk_a[0].contiguous(), pt, n, 3, 80, log_n)
    ob, oa = hi_ctx.mul_plain(enc.encode(hi_ctx, scale, dev(torch_cuda, m1)), cb, ca, n)
    got = host(enc.decode(lo_ctx, scale, lo_ctx.decrypt(sk, ob, oa, n)))
    want = m * m1
    e = max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag)))
    print("n=2^%d: mul_constant error 2^%.1f" % (log_n, math.log2(e)))
    assert e < 2.0 ** -32
    enc.status(like)


def test_status_word_and_refusals(fhe, cref, torch_cuda):
    from learn_fhe_amd import _lib
    lib = _lib.lib()
    n, l = 16, 8
    pr = primes(cref, 61, 4, 3)
    qs, ps, scale = pr[:2], pr[2:], pr[0]
    rns, enc = fhe.RnsContext(qs, ps), fhe.CkksEncoder(n)

    def status():
        try:
            enc.status(like)
        except fhe.FheError as err:
            return err.code
        return 0

    good = np.full((1, l), 0.5 + 0.25j)
    like = dev(torch_cuda, good)
    for bad_value in (float("nan"), float("inf"), 2.0 ** 70):
        bad = good.copy()
        bad[0, 3] = bad_value
        enc.encode(rns, scale, dev(torch_cuda, bad))  # returns: the device call is asynchronous
        assert status() == INVALID                       # .. and the word tells (and is cleared)
        assert status() == 0
        try:
            enc.encode(rns, scale, bad)                  # host memory: reported by the call itself
        except fhe.FheError as err:
            assert err.code == INVALID
        else:
            raise AssertionError("accepted")
        assert status() == 0
        pt = enc.encode(rns, scale, like)                # the next call works
        assert status() == 0
        back = host(enc.decode(rns, scale, pt))
        assert np.max(np.abs(back - good)) < 2.0 ** -50
    # refusals: none reaches a kernel
    h = C.c_void_p()
    for bad_n in (1, 24, 0, 1 << 16):
        assert lib.fhe_ckks_encoder_create(bad_n, 0, C.byref(h)) == INVALID and not h.value
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    pt = dev(torch_cuda, np.zeros((1, 2, n), dtype=np.uint64))
    st = None
    assert lib.fhe_ckks_encode(enc.handle, rns.handle, scale, None, None, 1, vp(pt), _lib.MEM_DEVICE, st) == INVALID   # NULL m_hi
    assert lib.fhe_ckks_decode(enc.handle, rns.handle, scale, vp(pt), 1, None, None, _lib.MEM_DEVICE, st) == INVALID
    assert lib.fhe_ckks_encode(enc.handle, rns.handle, scale, vp(like), None, 1, None, _lib.MEM_DEVICE, st) == INVALID
    assert lib.fhe_ckks_encode(enc.handle, rns.handle, 0, vp(like), None, 1, vp(pt), _lib.MEM_DEVICE, st) == INVALID
    assert lib.fhe_ckks_sifft(enc.handle, None, None, 1, _lib.MEM_DEVICE, st) == INVALID
    assert lib.fhe_ckks_encode(enc.handle, rns.handle, scale, None, None, 0, None, _lib.MEM_DEVICE, st) == 0              # batch == 0
    assert lib.fhe_ckks_sfft(enc.handle, None, None, 0, _lib.MEM_DEVICE, st) == 0
    host_only = fhe.CkksEncoder(n, device=-1)
    assert lib.fhe_ckks_encode(host_only.handle, rns.handle, scale, vp(like), None, 1, vp(pt), _lib.MEM_DEVICE, st) == INVALID
    assert lib.fhe_ckks_decode(host_only.handle, rns.handle, scale, vp(pt), 1, vp(like), None, _lib.MEM_DEVICE, st) == INVALID
    assert lib.fhe_ckks_sifft(host_only.handle, vp(like), None, 1, _lib.MEM_DEVICE, st) == INVALID
    # an encoder and a context on different devices: a host-only context is on none
    rns_host = fhe.RnsContext(qs, ps, device=-1)
    assert lib.fhe_ckks_encode(enc.handle, rns_host.handle, scale, vp(like), None, 1, vp(pt), _lib.MEM_DEVICE, st) == INVALID
    if torch_cuda.cuda.device_count() > 1:
        other = fhe.RnsContext(qs, ps, device=1)
        assert lib.fhe_ckks_encode(enc.handle, other.handle, scale, vp(like), None, 1, vp(pt), _lib.MEM_DEVICE, st) == INVALID


def test_reference_slot_to_coeff_on_device_entries(fhe, torch_cuda):
    """scheme/ckks/src/bootstrapping.rs:121-141 at log_n = 5, r = 3 (log_qi = 55, L = 8): the matrices are the chunked products of
    `sfft_fmats` (sfft.rs:75-94, bootstrapping.rs:23-31), formed densely in mpmath here and cut into diagonals; every `diag_rot(i, j)`
    is encoded by fhe_ckks_encode and applied last-to-first with fhe_ckks_mul_mat; the result decodes (fhe_ckks_decode) to
    sfft(bit_reverse(m0)) within 2^-30."""
    from oracle import pyref as P
    torch = torch_cuda
    log_n, r = 5, 3
    n, l = 1 << log_n, 1 << (log_n - 1)
    qs, ps = P.ckks_primes(log_n, 55, 8)
    scale = qs[-1]
    enc = fhe.CkksEncoder(n)
    zero, one = Mo.mpc(0), Mo.mpc(1)

    def fmat(log_k):  # sfft.rs:79-92 as a dense l x l matrix: dense[i][(i + d) % l] = diag_d[i]
        m = 1 << (log_n - 2 - log_k)
        tw = Mo.w(2 * m)
        bc = lambda pat: [pat[i % (2 * m)] for i in range(l)]  # noqa: E731  `AVec::broadcast`
        diags = {0: bc([one] * m + [-t for t in tw])}
        if log_k == 0:
            diags[l - m] = bc(tw + [one] * m)
        else:
            diags[l - m] = bc([zero] * m + [one] * m)
            diags[m] = bc(tw + [zero] * m)
        dense = [[zero] * l for _ in range(l)]
        for d, v in diags.items():
            for i in range(l):
                dense[i][(i + d) % l] += v[i]
        return dense

    def matmul(a, b):
        return [[sum((a[i][k] * b[k][j] for k in range(l)), zero) for j in range(l)] for i in range(l)]

    fm = [fmat(k) for k in range(log_n - 1)]
    mats = []
    for c in range(0, len(fm), r):  # bootstrapping.rs:24-25: the product of every chunk of r
        prod = fm[c]
        for nxt in fm[c + 1:c + r]:
            prod = matmul(prod, nxt)
        mats.append(prod)
    rng = np.random.Generator(np.random.PCG64(55))
    m0 = rng.uniform(0, 1, l) + 1j * rng.uniform(0, 1, l)
    bits = log_n - 1
    rev = [int(format(i, "0%db" % bits)[::-1], 2) for i in range(l)]
    want = Mo.sfft([Mo.mpc(complex(m0[rev[i]])) for i in range(l)])  # sfft(bit_reverse(m0))
    like = dev(torch, np.zeros(1, dtype=np.uint64))
    sk = fhe.sample_zo(0.5, 91, 0, like, n)
    sk_host = [int(v) for v in host(sk).view(np.int64)]
    ctxs = {lv: fhe.RnsContext(qs[:lv], ps) for lv in (8, 7, 6)}
    pk_b, pk_a = ctxs[8].sk_encrypt(sk, None, n, 1, 92, 0)
    cb, ca = ctxs[8].pk_encrypt(pk_b[0].contiguous(), pk_a[0].contiguous(), enc.encode(ctxs[8], scale, dev(torch, m0[None])), n, 1, 93, 0)
    stream = [100]

    def rot_key(ctx, idx):  # ckks.rs:174-184 `rtk_gen`
        sk_t = np.array(P.sk_automorphism(sk_host, pow(5, idx, 2 * n)), dtype=np.int64).view(np.uint64)
        stream[0] += 1
        kb, ka = ctx.ksk_gen(sk, dev(torch, sk_t), n, 94, stream[0])
        return fhe.CkksKey(ctx, kb, ka, n)

    level = 8
    for mat in reversed(mats):  # bootstrapping.rs:86-87
        diag = {d: [mat[i][(i + d) % l] for i in range(l)] for d in range(l)}
        diag = {d: v for d, v in diag.items() if any(abs(x) > Mo.mpf(2) ** -200 for x in v)}
        _, split = fhe.bsgs_split(diag.keys())
        hi_ctx, lo_ctx = ctxs[level], ctxs[level - 1]
        baby = sorted({j for js in split.values() for j in js})
        keys_hi = {j: rot_key(hi_ctx, j) for j in baby if j}
        keys_lo = {i: rot_key(lo_ctx, i) for i in split if i}
        terms = [(i, j) for i in sorted(split) for j in sorted(split[i])]
        d_hi = np.zeros((len(terms), l), dtype=np.complex128)
        d_lo = np.zeros((len(terms), l), dtype=np.complex128)
        for t, (i, j) in enumerate(terms):  # diag_rot(i, j) = diag(i + j).rot_iter(-i) (bootstrapping.rs:101)
            v = diag[i + j]
            for c in range(l):
                x = v[(c - i) % l]
                (rh, rl), (ih, il) = Mo.to_dd(x.real), Mo.to_dd(x.imag)
                d_hi[t, c], d_lo[t, c] = complex(rh, ih), complex(rl, il)
        pts = enc.encode(hi_ctx, scale, dev(torch, d_hi), dev(torch, d_lo))
        cb, ca = fhe.CkksDiagMatrix(hi_ctx, lo_ctx, n, split, pts, keys_hi, keys_lo).apply(cb, ca)
        level -= 1
    got = host(enc.decode(ctxs[level], scale, ctxs[level].decrypt(sk, cb, ca, n)))[0]
    e = max(max(abs(Mo.mpf(float(g.real)) - w.real), abs(Mo.mpf(float(g.imag)) - w.imag)) for g, w in zip(got, want))
    print("slot_to_coeff (log_n = 5, r = 3): error 2^%.1f" % log2(e))
    assert e < Mo.mpf(2) ** -30
    enc.status(like)
