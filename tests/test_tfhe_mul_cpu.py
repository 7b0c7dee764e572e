"""No-GPU checks of the TGLWE ciphertext product: the header's declarations and the library's exports, the rejections that need no
device, csrc/tfhe_mul.hpp as a host program against big-integer vectors, and the model of tests/tfhe_mul_model.py against a schoolbook
product, against an external-product model, and against the error bound of DESIGN.md 9.9."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import tfhe_cbs_model as CM
import tfhe_mul_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
M64 = 1 << 64
M128 = 1 << 128
ENTRIES = ("fhe_tglwe_rlk_gen", "fhe_tglwe_rlk_prepare", "fhe_tglwe_rlk_destroy", "fhe_tglwe_tensor", "fhe_tglwe_relin", "fhe_tglwe_mul")
INVALID, UNSUPPORTED = 1, 6


def test_entries_are_declared_and_exported(fhe):
    with open(os.path.join(ROOT, "include", "fhe_ring.h")) as f:
        header = f.read()
    assert "typedef struct fhe_tglwe_relin_key fhe_tglwe_relin_key;" in header
    lib = fhe.lib()
    for name in ENTRIES:
        assert re.search(r"\b(int|void)\s+%s\(" % name, header), name
        assert hasattr(lib, name), name
    for name in ("rlk_gen", "RelinKey", "tensor", "relin", "mul", "relin_composed", "lwe_mul", "dot", "lwe_mul_plain", "dot_plain"):
        assert hasattr(fhe.tfhe_mul, name), name
    assert fhe.tfhe_mul.dot_plain([1, -2, 3], [4, 5, -6]) == -24 and fhe.tfhe_mul.lwe_mul_plain([3, -2], [5, 7]) == [15, -14]


def test_library_rejections_need_no_device(fhe):
    lib = fhe.lib()
    bufs = [np.full(64, 0x5a5a5a5a5a5a5a5a, dtype=np.uint64) for _ in range(8)]
    v = [C.c_void_p(b.ctypes.data) for b in bufs]
    fake = v[7]  # stands for a context, a generator or a key: no entry may look inside before it has refused
    h = C.c_void_p()
    # NULL pointers
    assert lib.fhe_tglwe_rlk_gen(None, 7, 5, v[0], 256, 0.0, fake, 0, v[1], v[2], 0, None) == INVALID
    assert lib.fhe_tglwe_rlk_gen(fake, 7, 5, None, 256, 0.0, fake, 0, v[1], v[2], 0, None) == INVALID
    assert lib.fhe_tglwe_rlk_gen(fake, 7, 5, v[0], 256, 0.0, None, 0, v[1], v[2], 0, None) == INVALID
    assert lib.fhe_tglwe_rlk_prepare(None, 7, 5, v[0], v[1], 256, 0, None, C.byref(h)) == INVALID and not h.value
    assert lib.fhe_tglwe_rlk_prepare(fake, 7, 5, None, v[1], 256, 0, None, C.byref(h)) == INVALID and not h.value
    assert lib.fhe_tglwe_rlk_prepare(fake, 7, 5, v[0], v[1], 256, 0, None, None) == INVALID
    assert lib.fhe_tglwe_tensor(None, v[0], v[1], v[2], v[3], 256, 32, v[4], v[5], v[6], 1, 0, None) == INVALID
    assert lib.fhe_tglwe_tensor(fake, v[0], v[1], v[2], v[3], 256, 32, v[4], None, v[6], 1, 0, None) == INVALID
    assert lib.fhe_tglwe_relin(fake, None, v[0], v[1], v[2], v[3], v[4], 1, 0, None) == INVALID
    assert lib.fhe_tglwe_relin(None, fake, v[0], v[1], v[2], v[3], v[4], 1, 0, None) == INVALID
    assert lib.fhe_tglwe_mul(fake, None, v[0], v[1], v[2], v[3], 32, v[4], v[5], 1, 0, None) == INVALID
    assert lib.fhe_tglwe_mul(None, fake, v[0], v[1], v[2], v[3], 32, v[4], v[5], 1, 0, None) == INVALID
    lib.fhe_tglwe_rlk_destroy(None)
    # another ring
    for n in (0, 128, 300, 4096):
        assert lib.fhe_tglwe_rlk_gen(fake, 7, 5, v[0], n, 0.0, fake, 0, v[1], v[2], 0, None) == INVALID, n
        assert lib.fhe_tglwe_rlk_prepare(fake, 7, 5, v[0], v[1], n, 0, None, C.byref(h)) == INVALID and not h.value, n
        assert lib.fhe_tglwe_tensor(fake, v[0], v[1], v[2], v[3], n, 32, v[4], v[5], v[6], 1, 0, None) == INVALID, n
    # log_delta outside 1 .. 63
    for p in (0, 64, -1):
        assert lib.fhe_tglwe_tensor(fake, v[0], v[1], v[2], v[3], 256, p, v[4], v[5], v[6], 1, 0, None) == INVALID, p
        assert lib.fhe_tglwe_mul(fake, fake, v[0], v[1], v[2], v[3], p, v[4], v[5], 1, 0, None) == INVALID, p
    # the outputs of the tensor are neither its inputs nor each other
    assert lib.fhe_tglwe_tensor(fake, v[0], v[1], v[2], v[3], 256, 32, v[0], v[5], v[6], 1, 0, None) == INVALID
    assert lib.fhe_tglwe_tensor(fake, v[0], v[1], v[2], v[3], 256, 32, v[4], v[4], v[6], 1, 0, None) == INVALID
    # gadgets outside the admission rule
    for log_b, d, n in ((0, 5, 256), (7, 0, 256), (13, 5, 256), (43, 1, 2048), (46, 1, 256), (65, 1, 256)):
        assert lib.fhe_tglwe_rlk_gen(fake, log_b, d, v[0], n, 0.0, fake, 0, v[1], v[2], 0, None) == UNSUPPORTED, (log_b, d, n)
        assert lib.fhe_tglwe_rlk_prepare(fake, log_b, d, v[0], v[1], n, 0, None, C.byref(h)) == UNSUPPORTED and not h.value, (log_b, d, n)
    for b in bufs:
        assert (b == np.uint64(0x5a5a5a5a5a5a5a5a)).all(), "a refused call wrote"


def test_kronecker_products_equal_schoolbook():
    rnd = random.Random(9400)
    for n in (8, 16):
        for lim in (1 << 63, 4, 1 << 90):  # n 2^(90 + 63) stays inside a slot
            a = [rnd.randrange(-lim, lim) for _ in range(n)]
            b = [rnd.randrange(-(1 << 63), 1 << 63) for _ in range(n)]
            assert M.negacyclic(a, b) == M.schoolbook(a, b), (n, lim)
        a = [-(1 << 63)] * n
        assert M.negacyclic(a, a) == M.schoolbook(a, a)
        a = [(1 << 63) - 1] * n
        assert M.negacyclic(a, a) == M.schoolbook(a, a)


def r64(rng, *shape):
    return rng.integers(0, 1 << 63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)


@pytest.mark.parametrize("log_b,d", [(7, 5), (4, 2), (16, 4)])
def test_model_relin_equals_external_product_of_padded_key(log_b, d):
    """relin == external product of [RLK rows; d zero rows] on (C2, 0), plus (C1, C0): the first d rows multiply the digits of a"""
    n = 16
    rng = np.random.Generator(np.random.PCG64(9410 + log_b))
    rlk_a, rlk_b = r64(rng, d, n), r64(rng, d, n)
    c0, c1, c2 = r64(rng, n), r64(rng, n), r64(rng, n)
    c2[:3] = np.array([0, 1 << 63, M64 - 1], dtype=np.uint64)
    got_a, got_b = M.relin1(log_b, d, rlk_a, rlk_b, c0, c1, c2)
    zero = np.zeros((d, n), dtype=np.uint64)
    xa, xb = M.external_product1(log_b, d, np.concatenate([rlk_a, zero]), np.concatenate([rlk_b, zero]), c2, np.zeros(n, dtype=np.uint64))
    assert np.array_equal(got_a, xa + c1) and np.array_equal(got_b, xb + c0)
    # and the other order would not do: the rows in the last d places meet the digits of b = 0
    ya, yb = M.external_product1(log_b, d, np.concatenate([zero, rlk_a]), np.concatenate([zero, rlk_b]), c2, np.zeros(n, dtype=np.uint64))
    assert not ya.any() and not yb.any()


def test_rlk_plain_rows_have_the_gadget_phases():
    n, log_b, d = 16, 7, 5
    rng = np.random.Generator(np.random.PCG64(9420))
    sk = rng.integers(0, 2, size=n, dtype=np.uint64)
    rows = M.rlk_plain(log_b, d, sk)
    s2 = M.schoolbook([int(v) for v in sk], [int(v) for v in sk])
    g = CM.gadget(log_b, d)  # the weights fhe_torus_decompose's digits carry, least significant first
    assert g[d - 1] == 1 << (64 - log_b)
    for j in range(d):
        assert [int(v) for v in rows[j]] == [(c * g[j]) % M64 for c in s2]


@pytest.mark.parametrize("n", [16, 32, 64])
@pytest.mark.parametrize("log_b,d,p", [(7, 5, 56), (16, 4, 40), (8, 7, 60), (31, 2, 32)])
def test_model_mul_phase_is_the_product_within_the_bound(n, log_b, d, p):
    """noise-free encryptions under a binary key, noise-free key rows: phase(mul) = 2^p m1 m2 + err, |err| <= the bound of DESIGN.md
    9.9 (tfhe_mul_model.mul_error_bound with e = 0: the roundings of C0, C1, C2 and of the digits).  Random messages and the extremes
    that 2^p m1 m2 < 2^63 admits."""
    rng = np.random.Generator(np.random.PCG64(9430 + n + p))
    rnd = random.Random(9430 + n + p)
    sk = rng.integers(0, 2, size=n, dtype=np.uint64)
    plain = M.rlk_plain(log_b, d, sk)
    rows = [M.encrypt(rng, sk, [int(v) for v in plain[j]]) for j in range(d)]
    rlk_a, rlk_b = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    room = 1 << (63 - p)                      # |m1 m2| summed over a coefficient stays below this
    top = int((room // n) ** 0.5) - 1         # dense random messages: |coefficient| <= top, n top^2 < room
    cases = []
    for _ in range(3):
        if top >= 1:
            cases.append(([rnd.randrange(-top, top + 1) for _ in range(n)], [rnd.randrange(-top, top + 1) for _ in range(n)]))
        else:  # the room is tight (p = 60: 8): sparse random messages, room - 1 coefficients of +-1 each, so a coefficient sums < room terms
            sparse = lambda: [rnd.choice((-1, 1)) if i in pos else 0 for pos in [set(rnd.sample(range(n), min(n, room - 1)))] for i in range(n)]  # noqa: E731
            cases.append((sparse(), sparse()))
    big = int(room ** 0.5) - 1
    cases.append(([big] + [0] * (n - 1), [-big] + [0] * (n - 1)))          # one coefficient at the extreme, both signs
    cases.append(([0] * (n - 1) + [big], [0] * (n - 1) + [big]))          # ... wrapping round X^n = -1
    assert len(cases) == 5
    for m1, m2 in cases:
        ct1 = M.encrypt(rng, sk, [(v << p) % M64 for v in m1])
        ct2 = M.encrypt(rng, sk, [(v << p) % M64 for v in m2])
        oa, ob = M.mul(log_b, d, rlk_a, rlk_b, ct1[0], ct1[1], ct2[0], ct2[1], n, p)
        want = M.schoolbook(m1, m2)
        assert max(abs(v) for v in want) < room
        bound = M.mul_error_bound(n, log_b, d, p, sum(abs(v) for v in m1), 0)
        ph = M.phase(oa[0], ob[0], sk)
        for k in range(n):
            err = M.centred((ph[k] - (want[k] << p)) % M64)
            assert abs(err) <= bound, (k, err, bound)
        assert bound < (1 << (p - 1)), "the bound itself must leave the message readable"


def test_model_mul_with_noise_is_within_the_bound():
    """operands and key rows with noise: the wrap term u e 2^(64 - p) and the key-noise term are live"""
    n, log_b, d, p, e_max = 16, 7, 5, 56, 1 << 10
    rng = np.random.Generator(np.random.PCG64(9440))
    rnd = random.Random(9440)
    sk = rng.integers(0, 2, size=n, dtype=np.uint64)
    plain = M.rlk_plain(log_b, d, sk)
    noise = lambda: [rnd.randrange(-e_max, e_max + 1) for _ in range(n)]  # noqa: E731
    rows = [M.encrypt(rng, sk, [int(v) for v in plain[j]], noise()) for j in range(d)]
    rlk_a, rlk_b = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    m1, m2 = [rnd.randrange(-2, 3) for _ in range(n)], [rnd.randrange(-2, 3) for _ in range(n)]
    ct1 = M.encrypt(rng, sk, [(v << p) % M64 for v in m1], noise())
    ct2 = M.encrypt(rng, sk, [(v << p) % M64 for v in m2], noise())
    oa, ob = M.mul(log_b, d, rlk_a, rlk_b, ct1[0], ct1[1], ct2[0], ct2[1], n, p)
    want = M.schoolbook(m1, m2)
    bound = M.mul_error_bound(n, log_b, d, p, max(sum(abs(v) for v in m1), sum(abs(v) for v in m2)), e_max, key_noise=e_max)
    assert bound < (1 << (p - 1))
    ph = M.phase(oa[0], ob[0], sk)
    assert max(abs(M.centred((ph[k] - (want[k] << p)) % M64)) for k in range(n)) <= bound


def wide(x):
    x %= M128
    return "%016x %016x" % (x >> 64, x & (M64 - 1))


def split_for(rnd, x):
    """some H, L (128-bit two's complement) with H 2^32 + L = x mod 2^128"""
    L = rnd.randrange(-(1 << 108), 1 << 108)
    L += (x - L) % (1 << 32)
    return (x - L) >> 32, L


def host_vectors(path):
    rnd = random.Random(9450)
    lines = []
    for w in [0, 1, M64 - 1, 1 << 63, (1 << 63) - 1, 1 << 32, (1 << 32) - 1, 1 << 31, (1 << 63) + (1 << 31), 0xffffffff80000000] + [rnd.randrange(M64) for _ in range(64)]:
        sw = M.s64(w)
        lines.append("cut %016x %016x %016x" % (w, (sw >> 32) % M64, sw & 0xffffffff))
    ps = (1, 2, 31, 32, 33, 62, 63)
    lo, hi = -(1 << 63), (1 << 63) - 1
    for n in (256, 2048):
        for terms in (1, 2):  # C2 / C0 have one sum of n products, C1 two
            pieces = []
            # every word -2^63: hi = -2^31, lo = 0; the negacyclic coefficient k has k + 1 positive and n - 1 - k negative terms
            for k in (0, n // 2, n - 1):
                cnt = (2 * k + 2 - n) * terms
                pieces.append((cnt * lo * -(1 << 31), 0))
            # every word 2^63 - 1: hi = 2^31 - 1, lo = 2^32 - 1
            for k in (0, n - 1):
                cnt = (2 * k + 2 - n) * terms
                pieces.append((cnt * hi * ((1 << 31) - 1), cnt * hi * ((1 << 32) - 1)))
            # mixed signs
            pieces.append((n * terms * lo * ((1 << 31) - 1), n * terms * lo * ((1 << 32) - 1)))
            for H, L in pieces:
                for p in ps:
                    lines.append("rnd %s %s %d %016x" % (wide(H), wide(L), p, M.rnd(H * (1 << 32) + L, p) % M64))
    for p in ps:
        for k in (0, 1, -1, 5, -6, (1 << 62) + 3, -(1 << 62) - 3, (1 << 64) + 1, -(1 << 70) - 1):
            for x in (k * (1 << p) + (1 << (p - 1)), k * (1 << p) + (1 << (p - 1)) - 1, k * (1 << p) - (1 << (p - 1))):  # a tie, just below, the tie below
                H, L = split_for(rnd, x)
                lines.append("rnd %s %s %d %016x" % (wide(H), wide(L), p, M.rnd(x, p) % M64))
        for _ in range(32):
            H, L = rnd.randrange(-(1 << 107), 1 << 107), rnd.randrange(-(1 << 107), 1 << 107)
            lines.append("rnd %s %s %d %016x" % (wide(H), wide(L), p, M.rnd(H * (1 << 32) + L, p) % M64))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_host_header_as_a_program(tmp_path):
    """tests/tfhe_mul_host_test.cpp: a stand-alone program under AddressSanitizer and UBSan, run as its own process"""
    exe, vec = str(tmp_path / "tfhe_mul_host_test"), str(tmp_path / "vectors.txt")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HERE, "tfhe_mul_host_test.cpp")])
    host_vectors(vec)
    out = subprocess.run([exe, vec], capture_output=True, text=True)
    assert out.returncode == 0 and "tfhe_mul_host_test ok" in out.stdout, out.stdout + out.stderr
