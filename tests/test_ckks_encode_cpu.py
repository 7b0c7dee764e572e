"""CPU checks of the CKKS encoder's arithmetic (learn-fhe_amd/csrc/dd.hpp; include/fhe_ring.h fhe_ckks_encoder_*): the header compiles
for the host, so the butterflies, the integer conversions and the twiddle table the kernels use are exercised here without a GPU,
against the exact model of tests/ckks_encode_model.py (scheme/ckks/src/sfft.rs:7-72, ckks.rs:186-213 in mpmath at 300 bits)."""
import ctypes as C
import os
import random
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import ckks_encode_model as Mo

HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = Mo.mpf(2) ** -95


def build_host(tmp_path, sanitize=False):
    exe = str(tmp_path / ("dd_host_test_san" if sanitize else "dd_host_test"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-o", exe, os.path.join(HERE, "dd_host_test.cpp")])
    return exe


def run_host(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.split("\n")


def transform_script(msgs):
    return "".join("F %d\n" % len(hi) + "".join("%s %s %s %s\n" % (float(h.real).hex(), float(o.real).hex(), float(h.imag).hex(), float(o.imag).hex())
                                                 for h, o in zip(hi, lo)) for hi, lo in msgs)


def parse_cdd(lines, pos, l):
    vals = [[float.fromhex(t) for t in lines[pos + i].split()] for i in range(l)]
    return [Mo.mpc(Mo.from_dd(v[0], v[1]), Mo.from_dd(v[2], v[3])) for v in vals], vals


def messages(seed, sizes, with_lo):
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for l in sizes:
        hi = rng.uniform(-1, 1, l) + 1j * rng.uniform(-1, 1, l)
        lo = (rng.uniform(-1, 1, l) + 1j * rng.uniform(-1, 1, l)) * 2.0 ** -55 if with_lo else np.zeros(l, dtype=np.complex128)
        out.append((hi, lo))
    return out


SIZES = [1 << k for k in range(11)]  # l = 1 .. 1024


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_transforms_and_conversions(tmp_path, sanitize):
    """sifft within 2^-95 max|z| of the model, sfft of that output back within 2^-95 of the input, for l = 1 .. 1024 (with and without
    low words); the integer conversions at the edges.  The second build runs the same program under AddressSanitizer and UBSan."""
    exe = build_host(tmp_path, sanitize)
    msgs = messages(11, SIZES, False) + messages(12, [4, 64, 1024], True)
    lines = run_host(exe, transform_script(msgs))
    pos = 0
    for hi, lo in msgs:
        l = len(hi)
        x = Mo.cfrom(hi, lo)
        scale = max(max(abs(v.real), abs(v.imag)) for v in x)
        got, _ = parse_cdd(lines, pos, l)
        back, _ = parse_cdd(lines, pos + l, l)
        pos += 2 * l
        want = Mo.sifft(x)
        e1 = max(max(abs(g.real - t.real), abs(g.imag - t.imag)) for g, t in zip(got, want))
        e2 = max(max(abs(g.real - t.real), abs(g.imag - t.imag)) for g, t in zip(back, x))
        print("l=%d: sifft error 2^%.1f, round trip 2^%.1f (x max|z|)" % (l, float(Mo.M.log(e1 / scale + Mo.mpf(2) ** -200, 2)),
                                                                       float(Mo.M.log(e2 / scale + Mo.mpf(2) ** -200, 2))))
        assert e1 <= BOUND * scale, "sifft, l = %d" % l
        assert e2 <= BOUND * scale, "sfft(sifft), l = %d" % l
    # integers -> dd, correctly rounded (hi = RN(v), lo = RN(v - hi)), and back exactly where a dd holds v
    ints = [0, 1, -1]
    for s in (1, -1):
        ints += [s * (2 ** 63 + 1), s * (2 ** 63 - 1), s * (2 ** 126 - 1), s * (2 ** 106 - 1), s * (2 ** 53 + 1), s * (2 ** 54 + 3),
                 s * (2 ** 100 - 2 ** 40 - 1), s * (2 ** 64), s * (2 ** 125 + 2 ** 72 + 2 ** 19)]
    rnd = random.Random(5)
    ints += [rnd.getrandbits(126) * rnd.choice([1, -1]) for _ in range(40)]
    script = "".join("I %d %d %d\n" % (v < 0, abs(v) >> 64, abs(v) & (2 ** 64 - 1)) for v in ints)
    lines = run_host(exe, script)
    for i, v in enumerate(ints):
        hi, lo = (float.fromhex(t) for t in lines[2 * i].split())
        assert hi == float(v), v  # int -> float is correctly rounded
        assert lo == float(v - int(hi)), v
        ok, neg, h, low = (int(t) for t in lines[2 * i + 1].split())
        back = (-1 if neg else 1) * ((h << 64) | low)
        assert ok == 1 and back == int(hi) + int(lo), v
    # the named cases are all held exactly by a dd except those wider than 107 bits
    for v in (0, 1, -1, 2 ** 63 + 1, -(2 ** 63 - 1), 2 ** 126 - 1, -(2 ** 126 - 1)):
        i = ints.index(v)
        ok, neg, h, low = (int(t) for t in lines[2 * i + 1].split())
        assert (-1 if neg else 1) * ((h << 64) | low) == v
    # multi-word magnitudes, among them halves of exact ties and words of all ones
    words = [[2 ** 64 - 1] * 8, [0, 0, 0, 1], [1, 0, 0, 2 ** 63], [2 ** 63, 2 ** 10, 0, 0, 0], [0] * 15 + [2 ** 62]]
    words += [[rnd.getrandbits(64) for _ in range(k)] for k in (1, 2, 3, 8, 15, 16) for _ in range(4)]
    signs = [rnd.randrange(2) for _ in words]
    lines = run_host(exe, "".join("W %d %d %s\n" % (s, len(w), " ".join(map(str, w))) for s, w in zip(signs, words)))
    for i, (s, w) in enumerate(zip(signs, words)):
        v = sum(x << (64 * k) for k, x in enumerate(w)) * (-1 if s else 1)
        hi, lo = (float.fromhex(t) for t in lines[i].split())
        assert hi == float(v) and lo == float(v - int(hi)), w
    # dd -> integer, the fraction dropped toward zero; hi and lo of opposite signs, values next to integers, out of range
    dds = [(0.0, 0.0), (1.0, -2.0 ** -60), (-1.0, 2.0 ** -60), (1.0, 2.0 ** -60), (-1.0, -2.0 ** -60), (2.0 ** 63, -1.0), (-2.0 ** 63, 1.0),
           (2.0 ** 63, -0.5), (-2.0 ** 63, 0.5), (2.0 ** 126 * (1 - 2.0 ** -53), 2.0 ** 72 - 0.5), (5.0, -2.0 ** -1000), (-5.0, 2.0 ** -1000),
           (0.75, 0.0), (-0.75, 0.0), (0.5, 0.5), (-0.5, -0.5), (2.0 ** 80, -2.0 ** 20 - 0.25), (-2.0 ** 80, 2.0 ** 20 + 0.25), (3.5, 2.0 ** -54),
           (2.0 ** 100 + 2.0 ** 60, 123.75), (-(2.0 ** 100 + 2.0 ** 60), -123.75)]
    bad = [(2.0 ** 126, 0.0), (-2.0 ** 126, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("nan"))]
    lines = run_host(exe, "".join("D %s %s\n" % (a.hex() if a == a else "nan", b.hex() if b == b else "nan") for a, b in dds + bad))
    for i, (a, b) in enumerate(dds):
        exact = Fraction(a) + Fraction(b)  # (2^-1000 next to 5 lies below the model's 300 bits)
        want = -((-exact).__floor__()) if exact < 0 else exact.__floor__()
        ok, neg, h, low = (int(t) for t in lines[i].split())
        assert ok == 1 and (-1 if neg else 1) * ((h << 64) | low) == want, (a, b)
    for i in range(len(bad)):
        assert lines[len(dds) + i].split()[0] == "0"


@pytest.mark.parametrize("log_n", [1, 5, 10, 15])
def test_twiddles_of_a_host_only_handle(fhe, log_n):
    """fhe_ckks_encoder_twiddles (device = -1): every component of the 4 l powers of cis(pi / 2l) within 2^-100 of the model"""
    n = 1 << log_n
    l = n // 2
    tw = fhe.CkksEncoder(n, device=-1).twiddles()
    assert tw.shape == (4 * l, 4)
    idx = range(4 * l)  # every entry: each is computed on its own, so a sample would prove nothing about its neighbours
    worst = Mo.mpf(0)
    for i in idx:
        want = Mo.cis(i, 4 * l)
        worst = max(worst, abs(Mo.from_dd(tw[i, 0], tw[i, 1]) - want.real), abs(Mo.from_dd(tw[i, 2], tw[i, 3]) - want.imag))
    print("n=2^%d: worst twiddle error 2^%.1f over all %d entries" % (log_n, float(Mo.M.log(worst + Mo.mpf(2) ** -200, 2)), len(idx)))
    assert worst <= Mo.mpf(2) ** -100
    assert (tw[0] == [1.0, 0.0, 0.0, 0.0]).all() and (tw[l] == [0.0, 0.0, 1.0, 0.0]).all()


def test_host_only_handle_and_bad_sizes_are_refused(fhe):
    from learn_fhe_amd import _lib
    L = _lib.lib()
    INVALID = 1
    for n in (0, 1, 3, 24, 1 << 16):
        h = C.c_void_p()
        assert L.fhe_ckks_encoder_create(n, -1, C.byref(h)) == INVALID and not h.value
    enc = fhe.CkksEncoder(16, device=-1)
    z = np.zeros((1, 8), dtype=np.complex128)
    assert L.fhe_ckks_sifft(enc.handle, C.c_void_p(z.ctypes.data), None, 1, _lib.MEM_HOST, None) == INVALID
    assert L.fhe_ckks_sfft(enc.handle, C.c_void_p(z.ctypes.data), None, 1, _lib.MEM_HOST, None) == INVALID
    assert L.fhe_ckks_encoder_status(enc.handle, None, 0) == INVALID
    out = np.zeros(4)
    assert L.fhe_ckks_encoder_twiddles(enc.handle, out.ctypes.data_as(C.POINTER(C.c_double)), 4 * 8 + 1) == INVALID


def test_model_self_check():
    """the reference's `sifft_sfft` (sfft.rs:110-122) on the model: Horner evaluation of the sifft output at w and -w gives the slots"""
    rnd = random.Random(3)
    for log_n in range(1, 10):
        evals = [Mo.mpc(rnd.uniform(-1, 1), rnd.uniform(-1, 1)) for _ in range(1 << log_n)]
        assert Mo.self_check(log_n, evals) < Mo.mpf(2) ** -250
