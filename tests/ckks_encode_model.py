"""The exact model of the CKKS encoder for tests/test_ckks_encode_*.py: scheme/ckks/src/sfft.rs:7-72 (`sfft`, `sifft`, `w`) and
scheme/ckks/src/ckks.rs:186-213 (`encode`, `decode`) restated line by line in mpmath at 300 bits -- wider than the reference's own
256-bit floats, so against a 106-bit implementation it stands for exact arithmetic.  No Rust toolchain exists to produce golden
files from the reference; this model is the yardstick, and `self_check` is the reference's own `sifft_sfft` test applied to it."""
from fractions import Fraction

import mpmath
from mpmath import libmp

M = mpmath.mp.clone()
M.prec = 300
mpf, mpc = M.mpf, M.mpc

_CIS = {}


def cis(num, den):
    """exp(2 pi i num / den): entry num (4n / den) of `w(n)`'s table of powers of cis(pi / 2n) (sfft.rs:65-69)"""
    f = Fraction(num, den)
    f -= f.numerator // f.denominator
    v = _CIS.get(f)
    if v is None:
        v = _CIS[f] = M.expjpi(mpf(2 * f.numerator) / f.denominator)
    return v


def w(n, conj=False):
    """sfft.rs:46-54, 57-72: `w(n).iter()` -- n / 2 twiddles in powers-of-5-mod-4n order, negated exponents for `.conj()`"""
    out, j = [], 1 % (4 * n)
    for _ in range(n // 2):
        out.append(cis((-j) % (4 * n) if conj else j, 4 * n))
        j = j * 5 % (4 * n)
    return out


def bit_reverse(v):
    """util/src/misc.rs:29-42"""
    n = len(v)
    out = list(v)
    if n > 2:
        bits = n.bit_length() - 1
        for i in range(n):
            j = int(format(i, "0%db" % bits)[::-1], 2)
            if i < j:
                out[i], out[j] = out[j], out[i]
    return out


def sfft(z):
    """sfft.rs:7-19 (`Butterfly::dit`, util/src/ring/fft.rs:92-98)"""
    z = bit_reverse(z)
    n = len(z)
    assert n & (n - 1) == 0
    for log_m in range(n.bit_length() - 1):
        m = 1 << log_m
        tw = w(2 * m)
        for c in range(0, n, 2 * m):
            for k in range(m):
                a, tb = z[c + k], tw[k] * z[c + m + k]
                z[c + k], z[c + m + k] = a + tb, a - tb
    return z


def sifft(z):
    """sfft.rs:21-35 (`Butterfly::dif`, util/src/ring/fft.rs:100-106)"""
    z = list(z)
    n = len(z)
    assert n & (n - 1) == 0
    for log_m in reversed(range(n.bit_length() - 1)):
        m = 1 << log_m
        tw = w(2 * m, conj=True)
        for c in range(0, n, 2 * m):
            for k in range(m):
                a, b = z[c + k], z[c + m + k]
                z[c + k], z[c + m + k] = a + b, (a - b) * tw[k]
    z = bit_reverse(z)
    return [v / n for v in z]


def to_bigint(x):
    """`BigInt::from(&F256)` (util/src/complex/f256.rs:213-239): the magnitude shifted, the fraction dropped, then the sign"""
    v = int(M.floor(abs(x)))
    return -v if x < 0 else v


def encode_exact(m, scale):
    """ckks.rs:189-193 before the conversion: the n exact values z.re * scale ++ z.im * scale"""
    z = sifft(m)
    return [v.real * scale for v in z] + [v.imag * scale for v in z]


def encode(m, scale):
    """ckks.rs:186-198 -> the n integers `z_scaled` (RnsRq::from_bigint reduces them mod every q)"""
    return [to_bigint(x) for x in encode_exact(m, scale)]


def decode(coeffs, scale):
    """ckks.rs:200-213 from the centred integers `pt.into_bigint()` gives"""
    l = len(coeffs) // 2
    return sfft([mpc(mpf(coeffs[i]) / scale, mpf(coeffs[l + i]) / scale) for i in range(l)])


def horner(coeffs, t):
    acc = mpc(0)
    for c in reversed(coeffs):
        acc = acc * t + c
    return acc


def self_check(log_n, evals):
    """sfft.rs:110-122 `sifft_sfft` for one size: the sifft output evaluated at w and -w gives the slots back, and so does sfft;
    returns the largest deviation"""
    n = 1 << log_n
    assert len(evals) == n
    coeffs = sifft(evals)
    tw = w(n)
    pts = tw + [-t for t in tw]
    err = max(abs(horner(coeffs, t) - e) for t, e in zip(pts, evals))
    return max(err, max(abs(a - b) for a, b in zip(evals, sfft(coeffs))))


# ---- double-double <-> exact -----------------------------------------------------------------------------------------------------
def rn(x):
    """an mpf rounded to the nearest f64 (ties to even)"""
    return libmp.to_float(mpf(x)._mpf_, rnd=libmp.round_nearest)


def from_dd(hi, lo=0.0):
    return mpf(float(hi)) + mpf(float(lo))


def to_dd(x):
    hi = rn(x)
    return hi, rn(mpf(x) - mpf(hi))


def cfrom(hi, lo=None):
    """complex128 arrays (high words, low words or None) -> a list of mpc"""
    hi = list(hi)
    lo = [0j] * len(hi) if lo is None else list(lo)
    return [mpc(from_dd(h.real, o.real), from_dd(h.imag, o.imag)) for h, o in zip(hi, lo)]
