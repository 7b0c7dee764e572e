// Double-double arithmetic: the number format of the CKKS encoder (ckks_encode_kernels.hpp), the device form of the reference's
// 256-bit software floats (util/src/complex/f256.rs).
//
// A dd is an unevaluated sum hi + lo of two f64 with |lo| <= ulp(hi) / 2: about 106 significant bits.  Everything is built from the
// error-free transforms two_sum (Knuth) and two_prod (one fma), so every function needs IEEE f64 arithmetic WITHOUT reassociation
// or contraction (the library is built with -ffp-contract=off; every fma below is written out).  Relative error bounds (Hida, Li,
// Bailey, "Library for double-double and quad-double arithmetic", 2007; Joldes, Muller, Popescu, "Tight and rigorous error bounds
// for basic building blocks of double-word arithmetic", 2017):  add / sub 3 u^2, mul 5 u^2, div 10 u^2 with u = 2^-53.
//
// The file compiles for the host with plain g++ as well (tests/dd_host_test.cpp): host and device run the same operations in the
// same order on IEEE doubles, so the transforms below give the same bits on both.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define FHE_DD __host__ __device__ __forceinline__
#else
#define FHE_DD inline
#endif

namespace fhe {
namespace ddm {

typedef unsigned long long u64;
typedef unsigned __int128 u128;
typedef __int128 i128;

struct dd {
    double hi, lo;
};
struct cdd {
    dd re, im;
};

// ---- error-free transforms ---------------------------------------------------------------------------------------------------
// s + e == a + b exactly
FHE_DD void two_sum(double a, double b, double &s, double &e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
// the same for |a| >= |b| (or a == 0)
FHE_DD void quick_two_sum(double a, double b, double &s, double &e) {
    s = a + b;
    e = b - (s - a);
}
// p + e == a * b exactly (no overflow / underflow)
FHE_DD void two_prod(double a, double b, double &p, double &e) {
    p = a * b;
    e = __builtin_fma(a, b, -p);
}

// ---- dd ----------------------------------------------------------------------------------------------------------------------
FHE_DD dd from_double(double a) { return dd{a, 0.0}; }
FHE_DD dd neg(dd a) { return dd{-a.hi, -a.lo}; }
FHE_DD dd add(dd a, dd b) {
    double s1, s2, t1, t2;
    two_sum(a.hi, b.hi, s1, s2);
    two_sum(a.lo, b.lo, t1, t2);
    s2 += t1;
    quick_two_sum(s1, s2, s1, s2);
    s2 += t2;
    quick_two_sum(s1, s2, s1, s2);
    return dd{s1, s2};
}
FHE_DD dd sub(dd a, dd b) { return add(a, neg(b)); }
FHE_DD dd mul(dd a, dd b) {
    double p, e;
    two_prod(a.hi, b.hi, p, e);
    double t = a.hi * b.lo;
    t = __builtin_fma(a.lo, b.hi, t);
    e += t;
    quick_two_sum(p, e, p, e);
    return dd{p, e};
}
FHE_DD dd mul_d(dd a, double b) {
    double p, e;
    two_prod(a.hi, b, p, e);
    e = __builtin_fma(a.lo, b, e);
    quick_two_sum(p, e, p, e);
    return dd{p, e};
}
// a * p for p a power of two: exact
FHE_DD dd mul_pow2(dd a, double p) { return dd{a.hi * p, a.lo * p}; }
// a / b, b a dd that is exact (an integer below 2^106, such as the CKKS scale): long division, three quotient digits
FHE_DD dd div(dd a, dd b) {
    const double q1 = a.hi / b.hi;
    dd r = sub(a, mul_d(b, q1));
    const double q2 = r.hi / b.hi;
    r = sub(r, mul_d(b, q2));
    const double q3 = r.hi / b.hi;
    double s, e;
    quick_two_sum(q1, q2, s, e);
    return add(dd{s, e}, dd{q3, 0.0});
}

// ---- complex -----------------------------------------------------------------------------------------------------------------
FHE_DD cdd cadd(cdd a, cdd b) { return cdd{add(a.re, b.re), add(a.im, b.im)}; }
FHE_DD cdd csub(cdd a, cdd b) { return cdd{sub(a.re, b.re), sub(a.im, b.im)}; }
FHE_DD cdd cmul(cdd a, cdd b) {
    return cdd{sub(mul(a.re, b.re), mul(a.im, b.im)), add(mul(a.re, b.im), mul(a.im, b.re))};
}
FHE_DD cdd cconj(cdd a) { return cdd{a.re, neg(a.im)}; }
FHE_DD cdd cmul_pow2(cdd a, double p) { return cdd{mul_pow2(a.re, p), mul_pow2(a.im, p)}; }
// util/src/ring/fft.rs:92-98 `Butterfly::dit`: (a, b) <- (a + t b, a - t b)
FHE_DD void dit(cdd &a, cdd &b, cdd t) {
    const cdd tb = cmul(t, b);
    const cdd c = cadd(a, tb), d = csub(a, tb);
    a = c;
    b = d;
}
// util/src/ring/fft.rs:100-106 `Butterfly::dif`: (a, b) <- (a + b, (a - b) t)
FHE_DD void dif(cdd &a, cdd &b, cdd t) {
    const cdd c = cadd(a, b), d = cmul(csub(a, b), t);
    a = c;
    b = d;
}

// ---- integers ----------------------------------------------------------------------------------------------------------------
FHE_DD u64 bits_of(double x) {
    u64 b;
    __builtin_memcpy(&b, &x, 8);
    return b;
}
// an integer-valued double of magnitude below 2^127, exactly
FHE_DD i128 int_of(double t) {
    if (t == 0.0) return 0;
    const u64 b = bits_of(t);
    const int e = (int)((b >> 52) & 0x7ff) - 1075;
    const u64 m = (b & ((1ull << 52) - 1)) | (1ull << 52);
    const u128 v = e >= 0 ? (u128)m << e : (u128)(m >> -e);
    return (b >> 63) ? -(i128)v : (i128)v;
}
// The integer part of hi + lo, the fraction dropped TOWARD ZERO (`BigInt::from(&F256)`, f256.rs:213-239: the magnitude is shifted,
// then the sign applied), exact for every |x| < 2^126; ok = false (and 0) for a NaN, an infinity or |x| >= 2^126.
FHE_DD i128 to_i128(dd x, bool &ok) {
    // |hi + lo| < 2^126: a hi of exactly +-2^126 is in range when lo pulls it back
    ok = std::fabs(x.lo) < 0x1p126 &&
         (std::fabs(x.hi) < 0x1p126 || (x.hi == 0x1p126 && x.lo < 0.0) || (x.hi == -0x1p126 && x.lo > 0.0));
    if (!ok) return 0;
    const double th = std::trunc(x.hi), tl = std::trunc(x.lo);
    const double fh = x.hi - th, fl = x.lo - tl;  // exact, both in (-1, 1)
    double s, e;
    two_sum(fh, fl, s, e);  // the fraction, in (-2, 2): s + e exactly, |e| <= ulp(s) / 2
    // floor(s + e): a non-integer s is at least ulp(s) away from the integers, so e cannot carry it across one
    const double ks = std::floor(s);
    const bool s_int = ks == s;
    const int fl_f = (int)ks - ((s_int && e < 0.0) ? 1 : 0);
    const bool frac = !(s_int && e == 0.0);
    i128 v = int_of(th) + int_of(tl) + fl_f;  // floor(x)
    if (v < 0 && frac) v += 1;                // toward zero
    return v;
}

FHE_DD int clz64(u64 x) { return __builtin_clzll(x); }

// RN-even of the nw-word magnitude w (little endian) to f64.  Afterwards w holds |x - result|, neg says whether x < result.
FHE_DD double round_off(u64 *w, int nw, bool &neg) {
    neg = false;
    int top = -1;
    for (int i = nw - 1; i >= 0; --i)
        if (w[i]) { top = 64 * i + 63 - clz64(w[i]); break; }
    if (top < 0) return 0.0;
    if (top <= 52) {
        const double v = (double)w[0];
        w[0] = 0;
        return v;
    }
    const int sh = top - 52;  // bits dropped, >= 1
    const int wi = sh >> 6, off = sh & 63;
    u64 m = w[wi] >> off;
    if (off && wi + 1 < nw) m |= w[wi + 1] << (64 - off);
    m &= (1ull << 53) - 1;
    const int hb = sh - 1;
    const bool half = (w[hb >> 6] >> (hb & 63)) & 1;
    bool sticky = (w[hb >> 6] & ((1ull << (hb & 63)) - 1)) != 0;
    for (int i = 0; i < (hb >> 6); ++i) sticky = sticky || w[i] != 0;
    const bool up = half && (sticky || (m & 1));
    // r = x mod 2^sh
    for (int i = wi + 1; i < nw; ++i) w[i] = 0;
    w[wi] &= off ? ((1ull << off) - 1) : 0ull;
    if (up) {  // x - result = r - 2^sh < 0: w <- 2^sh - r, which is at most 2^(sh-1)
        m += 1;
        neg = true;
        u64 carry = 1;
        for (int i = 0; i <= wi && i < nw; ++i) {
            const u64 v = ~w[i] + carry;
            carry = (carry && v == 0) ? 1 : 0;
            w[i] = v;
        }
        w[wi] &= off ? ((1ull << off) - 1) : 0ull;
        // r == 2^(sh-1) exactly (a tie rounded up): 2^sh - r = 2^(sh-1) survives the mask; r > 2^(sh-1): smaller still
    }
    return std::ldexp((double)m, sh);
}
// The integer (-1)^neg * w, correctly rounded to dd: hi = RN(x), lo = RN(x - hi).  w is destroyed.  Magnitudes of 2^1024 and above
// give an infinite hi.
FHE_DD dd from_words(u64 *w, int nw, bool negative) {
    bool n1, n2;
    const double hi = round_off(w, nw, n1);
    double lo = round_off(w, nw, n2);
    if (n1) lo = -lo;
    return negative ? dd{-hi, -lo} : dd{hi, lo};
}
FHE_DD dd from_i128(i128 v) {
    const bool negative = v < 0;
    const u128 mag = negative ? (u128)0 - (u128)v : (u128)v;
    u64 w[2] = {(u64)mag, (u64)(mag >> 64)};
    return from_words(w, 2, negative);
}
FHE_DD dd from_u64(u64 v) {
    u64 w[1] = {v};
    return from_words(w, 1, false);
}

// ---- host only: the twiddle table -----------------------------------------------------------------------------------------------
// pi to three doubles (the third word makes i * pi exact to 2^-150)
constexpr double PI_0 = 3.141592653589793116e+00, PI_1 = 1.224646799147353207e-16, PI_2 = -2.994769809718339666e-33;

// cis(pi r / (2 l)) for 0 <= r <= l / 2 (the first octant), l a power of two: Taylor series at an argument of at most pi / 4,
// summed from the smallest term, 1 / k! by dd division.  Each component lands within a few 2^-106 of the true value.
inline cdd cis_octant(u64 r, u64 l) {
    if (r == 0) return cdd{dd{1.0, 0.0}, dd{0.0, 0.0}};
    // a = pi r / (2 l): r < 2^53 is exact in f64, 1 / (2 l) a power of two
    const double rd = (double)r, sc = 1.0 / (2.0 * (double)l);
    double p, e;
    two_prod(PI_0, rd, p, e);
    dd a = add(dd{p, e}, dd{PI_1 * rd, __builtin_fma(PI_1, rd, -(PI_1 * rd))});
    a = add(a, dd{PI_2 * rd, 0.0});
    a = mul_pow2(a, sc);
    const dd a2 = mul(a, a);
    // cos = sum (-1)^k a^(2k) / (2k)!, sin = a sum (-1)^k a^(2k) / (2k+1)!: Horner in a^2 from k = K down
    const int K = 20;  // (pi/4)^40 / 40! < 2^-172: far beyond dd
    dd c{0.0, 0.0}, s{0.0, 0.0};
    for (int k = K; k >= 1; --k) {
        // c <- 1 - a2 c' / ((2k-1)(2k)) form:  cos = 1 - a2/(1*2) (1 - a2/(3*4) (1 - ...)),  sin/a = 1 - a2/(2*3) (1 - a2/(4*5) (...))
        const dd one{1.0, 0.0};
        const dd fc = from_double((double)((2 * k - 1) * (2 * k))), fs = from_double((double)((2 * k) * (2 * k + 1)));
        c = div(mul(a2, sub(one, c)), fc);
        s = div(mul(a2, sub(one, s)), fs);
    }
    const dd one{1.0, 0.0};
    return cdd{sub(one, c), mul(a, sub(one, s))};
}
// The encoder's table: out[i] = cis(pi / (2 l))^i = exp(2 pi i / (4 l)) for 0 <= i < 4 l (scheme/ckks/src/sfft.rs:65-69), by the
// symmetries of the circle from the first octant: no running product, so no error accumulates along the table.
inline void twiddle_table(u64 l, cdd *out) {
    std::vector<cdd> oct(l / 2 + 1);
    for (u64 r = 0; r <= l / 2; ++r) oct[r] = cis_octant(r, l);
    for (u64 i = 0; i < 4 * l; ++i) {
        const u64 quad = i / l, r = i % l;
        cdd v = 2 * r <= l ? oct[r] : cdd{oct[l - r].im, oct[l - r].re};  // cos(pi/2 - x) = sin x
        switch (quad) {
            case 0: break;
            case 1: v = cdd{neg(v.im), v.re}; break;
            case 2: v = cdd{neg(v.re), neg(v.im)}; break;
            default: v = cdd{v.im, neg(v.re)}; break;
        }
        out[i] = v;
    }
}

// ---- the transforms as plain loops (scheme/ckks/src/sfft.rs:7-35): what the kernels compute, butterfly by butterfly -------------
// 5^k mod 4 l for k < max(l / 2, 1)
inline void pow5_table(u64 l, unsigned *out) {
    u64 v = 1 % (4 * l);
    for (u64 k = 0; k < (l / 2 ? l / 2 : 1); ++k) { out[k] = (unsigned)v; v = v * 5 % (4 * l); }
}
FHE_DD unsigned bit_rev(unsigned v, int bits) {
    if (!bits) return 0u;
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return v >> (32 - bits);
}
// the twiddle of butterfly k of the stage with half-length m: tw[(+-5^k mod 8m) * (4l / 8m)] (sfft.rs:46-54)
FHE_DD cdd stage_twiddle(const cdd *tw, const unsigned *pow5, unsigned l, unsigned m, unsigned k, bool conj) {
    const unsigned mask = 8 * m - 1;
    unsigned e = pow5[k] & mask;
    if (conj) e = (8 * m - e) & mask;
    return tw[(size_t)e * (l / (2 * m))];
}
inline void sifft_host(cdd *z, unsigned l, const cdd *tw, const unsigned *pow5) {
    int log_l = 0;
    while ((1u << log_l) < l) ++log_l;
    for (int lm = log_l - 1; lm >= 0; --lm) {
        const unsigned m = 1u << lm;
        for (unsigned c = 0; c < l; c += 2 * m)
            for (unsigned k = 0; k < m; ++k) dif(z[c + k], z[c + m + k], stage_twiddle(tw, pow5, l, m, k, true));
    }
    for (unsigned i = 0; i < l; ++i) {
        const unsigned j = bit_rev(i, log_l);
        if (i < j) { const cdd t = z[i]; z[i] = z[j]; z[j] = t; }
    }
    const double inv = 1.0 / (double)l;
    for (unsigned i = 0; i < l; ++i) z[i] = cmul_pow2(z[i], inv);
}
inline void sfft_host(cdd *z, unsigned l, const cdd *tw, const unsigned *pow5) {
    int log_l = 0;
    while ((1u << log_l) < l) ++log_l;
    for (unsigned i = 0; i < l; ++i) {
        const unsigned j = bit_rev(i, log_l);
        if (i < j) { const cdd t = z[i]; z[i] = z[j]; z[j] = t; }
    }
    for (int lm = 0; lm < log_l; ++lm) {
        const unsigned m = 1u << lm;
        for (unsigned c = 0; c < l; c += 2 * m)
            for (unsigned k = 0; k < m; ++k) dit(z[c + k], z[c + m + k], stage_twiddle(tw, pow5, l, m, k, false));
    }
}

}  // namespace ddm
}  // namespace fhe
