// Kernels of the CKKS polynomial evaluation (csrc/ckks_poly_api.hip): the linear combination of up to 16 ciphertexts with a constant,
// with or without the closing `rescale()` (util/src/ring/rns.rs:99-111, the K == 1 branch), and the tensor of `Ckks::mul`
// (scheme/ckks/src/ckks.rs:256-260) on evaluation-domain operands that lie on MORE limbs than the product (prefix read).
//
// Both are element-wise and memory bound.  One thread owns one coefficient of one half (b or a) of one ciphertext and walks the limbs:
// consecutive lanes read consecutive coefficients of every limb of every term (coalesced), the per-(term, limb) constants are the same
// for the whole grid and come through the constant address space (scalar loads).  No LDS.
#pragma once
#include "rns_kernels.hpp"

namespace fhe {

constexpr int POLY_MAX_TERMS = 16;

// term j: ct_j = (b[j], a[j]), each [batch][limbs[j]][n] with limbs[j] >= the limb count of the launch; only that prefix is read
struct PolyTerms {
    const u64 *b[POLY_MAX_TERMS];
    const u64 *a[POLY_MAX_TERMS];
    unsigned limbs[POLY_MAX_TERMS];
    int n_terms;
};

// y mod q for any 64-bit y: mu = floor(2^64 / q), the estimate misses the quotient by at most 2 (q < 2^62: 3q fits)
__device__ __forceinline__ u64 poly_red64(u64 y, u64 mu, u64 q) {
    const u64 r = y - __umul64hi(y, mu) * q;
    return csub(csub(r, q), q);
}

// sum_j k[j][l] x_j + addc mod q of limb l at (ciphertext p, coefficient i), k = ktab [n_terms + 1][ell] in [0, q_l).
//
// WIDE: the products are accumulated UNREDUCED in 128 bits and reduced once.  Bound: every k and x is < q, so the sum is at most
// 16 (q - 1)^2 + (q - 1) < 2^4 2^122 = 2^126 for q < 2^61 -- two bits of room, no carry out of the high word.  The reduction splits
// the sum S = hi 2^64 + lo: hi < 2^62 is reduced by poly_red64, multiplied by 2^64 mod q (Barrett: both factors < q) and added to
// lo mod q.  Primes in [2^61, 2^62), which the context admits, take the route that reduces every product (WIDE = false); it gives the
// same canonical residue, so which route ran never shows in a result.
template <bool WIDE>
__device__ __forceinline__ u64 poly_lin_limb(const PolyTerms &T, const u64 *__restrict__ ktab, const Barrett &m, u64 mu, int l, int ell, size_t p,
                                             size_t i, unsigned n, bool half_a, u64 addc) {
    if constexpr (WIDE) {
        u64 lo = addc, hi = 0;
        for (int j = 0; j < T.n_terms; ++j) {
            const u64 *src = half_a ? T.a[j] : T.b[j];
            const u64 x = src[(p * T.limbs[j] + l) * n + i], k = ldc(ktab, j * ell + l);
            const u64 pl = k * x;
            lo += pl;
            hi += __umul64hi(k, x) + (lo < pl);
        }
        const u64 c64 = poly_red64(0ULL - m.q, mu, m.q);  // 2^64 mod q
        const u64 t = mulmod_barrett(poly_red64(hi, mu, m.q), c64, m);
        return csub(t + poly_red64(lo, mu, m.q), m.q);
    } else {
        u64 s = addc;
        for (int j = 0; j < T.n_terms; ++j) {
            const u64 *src = half_a ? T.a[j] : T.b[j];
            const u64 x = src[(p * T.limbs[j] + l) * n + i];
            s = csub(s + mulmod_barrett(ldc(ktab, j * ell + l), x, m), m.q);
        }
        return s;
    }
}

// out = sum_j k_j ct_j + k0 e0 on `ell` limbs (REAL = false: out [batch][ell][n]), or the `rescale()` of that sum (REAL = true: out
// [batch][ell - 1][n]; R = the context's resc_last, the constants rns_rescale_kernel reads; the arithmetic is rescale_limb's K == 1 branch
// line by line).  ktab row n_terms is the constant, added to coefficient 0 of the b half only.  B, mu: the context's Barrett table and
// floor(2^64 / q_l).  An output may alias an input of the SAME layout (REAL = false, limbs[j] == ell): a thread reads every term of its
// element before it writes it, and no other thread touches that element.
template <bool REAL, bool WIDE>
__global__ void ckks_lincomb_kernel(PolyTerms T, const u64 *__restrict__ ktab, const Barrett *__restrict__ B, RescaleConsts R, u64 *out_b, u64 *out_a,
                                    unsigned n, int ell, size_t batch) {
    const size_t half = size_t(n) * batch, total = 2 * half;
    const int lo_limbs = REAL ? ell - 1 : ell;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const bool half_a = idx >= half;
        const size_t e = half_a ? idx - half : idx, p = e / n, i = e - p * n;
        const bool with_c = !half_a && i == 0;
        u64 *out = half_a ? out_a : out_b;
        u64 vp = 0;
        if constexpr (REAL) {
            const int l = ell - 1;
            const Barrett m{ldc(&B[l].q, 0), ldc(&B[l].mu, 0), ldc(&B[l].sh1, 0), ldc(&B[l].sh2, 0)};
            const u64 x = poly_lin_limb<WIDE>(T, ktab, m, ldc(R.red_mu, l), l, ell, p, i, n, half_a, with_c ? ldc(ktab, T.n_terms * ell + l) : 0);
            vp = csub(x + ldc(R.half_p, 0), m.q);
        }
        for (int l = 0; l < lo_limbs; ++l) {
            const Barrett m{ldc(&B[l].q, 0), ldc(&B[l].mu, 0), ldc(&B[l].sh1, 0), ldc(&B[l].sh2, 0)};
            const u64 q = m.q, mu = ldc(R.red_mu, l);
            u64 x = poly_lin_limb<WIDE>(T, ktab, m, mu, l, ell, p, i, n, half_a, with_c ? ldc(ktab, T.n_terms * ell + l) : 0);
            if constexpr (REAL) {  // rns.rs:104-111 with P = the last limb: ((x + half) - (vp mod q)) P^-1
                const u64 vq = csub(x + ldc(R.half_q, l), q), sw = poly_red64(vp, mu, q);
                const u64 diff = vq >= sw ? vq - sw : vq + q - sw;
                x = csub(mul_shoup_lazy(diff, ldc(R.pinv, l), ldc(R.pinv_s, l), q), q);
            }
            out[(p * lo_limbs + l) * n + i] = x;
        }
    }
}

// rns_tensor_kernel on operands that keep their own limb counts: x = (xb, xa) [batch][x_limbs][n], y = (yb, ya) [batch][y_limbs][n],
// evaluation domain, x_limbs, y_limbs >= limbs; d [3][batch][limbs][n] = (xb yb, xb ya + xa yb, xa ya) on the first `limbs` limbs.
FHE_HEADER_KERNEL void ckks_tensor_prefix_kernel(const u64 *__restrict__ xb, const u64 *__restrict__ xa, unsigned x_limbs, const u64 *__restrict__ yb,
                                                 const u64 *__restrict__ ya, unsigned y_limbs, u64 *__restrict__ d, unsigned n, unsigned limbs, size_t polys,
                                                 const Barrett *__restrict__ B) {
    const size_t plane = polys * n;
    for (size_t y = blockIdx.y; y < polys; y += gridDim.y) {
        const unsigned limb = unsigned(y % limbs);
        const size_t p = y / limbs;
        const Barrett m{ldc(&B[limb].q, 0), ldc(&B[limb].mu, 0), ldc(&B[limb].sh1, 0), ldc(&B[limb].sh2, 0)};
        const size_t base = y * n, bx = (p * x_limbs + limb) * n, by = (p * y_limbs + limb) * n;
        for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
            const u64 b0 = xb[bx + i], a0 = xa[bx + i], b1 = yb[by + i], a1 = ya[by + i];
            d[base + i] = mulmod_barrett(b0, b1, m);
            d[plane + base + i] = csub(mulmod_barrett(b0, a1, m) + mulmod_barrett(a0, b1, m), m.q);
            d[2 * plane + base + i] = mulmod_barrett(a0, a1, m);
        }
    }
}

}  // namespace fhe
