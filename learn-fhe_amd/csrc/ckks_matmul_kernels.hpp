// Kernels of the CKKS diagonal-matrix product (scheme/ckks/src/bootstrapping.rs:90-108 `Bootstrapping::mul_mat`, ckks_matmul_api.hip):
// the evaluation-domain multiply-accumulate of one giant step's terms and the rescale of their SUM.
//
// `mul_mat` rescales every term (`mul_constant`, ckks.rs:250-253) before it adds them.  `rescale()` (rns.rs:99-118, K == 1) is, on limb l,
//     out_l = (x_l + h_l - lift((x_last + h_last) mod q_last)) q_last^-1   mod q_l,          h = floor(q_last / 2),
// linear mod q_l in everything but the lift of the last limb, so for the J terms x^1 .. x^J of a giant step
//     sum_j rescale(x^j)_l = (sum_j x^j_l + J h_l - sum_j lift((x^j_last + h_last) mod q_last)) q_last^-1   mod q_l
// EXACTLY: limbs 0 .. L-2 accumulate in the evaluation domain (one inverse transform per giant step instead of one per term), only
// the last limb keeps every term's product on its own.  All arithmetic is exact mod q_l on canonical residues, so the result has
// the bits of the term-by-term form (tests/test_ckks_matmul_gpu.py, tests/test_ckks_matmul_cpu.py).
#pragma once
#include "dev_arith.hpp"
#include "arith.hpp"
#include "rns_kernels.hpp"

namespace fhe {

// the terms of giant step i are term_start[i] .. term_start[i + 1] - 1 (row-major over the present (i, j)); term t multiplies
// baby slot term_baby[t]
struct MatTerms {
    const int *term_start;  // [n_giant + 1]
    const int *term_baby;   // [terms]
};

// two adjacent coefficients per lane: every access of these kernels is 16 bytes wide (n >= 2 is a power of two and every
// polynomial starts on a multiple of n words of a 256-byte aligned allocation)
__device__ __forceinline__ ulonglong2 ld2(const u64 *p) { return *reinterpret_cast<const ulonglong2 *>(p); }
__device__ __forceinline__ void st2(u64 *p, u64 x, u64 y) { *reinterpret_cast<ulonglong2 *>(p) = ulonglong2{x, y}; }

// y mod q for any 64-bit y; mu = floor(2^64 / q) (RescaleConsts::red_mu): the estimate is short by at most 2
__device__ __forceinline__ u64 red64(u64 y, u64 mu, u64 q) { return csub(csub(y - __umul64hi(y, mu) * q, q), q); }

// acc (128 bits) += a * b
__device__ __forceinline__ void mac128(u64 &lo, u64 &hi, u64 a, u64 b) {
    const u64 pl = a * b, s = lo + pl;
    hi += __umul64hi(a, b) + (s < pl ? 1 : 0);
    lo = s;
}
// (hi 2^64 + lo) mod q, canonical: hi and lo reduced on their own, 2^64 mod q = c64 = -(q mu) mod 2^64 with mu = floor(2^64 / q)
__device__ __forceinline__ u64 reduce128(u64 lo, u64 hi, const Barrett &b, u64 mu) {
    const u64 c64 = 0 - b.q * mu;
    return csub(mulmod_barrett(red64(hi, mu, b.q), c64, b) + red64(lo, mu, b.q), b.q);
}

// Fold bound of the 128-bit dot product.  Between two reductions the accumulator holds r + sum of F products with r < q the
// residue the last reduction left (or 0) and every product <= (q - 1)^2, q < 2^b:
//     r + F (q - 1)^2 < q + F q^2 - 2 F q + F <= F q^2 < F 2^(2b)     (F >= 1, q >= 2),
// so no carry leaves bit 127 while F <= 2^(128 - 2b): 256 terms at 60 bits, 64 at 61, 16 at 62 (the widest modulus a context
// takes).  The host passes F for the widest limb of the launch (mat_fold_bound below); a launch whose giant steps all have at
// most F terms is instantiated without the counter (FOLD = false).
constexpr int mat_fold_bound(int bits) { return 128 - 2 * bits >= 20 ? (1 << 20) : (1 << (128 - 2 * bits)); }
static_assert(mat_fold_bound(60) == 256 && mat_fold_bound(61) == 64 && mat_fold_bound(62) == 16, "F = 2^(128 - 2b)");

// D[i, j] (.) R[j] summed over the terms of giant step i, in the evaluation domain.
//   rot   [n_baby][2][batch][L][n]   the baby-step rotations of (b, a), transformed
//   d_lo  [terms][L - 1][n], d_hi [terms][n]   the diagonals' evaluations on limbs 0 .. L-2 and on limb L-1
//   acc   [n_giant][2][batch][L - 1][n]   limb l < L-1: sum_j d_lo[t_j][l] rot[j][h][c][l] mod q_l, ONE reduction per output
//   last  [terms][2][batch][n]            limb L-1: every term's product on its own
// blockIdx.y walks (giant step, half, ciphertext, limb of L); a lane owns two adjacent coefficients.  Per output the kernel
// streams J + 1 operands of 16 bytes per lane and does two 64 x 64 -> 128 multiply-adds per term: it is shaped by HBM, not by issue.
template <bool FOLD>
__global__ void ckks_mat_mac_kernel(const u64 *__restrict__ rot, const u64 *__restrict__ d_lo, const u64 *__restrict__ d_hi, u64 *__restrict__ acc,
                                    u64 *__restrict__ last, MatTerms T, unsigned n, unsigned L, size_t batch, size_t rows, int fold,
                                    const Barrett *__restrict__ B, const u64 *__restrict__ red_mu) {
    const unsigned Ll = L - 1;
    for (size_t y = blockIdx.y; y < rows; y += gridDim.y) {
        const unsigned l = unsigned(y % L);
        const size_t hc = (y / L) % (2 * batch), i = y / (size_t(L) * 2 * batch);  // hc = half * batch + ciphertext
        const Barrett b{ldc(&B[l].q, 0), ldc(&B[l].mu, 0), ldc(&B[l].sh1, 0), ldc(&B[l].sh2, 0)};
        const u64 mu = ldc(red_mu, (int)l);
        const int t0 = ldc(T.term_start, (int)i), t1 = ldc(T.term_start, (int)i + 1);
        for (unsigned x = 2 * (blockIdx.x * blockDim.x + threadIdx.x); x < n; x += 2 * gridDim.x * blockDim.x) {
            if (l == Ll) {
                for (int t = t0; t < t1; ++t) {
                    const size_t jb = (size_t)ldc(T.term_baby, t);
                    const ulonglong2 r = ld2(rot + ((jb * 2 * batch + hc) * L + l) * n + x), d = ld2(d_hi + size_t(t) * n + x);
                    st2(last + (size_t(t) * 2 * batch + hc) * n + x, mulmod_barrett(d.x, r.x, b), mulmod_barrett(d.y, r.y, b));
                }
                continue;
            }
            u64 lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
            int left = fold;
            for (int t = t0; t < t1; ++t) {
                const size_t jb = (size_t)ldc(T.term_baby, t);
                const ulonglong2 r = ld2(rot + ((jb * 2 * batch + hc) * L + l) * n + x), d = ld2(d_lo + (size_t(t) * Ll + l) * n + x);
                if (FOLD && left == 0) {
                    lo0 = reduce128(lo0, hi0, b, mu); lo1 = reduce128(lo1, hi1, b, mu);
                    hi0 = hi1 = 0;
                    left = fold;
                }
                mac128(lo0, hi0, d.x, r.x);
                mac128(lo1, hi1, d.y, r.y);
                if (FOLD) --left;
            }
            st2(acc + ((i * 2 * batch + hc) * Ll + l) * n + x, reduce128(lo0, hi0, b, mu), reduce128(lo1, hi1, b, mu));
        }
    }
}

// The rescale of a giant step's SUM, in place on acc (coefficient domain by now):
//     acc_l <- (acc_l + J h_l - sum_j lift_j) q_last^-1 mod q_l,     lift_j = ((t_j + h_last) mod q_last) mod q_l,
// t_j the coefficient of term j on the last limb (`last`, coefficient domain).  Every lift is reduced into q_l BEFORE it is added (as
// integers J of them pass 2^64 from J = 16), and J h_l is formed by the same modular additions.  R = the context's `rescale()` constants
// (fhe_rns_ctx::resc_last, the ones rns_rescale_kernel reads); with J = 1 this is rescale_limb's K == 1 branch line by line.
FHE_HEADER_KERNEL void ckks_mat_rescale_kernel(u64 *__restrict__ acc, const u64 *__restrict__ last, MatTerms T, unsigned n, unsigned Ll, size_t batch,
                                               size_t rows, RescaleConsts R) {
    const u64 ql = ldc(R.p_mod, 0), hl = ldc(R.half_p, 0);
    for (size_t y = blockIdx.y; y < rows; y += gridDim.y) {
        const int l = int(y % Ll);
        const size_t hc = (y / Ll) % (2 * batch), i = y / (size_t(Ll) * 2 * batch);
        const u64 q = ldc(R.q_mod, l), hq = ldc(R.half_q, l), mu = ldc(R.red_mu, l), pinv = ldc(R.pinv, l), pinv_s = ldc(R.pinv_s, l);
        const int t0 = ldc(T.term_start, (int)i), t1 = ldc(T.term_start, (int)i + 1);
        for (unsigned x = 2 * (blockIdx.x * blockDim.x + threadIdx.x); x < n; x += 2 * gridDim.x * blockDim.x) {
            u64 *dst = acc + y * n + x;
            const ulonglong2 a = ld2(dst);
            u64 v0 = a.x, v1 = a.y, s0 = 0, s1 = 0;
            for (int t = t0; t < t1; ++t) {
                const ulonglong2 tv = ld2(last + (size_t(t) * 2 * batch + hc) * n + x);
                v0 = csub(v0 + hq, q); v1 = csub(v1 + hq, q);
                s0 = csub(s0 + red64(csub(tv.x + hl, ql), mu, q), q);
                s1 = csub(s1 + red64(csub(tv.y + hl, ql), mu, q), q);
            }
            const u64 d0 = v0 >= s0 ? v0 - s0 : v0 + q - s0, d1 = v1 >= s1 ? v1 - s1 : v1 + q - s1;
            st2(dst, csub(mul_shoup_lazy(d0, pinv, pinv_s, q), q), csub(mul_shoup_lazy(d1, pinv, pinv_s, q), q));
        }
    }
}

// out [polys][n] = sum_i steps[i][polys][n] (giant-step stride `stride` words) mod the limb's modulus: the closing sum of `mul_mat`.
// `out` is the caller's buffer, of which only 8-byte alignment is known: two 8-byte stores.
FHE_HEADER_KERNEL void ckks_mat_sum_kernel(const u64 *__restrict__ steps, size_t stride, int n_steps, u64 *__restrict__ out, unsigned n, unsigned limbs,
                                           size_t polys, const Barrett *__restrict__ B) {
    for (size_t y = blockIdx.y; y < polys; y += gridDim.y) {
        const u64 q = ldc(&B[unsigned(y % limbs)].q, 0);
        for (unsigned x = 2 * (blockIdx.x * blockDim.x + threadIdx.x); x < n; x += 2 * gridDim.x * blockDim.x) {
            ulonglong2 s = ld2(steps + y * n + x);
            for (int i = 1; i < n_steps; ++i) {
                const ulonglong2 v = ld2(steps + size_t(i) * stride + y * n + x);
                s.x = csub(s.x + v.x, q); s.y = csub(s.y + v.y, q);
            }
            out[y * n + x] = s.x;
            out[y * n + x + 1] = s.y;
        }
    }
}

}  // namespace fhe
