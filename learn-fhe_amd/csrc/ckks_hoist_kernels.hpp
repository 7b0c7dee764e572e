// Kernels of the hoisted CKKS rotations and the double-hoisted diagonal-matrix product (ckks_hoist_api.hip).
//
// A ciphertext (b, a) over qs is lifted once: a~ = (a || ext(a)) and b~ = P b over qs || ps, both transformed.  In the evaluation
// domain the automorphism sigma_t is the permutation pi_t of ckks_hoist.hpp, so the key switch of rotation j is, per point k of limb l,
//     u_j.b[k] = P b^[pi_j(k)] + K_j.b[k] a^[pi_j(k)],     u_j.a[k] = K_j.a[k] a^[pi_j(k)]          (u_0 = (P b^, P a^), no key),
// and a giant step's sum w_i = sum_j D_ij u_j is a gather-multiply-accumulate over the baby steps that never leaves qs || ps.
//
// Reduction schedule: u_j is reduced to a canonical residue (one Barrett product and one conditional subtraction), the products
// D u accumulate unreduced in 128 bits under the fold bound of ckks_hoist.hpp, one reduction per output.  Nothing is folded into the
// diagonals at prepare time: the device keeps the T (L + K) n words of the diagonals and the keys it already has, where folding
// D (.) K.b and D (.) K.a would keep 2 T (L + K) n more and save the one Barrett product per term of a kernel that waits for memory.
//
// Gather: a lane owns the adjacent points 2x, 2x + 1; pi(2x + 1) = pi(2x) ^ 1, so it reads ONE aligned 16-byte pair and swaps its
// halves where pi(2x) is odd.  A wave's 128 points read one aligned 1 KiB block of the operand (ckks_hoist.hpp: pairs, blocks): every
// byte of every cache line it touches is used, by that wave, in that instruction -- no LDS staging would save a byte.  The gathered
// limb (n words, 256 KiB at n = 2^15) is read once per giant step and stays in L2 between them.
#pragma once
#include "dev_arith.hpp"
#include "arith.hpp"
#include "rns_kernels.hpp"
#include "ckks_matmul_kernels.hpp"
#include "ckks_hoist.hpp"

namespace fhe {

static_assert(hoist_fold_bound(60) == mat_fold_bound(60) && hoist_fold_bound(61) == mat_fold_bound(61) && hoist_fold_bound(62) == mat_fold_bound(62),
              "one bound for both accumulations");

// the baby steps of a prepared matrix: slot j rotates by t[j] = 5^j' mod 2n with the key (kb[j], ka[j]), each [L + K][n] in the
// evaluation domain; t[j] == 0: the ciphertext itself (no key)
struct HoistBabies {
    const u64 *const *kb;
    const u64 *const *ka;
    const unsigned *t;
};

// P mod q_l from the rescale constants: P is odd, h = floor(P / 2) mod q_l, P = 2 floor(P / 2) + 1
__device__ __forceinline__ u64 hoist_p_mod(const u64 *half_q, int l, u64 q) { return csub(csub(2 * ldc(half_q, l), q) + 1, q); }

// the pair (v[pi(x)], v[pi(x) ^ 1]) for an even x: p = pi(x)
__device__ __forceinline__ ulonglong2 ld2_perm(const u64 *v, unsigned p) {
    const ulonglong2 r = ld2(v + (p & ~1u));
    return (p & 1u) ? ulonglong2{r.y, r.x} : r;
}

// sigma_t on evaluation-domain polynomials: out[y][k] = in[y][pi_t(k)], in / out [polys][n] (the caller's buffers: 8-byte accesses)
FHE_HEADER_KERNEL void rns_automorphism_eval_kernel(const u64 *__restrict__ in, u64 *__restrict__ out, int log_n, size_t polys, unsigned t) {
    const unsigned n = 1u << log_n;
    for (size_t y = blockIdx.y; y < polys; y += gridDim.y)
        for (unsigned k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) out[y * n + k] = in[y * n + hoist_pi(k, t, log_n)];
}

// b~ = P b on the q-limbs: in (the caller's) / out [polys][n], polys = batch * L
FHE_HEADER_KERNEL void ckks_hoist_scale_kernel(const u64 *__restrict__ in, u64 *__restrict__ out, unsigned n, unsigned L, size_t polys,
                                               const u64 *__restrict__ half_q, const Barrett *__restrict__ B) {
    for (size_t y = blockIdx.y; y < polys; y += gridDim.y) {
        const int l = int(y % L);
        const Barrett b{ldc(&B[l].q, 0), ldc(&B[l].mu, 0), ldc(&B[l].sh1, 0), ldc(&B[l].sh2, 0)};
        const u64 pm = hoist_p_mod(half_q, l, b.q);
        for (unsigned k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) out[y * n + k] = mulmod_barrett(in[y * n + k], pm, b);
    }
}

// u_j for one pair of points of limb l of ciphertext c.  h: 0 = the b half, 1 = the a half; kh = the key's half h on limb l (null:
// j = 0); ea = a^ of (c, l); eb = P b^ of (c, l) (read only where l < L); pm = P mod q_l (0 on the p-limbs)
__device__ __forceinline__ ulonglong2 hoist_u(const u64 *__restrict__ kh, const u64 *__restrict__ ea, const u64 *__restrict__ eb, bool h, bool q_limb,
                                              unsigned x, unsigned t, int log_n, u64 pm, const Barrett &b) {
    if (!kh) {
        if (!h) return q_limb ? ld2(eb + x) : ulonglong2{0, 0};
        if (!q_limb) return ulonglong2{0, 0};
        const ulonglong2 a = ld2(ea + x);
        return ulonglong2{mulmod_barrett(a.x, pm, b), mulmod_barrett(a.y, pm, b)};
    }
    const unsigned p = hoist_pi(x, t, log_n);
    const ulonglong2 a = ld2_perm(ea, p), k = ld2(kh + x);
    ulonglong2 u{mulmod_barrett(k.x, a.x, b), mulmod_barrett(k.y, a.y, b)};
    if (!h && q_limb) {
        const ulonglong2 v = ld2_perm(eb, p);
        u.x = csub(u.x + v.x, b.q);
        u.y = csub(u.y + v.y, b.q);
    }
    return u;
}

// One rotation of fhe_ckks_rotate_many: p [2][batch][L+K][n] = u (evaluation domain).  ext [batch][L+K][n], bh [batch][L][n];
// kb, ka [L+K][n]; blockIdx.y walks (half, ciphertext, limb)
FHE_HEADER_KERNEL void ckks_hoist_rot_kernel(const u64 *__restrict__ ext, const u64 *__restrict__ bh, const u64 *__restrict__ kb, const u64 *__restrict__ ka,
                                             u64 *__restrict__ p, unsigned t, int log_n, unsigned L, unsigned lk, size_t batch, size_t rows,
                                             const u64 *__restrict__ half_q, const Barrett *__restrict__ B) {
    const unsigned n = 1u << log_n;
    for (size_t y = blockIdx.y; y < rows; y += gridDim.y) {
        const unsigned l = unsigned(y % lk);
        const size_t c = (y / lk) % batch;
        const bool h = y / (size_t(lk) * batch) != 0, q_limb = l < L;
        const Barrett b{ldc(&B[l].q, 0), ldc(&B[l].mu, 0), ldc(&B[l].sh1, 0), ldc(&B[l].sh2, 0)};
        const u64 *kh = (h ? ka : kb) + size_t(l) * n, *ea = ext + (c * lk + l) * n, *eb = bh + (c * L + (q_limb ? l : 0)) * n;
        for (unsigned x = 2 * (blockIdx.x * blockDim.x + threadIdx.x); x < n; x += 2 * gridDim.x * blockDim.x) {
            const ulonglong2 u = hoist_u(kh, ea, eb, h, q_limb, x, t, log_n, 0, b);
            st2(p + y * n + x, u.x, u.y);
        }
    }
}

// w [n_giant][2][batch][L+K][n] = sum over the terms of giant step i of D[t] (.) u_{baby(t)}, evaluation domain over qs || ps.
//   ext [batch][L+K][n], bh [batch][L][n], dg [terms][L+K][n]; T as in ckks_mat_mac_kernel; red_mu [L+K] = floor(2^64 / modulus)
// blockIdx.y walks (giant step, half, ciphertext, limb); a lane owns two adjacent points.  FOLD: some giant step has more than
// `fold` terms.  Per output and term: one diagonal pair, one key pair, one or two gathered pairs, all 16 bytes wide.
template <bool FOLD>
__global__ void ckks_hoist_mac_kernel(const u64 *__restrict__ ext, const u64 *__restrict__ bh, const u64 *__restrict__ dg, u64 *__restrict__ w, MatTerms T,
                                      HoistBabies J, int log_n, unsigned L, unsigned lk, size_t batch, size_t rows, int fold,
                                      const u64 *__restrict__ half_q, const Barrett *__restrict__ B, const u64 *__restrict__ red_mu) {
    const unsigned n = 1u << log_n;
    for (size_t y = blockIdx.y; y < rows; y += gridDim.y) {
        const unsigned l = unsigned(y % lk);
        const size_t c = (y / lk) % batch, i = y / (size_t(lk) * 2 * batch);
        const bool h = (y / (size_t(lk) * batch)) % 2 != 0, q_limb = l < L;
        const Barrett b{ldc(&B[l].q, 0), ldc(&B[l].mu, 0), ldc(&B[l].sh1, 0), ldc(&B[l].sh2, 0)};
        const u64 mu = ldc(red_mu, (int)l), pm = q_limb ? hoist_p_mod(half_q, (int)l, b.q) : 0;
        const u64 *ea = ext + (c * lk + l) * n, *eb = bh + (c * L + (q_limb ? l : 0)) * n;
        const int t0 = ldc(T.term_start, (int)i), t1 = ldc(T.term_start, (int)i + 1);
        for (unsigned x = 2 * (blockIdx.x * blockDim.x + threadIdx.x); x < n; x += 2 * gridDim.x * blockDim.x) {
            u64 lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
            int left = fold;
            for (int t = t0; t < t1; ++t) {
                const int jb = ldc(T.term_baby, t);
                const unsigned tj = ldc(J.t, jb);
                const u64 *key = tj ? ldc(h ? J.ka : J.kb, jb) + size_t(l) * n : nullptr;
                const ulonglong2 u = hoist_u(key, ea, eb, h, q_limb, x, tj, log_n, pm, b), d = ld2(dg + (size_t(t) * lk + l) * n + x);
                if (FOLD && left == 0) {
                    lo0 = reduce128(lo0, hi0, b, mu); lo1 = reduce128(lo1, hi1, b, mu);
                    hi0 = hi1 = 0;
                    left = fold;
                }
                mac128(lo0, hi0, d.x, u.x);
                mac128(lo1, hi1, d.y, u.y);
                if (FOLD) --left;
            }
            st2(w + y * n + x, reduce128(lo0, hi0, b, mu), reduce128(lo1, hi1, b, mu));
        }
    }
}

}  // namespace fhe
