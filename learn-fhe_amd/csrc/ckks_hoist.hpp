// Host and device index logic of the hoisted CKKS rotations and the double-hoisted diagonal-matrix product (fhe_rns_automorphism_eval,
// fhe_ckks_rotate_many, fhe_ckks_mul_mat_hoisted): plain C++ (no HIP), so that it also builds into a stand-alone
// program (tests/ckks_hoist_host_test.cpp).  What is here: the permutation an automorphism is in the evaluation domain, the fold bound
// of the accumulation, the workspace layouts and the admission rules.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/fhe_ring.h"

#if defined(__HIPCC__)
#define FHE_HOIST_HD __host__ __device__ inline
#else
#define FHE_HOIST_HD inline
#endif

namespace fhe {

// the low `bits` bits of k reversed (bits <= 32; 0 for bits == 0)
FHE_HOIST_HD unsigned hoist_brev(unsigned k, int bits) {
#if defined(__clang__)
    const unsigned r = __builtin_bitreverse32(k);
#else
    unsigned r = k;
    r = ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
    r = ((r >> 2) & 0x33333333u) | ((r & 0x33333333u) << 2);
    r = ((r >> 4) & 0x0f0f0f0fu) | ((r & 0x0f0f0f0fu) << 4);
    r = ((r >> 8) & 0x00ff00ffu) | ((r & 0x00ff00ffu) << 8);
    r = (r >> 16) | (r << 16);
#endif
    return bits ? r >> (32 - bits) : 0u;
}

// The forward transform leaves, at index k of its bit-reversed output, the value of the polynomial at psi^e(k) with
// e(k) = 2 brev(k) + 1 and psi the primitive 2n-th root the twiddle table is made of (fhe_ctx_twiddles: the table is the powers of
// omega in bit-reversed order, and layer l of the transform multiplies by entry 2^l + i).  sigma_t(x)(psi^e) = x(psi^(e t)), so
//     ntt(sigma_t x)[k] = ntt(x)[pi_t(k)],     e(pi_t(k)) = e(k) t mod 2n:
// a pure permutation, no signs.  Only the low log_n + 1 bits of e t matter: the 32-bit product may wrap (n <= 2^30, t < 2n, t odd).
//
// Two facts the kernels lean on (the host test checks both at every ring it is given):
//   pairs:   pi_t(k ^ 1) = pi_t(k) ^ 1.  brev(k ^ 1) = brev(k) ^ (n / 2), so e moves by n, e t by n t = n mod 2n, brev((e t - 1) / 2)
//            by its lowest bit: the two adjacent outputs of a lane read two adjacent inputs, one 16-byte load and a swap.
//   blocks:  pi_t maps every aligned block of 2^s indices onto one aligned block of 2^s indices.  The high log_n - s bits of k are the
//            low bits of brev(k) and so of e; the low bits of e t depend on the low bits of e alone, and they are the high bits of
//            pi_t(k).  The 128 outputs of a wave read one 1 KiB block of the operand, every byte of it.
FHE_HOIST_HD unsigned hoist_pi(unsigned k, unsigned t, int log_n) {
    const unsigned e = 2 * hoist_brev(k, log_n) + 1;
    const unsigned m = (e * t) & ((2u << log_n) - 1);
    return hoist_brev(m >> 1, log_n);
}

// Fold bound of the 128-bit accumulation of ckks_hoist_mac_kernel.  Every term adds ONE product d u of two canonical residues of a
// modulus q < 2^b (u = P b^ + k_b a^ is reduced before it is multiplied), and between two reductions the accumulator holds
// r + sum of F such products with r < q:
//     r + F (q - 1)^2 < q + F q^2 - 2 F q + F <= F q^2 < F 2^(2b)     (F >= 1, q >= 2),
// so no carry leaves bit 127 while F <= 2^(128 - 2b): 256 terms at 60 bits, 64 at 61, 16 at 62 -- the bound of ckks_mat_mac_kernel,
// here over the widest of all L + K moduli.
constexpr int hoist_fold_bound(int bits) { return 128 - 2 * bits >= 20 ? (1 << 20) : (1 << (128 - 2 * bits)); }
static_assert(hoist_fold_bound(60) == 256 && hoist_fold_bound(61) == 64 && hoist_fold_bound(62) == 16, "F = 2^(128 - 2b)");

inline int hoist_bits(uint64_t q) {
    int b = 0;
    for (; q; q >>= 1) ++b;
    return b;
}

// no kernel of the hoisted entries walks more than 2^30 polynomials, and every index into the workspace fits 63 bits
constexpr size_t HOIST_MAX_ROWS = size_t(1) << 30;

// Workspace of fhe_ckks_rotate_many, in words, all regions multiples of n:
//   ext [batch][L+K][n]  a~ = (a || ext(a)), transformed      bh [batch][L][n]  P b, transformed
//   p   [2][batch][L+K][n]  u_r, one rotation at a time
struct HoistRotWs {
    size_t ext = 0, bh = 0, p = 0, total = 0;
};
inline bool hoist_rot_ws(size_t n, size_t L, size_t K, size_t batch, HoistRotWs *ws) {
    if (!n || !L || !batch || (n >> 30) || L + K >= HOIST_MAX_ROWS || batch >= HOIST_MAX_ROWS / (2 * (L + K))) return false;
    const size_t lk = L + K;
    ws->ext = 0;
    ws->bh = ws->ext + batch * lk * n;
    ws->p = ws->bh + batch * L * n;
    ws->total = ws->p + 2 * batch * lk * n;
    return true;
}

// Workspace of fhe_ckks_mul_mat_hoisted, in words:
//   ext [batch][L+K][n] | bh [batch][L][n]                 as above
//   w   [n_g][2][batch][L+K][n]   the giant steps' sums over qs || ps; once divided by P they are dead, and the region then keeps
//                                 acc [n_g][2][batch][L-1][n], the giant steps' inputs and outputs
//   x   [n_g][2][batch][L][n]     rescale_k(w)
//   tmp [2][batch][L-1][n]        the automorphism of one giant step
// (the giant steps' key switches take 3 batch (L - 1 + K) n words of their own from the same pool)
struct HoistMatWs {
    size_t ext = 0, bh = 0, w = 0, x = 0, tmp = 0, total = 0;
};
inline bool hoist_mat_ws(size_t n, size_t L, size_t K, size_t batch, size_t n_giant, HoistMatWs *ws) {
    if (!n || L < 2 || !batch || !n_giant || (n >> 30) || L + K >= HOIST_MAX_ROWS) return false;
    const size_t lk = L + K;
    if (n_giant >= HOIST_MAX_ROWS / (2 * lk) || batch >= HOIST_MAX_ROWS / (2 * lk * n_giant)) return false;
    ws->ext = 0;
    ws->bh = ws->ext + batch * lk * n;
    ws->w = ws->bh + batch * L * n;
    ws->x = ws->w + n_giant * 2 * batch * lk * n;
    ws->tmp = ws->x + n_giant * 2 * batch * L * n;
    ws->total = ws->tmp + 2 * batch * (L - 1) * n;
    return true;
}

// strictly ascending indices (what the prepare entries ask of `giant` and `baby`)
inline bool hoist_ascending(const uint32_t *v, int cnt) {
    for (int i = 1; i < cnt; ++i)
        if (v[i] <= v[i - 1]) return false;
    return true;
}

// The terms of a split: present [n_giant][n_baby] -> term_start [n_giant + 1] followed by term_baby [terms] in `tab` (room for
// n_giant + 1 + n_giant n_baby ints); returns the number of terms and the longest giant step in *max_terms
inline int hoist_terms(const uint8_t *present, int n_giant, int n_baby, int *tab, int *max_terms) {
    int terms = 0;
    *max_terms = 0;
    tab[0] = 0;
    for (int i = 0; i < n_giant; ++i) {
        int cnt = 0;
        for (int j = 0; j < n_baby; ++j)
            if (present[size_t(i) * n_baby + j]) { tab[n_giant + 1 + terms] = j; ++terms; ++cnt; }
        tab[i + 1] = terms;
        if (cnt > *max_terms) *max_terms = cnt;
    }
    return terms;
}

}  // namespace fhe
