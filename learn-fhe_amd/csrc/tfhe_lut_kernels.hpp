// Kernels of the encrypted table look-up (tfhe_lut.hpp, fhe_tfhe_lut_eval; k = 1): a CMUX-tree level and the rotation ladder, each ONE
// template over the form of the prepared fhe_tggsw_key (torus_forms.hpp: the policy gives the registers, the LDS and the CMUX).  They
// differ from the CMUX and blind-rotation kernels there in where a team finds its key rows -- the selector index comes from the
// CIPHERTEXT, c m + l for address bit l of ciphertext c -- and in the rotation amounts, which are the public constants 2N - 2^l.
//
//   tree level v   job p = (c n_acc + g) half + t, half = 2^(h - 1 - v): out[p] = CMUX(selector c m + r + v; in[2 p], in[2 p + 1])
//                  = in[2 p] + external_product(selector, in[2 p + 1] - in[2 p]) (tggsw.rs:114-121): the difference is formed in
//                  registers, the plain external product runs on it, in[2 p] is read again (from cache) and added.  Level 0 (polys !=
//                  null) reads the SHARED packed polynomials (g 2^h + 2 t, + 1) as the b halves of trivial ciphertexts: a = 0, not loaded.
//   ladder         job = c n_acc + g: acc <- CMUX(selector c m + l; acc, acc X^(-2^l)) for l = 0 .. r - 1 (the CMUX step of
//                  bootstrapping.rs:94-95 with the rotation 2N - 2^l), the accumulator in the team's registers throughout.  polys !=
//                  null (no tree): the accumulator starts as (0, polys[g]).
//   extraction     sample_extract(u 2^m) of accumulator c n_acc + g for every output o = g per_acc + u (tglwe.rs:115-127): written by the
//                  ladder itself from its registers (ext_a != null: a reversed, partly negated copy, one global store per coefficient
//                  and live output; the accumulator is then not stored at all), or by tfhe_lut_extract_kernel from stored accumulators
//
// Per ciphertext the arithmetic is that of fhe_tggsw_cmux, fhe_tglwe_rotate and fhe_tglwe_sample_extract chained: the same device
// functions on the same operands, so the same bits in every exact form and, on one device, in the fft64 form.
#pragma once
#include "torus_forms.hpp"

namespace fhe {

struct LutJobs {
    unsigned jobs;       // teams with work
    unsigned n_acc;      // accumulators per ciphertext (G)
    unsigned half;       // tree level: pairs per accumulator; ladder: unused
    unsigned m;          // selectors per ciphertext
    unsigned first;      // tree level: r + v, the selector of this level; ladder: 0
    unsigned steps;      // ladder: r
    unsigned log_polys;  // level 0: h (polynomials per accumulator = 2^h)
    unsigned n_out;      // ladder that extracts: outputs per ciphertext
    unsigned log_per;    // ... and log2 of the outputs that share an accumulator
};

// X^(-2^l) as an exponent in [0, 2N): 2N - 2^l
__device__ __forceinline__ unsigned lut_step_rotation(unsigned two_n, unsigned l) { return two_n - (1u << l); }
// A team is one wave or several, so whatever depends on the job alone is uniform across the wave.  The compiler cannot see that (the job
// comes from threadIdx): stated here, the ciphertext index, and with it every key-row address, lives in scalar registers -- as the
// key-row addresses of the blind rotation do, which do not depend on the ciphertext at all.
template <class W>
__device__ __forceinline__ unsigned lut_uniform(unsigned v) {
    static_assert(W::TEAM >= 64, "a team must span whole waves for its job to be wave-uniform");
    return __builtin_amdgcn_readfirstlane(v);
}

// The lane index again, opaque to the compiler: addresses formed from it are computed where they are used.  Without it the per-lane
// offsets of a load in front of the CMUX and of the store (or second load) behind it are one value kept alive through the whole CMUX --
// 4 to 11 registers that the blind rotation, which loads and stores through different index expressions, does not hold.
__device__ __forceinline__ int lut_fresh_lane(int lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}

// The end of a ladder.  ext_a == null: the accumulator goes back to acc_a, acc_b [job][n].  Else the team writes its extractions itself:
// for every live output o = g per_acc + u, i = u 2^m, row = c n_out + o: coefficient q of the a half goes to ext_a[row][i - q] for q <= i
// and, negated, to ext_a[row][n + i - q] above (tglwe.rs:115-127 read from the source's side), coefficient i of the b half to ext_b[row].
// PAIRS: the f64 forms' layout, x[e] = coefficient k_e, x[E + e] = coefficient k_e + M; else x[e] = coefficient k_e.
template <class W, bool PAIRS, int CNT>
__device__ __forceinline__ void lut_ladder_finish(const u64 (&ca)[CNT], const u64 (&cb)[CNT], u64 *__restrict__ acc_a, u64 *__restrict__ acc_b,
                                                  u64 *__restrict__ ext_a, u64 *__restrict__ ext_b, unsigned ju, unsigned c, unsigned g, const LutJobs &J, int lane) {
    constexpr unsigned N = PAIRS ? 2 * W::N : W::N;
    static_assert(CNT == (PAIRS ? 2 : 1) * W::E, "one register per coefficient of the lane");
    const int ln = lut_fresh_lane(lane);
    if (ext_a == nullptr) {
#pragma unroll
        for (int x = 0; x < CNT; ++x) {
            const unsigned q = unsigned(coef_index<W>(ln, x % W::E)) + unsigned(x / W::E) * W::N;
            acc_a[size_t(ju) * N + q] = ca[x];
            acc_b[size_t(ju) * N + q] = cb[x];
        }
        return;
    }
    const unsigned o0 = g << J.log_per, live = min(1u << J.log_per, J.n_out - o0);  // g < n_acc: o0 < n_out
#pragma unroll 1
    for (unsigned u = 0; u < live; ++u) {
        const unsigned i = u << J.m;
        const size_t row = size_t(c) * J.n_out + o0 + u;
        u64 *dst = ext_a + row * N;
#pragma unroll
        for (int x = 0; x < CNT; ++x) {
            const unsigned q = unsigned(coef_index<W>(ln, x % W::E)) + unsigned(x / W::E) * W::N;
            dst[q <= i ? i - q : N + i - q] = q <= i ? ca[x] : 0 - ca[x];
            if (q == i) ext_b[row] = cb[x];
        }
    }
}

// what a team of the tree level works on
struct LutPair {
    unsigned c;          // ciphertext
    size_t src;          // index of the pair's first node: in the shared polynomials (level 0) or in the level's input
};
template <class W>
__device__ __forceinline__ LutPair lut_pair(unsigned p, const LutJobs &J, bool level0) {
    const unsigned pu = lut_uniform<W>(p), cg = pu / J.half, t = pu - cg * J.half, c = cg / J.n_acc, g = cg - c * J.n_acc;
    return LutPair{c, level0 ? (size_t(g) << J.log_polys) + 2 * size_t(t) : 2 * size_t(p)};
}

// ---- one body per operation, in the key's form F (torus_forms.hpp) -----------------------------------------------------------------

// the pair's difference ct1 - ct0 into (da, db); level 0: da = 0
template <class F>
__device__ __forceinline__ void lut_pair_diff(const u64 *__restrict__ s0a, const u64 *__restrict__ s0b, bool level0, int lane, u64 (&da)[F::CNT], u64 (&db)[F::CNT]) {
    constexpr int CNT = F::CNT, N = F::N;
    u64 x[CNT];
    F::load(db, s0b + N, lane);
    F::load(x, s0b, lane);
#pragma unroll
    for (int e = 0; e < CNT; ++e) db[e] -= x[e];
    if (level0) {
#pragma unroll
        for (int e = 0; e < CNT; ++e) da[e] = 0;
    } else {
        F::load(da, s0a + N, lane);
        F::load(x, s0a, lane);
#pragma unroll
        for (int e = 0; e < CNT; ++e) da[e] -= x[e];
    }
}
// out <- ct0 + (xa, xb); ct0 is read again (from cache)
template <class F>
__device__ __forceinline__ void lut_pair_finish(const u64 *__restrict__ s0a, const u64 *__restrict__ s0b, bool level0, int lane, u64 (&xa)[F::CNT], u64 (&xb)[F::CNT],
                                                u64 *__restrict__ oa, u64 *__restrict__ ob) {
    constexpr int CNT = F::CNT;
    u64 x[CNT];
    const int ln = lut_fresh_lane(lane);
    F::load(x, s0b, ln);
#pragma unroll
    for (int e = 0; e < CNT; ++e) xb[e] += x[e];
    if (!level0) {
        F::load(x, s0a, ln);
#pragma unroll
        for (int e = 0; e < CNT; ++e) xa[e] += x[e];
    }
    F::store(xa, oa, ln);
    F::store(xb, ob, ln);
}

// out[p] = CMUX(selector; in[2 p], in[2 p + 1]) of one pair.  Both 30-bit forms run the unpacked external product, as fhe_tggsw_cmux does
// (the packed form is bit-identical).
template <class F>
__global__ __launch_bounds__(F::Ring::THREADS, F::MIN_WAVES) void tfhe_lut_level_kernel(const u64 *__restrict__ polys, const u64 *__restrict__ in_a,
                                                                                        const u64 *__restrict__ in_b, u64 *__restrict__ out_a,
                                                                                        u64 *__restrict__ out_b, LutJobs J, typename F::Key key) {
    using W = typename F::Ring;
    constexpr int CNT = F::CNT, N = F::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = W::lane(), team = W::team();
    const unsigned p = blockIdx.x * W::TEAMS + team;
    const typename F::Team tm = F::team_setup(key, smem_raw, team);
    if (p >= J.jobs) return;
    const bool level0 = polys != nullptr;
    const LutPair pr = lut_pair<W>(p, J, level0);
    const u64 *s0b = (level0 ? polys : in_b) + pr.src * N, *s0a = in_a + pr.src * N;
    u64 da[CNT], db[CNT];
    lut_pair_diff<F>(s0a, s0b, level0, lane, da, db);
    F::external_product(da, db, key, size_t(pr.c) * J.m + J.first, tm, lane);
    lut_pair_finish<F>(s0a, s0b, level0, lane, da, db, out_a + size_t(p) * N, out_b + size_t(p) * N);
}

// FROM_POLYS: there was no tree, the accumulator starts as (0, polys[g]).  The two starts are two instantiations: one kernel with both
// kept 28 registers more alive through the CMUX loop than either needs
template <class F, bool FROM_POLYS>
__global__ __launch_bounds__(F::Ring::THREADS, F::MIN_WAVES) void tfhe_lut_ladder_kernel(const u64 *__restrict__ polys, u64 *__restrict__ acc_a,
                                                                                         u64 *__restrict__ acc_b, u64 *__restrict__ ext_a,
                                                                                         u64 *__restrict__ ext_b, LutJobs J, typename F::Key key) {
    using W = typename F::Ring;
    constexpr int CNT = F::CNT, N = F::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = W::lane(), team = W::team();
    const unsigned job = blockIdx.x * W::TEAMS + team;
    const typename F::Team tm = F::team_setup(key, smem_raw, team);
    if (job >= J.jobs) return;
    const unsigned ju = lut_uniform<W>(job), c = ju / J.n_acc, g = ju - c * J.n_acc;
    u64 ca[CNT], cb[CNT];
    if constexpr (FROM_POLYS) {
        F::load(cb, polys + size_t(g) * N, lane);
#pragma unroll
        for (int e = 0; e < CNT; ++e) ca[e] = 0;
    } else {
        F::load(cb, acc_b + size_t(ju) * N, lane);
        F::load(ca, acc_a + size_t(ju) * N, lane);
    }
    const size_t first = size_t(c) * J.m;
#pragma unroll 1
    for (unsigned l = 0; l < J.steps; ++l) F::cmux(ca, cb, lut_step_rotation(2 * N, l), key, first + l, tm, lane);
    lut_ladder_finish<W, F::PAIRS>(ca, cb, acc_a, acc_b, ext_a, ext_b, ju, c, g, J, lane);
}

// ---- extraction ------------------------------------------------------------------------------------------------------------------
// tglwe.rs:115-127 (k = 1) at index u 2^m of accumulator c n_acc + g for output o = g per_acc + u: acc [batch n_acc][n] ->
// out_a [batch][n_out][n], out_b [batch][n_out].  log_per = log2 per_acc (a power of two); rows = batch n_out.
FHE_HEADER_KERNEL void tfhe_lut_extract_kernel(const u64 *__restrict__ acc_a, const u64 *__restrict__ acc_b, unsigned n, unsigned m, unsigned log_per,
                                               unsigned n_acc, unsigned n_out, size_t rows, u64 *__restrict__ out_a, u64 *__restrict__ out_b) {
    const size_t total = size_t(n) * rows;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const size_t row = idx / n, c = row / n_out;
        const unsigned j = unsigned(idx - row * n), o = unsigned(row - c * n_out);
        const unsigned g = o >> log_per, i = (o & ((1u << log_per) - 1)) << m;
        const size_t src = (c * n_acc + g) * n;
        // a[..i+1].rev() ++ a[i+1..].rev().map(neg)
        out_a[idx] = j <= i ? acc_a[src + (i - j)] : 0 - acc_a[src + (n - 1 - (j - i - 1))];
        if (j == 0) out_b[row] = acc_b[src + i];
    }
}

}  // namespace fhe
