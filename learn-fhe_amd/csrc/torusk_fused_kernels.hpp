// Row T at TGLWE rank k = 2 and 3, fused: the three-piece exact form of torusf_kernels.hpp (a key word = k0 + k1 2^22 + k2 2^43, each piece
// multiplied through f64 transforms of N / 2 complex slots, rounded, recombined mod 2^64) with K1 = k + 1 polynomials per ciphertext.
// One team (WaveRing over the N / 2 slots, the k = 1 shapes) owns a ciphertext for a whole blind rotation: the composed route of
// torusk_kernels.hpp sends the accumulator through HBM four times per CMUX, here it leaves the team once, at the end.
//
// One CMUX (tggsw.rs:114-121 with ct0 = acc, ct1 = acc X^r; tggsw.rs:100-112 the product inside):
//   the K1 difference polynomials acc_p X^r - acc_p are formed one at a time and their d digits each parked as signed bytes in the team's
//   LDS (K1 d limbs, digit-major per polynomial as tggsw.rs:106-108 orders them);
//   K1 output passes, each over all K1 d limbs: the limb's three key-piece rows are requested, the limb is transformed, three
//   multiply-accumulates per slot; then three inverse transforms, the cheap rounding and p0 + (p1 << 22) + (p2 << 43) in wrapping u64.
//   Every limb is transformed once per output pass ((k + 1)^2 d forward transforms a CMUX): torusf_kernels.hpp measured the
//   alternatives at k = 1 (limbs transformed once and kept; all outputs in one pass) and found the key rows waited for in full.
//   Only the polynomial a pass adds to is in registers; the other k wait in lane-private LDS slots (k N words a team).
// Key rows: [entry][K1 d limbs][K1 outputs][3 pieces][N / 2] complex evaluations, evaluation lane * E + r of a row at slot r * TEAM + lane.
// Exactness: K1 d products are summed per output where k = 1 sums 2d: the bound of torusf_kernels.hpp with 2d replaced,
// err <= K1 d N 2^(log_b + 20) 160 2^-53 <= 0.04 while K1 d N 2^log_b <= 2^21 (the host's rule, torusk_api.hip).
#pragma once
#include "torus_forms.hpp"

namespace fhe {

template <class W, int K1>
struct TorusKX3 {
    using Ring = W;
    static constexpr int M = W::N, N = 2 * W::N, E = W::E, CNT = 2 * W::E, K = K1 - 1;
    static constexpr int IMG_WORDS = TorusX3<W>::IMG_WORDS;
    static constexpr int DIG_WORDS_PER_LIMB = TorusX3<W>::DIG_WORDS_PER_LIMB;
    static_assert(K1 == 3 || K1 == 4, "fused rank-k kernels cover k = 2 and k = 3");
    // per team: exchange / rotation image | k parked polynomials (lane-private slots) | the digits of one CMUX; behind the teams the
    // workgroup's copy of the twiddle tree
    static __host__ __device__ constexpr int lds_words(int limbs, int k) { return IMG_WORDS + k * N + limbs * DIG_WORDS_PER_LIMB; }
    static __host__ __device__ constexpr size_t lds_bytes(int limbs, int k) { return size_t(lds_words(limbs, k) * W::TEAMS + 2 * N) * 8; }
    struct Key {
        const double2 *__restrict__ rows;  // from the call's first entry on
        TDecomp P;
        const double2 *__restrict__ tw;    // the twiddle tree in HBM
    };
    struct Team {
        u64 *lds;
        ArithC64::K k;
    };
    static __host__ __device__ __forceinline__ size_t per(const TDecomp &P) { return size_t(K1 * P.d) * K1 * 3 * M; }
    // every thread of the workgroup: stages the twiddle tree (a workgroup barrier inside), in front of the early return of idle teams
    static __device__ __forceinline__ Team team_setup(const Key &key, unsigned char *smem_raw, int team) {
        const int words = lds_words(K1 * key.P.d, K);
        double2 *tw = reinterpret_cast<double2 *>(reinterpret_cast<u64 *>(smem_raw) + words * W::TEAMS);
        for (int i = threadIdx.x; i < N; i += W::THREADS) tw[i] = key.tw[i];
        __syncthreads();
        return Team{reinterpret_cast<u64 *>(smem_raw) + team * words, ArithC64::make(tw, W::LOG_N)};
    }
};

// key_pieces of torusf_kernels.hpp with every subtraction in u64: k - p0 leaves the signed range for k near 2^63 - 1 and wraps to
// -2^63, which the arithmetic shift then reads as meant (k = p0 + p1 2^22 + p2 2^43 mod 2^64, |p0| <= 2^21, |p1|, |p2| <= 2^20)
__device__ __forceinline__ void key_pieces_wrapping(u64 k, double (&p)[3]) {
    const long long p0 = (long long)(k << 42) >> 42;              // low 22 bits, sign extended
    const long long rem = (long long)(k - (u64)p0) >> 22;         // exact
    const long long p1 = (long long)((u64)rem << 43) >> 43;       // low 21 bits, sign extended
    const long long p2 = (long long)((u64)rem - (u64)p1) >> 21;   // |p2| <= 2^20
    p[0] = (double)p0; p[1] = (double)p1; p[2] = (double)p2;
}

// the d x 2E digits of ONE difference polynomial (park_digits_x3 for one polynomial): dig[(j * 2 + h) * TEAM + lane] packs the E digits
// of the lane's slots (h = 0: coefficients k_e, h = 1: coefficients k_e + M) as signed bytes; dig: the polynomial's first limb
template <class W>
__device__ __forceinline__ void park_digits_poly(const u64 (&dd)[2 * W::E], const TDecomp &P, int lane, unsigned *dig) {
    constexpr int E = W::E;
    const unsigned mask = (unsigned)P.mask;
    unsigned st[2 * E];  // log_b d <= 31 on this path: the state fits a dword after the rounding shift
#pragma unroll
    for (int e = 0; e < 2 * E; ++e) st[e] = (unsigned)((dd[e] + P.rnd) >> P.rb);
#pragma unroll 1
    for (int j = 0; j < P.d; ++j) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            unsigned w = 0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                unsigned &c = st[h * E + e];
                const unsigned limb = c & mask;
                c >>= P.log_b;
                const unsigned carry = (((limb - 1) | c) & limb) >> (P.log_b - 1);
                c += carry;
                w |= ((limb - (carry << P.log_b)) & 0xffu) << (8 * e);
            }
            dig[(j * 2 + h) * W::TEAM + lane] = w;
        }
    }
}

// output o of the external product from the parked digits (x3_output with K1 outputs a limb): out[e], out[E + e] = the exact
// coefficients mod 2^64
template <class W, int K1>
__device__ __forceinline__ void xk_output(const unsigned *dig, const double2 *__restrict__ rows, int limbs, int o, int lane, double2 *lds,
                                          const ArithC64::K &k, u64 (&out)[2 * W::E]) {
    using A = ArithC64;
    constexpr int E = W::E, M = W::N;
    double2 s0[E], s1[E], s2[E];
#pragma unroll
    for (int e = 0; e < E; ++e) s0[e] = s1[e] = s2[e] = double2{0.0, 0.0};
    const double2 *row = rows + size_t(o) * 3 * M;  // rows: [limb][output][piece][M]
#pragma unroll 1
    for (int j = 0; j < limbs; ++j) {
        const unsigned wl = dig[(j * 2 + 0) * W::TEAM + lane], wh = dig[(j * 2 + 1) * W::TEAM + lane];
        double2 x[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            x[e].x = (double)((int)(wl << (24 - 8 * e)) >> 24);
            x[e].y = (double)((int)(wh << (24 - 8 * e)) >> 24);
        }
        // requested BEFORE the limb's transform, consumed after it (x3_output has why).  Measured and dropped: the rows requested one limb
        // further ahead (a second set of row registers; four slots a lane spill 2 with it, so two slots a lane only): k = 3, N = 256,
        // n_lwe = 630 took 21.6 ms instead of 19.9 at batch 1 and 23.3 instead of 22.0 at batch 1024 -- the rows are not what a lone wave
        // waits for; its transforms' exchanges are.
        double2 k0[E], k1[E], k2[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int slot = e * W::TEAM + lane;
            k0[e] = row[slot]; k1[e] = row[M + slot]; k2[e] = row[2 * M + slot];
        }
        fwd_run<A, typename W::C, W::LOG_N, W::LOG_E, 0, true, W::WAVE>(x, lane, nullptr, lds, true, k);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            cmac(s0[e], x[e], k0[e]);
            cmac(s1[e], x[e], k1[e]);
            cmac(s2[e], x[e], k2[e]);
        }
        row += K1 * 3 * M;
    }
    inv_run<A, typename W::C, W::LOG_N, W::LOG_E, W::LOG_N, true, W::WAVE>(s0, lane, nullptr, lds, true, k);
    inv_run<A, typename W::C, W::LOG_N, W::LOG_E, W::LOG_N, true, W::WAVE>(s1, lane, nullptr, lds, true, k);
    inv_run<A, typename W::C, W::LOG_N, W::LOG_E, W::LOG_N, true, W::WAVE>(s2, lane, nullptr, lds, true, k);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        out[e] = (u64)round_small(s0[e].x) + ((u64)round_small(s1[e].x) << 22) + ((u64)round_small(s2[e].x) << 43);
        out[E + e] = (u64)round_small(s0[e].y) + ((u64)round_small(s1[e].y) << 22) + ((u64)round_small(s2[e].y) << 43);
    }
}

// r = 0xffffffff: plain external product, c <- key (.) c; else one CMUX step of the blind rotation, c <- c + key (.) (c X^r - c),
// r in [0, 2N), r = 0 leaves c as it is.  c: the K1 polynomials in the pairs layout; rows: the key entry; lds64: the team's LDS
template <class W, int K1>
__device__ __forceinline__ void teamxk_cmux(u64 (&c)[K1][2 * W::E], unsigned r, const double2 *__restrict__ rows, const TDecomp &P, const ArithC64::K &k,
                                            int lane, u64 *lds64) {
    using X = TorusKX3<W, K1>;
    constexpr int CNT = X::CNT, K = X::K;
    const bool plain = r == 0xffffffffu;
    if (r == 0) return;  // team-uniform
    u64 *park = lds64 + X::IMG_WORDS;
    unsigned *dig = reinterpret_cast<unsigned *>(park + K * X::N);
#pragma unroll
    for (int p = 0; p < K1; ++p) {
        u64 dd[CNT];
#pragma unroll
        for (int e = 0; e < CNT; ++e) dd[e] = c[p][e];
        if (!plain) {
            pairs_rotate<W>(dd, r, lane, lds64);
#pragma unroll
            for (int e = 0; e < CNT; ++e) dd[e] -= c[p][e];
        }
        park_digits_poly<W>(dd, P, lane, dig + p * P.d * 2 * W::TEAM);
    }
    // slot s holds polynomial s + 1 until pass s has run, polynomial s afterwards
#pragma unroll
    for (int p = 1; p < K1; ++p)
#pragma unroll
        for (int e = 0; e < CNT; ++e) park[((p - 1) * CNT + e) * W::TEAM + lane] = c[p][e];
#pragma unroll
    for (int o = 0; o < K1; ++o) {
        u64 x[CNT];
        xk_output<W, K1>(dig, rows, K1 * P.d, o, lane, reinterpret_cast<double2 *>(lds64), k, x);
        const int next = o < K ? o + 1 : o;
#pragma unroll
        for (int e = 0; e < CNT; ++e) {
            c[o][e] = plain ? x[e] : c[o][e] + x[e];
            if (o < K) {
                u64 *slot = park + (o * CNT + e) * W::TEAM + lane;
                c[next][e] = *slot;
                *slot = c[o][e];
            }
        }
    }
#pragma unroll
    for (int p = 0; p < K; ++p)
#pragma unroll
        for (int e = 0; e < CNT; ++e) c[p][e] = park[(p * CNT + e) * W::TEAM + lane];
}

// ---- blind rotation: bootstrapping.rs:84-96 at rank k, the whole fold in ONE launch ----------------------------------------------
// acc = (0, .., 0, v X^-b) in the team's registers, then acc <- cmux(brk_i, acc, acc X^(a_i)) for i = 0 .. n_lwe - 1; out [batch][K1][N].
// table_of as in blind_rotate_body (torus_forms.hpp): null = v [N] serves the batch, else ciphertext ct starts from v + table_of[ct] * N;
// the index is team-uniform, read once, NOT range-checked here.
template <class W, int K1>
__global__ __launch_bounds__(W::THREADS, TF_MIN_WAVES) void torusk_x3_blind_rotate_kernel(
    const u64 *__restrict__ v, const unsigned *__restrict__ table_of, const u64 *__restrict__ a_tilde, const u64 *__restrict__ b_tilde, unsigned n_lwe,
    unsigned batch, typename TorusKX3<W, K1>::Key key, u64 *__restrict__ out) {
    using X = TorusKX3<W, K1>;
    constexpr int CNT = X::CNT, N = X::N, K = X::K;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = W::lane(), team = W::team();
    const unsigned ct = blockIdx.x * W::TEAMS + team;
    const typename X::Team tm = X::team_setup(key, smem_raw, team);
    if (ct >= batch) return;
    u64 c[K1][CNT];
    if (table_of != nullptr) v += size_t(__builtin_amdgcn_readfirstlane(table_of[ct])) * N;  // this ciphertext's own table
    pairs_load<W>(c[K], v, lane);
#pragma unroll
    for (int p = 0; p < K; ++p)
#pragma unroll
        for (int e = 0; e < CNT; ++e) c[p][e] = 0;
    pairs_rotate<W>(c[K], (2 * N - (unsigned(b_tilde[ct]) & (2 * N - 1))) & (2 * N - 1), lane, tm.lds);  // (0, .., 0, v).rotate(-b)
    const u64 *a = a_tilde + size_t(ct) * n_lwe;
    const size_t per = X::per(key.P);
#pragma unroll 1
    for (unsigned i = 0; i < n_lwe; ++i) {
        const unsigned r = __builtin_amdgcn_readfirstlane(unsigned(a[i]) & (2 * N - 1));
        teamxk_cmux<W, K1>(c, r, key.rows + i * per, key.P, tm.k, lane, tm.lds);
    }
#pragma unroll
    for (int p = 0; p < K1; ++p) pairs_store<W>(c[p], out + (size_t(ct) * K1 + p) * N, lane);
}

// tggsw.rs:100-112 at rank k, in place on ct [batch][K1][N] under the key entry `key` starts at
template <class W, int K1>
__global__ __launch_bounds__(W::THREADS, TF_MIN_WAVES) void torusk_x3_external_product_kernel(u64 *__restrict__ ct_all, unsigned batch,
                                                                                               typename TorusKX3<W, K1>::Key key) {
    using X = TorusKX3<W, K1>;
    constexpr int CNT = X::CNT, N = X::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = W::lane(), team = W::team();
    const unsigned ct = blockIdx.x * W::TEAMS + team;
    const typename X::Team tm = X::team_setup(key, smem_raw, team);
    if (ct >= batch) return;
    u64 *g = ct_all + size_t(ct) * K1 * N;
    u64 c[K1][CNT];
#pragma unroll
    for (int p = 0; p < K1; ++p) pairs_load<W>(c[p], g + size_t(p) * N, lane);
    teamxk_cmux<W, K1>(c, 0xffffffffu, key.rows, key.P, tm.k, lane, tm.lds);
#pragma unroll
    for (int p = 0; p < K1; ++p) pairs_store<W>(c[p], g + size_t(p) * N, lane);
}

// tggsw.rs:114-121 at rank k: out = ct0 + external_product(key, ct1 - ct0), [batch][K1][N] each.  out may be ct0 or ct1: a team reads
// everything of its ciphertext (the difference from two loads, ct0 once more for the sum) before it stores any of it.
template <class W, int K1>
__global__ __launch_bounds__(W::THREADS, TF_MIN_WAVES) void torusk_x3_cmux_kernel(const u64 *ct0, const u64 *ct1, u64 *out, unsigned batch,
                                                                                   typename TorusKX3<W, K1>::Key key) {
    using X = TorusKX3<W, K1>;
    constexpr int CNT = X::CNT, N = X::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = W::lane(), team = W::team();
    const unsigned ct = blockIdx.x * W::TEAMS + team;
    const typename X::Team tm = X::team_setup(key, smem_raw, team);
    if (ct >= batch) return;
    const size_t base = size_t(ct) * K1 * N;
    u64 c[K1][CNT];
#pragma unroll
    for (int p = 0; p < K1; ++p) {
        u64 z[CNT];
        pairs_load<W>(c[p], ct1 + base + size_t(p) * N, lane);
        pairs_load<W>(z, ct0 + base + size_t(p) * N, lane);
#pragma unroll
        for (int e = 0; e < CNT; ++e) c[p][e] -= z[e];
    }
    teamxk_cmux<W, K1>(c, 0xffffffffu, key.rows, key.P, tm.k, lane, tm.lds);
#pragma unroll
    for (int p = 0; p < K1; ++p) {
        u64 z[CNT];
        pairs_load<W>(z, ct0 + base + size_t(p) * N, lane);
#pragma unroll
        for (int e = 0; e < CNT; ++e) c[p][e] += z[e];
    }
#pragma unroll
    for (int p = 0; p < K1; ++p) pairs_store<W>(c[p], out + base + size_t(p) * N, lane);
}

// key preparation: rows [polys][N] signed torus words, polys = count (k + 1) d (k + 1) in sk_encrypt's order, -> [poly][3 pieces][M]
// complex evaluations: job = (poly, piece).  The order of the polynomials IS [entry][limb][output].
template <class W>
__global__ __launch_bounds__(W::THREADS) void torusk_x3_key_prepare_kernel(const u64 *__restrict__ rows, size_t polys, const double2 *__restrict__ tw,
                                                                           double2 *__restrict__ out) {
    constexpr int E = W::E, M = W::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = W::lane(), team = W::team();
    const size_t job = size_t(blockIdx.x) * W::TEAMS + team;
    const ArithC64::K k = ArithC64::make(stage_twiddles<W>(tw, smem_raw), W::LOG_N);
    if (job >= 3 * polys) return;
    double2 *lds = reinterpret_cast<double2 *>(reinterpret_cast<u64 *>(smem_raw) + team * TorusF<W>::LDS_WORDS);
    const int piece = int(job % 3);
    const u64 *src = rows + (job / 3) * (2 * M);
    double2 x[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int c = coef_index<W>(lane, e);
        double plo[3], phi[3];
        key_pieces_wrapping(src[c], plo);
        key_pieces_wrapping(src[c + M], phi);
        x[e].x = piece == 0 ? plo[0] : (piece == 1 ? plo[1] : plo[2]);
        x[e].y = piece == 0 ? phi[0] : (piece == 1 ? phi[1] : phi[2]);
    }
    fwd_run<ArithC64, typename W::C, W::LOG_N, W::LOG_E, 0, true, W::WAVE>(x, lane, nullptr, lds, true, k);
    double2 *dst = out + job * M;
#pragma unroll
    for (int e = 0; e < E; ++e) dst[e * W::TEAM + lane] = x[e];
}

}  // namespace fhe
