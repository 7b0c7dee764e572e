// TGLWE x TGLWE product on the torus, k = 1: tensor, exact division by 2^p, relinearisation of the S^2 part.
//   tensor : C2 = rnd_p(s(A1) s(A2)), C1 = rnd_p(s(A1) s(B2) + s(B1) s(A2)), C0 = rnd_p(s(B1) s(B2)) mod 2^64, products over the integers
//   relin  : out_a = C1 + sum_j digit_j(C2) RLK_j.a, out_b = C0 + sum_j digit_j(C2) RLK_j.b mod 2^64
// One team (fhew_kernels.hpp: WaveRing, the torus shapes) owns a ciphertext pair; the evaluations of the operands and of their pieces stay in its registers.
// The tensor, per prime: forward transforms of A1, B1 and of the signed-high / unsigned-low 32-bit pieces of A2, B2 (tfhe_mul.hpp: mul_cut)
// through ONE instance of the transform (a loop with team-uniform selects), then for each of T = A1 A2, R = A1 B2 + B1 A2, B = B1 B2 the
// pointwise products with the high and the low pieces and two inverse transforms, again through one instance.  The first prime's six
// residue polynomials wait in the team's LDS parking area (each lane its own slots); behind the second prime's inverse transforms the
// Chinese remainder gives both piece integers as signed 128-bit values, tfhe_mul.hpp recombines and rounds.
// The relinearisation is team_torus_gadget<W, false> (torus_kernels.hpp): the d rows of the key against the digits of C2 alone.
// tglwe_mul_kernel runs one after the other on the same registers: nothing but the inputs and the result crosses HBM.
#pragma once
#include "dispatch.hpp"  // launch()
#include "torus_kernels.hpp"
#include "tfhe_mul.hpp"

namespace fhe {

// words of LDS per team: the exchange image and six parked residue polynomials (the relinearisation parks two)
template <class W>
constexpr int mul_lds_words() { return W::PN + 6 * W::N; }
template <class W>
constexpr size_t mul_lds_bytes() { return size_t(mul_lds_words<W>()) * 8 * W::TEAMS; }
// waves per SIMD the kernels are compiled for: the parked residues bound the residency of the multi-wave teams to two anyway
template <class W>
constexpr int mul_min_waves() { return W::WAVE ? 1 : 2; }

// a prepared relinearisation key: evaluation-domain rows per prime, [d][2][N] in key_perm layout (fhew_kernels.hpp)
struct RelinKeyArg {
    const u64 *__restrict__ rows0, *__restrict__ rows1;
    TorusConsts T;
    TDecomp P;
};

// x = r0 (mod p0), x = r1 (mod p1), |x| < p0 p1 / 2  ->  x as a signed 128-bit integer (crt2_mod64 with the high word kept)
__device__ __forceinline__ MulWide crt2_wide(u64 r0, u64 r1, const TorusConsts &T) {
    const u64 r0m = csub(r0, T.p1);
    const u64 diff = r1 >= r0m ? r1 - r0m : r1 + T.p1 - r0m;
    const u64 t = csub(mul_shoup_lazy(diff, T.inv01, T.inv01_s, T.p1), T.p1);
    const u64 lo_prod = T.p0 * t, hi_prod = __umul64hi(T.p0, t);
    u64 lo = lo_prod + r0;
    u64 hi = hi_prod + (lo < lo_prod);
    const bool upper = hi > T.Ph_hi || (hi == T.Ph_hi && lo > T.Ph_lo);
    if (upper) {  // minus p0 p1 = 2 floor(p0 p1 / 2) + 1
        const u64 P_hi = (T.Ph_hi << 1) | (T.Ph_lo >> 63);
        const u64 borrow = lo < T.P_lo;
        lo -= T.P_lo;
        hi = hi - P_hi - borrow;
    }
    return MulWide{lo, hi};
}

// residue mod p of a signed value of magnitude below p
__device__ __forceinline__ u64 small_residue(long long v, u64 p) { return v < 0 ? p - u64(-v) : u64(v); }

// (c0, c1, c2) <- tensor((a1, b1), (a2, b2), log_delta), in the coefficient layout of the team's registers.  The operands are read
// from memory once per prime (four polynomials held across the transforms would cost 8 E registers; the lines are in L2 the second time);
// nothing is written to memory here, so the caller may store over them afterwards.
template <class W>
__device__ __forceinline__ void team_tglwe_tensor(const u64 *a1, const u64 *b1, const u64 *a2, const u64 *b2, int log_delta, const TorusConsts &T,
                                                  int lane, u64 *lds, u64 (&c0)[W::E], u64 (&c1)[W::E], u64 (&c2)[W::E]) {
    using A = ArithPM<60>;
    constexpr int E = W::E;
    u64 *park = lds + W::PN;  // [3 outputs][2 pieces][E][TEAM]
#pragma unroll 1
    for (int pi = 0; pi < 2; ++pi) {
        const typename A::K k = A::make(T.descs[pi], W::LOG_N, 0, 0);
        const u64 p = pi ? T.p1 : T.p0;
        // evaluations: fa, fb of A1, B1 as the transform leaves them (multiplicands), the pieces of A2, B2 canonical (multipliers)
        u64 fa[E], fb[E], ah[E], al[E], bh[E], bl[E];
#pragma unroll 1
        for (int i = 0; i < 6; ++i) {
            u64 x[E];
            wave_load<W>(x, i == 0 ? a1 : i == 1 ? b1 : i < 4 ? a2 : b2, lane);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const MulCut c = mul_cut(x[e]);
                x[e] = i < 2 ? signed_residue(x[e], p) : (i & 1) ? c.lo : small_residue(c.hi, p);
            }
            fwd_run<A, typename W::C, W::LOG_N, W::LOG_E, 0, true, W::WAVE>(x, lane, nullptr, lds, true, k);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (i == 0) fa[e] = x[e];
                else if (i == 1) fb[e] = x[e];
                else {
                    const u64 v = A::canon_fwd(x[e], k);
                    if (i == 2) ah[e] = v;
                    else if (i == 3) al[e] = v;
                    else if (i == 4) bh[e] = v;
                    else bl[e] = v;
                }
            }
        }
#pragma unroll 1
        for (int o = 0; o < 3; ++o) {  // 0: T = A1 A2 -> c2, 1: R = A1 B2 + B1 A2 -> c1, 2: B = B1 B2 -> c0
            u64 sh[E], sl[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const u64 m = o == 2 ? fb[e] : fa[e];
                const u64 yh = o == 0 ? ah[e] : bh[e], yl = o == 0 ? al[e] : bl[e];
                u64 vh = csub(A::mulvar(m, yh, k), k.m.q), vl = csub(A::mulvar(m, yl, k), k.m.q);
                if (o == 1) {
                    vh = csub(vh + csub(A::mulvar(fb[e], ah[e], k), k.m.q), k.m.q);
                    vl = csub(vl + csub(A::mulvar(fb[e], al[e], k), k.m.q), k.m.q);
                }
                sh[e] = vh;
                sl[e] = vl;
            }
#pragma unroll 1
            for (int s = 0; s < 2; ++s) {  // two inverse transforms through one instance
                inv_run<A, typename W::C, W::LOG_N, W::LOG_E, W::LOG_N, true, W::WAVE>(sh, lane, nullptr, lds, true, k);
#pragma unroll
                for (int e = 0; e < E; ++e) { const u64 t = sh[e]; sh[e] = sl[e]; sl[e] = t; }
            }
            u64 *ph = park + size_t(o * 2) * W::N, *pl = ph + W::N;
            if (pi == 0) {
#pragma unroll
                for (int e = 0; e < E; ++e) { ph[e * W::TEAM + lane] = sh[e]; pl[e * W::TEAM + lane] = sl[e]; }
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const MulWide H = crt2_wide(ph[e * W::TEAM + lane], sh[e], T), L = crt2_wide(pl[e * W::TEAM + lane], sl[e], T);
                    ph[e * W::TEAM + lane] = tensor_round(tensor_recombine(H, L), log_delta);  // the lane's own slot, read above
                }
            }
        }
    }
    // the results waited in the parking area: three arrays live across the loops would cost 6 E registers there
#pragma unroll
    for (int e = 0; e < E; ++e) {
        c2[e] = park[e * W::TEAM + lane];
        c1[e] = park[2 * W::N + e * W::TEAM + lane];
        c0[e] = park[4 * W::N + e * W::TEAM + lane];
    }
}

// (c1, c0) <- (c1, c0) + sum_j digit_j(c2) RLK_j: team_torus_gadget over one polynomial's digits for both primes, then the Chinese
// remainder mod 2^64
template <class W>
__device__ __forceinline__ void team_tglwe_relin(u64 (&c0)[W::E], u64 (&c1)[W::E], const u64 (&c2)[W::E], const RelinKeyArg &key, int lane, u64 *lds) {
    using A = ArithPM<60>;
    constexpr int E = W::E;
    u64 *park = lds + W::PN;
    u64 xa[E], xb[E];
    {
        const typename A::K k0 = A::make(key.T.descs[0], W::LOG_N, 0, 0);
        team_torus_gadget<W, false>(c2, c2, key.rows0, key.P, key.T.p0, lane, lds, key.T.B0, k0, xa, xb);
#pragma unroll
        for (int e = 0; e < E; ++e) { park[e * W::TEAM + lane] = xa[e]; park[(E + e) * W::TEAM + lane] = xb[e]; }
    }
    {
        const typename A::K k1 = A::make(key.T.descs[1], W::LOG_N, 0, 0);
        team_torus_gadget<W, false>(c2, c2, key.rows1, key.P, key.T.p1, lane, lds, key.T.B1, k1, xa, xb);
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        c1[e] += crt2_mod64(park[e * W::TEAM + lane], xa[e], key.T);
        c0[e] += crt2_mod64(park[(E + e) * W::TEAM + lane], xb[e], key.T);
    }
}

// ct0, ct1 [batch][N] halves -> c0, c1, c2 [batch][N]; ceil(batch / W::TEAMS) workgroups, dynamic LDS mul_lds_bytes<W>()
template <class W>
__global__ __launch_bounds__(W::THREADS, (mul_min_waves<W>())) void tglwe_tensor_kernel(const u64 *ct0_a, const u64 *ct0_b, const u64 *ct1_a, const u64 *ct1_b,
                                                                                        int log_delta, TorusConsts T, u64 *__restrict__ c0,
                                                                                        u64 *__restrict__ c1, u64 *__restrict__ c2, unsigned batch) {
    constexpr int E = W::E, N = W::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = W::lane(), team = W::team();
    const unsigned ct = blockIdx.x * W::TEAMS + team;
    if (ct >= batch) return;  // team-uniform exit (a multi-wave team is a whole block: barriers stay matched)
    u64 *lds = reinterpret_cast<u64 *>(smem_raw) + team * mul_lds_words<W>();
    const size_t off = size_t(ct) * N;
    u64 r0[E], r1[E], r2[E];
    team_tglwe_tensor<W>(ct0_a + off, ct0_b + off, ct1_a + off, ct1_b + off, log_delta, T, lane, lds, r0, r1, r2);
    wave_store<W>(r0, c0 + off, lane);
    wave_store<W>(r1, c1 + off, lane);
    wave_store<W>(r2, c2 + off, lane);
}

// c0, c1, c2 [batch][N] -> out_a, out_b [batch][N] (may be c1, c0: a team reads its three polynomials before it stores); dynamic LDS
// W::TORUS_LDS_BYTES
template <class W>
__global__ __launch_bounds__(W::THREADS, (mul_min_waves<W>())) void tglwe_relin_kernel(RelinKeyArg key, const u64 *c0, const u64 *c1, const u64 *c2, u64 *out_a,
                                                                                       u64 *out_b, unsigned batch) {
    constexpr int E = W::E, N = W::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = W::lane(), team = W::team();
    const unsigned ct = blockIdx.x * W::TEAMS + team;
    if (ct >= batch) return;
    u64 *lds = reinterpret_cast<u64 *>(smem_raw) + team * W::TORUS_LDS_WORDS;
    const size_t off = size_t(ct) * N;
    u64 r0[E], r1[E], r2[E];
    wave_load<W>(r0, c0 + off, lane);
    wave_load<W>(r1, c1 + off, lane);
    wave_load<W>(r2, c2 + off, lane);
    team_tglwe_relin<W>(r0, r1, r2, key, lane, lds);
    wave_store<W>(r1, out_a + off, lane);
    wave_store<W>(r0, out_b + off, lane);
}

// relin(tensor(ct0, ct1, log_delta)) in one launch; out may be either input (a team stores only after its last read of them);
// dynamic LDS mul_lds_bytes<W>()
template <class W>
__global__ __launch_bounds__(W::THREADS, (mul_min_waves<W>())) void tglwe_mul_kernel(RelinKeyArg key, const u64 *ct0_a, const u64 *ct0_b, const u64 *ct1_a,
                                                                                     const u64 *ct1_b, int log_delta, u64 *out_a, u64 *out_b, unsigned batch) {
    constexpr int E = W::E, N = W::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = W::lane(), team = W::team();
    const unsigned ct = blockIdx.x * W::TEAMS + team;
    if (ct >= batch) return;
    u64 *lds = reinterpret_cast<u64 *>(smem_raw) + team * mul_lds_words<W>();
    const size_t off = size_t(ct) * N;
    u64 r0[E], r1[E], r2[E];
    team_tglwe_tensor<W>(ct0_a + off, ct0_b + off, ct1_a + off, ct1_b + off, log_delta, key.T, lane, lds, r0, r1, r2);
    team_tglwe_relin<W>(r0, r1, r2, key, lane, lds);
    wave_store<W>(r1, out_a + off, lane);
    wave_store<W>(r0, out_b + off, lane);
}

// the plaintext rows of a relinearisation key: out[j] = 2^(64 - log_b (d - j)) S^2 (the weight of digit j of fhe_torus_decompose, least significant first), S^2 the negacyclic integer square of sk mod 2^64.
// One thread per coefficient (key generation: n^2 word products once per key).
FHE_HEADER_KERNEL void rlk_plain_kernel(const u64 *__restrict__ sk, unsigned n, int log_b, int d, u64 *__restrict__ out) {
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        u64 acc = 0;
        for (unsigned j = 0; j < n; ++j) {
            const u64 prod = sk[j] * sk[(i - j) & (n - 1)];
            acc += j <= i ? prod : u64(0) - prod;
        }
        for (int j = 0; j < d; ++j) out[size_t(j) * n + i] = acc << (64 - log_b * (d - j));
    }
}

}  // namespace fhe
