// TGLWE automorphism key switch, trace and the merge step of the ring packing on the torus, k = 1.
//   autks_g : out_a = sum_j digit_j(sigma_g(a)) AK_j.a,  out_b = sigma_g(b) + sum_j digit_j(sigma_g(a)) AK_j.b   mod 2^64
//   trace   : ct <- ct + autks_{2^u + 1}(ct) for u = hi .. lo + 1
//   merge_l : (E, O) -> (E + X^(n/l) O) + autks_{l+1}(E - X^(n/l) O)
// One team (fhew_kernels.hpp: WaveRing, the torus shapes) owns a ciphertext.  The key switch is team_tglwe_relin (tfhe_mul_kernels.hpp)
// on (c0, c1, c2) = (sigma_g(b), 0, sigma_g(a)) under rows that encrypt -h_j sigma_g(S).  The signed permutation goes through the team's
// exchange image one polynomial at a time: every lane scatters its coefficients to i g mod 2n with the sign, the team synchronises, every
// lane reads its own coefficients back.  The image is addressed WITHOUT the transforms' padding here: 16 consecutive coefficients (one
// lane group of an 8-byte store) land g words apart, g odd, on 16 different 8-byte bank pairs, and the read-back is lane-contiguous
// (tools/tfhe_trace_bank_sim.py: multiplicity 1 both ways at every ring and g; with the padded addressing the scatter is up to 5-way and the read-back 2-way).
// tglwe_trace_kernel keeps the ciphertext in registers over all its steps, each under another key of a by-value table: nothing but the
// input and the result crosses HBM.  The rotation by n / l of a merge and the embedding of a TLWE input are index arithmetic in the load.
#pragma once
#include "dispatch.hpp"  // launch()
#include "tfhe_mul_kernels.hpp"
#include "tfhe_trace.hpp"

namespace fhe {

// the keys of up to TRACE_MAX_STEPS consecutive key switches: per step the Galois element and the two primes' rows, [d][2][N] key_perm
struct TraceKeysArg {
    const u64 *rows0[TRACE_MAX_STEPS], *rows1[TRACE_MAX_STEPS];
    unsigned g[TRACE_MAX_STEPS];
    int steps;
    TorusConsts T;
    TDecomp P;
};

// c <- sigma_g(c) through the team's LDS image (unpadded addressing: see above)
template <class W>
__device__ __forceinline__ void team_torus_automorphism(u64 (&c)[W::E], unsigned g, int lane, u64 *lds) {
    constexpr int E = W::E;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const SignedIdx t = auto_target(unsigned(coef_index<W>(lane, e)), g, W::LOG_N);
        lds[t.idx] = t.neg ? 0 - c[e] : c[e];
    }
    exchange_sync<W::WAVE>();
#pragma unroll
    for (int e = 0; e < E; ++e) c[e] = lds[coef_index<W>(lane, e)];
    exchange_sync<W::WAVE>();
}

// (a, b) <- X^r times a ciphertext in memory, in the coefficient layout of the team's registers.  embed = false: src_a, src_b are its
// polynomials; embed = true: src_a [N] is the mask of a TLWE ciphertext and src_b its one body word, and the ciphertext is embed of it
template <class W>
__device__ __forceinline__ void team_load_rotated(u64 (&a)[W::E], u64 (&b)[W::E], const u64 *__restrict__ src_a, const u64 *__restrict__ src_b,
                                                  unsigned r, bool embed, int lane) {
#pragma unroll
    for (int e = 0; e < W::E; ++e) {
        const SignedIdx s = rot_source(unsigned(coef_index<W>(lane, e)), r, W::LOG_N);
        u64 va, vb;
        if (embed) {
            const SignedIdx m = embed_source(s.idx, W::LOG_N);
            va = src_a[m.idx];
            if (m.neg) va = 0 - va;
            vb = s.idx == 0 ? src_b[0] : 0;
        } else {
            va = src_a[s.idx];
            vb = src_b[s.idx];
        }
        a[e] = s.neg ? 0 - va : va;
        b[e] = s.neg ? 0 - vb : vb;
    }
}

// (ca, cb) <- keep (ca, cb) + autks_g(ca, cb) with keep = 0 or 1 (team-uniform)
template <class W>
__device__ __forceinline__ void team_tglwe_autks(u64 (&ca)[W::E], u64 (&cb)[W::E], unsigned g, bool keep, const RelinKeyArg &key, int lane, u64 *lds) {
    constexpr int E = W::E;
    u64 pa[E];
    {
        u64 pb[E];
#pragma unroll
        for (int e = 0; e < E; ++e) { pa[e] = ca[e]; pb[e] = cb[e]; }
        team_torus_automorphism<W>(pa, g, lane, lds);
        team_torus_automorphism<W>(pb, g, lane, lds);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            ca[e] = keep ? ca[e] : 0;
            cb[e] = (keep ? cb[e] : 0) + pb[e];
        }
    }
    team_tglwe_relin<W>(cb, ca, pa, key, lane, lds);
}

// in [batch] ciphertexts -> out [batch][N] halves (out may be in: a team reads its ciphertext before it stores): keys.steps key switches,
// each ct <- keep ct + autks(ct).  embed: in_a [batch][N], in_b [batch] are TLWE ciphertexts, embedded in the load.
// ceil(batch / W::TEAMS) workgroups, dynamic LDS W::TORUS_LDS_BYTES
template <class W>
__global__ __launch_bounds__(W::THREADS, (mul_min_waves<W>())) void tglwe_trace_kernel(TraceKeysArg keys, const u64 *in_a, const u64 *in_b, unsigned keep,
                                                                                       unsigned embed, u64 *out_a, u64 *out_b, unsigned batch) {
    constexpr int E = W::E, N = W::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = W::lane(), team = W::team();
    const unsigned ct = blockIdx.x * W::TEAMS + team;
    if (ct >= batch) return;  // team-uniform exit (a multi-wave team is a whole block: barriers stay matched)
    u64 *lds = reinterpret_cast<u64 *>(smem_raw) + team * W::TORUS_LDS_WORDS;
    const size_t off = size_t(ct) * N;
    u64 ca[E], cb[E];
    team_load_rotated<W>(ca, cb, in_a + off, embed ? in_b + ct : in_b + off, 0, embed != 0, lane);
#pragma unroll 1
    for (int s = 0; s < keys.steps; ++s) {
        const RelinKeyArg key{keys.rows0[s], keys.rows1[s], keys.T, keys.P};
        team_tglwe_autks<W>(ca, cb, keys.g[s], keep != 0, key, lane, lds);
    }
    wave_store<W>(ca, out_a + off, lane);
    wave_store<W>(cb, out_b + off, lane);
}

// One level of the packing tree (tfhe_trace.hpp: pack_level).  Team T < teams: pack T / nodes, node o = T % nodes; it reads nodes o and
// o + nodes of its pack among the 2 nodes a pack of the level below, merges them under g with the rotation rot, and writes ciphertext
// T of out.  embed: the level below is the TLWE inputs, in_a [..][N], in_b [..].  out overlaps no input.
template <class W>
__global__ __launch_bounds__(W::THREADS, (mul_min_waves<W>())) void tglwe_merge_kernel(RelinKeyArg key, const u64 *in_a, const u64 *in_b, unsigned g, unsigned rot,
                                                                                       unsigned nodes, unsigned embed, u64 *__restrict__ out_a,
                                                                                       u64 *__restrict__ out_b, unsigned teams) {
    constexpr int E = W::E, N = W::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = W::lane(), team = W::team();
    const unsigned T = blockIdx.x * W::TEAMS + team;
    if (T >= teams) return;
    u64 *lds = reinterpret_cast<u64 *>(smem_raw) + team * W::TORUS_LDS_WORDS;
    const size_t ie = size_t(T / nodes) * 2 * nodes + T % nodes, io = ie + nodes;
    u64 sa[E], sb[E], da[E], db[E];
    team_load_rotated<W>(sa, sb, in_a + ie * N, embed ? in_b + ie : in_b + ie * N, 0, embed != 0, lane);
    team_load_rotated<W>(da, db, in_a + io * N, embed ? in_b + io : in_b + io * N, rot, embed != 0, lane);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const u64 ea = sa[e], eb = sb[e];
        sa[e] = ea + da[e]; sb[e] = eb + db[e];
        da[e] = ea - da[e]; db[e] = eb - db[e];
    }
    team_torus_automorphism<W>(da, g, lane, lds);
    team_torus_automorphism<W>(db, g, lane, lds);
#pragma unroll
    for (int e = 0; e < E; ++e) sb[e] += db[e];
    team_tglwe_relin<W>(sb, sa, da, key, lane, lds);
    wave_store<W>(sa, out_a + size_t(T) * N, lane);
    wave_store<W>(sb, out_b + size_t(T) * N, lane);
}

// the plaintext rows of a set of automorphism keys: out[q][j] = -2^(64 - log_b (d - j)) sigma_{g_q}(sk) mod 2^64; one thread per
// (key, coefficient)
FHE_HEADER_KERNEL void atk_plain_kernel(const u64 *__restrict__ sk, unsigned n, int log_n, const unsigned *__restrict__ gs, unsigned n_g, int log_b, int d,
                                        u64 *__restrict__ out) {
    const size_t total = size_t(n_g) * n;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const size_t q = idx / n;
        const unsigned i = unsigned(idx - q * n);
        const SignedIdx t = auto_target(i, gs[q], log_n);
        const u64 v = t.neg ? sk[i] : 0 - sk[i];  // -sigma(S) at coefficient t.idx
        for (int j = 0; j < d; ++j) out[(q * d + j) * n + t.idx] = v << (64 - log_b * (d - j));
    }
}

}  // namespace fhe
