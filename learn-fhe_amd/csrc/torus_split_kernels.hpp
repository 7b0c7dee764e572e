// Low-latency TFHE blind rotation: a CLUSTER of G workgroups (G = 2, 6) owns one ciphertext for its whole walk.
//
// torusx3_blind_rotate_kernel (torus_forms.hpp) gives a ciphertext to one workgroup: at batch 1 one compute unit of the chip works.
// One CMUX of the three-piece f64 form (torusf_kernels.hpp: teamx3_cmux) is the digits once, then per output (a, b) 2d forward
// transforms, one multiply-accumulate sum and one inverse transform per key piece, and the roundings.  The two outputs are
// independent, and so are the three pieces of one output: member `rank` of a cluster computes the (output, pieces) share that
// tfhe_split.hpp names, publishes it as N words  sum over its pieces of round(s_p) << {0, 22, 43}[p],  and adds the shares of the
// others ("all-gather": every member holds the whole accumulator throughout, a step costs ONE hand-off).  The rotation, the
// difference and the digits are recomputed by every member: cheap, and no exchange.
//
// Bit-identical by construction: each rounded piece value is the exact integer of the one-workgroup kernel (the bound beside TorusX3
// does not depend on who computes it), and the shares are combined with wrapping 64-bit additions, which are associative: arrival
// order, placement and G cannot show in the result.
//
// The hand-off is that of fhew_split_kernels.hpp as it stands (its head comment has the protocol and why the double buffer is
// enough): 16-byte write-through stores of the share, every wave drains them, workgroup barrier, one lane's agent-scope store of the
// epoch; wave 0 polls the flags and the cluster's timeout word, one agent-scope acquire, barrier, 16-byte loads.  The epoch is the
// count of hand-offs so far + 1 and the slab is chosen by that count's parity: a step with a~_i = 0 is skipped by the whole cluster
// (the value is the same in every member) and counts as no hand-off, so that consecutive hand-offs always alternate slabs.  Every
// wait is bounded; a member that gives up stores the cluster's timeout word, every member then stores BR_STATUS_TIMEOUT into the
// call's status word and nobody writes the ciphertext's output.  All members of a launch must be co-resident: the host launches
// batch * G <= compute units workgroups, and zeroes the polled words in front of the launch.
#pragma once
#include "fhew_split_kernels.hpp"
#include "tfhe_split.hpp"
#include "torus_forms.hpp"

namespace fhe {

static_assert(TFHE_SPLIT_CTL_BYTES == SPLIT_CTL_WORDS * sizeof(unsigned), "one control line per cluster");

struct TorusSplitWs {
    unsigned *ctl;  // [batch][SPLIT_CTL_WORDS] polled words, zeroed before every launch
    u64 *slabs;     // [2 (hand-off parity)][batch][G][N] shares
    int *status;    // the call's status word
};

// The share (output o; NP pieces from p0 on: all three, or one) of the external product from the parked digits, already recombined:
// out = sum over the pieces of round(s_p) << {0, 22, 43}[p].  Per piece the operation sequence of x3_output.
template <class W, int NP>
__device__ __forceinline__ void x3_output_pieces(const unsigned *dig, const double2 *__restrict__ rows, int d2, int o, int p0, int lane, double2 *lds,
                                                 const ArithC64::K &k, u64 (&out)[2 * W::E]) {
    using A = ArithC64;
    constexpr int E = W::E, M = W::N;
    static_assert(NP == 1 || NP == 3, "one piece, or all of them");
    double2 s[NP][E];
#pragma unroll
    for (int q = 0; q < NP; ++q)
#pragma unroll
        for (int e = 0; e < E; ++e) s[q][e] = double2{0.0, 0.0};
    const double2 *row = rows + size_t(o) * 3 * M + size_t(p0) * M;  // rows: [limb][a | b][piece][M]
#pragma unroll 1
    for (int j = 0; j < d2; ++j) {
        const unsigned wl = dig[(j * 2 + 0) * W::TEAM + lane], wh = dig[(j * 2 + 1) * W::TEAM + lane];
        double2 x[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            x[e].x = (double)((int)(wl << (24 - 8 * e)) >> 24);
            x[e].y = (double)((int)(wh << (24 - 8 * e)) >> 24);
        }
        double2 kk[NP][E];  // requested before the transform, consumed after it (x3_output says why)
#pragma unroll
        for (int q = 0; q < NP; ++q)
#pragma unroll
            for (int e = 0; e < E; ++e) kk[q][e] = row[q * M + e * W::TEAM + lane];
        fwd_run<A, typename W::C, W::LOG_N, W::LOG_E, 0, true, W::WAVE>(x, lane, nullptr, lds, true, k);
#pragma unroll
        for (int q = 0; q < NP; ++q)
#pragma unroll
            for (int e = 0; e < E; ++e) cmac(s[q][e], x[e], kk[q][e]);
        row += 6 * M;
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) inv_run<A, typename W::C, W::LOG_N, W::LOG_E, W::LOG_N, true, W::WAVE>(s[q], lane, nullptr, lds, true, k);
    const int sh0 = p0 == 0 ? 0 : (p0 == 1 ? 22 : 43);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if constexpr (NP == 3) {
            out[e] = (u64)round_small(s[0][e].x) + ((u64)round_small(s[1][e].x) << 22) + ((u64)round_small(s[2][e].x) << 43);
            out[E + e] = (u64)round_small(s[0][e].y) + ((u64)round_small(s[1][e].y) << 22) + ((u64)round_small(s[2][e].y) << 43);
        } else {
            out[e] = (u64)round_small(s[0][e].x) << sh0;
            out[E + e] = (u64)round_small(s[0][e].y) << sh0;
        }
    }
}

// One CMUX step (r in [1, 2N)) on a cluster.  (ca, cb): the whole accumulator, in and out, identical in every member.  `handoff`:
// hand-offs of this cluster so far.  false: the cluster gave up (workgroup-uniform).  lds64: the team's image, then the area where
// teamx3_cmux parks an accumulator half (here: the broadcast word of the wait's outcome), then the digits.
template <class W, int G>
__device__ __forceinline__ bool teamx3_cmux_split(u64 (&ca)[2 * W::E], u64 (&cb)[2 * W::E], unsigned r, const double2 *__restrict__ rows, const TDecomp &P,
                                                  const ArithC64::K &k, int lane, u64 *lds64, unsigned *ctl, u64 *slabs, unsigned parity_words, int rank,
                                                  unsigned handoff) {
    typedef __attribute__((ext_vector_type(4))) unsigned v4u;
    constexpr int E = W::E, N = TorusX3<W>::N;
    static_assert(G == 2 || G == 6, "the role map of tfhe_split.hpp");
    static_assert(W::TEAMS == 1 && !W::WAVE && E % 2 == 0, "one multi-wave team per workgroup, 16-byte accesses");
    u64 *park = lds64 + TorusX3<W>::IMG_WORDS;
    unsigned *dig = reinterpret_cast<unsigned *>(park + N);
    {
        u64 da[2 * E], db[2 * E];
#pragma unroll
        for (int e = 0; e < 2 * E; ++e) { da[e] = ca[e]; db[e] = cb[e]; }
        pairs_rotate<W>(da, r, lane, lds64);
        pairs_rotate<W>(db, r, lane, lds64);
#pragma unroll
        for (int e = 0; e < 2 * E; ++e) { da[e] -= ca[e]; db[e] -= cb[e]; }
        park_digits_x3<W>(da, db, P, lane, dig);
    }
    const TfheSplitRole role = tfhe_split_role(G, rank);  // workgroup-uniform
    u64 x[2 * E];
    if constexpr (G == 2) x3_output_pieces<W, 3>(dig, rows, 2 * P.d, role.output, 0, lane, reinterpret_cast<double2 *>(lds64), k, x);
    else x3_output_pieces<W, 1>(dig, rows, 2 * P.d, role.output, rank >> 1, lane, reinterpret_cast<double2 *>(lds64), k, x);

    // ---- publish: pair r2 of the lane (x[2 r2], x[2 r2 + 1]) at 16-byte slot r2 * TEAM + lane of the member's slab ----
    u64 *slab0 = slabs + ((handoff & 1) ? parity_words : 0u);  // this cluster's G slabs of this parity
    {
        const u64 mine = reinterpret_cast<u64>(slab0 + size_t(rank) * N);
        const unsigned mine_lo = unsigned(__builtin_amdgcn_readfirstlane(int(unsigned(mine))));
        const unsigned mine_hi = unsigned(__builtin_amdgcn_readfirstlane(int(unsigned(mine >> 32))));
        const u64 mine_u = (u64(mine_hi) << 32) | u64(mine_lo);
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<u64 *>(mine_u), 0, N * 8, 0x00020000);
#pragma unroll
        for (int r2 = 0; r2 < E; ++r2) {
            const int off = (r2 * W::TEAM + lane) * 16;  // < N * 8: E * TEAM * 16 = N * 8
            const v4u v = {unsigned(x[2 * r2]), unsigned(x[2 * r2] >> 32), unsigned(x[2 * r2 + 1]), unsigned(x[2 * r2 + 1] >> 32)};
            __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, off, 0, 16);  // aux 16 = sc1: write-through
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // EVERY storing wave drains its stores ...
    __syncthreads();                                   // ... before the one lane that signals for all of them
    const unsigned epoch = handoff + 1;
    if (threadIdx.x == 0) __hip_atomic_store((gu32 *)ctl + rank, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    // ---- consume ----
    unsigned *okw = reinterpret_cast<unsigned *>(park);  // workgroup broadcast of the wait's outcome
    if (threadIdx.x < 64) {
        const bool ok = split_wait(ctl, G, epoch, threadIdx.x);
        if (ok) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // holds the barrier until the invalidate has completed
        }
        if (threadIdx.x == 0) *okw = ok ? 1u : 0u;
    }
    __syncthreads();
    if (*okw == 0) return false;
    // Member rank + i (mod G) holds a share of this member's output for even i, of the other output for odd i (G is even and the
    // output is the rank's parity).  All G - 1 foreign shares are requested before the first is added: one round trip, not G - 1.
    {
        u64x2 t[G - 1][E];
        unsigned rv = unsigned(rank);
        asm volatile("" : "+v"(rv));  // slab addresses in vector registers, as split_gather keeps them
#pragma unroll
        for (int i = 1; i < G; ++i) {
            unsigned g = rv + unsigned(i);
            g = g >= unsigned(G) ? g - unsigned(G) : g;
            const gv2 *p = (const gv2 *)(slab0 + size_t(g) * N);  // global, not flat, loads
#pragma unroll
            for (int r2 = 0; r2 < E; ++r2) t[i - 1][r2] = p[r2 * W::TEAM + lane];
        }
        u64 other[2 * E];
#pragma unroll
        for (int e = 0; e < 2 * E; ++e) other[e] = 0;
#pragma unroll
        for (int i = 1; i < G; ++i) {
#pragma unroll
            for (int r2 = 0; r2 < E; ++r2) {
                if (i & 1) { other[2 * r2] += t[i - 1][r2].x; other[2 * r2 + 1] += t[i - 1][r2].y; }
                else { x[2 * r2] += t[i - 1][r2].x; x[2 * r2 + 1] += t[i - 1][r2].y; }
            }
        }
        const bool mine_is_a = role.output == 0;
#pragma unroll
        for (int e = 0; e < 2 * E; ++e) {
            ca[e] += mine_is_a ? x[e] : other[e];
            cb[e] += mine_is_a ? other[e] : x[e];
        }
    }
    return true;
}

// grid = batch * G workgroups of W::THREADS (one team each); workgroup b is member b % G of cluster b / G.  The arguments of
// torusx3_blind_rotate_kernel, and the call's workspace.  Dynamic LDS: FormF<W, true>::lds_bytes(d), one team's.
template <class W, int G>
__global__ __launch_bounds__(W::THREADS) void torusx3_blind_rotate_split_kernel(
    const u64 *__restrict__ v, const unsigned *__restrict__ table_of, const u64 *__restrict__ a_tilde, const u64 *__restrict__ b_tilde, unsigned n_lwe,
    unsigned batch, typename FormF<W, true>::Key key, TorusSplitWs S, u64 *__restrict__ out_a, u64 *__restrict__ out_b) {
    using F = FormF<W, true>;
    constexpr int CNT = F::CNT, N = F::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = W::lane();
    const unsigned ct = blockIdx.x / unsigned(G);
    const int rank = int(blockIdx.x % unsigned(G));
    const typename F::Team tm = F::team_setup(key, smem_raw, 0);
    if (ct >= batch) return;
    // the start, in every member, as blind_rotate_body builds it
    u64 ca[CNT], cb[CNT];
    if (table_of != nullptr) v += size_t(__builtin_amdgcn_readfirstlane(table_of[ct])) * N;
    F::load(cb, v, lane);
#pragma unroll
    for (int e = 0; e < CNT; ++e) ca[e] = 0;
    F::rotate(cb, (2 * N - (unsigned(b_tilde[ct]) & (2 * N - 1))) & (2 * N - 1), lane, tm);  // (0, v).rotate(-b)
    const u64 *a = a_tilde + size_t(ct) * n_lwe;
    unsigned *ctl = S.ctl + size_t(ct) * SPLIT_CTL_WORDS;
    u64 *slabs = S.slabs + size_t(ct) * G * N;
    const unsigned parity_words = batch * unsigned(G) * N;  // batch * G <= compute units: far below 2^32
    unsigned handoff = 0;
    bool ok = true;
#pragma unroll 1
    for (unsigned i = 0; i < n_lwe && ok; ++i) {
        const unsigned r = __builtin_amdgcn_readfirstlane(unsigned(a[i]) & (2 * N - 1));
        if (r == 0) continue;  // the same in every member: no hand-off
        ok = teamx3_cmux_split<W, G>(ca, cb, r, key.rows + size_t(i) * F::per(key.P), key.P, tm.k, lane, tm.lds, ctl, slabs, parity_words, rank, handoff);
        ++handoff;
    }
    if (!ok) {
        if (threadIdx.x == 0) __hip_atomic_store((gu32 *)S.status, (unsigned)BR_STATUS_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    if (rank != 0) return;  // every member holds the result; member 0 writes it, and nobody after a timeout
    F::store(ca, out_a + size_t(ct) * N, lane);
    F::store(cb, out_b + size_t(ct) * N, lane);
}

}  // namespace fhe
