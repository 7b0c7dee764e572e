// Low-latency LMKCDEY blind rotation: a CLUSTER of G workgroups (G = 2, 4, 8) owns one ciphertext for its whole op list.
//
// blind_rotate_kernel (fhew_kernels.hpp) gives a ciphertext to one workgroup: at batch 1 one CU of the chip works.  Inside one
// step of the walk the 2d (external product) or d (key switch) digit polynomials are independent: each is decomposed,
// forward-transformed and multiplied into two evaluation-domain sums.  Here member `rank` of a cluster takes the digits
// j = rank (mod G), and the partial sums are combined through global memory ("all-gather": every member publishes its pair of
// partial sums, reads the other G - 1 pairs, and runs both inverse transforms itself, so every member holds the whole
// accumulator and a step costs ONE hand-off).
//
// Bit-identical by construction: a partial sum is brought to its canonical value in [0, q) before it is published, partials are
// added with canonical modular additions, and the inverse transform returns the canonical representative of an exact result mod
// q.  Nothing depends on arrival order, timing or placement.  A member without a digit (d = 3 under G = 8) publishes zeros.
//
// Hand-off (per step `o`, epoch = o + 1, never 0; slabs double-buffered by o & 1):
//   publish: 16-byte write-through (sc1) stores of the partial pair -> EVERY wave `s_waitcnt vmcnt(0)` -> workgroup barrier ->
//            ONE lane stores the epoch to the member's flag word with an agent-scope atomic store
//   consume: wave 0 polls the G flag words (one lane each) and the cluster's timeout word with relaxed agent-scope loads ->
//            ONE agent-scope acquire -> `s_waitcnt vmcnt(0)` -> workgroup barrier -> every wave loads the slabs (vector loads)
// A member's flag only grows, and a poll accepts flag >= epoch: a fast member may already have published step o + 1 (into the
// OTHER slab) when a slow one polls for step o.  It cannot have published step o + 2, which overwrites slab o & 1: that needs
// every member's step-(o + 1) flag, which a member stores only after it has read the slabs of step o.
//
// Every wait is bounded (SPLIT_SPIN_LIMIT polls).  The member that gives up stores the cluster's timeout word and leaves the step
// loop; the others see that word in their next poll and leave too; each stores the call's status word, and nobody writes the
// ciphertext's output.  All members of a launch must be co-resident: the host launches batch * G <= compute units workgroups.
// The polled words (flags, timeout) are zeroed by a hipMemsetAsync in front of every launch.
#pragma once
#include "fhew_kernels.hpp"

namespace fhe {

typedef __attribute__((address_space(1))) unsigned gu32;  // a GLOBAL agent-scope word (never flat)
typedef u64 u64x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) u64x2 gv2;      // 16 bytes of a slab

constexpr int SPLIT_MAX_G = 8;
constexpr int SPLIT_CTL_WORDS = 16;          // per cluster: [0, 8) member flags, [8] timeout word, rest padding (one 64-byte line)
constexpr int SPLIT_TMO_WORD = 8;
// polls of one wait before a member gives up: a poll is an L2 round trip plus s_sleep (about 1 us), a legitimate wait is the time
// the slowest member needs for its share of one step (tens of microseconds) or, at the first step, the skew of the launch
constexpr unsigned SPLIT_SPIN_LIMIT = 1u << 21;
constexpr int BR_STATUS_TIMEOUT = 3;         // value of the call's status word (1, 2: the schedule kernel's data checks)

struct SplitWs {
    unsigned *ctl;  // [batch][SPLIT_CTL_WORDS] polled words, zeroed before every launch
    u64 *slabs;     // [2 (step parity)][batch][G][2 (a, b)][N] canonical partial sums, key_perm order
    int *status;    // the call's status word
};

// one cluster's share of the workspace
struct SplitCluster {
    unsigned *ctl;          // its SPLIT_CTL_WORDS polled words
    u64 *slabs;             // its G slabs of even steps; those of odd steps lie parity_words further
    unsigned parity_words;  // batch * G * 2 * N
};

// wave 0: lane g < G watches member g's flag, the other lanes the cluster's timeout word.  true: every member has published
// `epoch`; false: a member gave up, here (the timeout word is then set) or elsewhere.  Wave-uniform result.
__device__ __forceinline__ bool split_wait(unsigned *ctl, int G, unsigned epoch, int lane) {
    gu32 *word = (gu32 *)ctl + (lane < G ? lane : SPLIT_TMO_WORD);
    for (unsigned spins = 0;; ++spins) {
        const unsigned v = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__any(lane >= G && v != 0)) return false;
        if (__all(lane >= G || v >= epoch)) return true;
        if (spins >= SPLIT_SPIN_LIMIT) {
            if (lane == 0) __hip_atomic_store((gu32 *)ctl + SPLIT_TMO_WORD, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
        __builtin_amdgcn_s_sleep(2);
    }
}

// adds the partial pairs of the other GG - 1 members (slabs g = rank + 1, rank + 2, .. mod GG: canonical modular additions, so the
// order is free) to the member's own pair in registers; vector loads of lane-dependent addresses behind the acquire
template <class W, int GG>
__device__ __forceinline__ void split_gather(u64 (&sa)[W::E], u64 (&sb)[W::E], const u64 *slab0, int rank, int lane, u64 q) {
    constexpr int E = W::E, N = W::N;
    ulonglong2 ta[GG - 1][E / 2], tb[GG - 1][E / 2];
    unsigned rv = unsigned(rank);
    asm volatile("" : "+v"(rv));  // slab addresses in vector registers: GG - 1 scalar base pointers would not fit the scalar file
#pragma unroll
    for (int i = 1; i < GG; ++i) {
        const gv2 *pa = (const gv2 *)(slab0 + size_t((rv + i) & (GG - 1)) * 2 * N);  // global, not flat, loads
        const gv2 *pb = pa + N / 2;
#pragma unroll
        for (int r2 = 0; r2 < E / 2; ++r2) {
            const u64x2 a = pa[r2 * W::TEAM + lane], b = pb[r2 * W::TEAM + lane];
            ta[i - 1][r2] = ulonglong2{a.x, a.y};
            tb[i - 1][r2] = ulonglong2{b.x, b.y};
        }
    }
#pragma unroll
    for (int i = 1; i < GG; ++i) {
#pragma unroll
        for (int r2 = 0; r2 < E / 2; ++r2) {
            sa[2 * r2] = csub(sa[2 * r2] + ta[i - 1][r2].x, q);
            sa[2 * r2 + 1] = csub(sa[2 * r2 + 1] + ta[i - 1][r2].y, q);
            sb[2 * r2] = csub(sb[2 * r2] + tb[i - 1][r2].x, q);
            sb[2 * r2 + 1] = csub(sb[2 * r2 + 1] + tb[i - 1][r2].y, q);
        }
    }
}

// One step of the walk on a cluster.  (ca, cb): the whole accumulator, coefficient layout, canonical, in and out -- identical in
// every member.  false: the cluster gave up (workgroup-uniform).
template <class A, class W>
__device__ __forceinline__ bool split_gadget_product(u64 (&ca)[W::E], u64 (&cb)[W::E], const u64 *__restrict__ rows, const DecompParams &P,
                                                     bool both, int lane, u64 *lds, const RingConsts &K, const typename A::K &k,
                                                     const SplitCluster &S, int G, int rank, unsigned step) {
    typedef __attribute__((ext_vector_type(4))) unsigned v4u;
    constexpr int E = W::E, N = W::N;
    const u64 q = K.B.q;
    typename A::MacAcc ma[E], mb[E];
    u64 sa[E], sb[E], st[E];
#pragma unroll
    for (int e = 0; e < E; ++e) { ma[e] = mb[e] = A::mac_zero(); st[e] = decomp_init(ca[e], P); }
    const int total = both ? 2 * P.d : P.d;
    KeyRow<W> kr;
    if (rank < total) load_row<W>(kr, rows + size_t(rank) * 2 * N, lane);
    int term = 0;
#pragma unroll 1
    for (int j = 0; j < total; ++j) {
        if (both && j == P.d) {
#pragma unroll
            for (int e = 0; e < E; ++e) st[e] = decomp_init(cb[e], P);
        }
        // the digits of a coefficient are peeled one after the other: every member walks all of them, and transforms its own
        u64 x[E];
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = decomp_next(st[e], P);
        if ((j & (G - 1)) != rank) continue;  // workgroup-uniform
        fwd_run<A, typename W::C, W::LOG_N, W::LOG_E, 0, true, W::WAVE>(x, lane, nullptr, lds, true, k);
        mac_row<A, W>(x, ma, mb, kr, term++, K, k);
        if (j + G < total) load_row<W>(kr, rows + size_t(j + G) * 2 * N, lane);
    }
    // canonical partial sums (mac_finish may leave q + eps)
#pragma unroll
    for (int e = 0; e < E; ++e) { sa[e] = csub(A::mac_finish(ma[e], k), q); sb[e] = csub(A::mac_finish(mb[e], k), q); }

    // ---- publish ----
    u64 *slab0 = S.slabs + ((step & 1) ? S.parity_words : 0u);  // this cluster's G slabs of this parity
    {
        // (the cluster's pointers live in vector registers to spare the scalar file: made uniform again for the descriptor)
        const u64 mine = reinterpret_cast<u64>(slab0 + size_t(rank) * 2 * N);
        const unsigned mine_lo = unsigned(__builtin_amdgcn_readfirstlane(int(unsigned(mine))));
        const unsigned mine_hi = unsigned(__builtin_amdgcn_readfirstlane(int(unsigned(mine >> 32))));
        const u64 mine_u = (u64(mine_hi) << 32) | u64(mine_lo);  // (both halves unsigned: a sign-extended low half would move the base)
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<u64 *>(mine_u), 0, 2 * N * 8, 0x00020000);
#pragma unroll
        for (int r2 = 0; r2 < E / 2; ++r2) {
            const int off = (r2 * W::TEAM + lane) * 16;
            const v4u va = {unsigned(sa[2 * r2]), unsigned(sa[2 * r2] >> 32), unsigned(sa[2 * r2 + 1]), unsigned(sa[2 * r2 + 1] >> 32)};
            const v4u vb = {unsigned(sb[2 * r2]), unsigned(sb[2 * r2] >> 32), unsigned(sb[2 * r2 + 1]), unsigned(sb[2 * r2 + 1] >> 32)};
            __builtin_amdgcn_raw_buffer_store_b128(va, rsrc, off, 0, 16);           // aux 16 = sc1: write-through
            __builtin_amdgcn_raw_buffer_store_b128(vb, rsrc, N * 8 + off, 0, 16);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // EVERY storing wave drains its stores ...
    __syncthreads();                                   // ... before the one lane that signals for all of them
    const unsigned epoch = step + 1;
    if (threadIdx.x == 0) __hip_atomic_store((gu32 *)S.ctl + rank, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    // ---- consume ----
    unsigned *okw = reinterpret_cast<unsigned *>(lds + W::PN);  // workgroup broadcast of the wait's outcome
    if (threadIdx.x < 64) {
        const bool ok = split_wait(S.ctl, G, epoch, threadIdx.x);
        if (ok) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // holds the barrier until the invalidate has completed
        }
        if (threadIdx.x == 0) *okw = ok ? 1u : 0u;
    }
    __syncthreads();
    if (*okw == 0) return false;
    // all G - 1 foreign pairs are requested before the first is added (the loads are latency bound: one round trip, not G - 1)
    if (G == 8) split_gather<W, 8>(sa, sb, slab0, rank, lane, q);
    else if (G == 4) split_gather<W, 4>(sa, sb, slab0, rank, lane, q);
    else split_gather<W, 2>(sa, sb, slab0, rank, lane, q);
    // two inverse transforms through ONE instance, as wave_gadget_product runs them
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
        inv_run<A, typename W::C, W::LOG_N, W::LOG_E, W::LOG_N, true, W::WAVE>(sa, lane, nullptr, lds, true, k);
#pragma unroll
        for (int e = 0; e < E; ++e) { const u64 t = sa[e]; sa[e] = sb[e]; sb[e] = t; }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        ca[e] = sa[e];
        cb[e] = both ? sb[e] : csub(sb[e] + cb[e], q);
    }
    return true;
}

// dynamic LDS of the split kernel: the exchange image and the broadcast word (16 bytes keep every carve offset aligned)
template <class W>
constexpr size_t split_lds_bytes() { return size_t(W::PN) * 8 + 16; }

// grid = batch * G workgroups of W::THREADS (W::TEAMS = 1); workgroup b is member b % G of cluster b / G
template <class A, class W>
__global__ __launch_bounds__(W::THREADS) void blind_rotate_split_kernel(BlindRotateParams BR, SplitWs S, u64 *__restrict__ out_a,
                                                                       u64 *__restrict__ out_b, unsigned batch, int G, RingConsts K) {
    static_assert(W::TEAMS == 1 && !W::WAVE, "one multi-wave team per workgroup");
    constexpr int E = W::E, N = W::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = W::lane();
    const unsigned ct = blockIdx.x / unsigned(G);
    const int rank = int(blockIdx.x % unsigned(G));
    if (ct >= batch) return;
    u64 *lds = reinterpret_cast<u64 *>(smem_raw);
    const typename A::K k = A::make(*K.desc, W::LOG_N, 0, 0);
    u64 ca[E], cb[E];
    // acc = (0, f.automorphism(-g) * X^(b*g)) as blind_rotate_kernel builds it, in every member
    {
        const u64 *f = BR.f + size_t(ct) * BR.f_stride;
        const unsigned b = unsigned(BR.lwe_b[ct] & (2 * N - 1));
        const unsigned kmono = (b * 5u) & (2 * N - 1);
        const unsigned tneg = (2 * N - 5u) & (2 * N - 1);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const unsigned i = coef_index<W>(lane, e);
            const u64 v = f[i];
            unsigned pos = (i * tneg) & (2 * N - 1);
            pos = (pos + kmono) & (2 * N - 1);
            lds[lds_phys(pos & (N - 1))] = pos < N ? v : (v ? K.B.q - v : 0);
        }
        exchange_sync<W::WAVE>();
#pragma unroll
        for (int e = 0; e < E; ++e) { cb[e] = lds[lds_phys(coef_index<W>(lane, e))]; ca[e] = 0; }
        exchange_sync<W::WAVE>();
    }
    const unsigned *ops = BR.ops + size_t(ct) * BR.max_ops;
    const unsigned nops = BR.nops[ct];
    SplitCluster C;
    C.ctl = S.ctl + size_t(ct) * SPLIT_CTL_WORDS;
    C.slabs = S.slabs + size_t(ct) * G * 2 * N;
    C.parity_words = batch * unsigned(G) * 2 * N;  // batch * G <= compute units: far below 2^32
    int *status = S.status;
    // uniform values that only memory instructions use: kept in vector registers, the scalar file is full (no spill either way)
    u64 *oa = out_a + size_t(ct) * N, *ob = out_b + size_t(ct) * N;
    const unsigned *ak_t = BR.ak_t;
    asm volatile("" : "+v"(C.ctl), "+v"(C.slabs), "+v"(status), "+v"(oa), "+v"(ob), "+v"(ops), "+v"(ak_t));
    bool ok = true;
    for (unsigned o = 0; o < nops && ok; ++o) {
        const unsigned op = __builtin_amdgcn_readfirstlane(ops[o]);
        const bool is_ak = (op & BR_OP_AK) != 0;
        const unsigned idx = op & 0x7fffffffu;
        if (is_ak) {
            const unsigned t = __builtin_amdgcn_readfirstlane(ak_t[idx]);
            wave_automorphism<W>(ca, t, lane, lds, K.B.q);
            wave_automorphism<W>(cb, t, lane, lds, K.B.q);
        }
        const FhewKey &key = is_ak ? BR.ak : BR.brk;
        ok = split_gadget_product<A, W>(ca, cb, key.rows + size_t(idx) * key.rows_per_ct * 2 * N, key.P, !is_ak, lane, lds, K, k, C, G, rank, o);
    }
    if (!ok) {  // the call's status word: the schedule kernel's data checks (1, 2) give way to this
        if (threadIdx.x == 0) __hip_atomic_store((gu32 *)status, (unsigned)BR_STATUS_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    if (rank != 0) return;  // every member holds the result; member 0 writes it, and nobody after a timeout
    wave_store<W>(ca, oa, lane);
    wave_store<W>(cb, ob, lane);
}

}  // namespace fhe
