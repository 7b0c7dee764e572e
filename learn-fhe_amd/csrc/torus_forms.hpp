// The forms a prepared fhe_tggsw_key can have, each named ONCE: a policy class per form over its team shape W, and the kernels whose
// bodies are the same text in every form -- the external product and the blind rotation (the table look-up's tree level and
// ladder, tfhe_lut_kernels.hpp, are written over the same policies).  A policy gives
//   Key                 what a kernel takes by value: the key rows from the call's first entry on, the gadget, the form's constants
//   per(P)              words from one key entry to the next, in the rows' own element type
//   CNT, N              registers per lane and half of a ciphertext, and the polynomial length
//   PAIRS               the f64 forms' register layout: x[e] = coefficient k_e, x[E + e] = coefficient k_e + N / 2
//   load, store, rotate a half between global memory and the team's registers; times X^r through the team's LDS image
//   team_setup          the team's LDS and what its transforms need; runs on EVERY thread of the workgroup, in front of the early
//                       return of idle teams: the f64 forms stage the twiddle tree into LDS there (a workgroup barrier inside)
//   cmux                acc <- acc + external_product(key[entry], acc X^r - acc); r = 0 leaves acc as it is
//   external_product    (a, b) <- external_product(key[entry], (a, b)), the unpacked product in both 30-bit forms
//   lds_bytes(d)        dynamic LDS of a workgroup (host)
//   MIN_WAVES           the launch bound
// and forwards to the team device functions of torus_kernels.hpp, torus30_kernels.hpp and torusf_kernels.hpp, which are as they were.
// The host picks the policy in torus_dispatch.hpp (with_key_form).
#pragma once
#include "torus_kernels.hpp"
#include "torus30_kernels.hpp"
#include "torusf_kernels.hpp"

namespace fhe {

constexpr int TF_MIN_WAVES = 2;  // the f64 forms: two waves per SIMD (torusf_kernels.hpp has what was measured against it)

// two 60-bit primes; rows0, rows1: [..][2d][2][N] per prime, key_perm layout
template <class W>
struct Form60 {
    using Ring = W;
    static constexpr int CNT = W::E, N = W::N, MIN_WAVES = W::MIN_WAVES;
    static constexpr bool PAIRS = false;
    struct Key {
        const u64 *__restrict__ rows0, *__restrict__ rows1;
        TDecomp P;
        TorusConsts T;
    };
    struct Team {
        u64 *lds;
    };
    static __host__ __device__ __forceinline__ size_t per(const TDecomp &P) { return size_t(2 * P.d) * 2 * W::N; }
    static size_t lds_bytes(int) { return W::TORUS_LDS_BYTES; }
    static __device__ __forceinline__ Team team_setup(const Key &, unsigned char *smem_raw, int team) {
        return Team{reinterpret_cast<u64 *>(smem_raw) + team * W::TORUS_LDS_WORDS};
    }
    static __device__ __forceinline__ void load(u64 (&c)[CNT], const u64 *__restrict__ g, int lane) { wave_load<W>(c, g, lane); }
    static __device__ __forceinline__ void store(const u64 (&c)[CNT], u64 *__restrict__ g, int lane) { wave_store<W>(c, g, lane); }
    static __device__ __forceinline__ void rotate(u64 (&c)[CNT], unsigned r, int lane, const Team &tm) { team_torus_rotate<W>(c, r, lane, tm.lds); }
    static __device__ __forceinline__ void cmux(u64 (&ca)[CNT], u64 (&cb)[CNT], unsigned r, const Key &key, size_t entry, const Team &tm, int lane) {
        const size_t off = entry * per(key.P);
        team_torus_cmux<W>(ca, cb, r, key.rows0 + off, key.rows1 + off, key.P, key.T, lane, tm.lds);
    }
    static __device__ __forceinline__ void external_product(u64 (&ca)[CNT], u64 (&cb)[CNT], const Key &key, size_t entry, const Team &tm, int lane) {
        const size_t off = entry * per(key.P);
        u64 xa[CNT], xb[CNT];
        team_torus_external_product<W>(ca, cb, key.rows0 + off, key.rows1 + off, key.P, key.T, lane, tm.lds, xa, xb);
#pragma unroll
        for (int e = 0; e < CNT; ++e) { ca[e] = xa[e]; cb[e] = xb[e]; }
    }
};

// three 30-bit primes; rows: the first prime's [..][2d][2][N] u32 (key_perm30 layout), `plane` words to the next prime's.
// PACKED: the CMUX whose digits are computed once (team_torus_cmux30_pk; its LDS carries the digit area, sized by the gadget)
template <class W, bool PACKED>
struct Form30 {
    using Ring = W;
    static constexpr int CNT = W::E, N = W::N, MIN_WAVES = W::MIN_WAVES;
    static constexpr bool PAIRS = false;
    struct Key {
        const unsigned *__restrict__ rows;
        size_t plane;
        TDecomp P;
        Torus30Consts T;
    };
    struct Team {
        u64 *lds;
    };
    static __host__ __device__ __forceinline__ size_t per(const TDecomp &P) { return size_t(2 * P.d) * 2 * W::N; }
    static size_t lds_bytes(int d) { return PACKED ? W::torus_pk_lds_bytes(2 * d) : W::TORUS_LDS_BYTES; }
    static __device__ __forceinline__ Team team_setup(const Key &key, unsigned char *smem_raw, int team) {
        // exchange image | parking area of two residue pairs | PACKED: the digits of one CMUX (at cfg5, N = 2^10, d = 3: 31 232 bytes a team)
        return Team{reinterpret_cast<u64 *>(smem_raw) + team * (W::TORUS_LDS_WORDS + (PACKED ? W::torus_dig_words(2 * key.P.d) : 0))};
    }
    static __device__ __forceinline__ void load(u64 (&c)[CNT], const u64 *__restrict__ g, int lane) { wave_load<W>(c, g, lane); }
    static __device__ __forceinline__ void store(const u64 (&c)[CNT], u64 *__restrict__ g, int lane) { wave_store<W>(c, g, lane); }
    static __device__ __forceinline__ void rotate(u64 (&c)[CNT], unsigned r, int lane, const Team &tm) { team_torus_rotate<W>(c, r, lane, tm.lds); }
    static __device__ __forceinline__ void cmux(u64 (&ca)[CNT], u64 (&cb)[CNT], unsigned r, const Key &key, size_t entry, const Team &tm, int lane) {
        const unsigned *k0 = key.rows + entry * per(key.P);
        if constexpr (PACKED) team_torus_cmux30_pk<W>(ca, cb, r, k0, k0 + key.plane, k0 + 2 * key.plane, key.P, key.T, lane, tm.lds);
        else team_torus_cmux30<W>(ca, cb, r, k0, k0 + key.plane, k0 + 2 * key.plane, key.P, key.T, lane, tm.lds);
    }
    static __device__ __forceinline__ void external_product(u64 (&ca)[CNT], u64 (&cb)[CNT], const Key &key, size_t entry, const Team &tm, int lane) {
        const unsigned *k0 = key.rows + entry * per(key.P);
        u64 xa[CNT], xb[CNT];
        team_torus_external_product30<W>(ca, cb, k0, k0 + key.plane, k0 + 2 * key.plane, key.P, key.T, lane, tm.lds, xa, xb);
#pragma unroll
        for (int e = 0; e < CNT; ++e) { ca[e] = xa[e]; cb[e] = xb[e]; }
    }
};

// The f64 forms, a team over the N / 2 complex slots of a polynomial.  fft64: rows [..][2d][2][N / 2] complex; X3, exact through three key
// pieces: rows [..][2d][2][3][N / 2] complex.  tw: the twiddle tree in HBM.
template <class W, bool X3>
struct FormF {
    using Ring = W;
    static constexpr int CNT = 2 * W::E, N = 2 * W::N, MIN_WAVES = TF_MIN_WAVES;
    static constexpr bool PAIRS = true;
    struct Key {
        const double2 *__restrict__ rows;
        TDecomp P;
        const double2 *__restrict__ tw;
    };
    struct Team {
        u64 *lds;
        ArithC64::K k;
    };
    static __host__ __device__ __forceinline__ size_t per(const TDecomp &P) { return size_t(2 * P.d) * (X3 ? 6 : 2) * W::N; }
    static size_t lds_bytes(int d) { return X3 ? TorusX3<W>::lds_bytes(2 * d) : TorusF<W>::LDS_BYTES; }
    static __device__ __forceinline__ Team team_setup(const Key &key, unsigned char *smem_raw, int team) {
        const int limbs = 2 * key.P.d;
        const double2 *tw = X3 ? stage_twiddles_x3<W>(key.tw, smem_raw, limbs) : stage_twiddles<W>(key.tw, smem_raw);
        return Team{reinterpret_cast<u64 *>(smem_raw) + team * (X3 ? TorusX3<W>::lds_words(limbs) : TorusF<W>::LDS_WORDS), ArithC64::make(tw, W::LOG_N)};
    }
    static __device__ __forceinline__ void load(u64 (&c)[CNT], const u64 *__restrict__ g, int lane) { pairs_load<W>(c, g, lane); }
    static __device__ __forceinline__ void store(const u64 (&c)[CNT], u64 *__restrict__ g, int lane) { pairs_store<W>(c, g, lane); }
    static __device__ __forceinline__ void rotate(u64 (&c)[CNT], unsigned r, int lane, const Team &tm) { pairs_rotate<W>(c, r, lane, tm.lds); }
    static __device__ __forceinline__ void cmux(u64 (&ca)[CNT], u64 (&cb)[CNT], unsigned r, const Key &key, size_t entry, const Team &tm, int lane) {
        const double2 *row = key.rows + entry * per(key.P);
        if constexpr (X3) teamx3_cmux<W>(ca, cb, r, row, key.P, tm.k, lane, tm.lds);
        else teamf_cmux<W>(ca, cb, r, row, key.P, tm.k, lane, tm.lds);
    }
    static __device__ __forceinline__ void external_product(u64 (&ca)[CNT], u64 (&cb)[CNT], const Key &key, size_t entry, const Team &tm, int lane) {
        cmux(ca, cb, 0xffffffffu, key, entry, tm, lane);  // the f64 team functions' own mark of the plain product
    }
};

// ---- external product ----------------------------------------------------------------------------------------------------------------
// scheme/tfhe/src/tggsw.rs:100-112 for k = 1, one team (fhew_kernels.hpp: WaveRing) per ciphertext, in place:
// (a, b) <- external_product(key, (a, b)) under the key entry `key` starts at
template <class F>
__global__ __launch_bounds__(F::Ring::THREADS, F::MIN_WAVES) void torus_external_product_kernel(u64 *__restrict__ acc_a, u64 *__restrict__ acc_b, unsigned batch,
                                                                                                typename F::Key key) {
    using W = typename F::Ring;
    constexpr int CNT = F::CNT, N = F::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = W::lane(), team = W::team();
    const unsigned ct = blockIdx.x * W::TEAMS + team;
    const typename F::Team tm = F::team_setup(key, smem_raw, team);
    if (ct >= batch) return;
    u64 *ga = acc_a + size_t(ct) * N, *gb = acc_b + size_t(ct) * N;
    u64 ca[CNT], cb[CNT];
    F::load(ca, ga, lane);
    F::load(cb, gb, lane);
    F::external_product(ca, cb, key, 0, tm, lane);
    F::store(ca, ga, lane);
    F::store(cb, gb, lane);
}

// ---- blind rotation ----------------------------------------------------------------------------------------------------------------
// scheme/tfhe/src/bootstrapping.rs:84-96 `blind_rotate` (k = 1), the whole fold in ONE launch: acc = (0, v X^-b), then
// acc <- cmux(brk_i, acc, acc X^(a_i)) for i = 0 .. n_lwe-1, the accumulator in the team's registers throughout.
// key: the key set, entry i = brk_i; a_tilde [batch][n_lwe], b_tilde [batch] mod 2N.
// table_of: null = every ciphertext starts from v; else ciphertext ct starts from v + table_of[ct] * N (v: [n_tables][N]).  The index is
// uniform across the team, read once and kept scalar; it is NOT range-checked here: the entry points check host-memory indices,
// device-memory callers guarantee table_of[ct] < n_tables.
template <class F>
__device__ __forceinline__ void blind_rotate_body(const u64 *__restrict__ v, const unsigned *__restrict__ table_of, const u64 *__restrict__ a_tilde,
                                                  const u64 *__restrict__ b_tilde, unsigned n_lwe, unsigned batch, const typename F::Key &key,
                                                  u64 *__restrict__ out_a, u64 *__restrict__ out_b) {
    using W = typename F::Ring;
    constexpr int CNT = F::CNT, N = F::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = W::lane(), team = W::team();
    const unsigned ct = blockIdx.x * W::TEAMS + team;
    const typename F::Team tm = F::team_setup(key, smem_raw, team);
    if (ct >= batch) return;
    u64 ca[CNT], cb[CNT];
    if (table_of != nullptr) v += size_t(__builtin_amdgcn_readfirstlane(table_of[ct])) * N;  // this ciphertext's own table
    F::load(cb, v, lane);
#pragma unroll
    for (int e = 0; e < CNT; ++e) ca[e] = 0;
    F::rotate(cb, (2 * N - (unsigned(b_tilde[ct]) & (2 * N - 1))) & (2 * N - 1), lane, tm);  // (0, v).rotate(-b)
    const u64 *a = a_tilde + size_t(ct) * n_lwe;
#pragma unroll 1
    for (unsigned i = 0; i < n_lwe; ++i) {
        const unsigned r = __builtin_amdgcn_readfirstlane(unsigned(a[i]) & (2 * N - 1));
        F::cmux(ca, cb, r, key, i, tm, lane);
    }
    F::store(ca, out_a + size_t(ct) * N, lane);
    F::store(cb, out_b + size_t(ct) * N, lane);
}

// One kernel name per form: the benchmark's roofline labels and tools/summarize_profiles.py tell the forms apart by them.
template <class W>
__global__ __launch_bounds__(W::THREADS, W::MIN_WAVES) void torus_blind_rotate_kernel(
    const u64 *__restrict__ v, const unsigned *__restrict__ table_of, const u64 *__restrict__ a_tilde, const u64 *__restrict__ b_tilde, unsigned n_lwe,
    unsigned batch, typename Form60<W>::Key key, u64 *__restrict__ out_a, u64 *__restrict__ out_b) {
    blind_rotate_body<Form60<W>>(v, table_of, a_tilde, b_tilde, n_lwe, batch, key, out_a, out_b);
}
template <class W>
__global__ __launch_bounds__(W::THREADS, W::MIN_WAVES) void torus30_blind_rotate_kernel(
    const u64 *__restrict__ v, const unsigned *__restrict__ table_of, const u64 *__restrict__ a_tilde, const u64 *__restrict__ b_tilde, unsigned n_lwe,
    unsigned batch, typename Form30<W, false>::Key key, u64 *__restrict__ out_a, u64 *__restrict__ out_b) {
    blind_rotate_body<Form30<W, false>>(v, table_of, a_tilde, b_tilde, n_lwe, batch, key, out_a, out_b);
}
// torus30_kernels.hpp has what was measured against this one's two waves per SIMD
template <class W>
__global__ __launch_bounds__(W::THREADS, W::MIN_WAVES) void torus30_blind_rotate_pk_kernel(
    const u64 *__restrict__ v, const unsigned *__restrict__ table_of, const u64 *__restrict__ a_tilde, const u64 *__restrict__ b_tilde, unsigned n_lwe,
    unsigned batch, typename Form30<W, true>::Key key, u64 *__restrict__ out_a, u64 *__restrict__ out_b) {
    blind_rotate_body<Form30<W, true>>(v, table_of, a_tilde, b_tilde, n_lwe, batch, key, out_a, out_b);
}
template <class W>
__global__ __launch_bounds__(W::THREADS, TF_MIN_WAVES) void torusf_blind_rotate_kernel(
    const u64 *__restrict__ v, const unsigned *__restrict__ table_of, const u64 *__restrict__ a_tilde, const u64 *__restrict__ b_tilde, unsigned n_lwe,
    unsigned batch, typename FormF<W, false>::Key key, u64 *__restrict__ out_a, u64 *__restrict__ out_b) {
    blind_rotate_body<FormF<W, false>>(v, table_of, a_tilde, b_tilde, n_lwe, batch, key, out_a, out_b);
}
template <class W>
__global__ __launch_bounds__(W::THREADS, TF_MIN_WAVES) void torusx3_blind_rotate_kernel(
    const u64 *__restrict__ v, const unsigned *__restrict__ table_of, const u64 *__restrict__ a_tilde, const u64 *__restrict__ b_tilde, unsigned n_lwe,
    unsigned batch, typename FormF<W, true>::Key key, u64 *__restrict__ out_a, u64 *__restrict__ out_b) {
    blind_rotate_body<FormF<W, true>>(v, table_of, a_tilde, b_tilde, n_lwe, batch, key, out_a, out_b);
}

}  // namespace fhe
